"""Cases, float64 references, per-entry scales and bounds of the bf16-operand GEMMs
(csrc/gemm_bf16*.hip: mrl_gemm_bf16 and mrl_gemm_bf16_tn): tests/test_gemm_bf16_host.py on the
CPU, tests/test_gpu_gemm_bf16.py on the device.  Built in the manner of tests/gemm_cases.py, whose
``evaluate`` (value and scale), ``distance`` and constants it uses.  Nothing here reads a device.

Dispatch.  ``route`` restates nn_route / tn_route of the C code (the CU count and the
environment thresholds are parameters), ``plan`` the grids, K-stage / quarter / chunk counts,
slab split, XCD remap and per-kernel predicates, ``branches`` the facts of a case the host test
counts.  A case names the kernel it was written for (``kernel``) and carries the settings that
force it at a small M (``env_of``, ``lds``); the streaming cases whose rows are shorter than the
K plan's last k-step are written for the launcher's refusal (``route`` gives the tiled kernel).

Operands.  Every value is bf16-exact: an 8-bit mantissa in +-[0.5, 1) times 2^e_i (row of A) or
2^f_j (column of B), e and f integers of [-8, 8]; H is a multiple of 2^-8 in (-1, 1).  The
rounding contract therefore costs nothing, every product is exact in float32, and one missing
term moves an entry by at least 0.25 / (terms + 2^8) of its scale.  Row 1 of A is zero where
there are 3 rows: without a bias those entries have scale 0 and must be exact.  ``layout`` builds
the bf16 images (uint16): the padding columns K..ld of A, A2, Bt and Bt2 are zero (the contract);
GUARD rows before and after every operand and H, the padding columns of H, the TN operands'
padding columns and the floats around the bias are NaN; C, the slabs, their padding columns,
guard rows and the gaps between slabs hold a sentinel (SENT_BITS, or SENT16 for bf16 output).

Reference and bound.  ``reference`` is gemm_cases.evaluate in float64, per slab over the slab's
own k range for TN (the ones-row with scale sum_k |b_kj|).  ``restatement`` is numpy float32,
one accumulation per k in ascending order, tanh_fast_f32, 1 - h * h as one rounding.
FLOOR[(kernel, epilogue)] is its largest distance from the reference over CASES, TOL = 4 x FLOOR
(the margin argued in gemm_cases), capped by the a-priori (terms + 2) u; where FLOOR is 0 (exact
sums) the a-priori bound alone.  bf16 output adds half a bf16 ulp of the reference per entry, one
RNE rounding to 8 significant bits: 2^-8 of the reference's power of two, which lies between 2^-9
and 2^-8 of |reference| (derived, not measured; 2^-9 |reference| itself is what a correct rounding
stays under only next to the powers of two, so it cannot serve as the bound)."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from tests.gemm_cases import GUARD, SENT_BITS, SLAB_GAP, U, distance, evaluate
from tests.mlp_width_cases import round_up2, tanh_fast_f32  # noqa: F401  (round_up2: how FLOOR is rounded)

SENT16 = np.uint16(0xC9A5)  # bf16 of about -1.35e6
NAN16 = np.uint16(0x7FC0)
BIAS_LEAD = 4               # NaN floats in front of the bias (keeps its 16-byte alignment)
EPIS = ("store", "tanh", "dtanh")
NCU = 256                   # the CU count the case list was written for (MI355X)

# kind "nn": C[m, n] = A[m, k] Bt[n, k]^T (+ A2 Bt2^T) + bias; "tn": slabs [m, n] over k rows,
# m = m_real + ones.  lay: the ldc / ldh form; ldx: bf16 added to ld8(.) of lda / ldb.
Case = namedtuple("Case", "kind kernel m n k dual bias epi bf ones splits lay ldx lds")

ROUTES = ("none", "tiled128_bk64", "tiled128_bk32", "tiled32_bk64", "tiled32_bk32", "small", "stream384", "stream512",
          "big", "tn_tiled32", "tn_tiled128", "tn_big")
ROUTE_ID = {r: i for i, r in enumerate(ROUTES)}  # the MRL_GEMM_ROUTE_* values of include/mrl_hip.h

DEFAULT_ENV = {"MRL_GEMM_BIG_MIN_M": 65536, "MRL_GEMM_STREAM_MIN_M": 32768, "MRL_GEMM_SMALL_MAX_M": 8192,
               "MRL_GEMM_TN_BIG": 1}
TILED_ENV = {"MRL_GEMM_BIG_MIN_M": 0, "MRL_GEMM_STREAM_MIN_M": 0, "MRL_GEMM_SMALL_MAX_M": 0, "MRL_GEMM_TN_BIG": 0}


def env_of(c):
    """The thresholds that force the case's kernel at its small M."""
    e = dict(TILED_ENV)
    if c.kernel == "small":
        e["MRL_GEMM_SMALL_MAX_M"] = 8192
    elif c.kernel == "stream":
        e["MRL_GEMM_STREAM_MIN_M"] = 1
    elif c.kernel == "big":
        e["MRL_GEMM_BIG_MIN_M"] = 1
    elif c.kernel == "tn_big":
        e["MRL_GEMM_TN_BIG"] = 1
    return e


def case_id(c):
    return "%s-%s-%dx%dx%d-%s%s%s%s%s%s-%s%s%s" % (
        c.kind, c.kernel, c.m, c.n, c.k, c.epi, "-dual" if c.dual else "", "-bias" if c.bias else "",
        "-bf" if c.bf else "", "-ones" if c.ones else "", "-s%d" % c.splits if c.kind == "tn" else "", c.lay,
        "-ldx%d" % c.ldx if c.ldx else "", "-lds%d" % c.lds if c.lds else "")


def ld8(x):
    return (x + 7) // 8 * 8


# ------------------------------------------------------------------ the host dispatch, restated
def cu_count(ncu):
    """cu_count() of gemm_bf16_host.h: at least 8 and a multiple of 8, else 0."""
    return ncu if ncu >= 8 and ncu % 8 == 0 else 0


def dims(c):
    """Extents, leading dimensions and element offsets of the stored operands and outputs."""
    d = SimpleNamespace(mr=c.m - c.ones)
    if c.kind == "nn":
        d.lda = d.ldb = max(8, ld8(c.k)) + c.ldx  # K = 0: one chunk of zero padding, a non-empty allocation
    else:
        d.lda, d.ldb = ld8(d.mr) + c.ldx, ld8(c.n) + c.ldx
    n8 = ld8(c.n)
    d.ldc, d.ldh = {"tight": (c.n, c.n), "n1": (c.n + 1, c.n + 1), "r8": (n8, n8), "hodd": (n8, n8 + 1),
                    "codd": (n8 + 1, n8), "r4": (n8 + 4, n8 + 4), "pad3": (c.n + 3, c.n + 3)}[c.lay]
    d.S = len(k_ranges(c))
    d.slab_stride = c.m * d.ldc + SLAB_GAP if c.kind == "tn" else 0
    d.c_off = GUARD * d.ldc
    d.c_size = 2 * GUARD * d.ldc + (d.S * d.slab_stride if c.kind == "tn" else c.m * d.ldc)
    return d


def tn_chunk(c):
    """k_chunk of tn_route: the split of mrl_gemm_slab_splits, whole 32-row steps."""
    req = max(1, c.splits)
    return max(32, (-(-c.k // req) + 31) // 32 * 32)


def k_ranges(c):
    """[(kbeg, kend)] per slab; one range for an NN product; K = 0 gives one empty slab."""
    if c.kind == "nn" or c.k <= 0:
        return [(0, c.k)]
    ch = tn_chunk(c)
    return [(z * ch, min(c.k, (z + 1) * ch)) for z in range(-(-c.k // ch))]


def big_plan(c, ncu, env):
    """big_gemm_plan: None, or (row tiles, column tiles, blocks per XCD)."""
    nst = (2 if c.dual else 1) * -(-c.k // 32)
    min_m = env["MRL_GEMM_BIG_MIN_M"]
    if min_m <= 0 or c.m < min_m or c.n < 128 or nst <= 0 or nst % 4:
        return None
    cu = cu_count(ncu)
    if cu == 0:
        return None
    ntn = -(-c.n // 256)
    per_xcd = (cu // 8) // ntn * ntn
    return (-(-c.m // 256), ntn, per_xcd) if per_xcd >= ntn else None


def stream_plan(c, ncu, env):
    """stream_gemm_plan: None, or (K plan, column slices, row groups per XCD)."""
    min_m = env["MRL_GEMM_STREAM_MIN_M"]
    if min_m <= 0 or c.dual or c.m < min_m or c.n < 64 or c.k <= 256 or c.k > 512:
        return None
    kp = 384 if c.k <= 384 else 512
    if dims(c).lda < kp - 16:  # a row must reach the plan's last k-step, the only masked one
        return None
    cu = cu_count(ncu)
    if cu == 0:
        return None
    nslice = -(-c.n // 128)
    groups = (cu // 8) // nslice
    return (kp, nslice, groups) if groups >= 1 else None


def route(c, ncu=NCU, env=None):
    """nn_route / tn_route: the name of the kernel a launch of the case runs."""
    env = env_of(c) if env is None else env
    if c.m <= 0 or c.n <= 0:
        return "none"
    if c.kind == "tn":
        mr = c.m - c.ones
        if env["MRL_GEMM_TN_BIG"] != 0 and c.lds <= 0 and mr >= 256 and c.n >= 256 and mr % 8 == 0 and c.n % 8 == 0:
            return "tn_big"
        return "tn_tiled32" if c.n <= 32 else "tn_tiled128"
    w = "32" if c.n <= 32 else "128"
    if c.lds > 0:
        k64 = 2 * 2 * (128 + int(w)) * (64 + 8) <= c.lds
        return "tiled%s_bk%d" % (w, 64 if k64 else 32)
    if big_plan(c, ncu, env):
        return "big"
    if not c.dual and c.m <= env["MRL_GEMM_SMALL_MAX_M"] and c.k <= 512 and c.n >= 64 and c.epi != "dtanh":
        return "small"
    sp = stream_plan(c, ncu, env)
    if sp:
        return "stream%d" % sp[0]
    return "tiled%s_bk64" % w


def plan(c, ncu=NCU, env=None):
    """What the routed kernel does with the case: grid, tile, K stages, remap, epilogue ``vec``,
    and per kernel its own counts (see ``branches``)."""
    r, d = route(c, ncu, env), dims(c)
    env = env_of(c) if env is None else env
    p = SimpleNamespace(route=r)
    nprod = 2 if c.dual else 1
    vec4 = d.ldc % 4 == 0 and (c.epi != "dtanh" or d.ldh % 4 == 0)
    if r.startswith("tiled"):
        p.bm, p.bn, p.bk = 128, int(r[5:].split("_")[0]), int(r[-2:])
        p.grid = (-(-c.n // p.bn), -(-c.m // 128), 1)
        p.remap = (p.grid[0] * p.grid[1]) % 8 == 0
        p.stages = nprod * -(-c.k // p.bk)
        p.vec = vec4
    elif r == "small":
        p.bm = p.bn = 64
        p.grid = (-(-c.n // 64), -(-c.m // 64), 1)
        p.remap, p.quarters, p.vec = False, -(-c.k // 128), d.ldc % 4 == 0
        p.chunks = -(-c.k // 8)  # 16-byte chunks that read memory; the rest read the zero block
    elif r.startswith("stream"):
        kp, nslice, groups = stream_plan(c, ncu, env)
        p.bm, p.bn, p.kp, p.nslice, p.groups = 256, 128, kp, nslice, groups
        p.grid = (cu_count(ncu), 1, 1)
        p.ntiles = -(-c.m // 256)
        p.tiles_per_block = -(-p.ntiles // (8 * groups))  # of the busiest block
        p.remap, p.vec, p.chunks = False, vec4, 4
        p.last_step_masked = d.lda < kp
    elif r == "big":
        ntm, ntn, per_xcd = big_plan(c, ncu, env)
        p.bm = p.bn = 256
        p.grid = (8 * per_xcd, 1, 1)
        p.ntm, p.ntn, p.rows_per_round = ntm, ntn, per_xcd // ntn
        p.tiles_per_block = -(-ntm // (8 * p.rows_per_round))
        p.stages = nprod * -(-c.k // 32)
        p.remap = False
        p.vec = d.ldc % 8 == 0 and (c.epi != "dtanh" or d.ldh % 8 == 0)
    elif r.startswith("tn_tiled"):
        p.bm, p.bn = 128, int(r[8:])
        p.grid = (-(-c.n // p.bn), -(-c.m // 128), d.S)
        p.k_chunk, p.remap = tn_chunk(c), False
    elif r == "tn_big":
        p.bm = p.bn = 256
        p.ntm, p.ntn = -(-d.mr // 256), -(-c.n // 256)
        p.rounds = -(-d.S // 8)
        p.grid = (8 * p.rounds * p.ntm * p.ntn, 1, 1)
        p.k_chunk, p.remap = tn_chunk(c), False
    return p


def branches(c, ncu=NCU):
    """The facts of a case the host test counts, prefixed by the routed kernel's family."""
    p, d = plan(c, ncu), dims(c)
    fam = family(p.route)
    b = {"intended" if fam == c.kernel else "declined_to_" + fam}
    if c.kind == "nn":
        b |= {"dual" if c.dual else "single", "bias" if c.bias else "nobias", c.epi, "bf16out" if c.bf else "f32out",
              "vec" if p.vec else "scalar"}
        if p.vec and c.n % (8 if fam == "big" else 4):
            b.add("vec_partial_run")
        if c.epi == "dtanh":
            b.add("ldh_eq_ldc" if d.ldh == d.ldc else "ldh_ne_ldc")
        b.add("m_edge" if c.m % p.bm else "m_even")
        b.add("n_edge" if c.n % p.bn else "n_even")
        b.add("lda_padded" if c.ldx else "lda_ld8")
    if fam == "tiled":
        b |= {"tile%d" % p.bn, "bk%d" % p.bk, "remap" if p.remap else "noremap"}
        b.add("k0" if c.k == 0 else "ktail" if c.k % p.bk else "kfull")
        if c.k % 8:
            b.add("k_chunk_partial")
        if c.dual and c.k % p.bk:
            b.add("dual_ktail")
        if p.grid[0] * p.grid[1] > 1:
            b.add("blocks>1")
    elif fam == "small":
        b |= {"quarters%d" % p.quarters, "blocks>1" if p.grid[0] * p.grid[1] > 1 else "block1"}
        if c.k % 128:
            b.add("partial_quarter")
        if c.k % 8:
            b.add("chunk_past_k")
        if c.m % 64:
            b.add("rows_clamped")
        if c.n % 64:
            b.add("cols_clamped")
    elif fam == "stream":
        b |= {"plan%d" % p.kp, "slices%d" % p.nslice}
        if c.n % 128:
            b.add("partial_slice")
        b.add("last_step_masked" if p.last_step_masked else "last_step_read")
        if c.k < p.kp - 16:
            b.add("k_steps_of_zeros")
        b.add("two_row_tiles" if p.tiles_per_block >= 2 else "one_row_tile")
        if p.ntiles < 8 * p.groups:
            b.add("idle_groups")
    elif fam == "big":
        b |= {"ntn%d" % p.ntn, "stages%d" % p.stages}
        b.add("interior_dma" if c.m >= 256 and c.n >= 256 and c.k >= 32 else "edge_dma_only")
        if c.k % 32:
            b.add("ktail")
        if c.k % 8:
            b.add("k_chunk_partial")
        b.add("two_row_tiles" if p.tiles_per_block >= 2 else "one_row_tile")
        if p.ntm < 8 * p.rows_per_round:
            b.add("idle_blocks")
    elif fam in ("tn_tiled", "tn_big"):
        b |= {"ones" if c.ones else "noones", "slabs%d" % d.S, "ldc_tight" if d.ldc == c.n else "ldc_padded"}
        ch, last = p.k_chunk, k_ranges(c)[-1]
        if c.k == 0:
            b.add("k0")
        else:
            if d.S < min(max(1, c.splits), c.k):
                b.add("slab_clamped")
            b.add("slab_exact" if c.k % ch == 0 else "slab_ragged")
            if (last[1] - last[0]) % 32:
                b.add("stage_ragged")
        if fam == "tn_tiled":
            b.add("tile%d" % p.bn)
            if c.ones:
                b.add("ones_alone" if d.mr % 128 == 0 else "ones_shared")
            if d.mr % 8:
                b.add("chunk_straddles_m_real")
            if c.n % 8:
                b.add("chunk_straddles_n")
        else:
            b |= {"rounds%d" % p.rounds, "ntm%d" % p.ntm, "ntn%d" % p.ntn}
            stages = {-(-(e - s) // 32) for s, e in k_ranges(c)}
            b |= {"stages<4" if s < 4 else "stages>=4" for s in stages}
            if c.ones and c.n % 32 in range(1, 17):
                b.add("ones_second_half_cut")
            if d.mr % 256:
                b.add("m_edge")
            if c.n % 256:
                b.add("n_edge")
    return {fam + ":" + x for x in b}


def family(r):
    return "tn_tiled" if r.startswith("tn_tiled") else "tiled" if r.startswith("tiled") else \
        "stream" if r.startswith("stream") else r


# ------------------------------------------------------------------ the case list
LAYS = ("tight", "n1", "r8", "hodd", "codd", "r4")
DT_LAYS = ("hodd", "codd", "r8", "tight", "n1", "r4")  # DTANH: ldh against ldc first


def _nn(kernel, m, n, k, i, dual=None, epi=None, ldx=0, lds=0, lay=None):
    """Case i of a list: the options cycle with i at coprime periods."""
    if epi is None:  # a one-row or one-column shape avoids TANH: its few entries could all saturate
        epi = "dtanh" if EPIS[i % 3] == "tanh" and min(m, n) == 1 else EPIS[i % 3]
    dual = (i // 2) % 2 if dual is None else dual
    if lay is None:
        lay = DT_LAYS[(i // 3) % 6] if epi == "dtanh" else LAYS[i % 6]
    return Case("nn", kernel, m, n, k, int(dual), (i // 3) % 2, epi, i % 2, 0, 0, lay, ldx, lds)


def _cycle(vals, i, step=1):
    return vals[(i * step) % len(vals)]


# tiled NN: every M, N, K edge value at least once (COVER), BK 64 and 32 by lds_limit, both tile
# widths; 1000 rows give 8 row tiles (the XCD remap) at either width
T_M, T_N = (1, 127, 128, 129, 257), (1, 31, 32, 33, 127, 128, 129, 257)
T_K = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130)
TILED = [_nn("tiled", _cycle(T_M, i), _cycle(T_N, i, 3), _cycle(T_K, i), i, lds=(0, 81920, 65536, 40960)[i % 4])
         for i in range(24)]
TILED += [_nn("tiled", 1000, 33, 65, 24), _nn("tiled", 1000, 31, 33, 25, lds=40960), _nn("tiled", 1000, 129, 130, 26),
          _nn("tiled", 129, 33, 0, 27, dual=0, epi="store"), _nn("tiled", 33, 31, 0, 30, dual=1, epi="tanh")]
# a modest product on one ragged shape: epilogue x dual x bias x output, layouts cycling
TILED += [Case("nn", "tiled", 129, 130, 65, du, bi, epi, bf, 0, 0, LAYS[(3 * ei + 2 * du + bi + bf) % 6], 0,
               (0, 65536)[(du + bf) % 2])
          for ei, epi in enumerate(EPIS) for du in (0, 1) for bi in (0, 1) for bf in (0, 1)]

S_M, S_N, S_K = (1, 63, 64, 65, 130), (64, 65, 127, 200), (1, 8, 120, 127, 128, 129, 200, 376, 385, 512)
SMALL = [_nn("small", _cycle(S_M, i), _cycle(S_N, i), _cycle(S_K, i), i, dual=0, epi=("store", "tanh")[(i // 2) % 2])
         for i in range(10)]
SMALL += [_nn("small", 130, 200, 512, 10, dual=0, epi="tanh", lay="r8"), _nn("small", 65, 64, 129, 11, dual=0, epi="store")]

# streaming with lda = ldb = ld8(K): K <= 367 (plan 384) and 385..495 (plan 512) must be refused
# by the launcher (their rows end before the plan's last k-step) and run tiled; the same K with
# rows as long as the plan (ldx) stream, as do 368..384 and 496..512
ST_K = (257, 264, 300, 360, 367, 368, 376, 384, 385, 392, 440, 495, 496, 504, 512)
ST_M, ST_N = (1, 31, 32, 33, 255, 256, 257, 300), (64, 65, 128, 129, 200, 300)
STREAM = [_nn("stream", _cycle(ST_M, i), _cycle(ST_N, i), k, i, dual=0) for i, k in enumerate(ST_K)]
STREAM += [_nn("stream", _cycle(ST_M, i, 3), _cycle(ST_N, i, 5), k, i + 1, dual=0, ldx=(384 if k <= 384 else 512) - ld8(k))
           for i, k in enumerate((257, 300, 367, 385, 440, 495))]
STREAM += [_nn("stream", 300, 300, 360, 4, dual=0, ldx=8)]  # lda = 368 = KP - 16: the shortest row that streams
# N = 512 is 4 slices, 8 groups per XCD on 256 CUs: 64 row groups, so 65 + 1 row tiles give the
# first blocks a second tile and the last one a ragged one
STREAM_TALL = _nn("stream", 8 * (NCU // 8 // 4) * 256 + 300, 512, 376, 1, dual=0, epi="tanh", lay="tight")
STREAM.append(STREAM_TALL)

B_KS, B_KD = (97, 100, 120, 128, 225, 250, 256), (33, 40, 64, 97, 128)
B_M, B_N = (1, 255, 256, 257, 300), (128, 129, 255, 256, 257, 300)
BIG = [_nn("big", _cycle(B_M, i), _cycle(B_N, i), k, i, dual=0) for i, k in enumerate(B_KS)]
BIG += [_nn("big", _cycle(B_M, i, 2), _cycle(B_N, i, 5), k, i + 1, dual=1) for i, k in enumerate(B_KD)]
BIG += [_nn("big", 300, 300, 128, 2, dual=0, lay="r8"), _nn("big", 257, 256, 64, 5, dual=1, lay="tight")]
# N = 300 is 2 column tiles, 16 row tiles per round and XCD on 256 CUs: 128 + 2 row tiles
BIG_TALL = _nn("big", 8 * (NCU // 8 // 2) * 256 + 300, 300, 100, 0, dual=0, epi="store", lay="r8")
BIG.append(BIG_TALL)


def _tn(kernel, mr, n, k, splits, ones, lay, ldx=0):
    return Case("tn", kernel, mr + ones, n, k, 0, 0, "slab", 0, int(ones), splits, lay, ldx, 0)


TN_M, TN_N = (1, 7, 8, 9, 127, 128, 129, 255), (1, 31, 32, 33, 128, 129, 130)
TN_K, TN_S = (0, 1, 31, 32, 33, 96, 100, 1287), (1, 3, 4, 41, 64)
TN_TILED = [_tn("tn_tiled", _cycle(TN_M, i), _cycle(TN_N, i, 2), _cycle(TN_K, i, 3), _cycle(TN_S, i + 1, 2), i % 2,
                ("tight", "pad3")[(i // 2) % 2], ldx=8 * ((i // 4) % 2)) for i in range(16)]
TN_TILED += [_tn("tn_tiled", 128, 130, 1287, 41, 1, "pad3"), _tn("tn_tiled", 129, 32, 100, 4, 1, "tight"),
             _tn("tn_tiled", 255, 33, 96, 3, 0, "pad3"), _tn("tn_tiled", 8, 1, 33, 64, 1, "tight")]
# (m_real, n, k, splits): one slab of 5 rows; 7 slabs of 32; 8 of 64; 9 of 96 (two rounds per
# XCD, three stages: fewer than the pipeline's four buffers); 3 of 128 with a ragged last one;
# 9 of 32, the last of 22 rows
TN_BIG = [_tn("tn_big", 256, 256, 5, 1, 1, "tight"), _tn("tn_big", 264, 256, 224, 7, 0, "pad3"),
          _tn("tn_big", 256, 264, 512, 8, 1, "pad3"), _tn("tn_big", 376, 512, 864, 9, 1, "tight"),
          _tn("tn_big", 512, 520, 306, 3, 1, "pad3", ldx=8), _tn("tn_big", 256, 256, 278, 9, 0, "tight"),
          _tn("tn_big", 264, 264, 100, 1, 1, "tight")]

GROUPS = {"tiled-cover": TILED[:29], "tiled-product": TILED[29:], "small": SMALL, "stream": STREAM[:-1],
          "stream-tall": STREAM[-1:], "big": BIG[:-1], "big-tall": BIG[-1:], "tn-tiled": TN_TILED, "tn-big": TN_BIG}
CASES = [c for g in GROUPS.values() for c in g]


# ------------------------------------------------------------------ operands
def bits16(a):
    """The bf16 bit patterns of bf16-exact float32 values."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not bf16-exact"
    return (u >> 16).astype(np.uint16)


def rne_bits(x):
    """float32 -> bf16 bits, round to nearest even; inf stays inf, the largest finite values
    round to inf, a NaN stays a NaN (quiet bit set, as the device's conversion)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = (u[nan] >> 16) | 0x40
    return r.astype(np.uint16)


def from_bits16(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=8)
def operands(mr, n, k):
    """The logical operands of every case of one shape, float32 and bf16-exact: A [mr, k],
    B [k, n], the second pair, bias [n], H [mr, n]."""
    rng = np.random.default_rng([16, mr, n, k])

    def mant(*s):
        return rng.integers(128, 256, s) / 256.0 * rng.choice([-1.0, 1.0], s)

    e, f = 2.0 ** rng.integers(-8, 9, mr), 2.0 ** rng.integers(-8, 9, n)
    o = SimpleNamespace(A=mant(mr, k) * e[:, None], B=mant(k, n) * f[None, :], A2=mant(mr, k) * e[:, None],
                        B2=mant(k, n) * f[None, :], bias=mant(n) * f, H=rng.integers(-255, 256, (mr, n)) / 256.0)
    for name, a in vars(o).items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if mr >= 3 and name in ("A", "A2"):
            a[1] = 0
        a.setflags(write=False)
        setattr(o, name, a)
    return o


def case_operands(c):
    return operands(c.m - c.ones, c.n, c.k)


def _image(rows, ext, ld, data, pad):
    """[GUARD + rows + GUARD, ld] bf16 bits: NaN guard rows, ``pad`` in the columns ext..ld."""
    img = np.full((rows + 2 * GUARD, ld), NAN16, dtype=np.uint16)
    img[GUARD:GUARD + rows, ext:] = pad
    img[GUARD:GUARD + rows, :ext] = bits16(data)
    return img.reshape(-1)


def layout(c):
    """``dims`` plus the flat host buffers of a launch (a base is buffer + *_off elements) and
    the output buffer ``C`` of sentinels (uint32, or uint16 for bf16 output)."""
    o, d = case_operands(c), dims(c)
    d.a_off, d.b_off, d.h_off, d.bias_off = GUARD * d.lda, GUARD * d.ldb, GUARD * d.ldh, BIAS_LEAD
    d.A2 = d.B2 = d.bias = d.H = None
    if c.kind == "nn":
        d.A, d.B = _image(c.m, c.k, d.lda, o.A, 0), _image(c.n, c.k, d.ldb, o.B.T, 0)
        if c.dual:
            d.A2, d.B2 = _image(c.m, c.k, d.lda, o.A2, 0), _image(c.n, c.k, d.ldb, o.B2.T, 0)
        if c.bias:
            nan = np.full(BIAS_LEAD, np.nan, dtype=np.float32)
            d.bias = np.concatenate([nan, o.bias, nan[:GUARD]])
        if c.epi == "dtanh":
            d.H = _image(c.m, c.n, d.ldh, o.H, NAN16)
    else:  # row-major over the k rows; the padding columns are never read by design
        d.A, d.B = _image(c.k, d.mr, d.lda, o.A.T, NAN16), _image(c.k, c.n, d.ldb, o.B, NAN16)
    d.C = np.full(d.c_size, SENT16 if c.bf else SENT_BITS, dtype=np.uint16 if c.bf else np.uint32)
    return d


@functools.lru_cache(maxsize=64)
def _valid_index(m, n, ldc, S, stride, off):
    return off + (np.arange(S)[:, None, None] * stride + np.arange(m)[None, :, None] * ldc + np.arange(n)[None, None, :])


def valid_index(c):
    """Flat indices [S, m, n] of the valid entries in the C buffer."""
    d = dims(c)
    return _valid_index(c.m, c.n, d.ldc, d.S, d.slab_stride, d.c_off)


def to_bits(c, values):
    v = np.asarray(values, dtype=np.float32)
    return rne_bits(v) if c.bf else v.view(np.uint32)


def to_values(c, bits):
    return from_bits16(bits) if c.bf else np.asarray(bits, dtype=np.uint32).view(np.float32)


def embed(c, values):
    """The C buffer (bits) after a launch that wrote ``values`` [S, m, n] and nothing else."""
    buf = layout_c(c)
    buf[valid_index(c)] = to_bits(c, values)
    return buf


def layout_c(c):
    return np.full(dims(c).c_size, SENT16 if c.bf else SENT_BITS, dtype=np.uint16 if c.bf else np.uint32)


# ------------------------------------------------------------------ float64 reference and scales
def _f64_operands(c):
    o = case_operands(c)
    return tuple(getattr(o, x).astype(np.float64) for x in ("A", "B", "A2", "B2", "bias", "H"))


def _ref_key(c):
    return c._replace(kernel="", bf=0, lay="tight", ldx=0, lds=0, splits=tn_chunk(c) if c.kind == "tn" else 0)


@functools.lru_cache(maxsize=4)
def _reference(key, ranges):
    v, sc = evaluate(key, *_f64_operands(key), ranges=list(ranges))
    v.setflags(write=False)
    sc.setflags(write=False)
    return v, sc


def reference(c):
    """(value, scale) [S, m, n] in float64; per slab over the slab's own k range."""
    return _reference(_ref_key(c)._replace(splits=0), tuple(k_ranges(c)))


def terms(c):
    return np.array([(e - s) * (2 if c.dual else 1) + c.bias for s, e in k_ranges(c)], dtype=np.float64)[:, None, None]


def apriori(c):
    return (terms(c) + 2) * U


# ------------------------------------------------------------------ float32 restatement
@functools.lru_cache(maxsize=4)
def _pre_f32(mr, n, k, dual, ones, ranges):
    o = operands(mr, n, k)
    A = np.vstack([o.A, np.ones((1, k), dtype=np.float32)]) if ones else o.A
    out = []
    for s, e in ranges:
        acc = np.zeros((mr + ones, n), dtype=np.float32)
        for ops in ((A, o.B), (o.A2, o.B2))[:2 if dual else 1]:
            for kk in range(s, e):
                acc += ops[0][:, kk, None] * ops[1][None, kk, :]
        out.append(acc)
    out = np.stack(out)
    out.setflags(write=False)
    return out


def restatement(c, rounded=True):
    """The case in numpy float32 [S, m, n]; ``rounded``: bf16 output rounded (RNE) as stored."""
    o = case_operands(c)
    v = _pre_f32(c.m - c.ones, c.n, c.k, c.dual, c.ones, tuple(k_ranges(c)))
    if c.bias:
        v = v + o.bias
    if c.epi == "tanh":
        with np.errstate(over="ignore"):
            v = tanh_fast_f32(v)
    elif c.epi == "dtanh":
        v = v * (1.0 - o.H.astype(np.float64) ** 2).astype(np.float32)  # fmaf(-h, h, 1): one rounding
    v = np.asarray(v, dtype=np.float32)
    return from_bits16(rne_bits(v)) if (c.bf and rounded) else v


# ------------------------------------------------------------------ distances and bounds
def half_ulp16(want):
    """Half a bf16 ulp at ``want`` (8 significant bits): 2^(floor(log2 |want|) - 8); 0 at 0."""
    m, e = np.frexp(np.abs(want))  # |want| = m 2^e, m in [0.5, 1)
    return np.where(m > 0, np.ldexp(1.0, e - 1 - 8), 0.0)



def case_distance(c, got):
    """Per slab [S, 1, 1]: the largest error in scale units; for bf16 output the part of the
    error above half a bf16 ulp of the reference.  inf for a NaN, an inf or an inexact scale-0 entry."""
    want, scale = reference(c)
    got = np.asarray(got, dtype=np.float64)
    if c.bf and got.shape == want.shape:
        with np.errstate(invalid="ignore"):
            got = want + np.maximum(np.abs(got - want) - half_ulp16(want), 0.0)
    return distance(got, want, scale)


def measure_floors(visit=None):
    """FLOOR recomputed: the unrounded restatements against the float64 reference over CASES;
    ``visit(case, rounded restatement)`` sees each case on the way."""
    worst = {}
    for c in CASES:
        r = restatement(c, rounded=False)
        if visit is not None:
            visit(c, restatement(c))
        key = (c.kernel, c.epi)
        worst[key] = max(worst.get(key, 0.0), float(distance(r, *reference(c)).max()))
    return worst


# measure_floors() on the CPU, rounded up to two digits (numpy 2.2)
FLOOR = {
    # products of two 8-bit mantissas are exact and a few dozen terms of one entry's common scale
    # sum without rounding in float32: what is measured is the tail of the longer sums, the bias
    # and the epilogue; a slab has neither and at most 96 .. 128 terms here
    ("tiled", "store"): 5.8e-08, ("tiled", "tanh"): 3.3e-08, ("tiled", "dtanh"): 3.9e-08,
    ("small", "store"): 4.8e-08, ("small", "tanh"): 2.6e-08,
    ("stream", "store"): 3.5e-08, ("stream", "tanh"): 2.8e-08, ("stream", "dtanh"): 4.1e-08,
    ("big", "store"): 4.9e-08, ("big", "tanh"): 3.3e-08, ("big", "dtanh"): 4.7e-08,
    ("tn_tiled", "slab"): 0.0, ("tn_big", "slab"): 0.0,
}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}  # 0: the a-priori bound holds alone (``tol``)


def tol(c):
    """The f32 bound in scale units, per slab [S, 1, 1]: 4 x FLOOR capped by the a-priori bound of
    the slab's own term count; the a-priori bound where FLOOR is 0 (exact sums)."""
    f = FLOOR[(c.kernel, c.epi)]
    return np.minimum(4.0 * f, apriori(c)) if f > 0 else apriori(c)


def within(c, bits):
    """[] or what is wrong with the flat C buffer ``bits`` (uint32, or uint16 for bf16 output)
    after a launch of the case: a disturbed sentinel (padding columns, guard rows, slab gaps), a
    NaN among the valid entries, a slab over its bound."""
    want_dt = np.uint16 if c.bf else np.uint32
    bits = np.asarray(bits).reshape(-1)
    d, bad = dims(c), []
    if bits.dtype != want_dt or bits.size != d.c_size:
        return [("buffer", str(bits.dtype), bits.size, d.c_size)]
    idx = valid_index(c)
    outside = np.ones(bits.size, dtype=bool)
    outside[idx.reshape(-1)] = False
    moved = np.flatnonzero(outside & (bits != (SENT16 if c.bf else SENT_BITS)))
    if moved.size:
        bad.append(("sentinel", int(moved.size), int(moved[0])))
    got = to_values(c, bits[idx])
    if np.isnan(got).any():
        bad.append(("nan", int(np.isnan(got).sum()), None))
    dist, t = case_distance(c, got), tol(c)
    for z in np.flatnonzero(~(dist <= t).reshape(-1)):
        bad.append(("slab %d" % z, float(dist[z, 0, 0]), float(t[z, 0, 0])))
    return bad


# ------------------------------------------------------------------ wrong twins
def twins(c):
    """(name, values [S, m, n], smallest removed term / scale or None) of every wrong twin that
    applies to the case: each differs from the reference at one edge."""
    A, B, A2, B2, bias, H = _f64_operands(c)
    mr, K, N = c.m - c.ones, c.k, c.n
    ranges = k_ranges(c)
    key = _ref_key(c)
    ev = lambda *a, ranges=ranges, ones_ranges=None: evaluate(key, *a, ranges=ranges, ones_ranges=ones_ranges)[0]  # noqa: E731
    _, S = evaluate(key._replace(epi="slab" if c.kind == "tn" else "store"), A, B, A2, B2, bias, H, ranges=ranges)

    def removed(term, z=slice(None)):
        sc = np.broadcast_to(S[z], np.broadcast(term, S[z]).shape)
        t = np.broadcast_to(np.abs(term), sc.shape)
        m = t > 0
        return float((t[m] / sc[m]).min()) if m.any() else None

    def zeroed(a, rows=None, cols=None):
        a = a.copy()
        if rows is not None:
            a[rows] = 0
        if cols is not None:
            a[:, cols] = 0
        return a

    base = ev(A, B, A2, B2, bias, H)
    if K >= 1:
        term = A[:, K - 1, None] * B[None, K - 1, :]
        if c.ones:
            term = np.vstack([term, B[None, K - 1, :]])
        yield ("last k dropped", ev(zeroed(A, cols=K - 1), zeroed(B, rows=K - 1), zeroed(A2, cols=K - 1), B2, bias, H),
               removed(term[None], slice(len(ranges) - 1, None)))
        if mr >= 1 and (mr > 1 or not c.ones):
            yield "last row of A dropped", ev(zeroed(A, rows=mr - 1), B, zeroed(A2, rows=mr - 1), B2, bias, H), None
        yield "last column of B dropped", ev(A, zeroed(B, cols=N - 1), A2, zeroed(B2, cols=N - 1), bias, H), None
    if c.dual and K >= 1:
        k0 = (-(-K // 32) - 1) * 32
        term = A2[:, K - 1, None] * B2[None, K - 1, :]
        yield ("second product missing on the last K stage", ev(A, B, zeroed(A2, cols=slice(k0, K)), B2, bias, H),
               removed(term[None]))
    if c.bias and N >= 2:
        yield "bias shifted by one column", ev(A, B, A2, B2, np.roll(bias, 1), H), None
    d = dims(c)
    if c.epi == "dtanh" and d.ldh != d.ldc and c.m >= 2 and K >= 1:
        flat = np.nan_to_num(from_bits16(layout(c).H).astype(np.float64))[GUARD * d.ldh:]  # the padding read as 0
        Hw = flat[np.arange(c.m)[:, None] * d.ldc + np.arange(N)[None, :]]
        yield "H indexed with ldc", ev(A, B, A2, B2, bias, Hw), None
    if c.kind == "tn" and len(ranges) >= 2:
        if c.ones:
            term = np.vstack([np.zeros((mr, N)), B[None, ranges[0][1], :]])
            yield ("ones-row one k past its slab", ev(A, B, A2, B2, bias, H, ones_ranges=[(s, min(K, e + 1)) for s, e in ranges]),
                   removed(term[None], slice(0, 1)))
        s1 = ranges[1][0]
        term = A[:, s1 - 1, None] * B[None, s1 - 1, :]
        if c.ones:
            term = np.vstack([term, B[None, s1 - 1, :]])
        wide = [(max(0, s - 1), e) for s, e in ranges]
        yield ("a k counted in two adjacent slabs", ev(A, B, A2, B2, bias, H, ranges=wide, ones_ranges=wide),
               removed(term[None], slice(1, 2)))
    if c.kind == "tn" and c.ones and N > 16 and K >= 1:
        v = base.copy()  # the two-output lane form: column j's sum stored at j + 16
        v[:, mr, 16:] = base[:, mr, :-16]
        yield "ones-row column j written at j + 16", v, None
    v = base.copy()
    v[-1, c.m - 1, N - 1] = np.nan
    yield "a NaN in the last valid row", v, None
