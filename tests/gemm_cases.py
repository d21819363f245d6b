"""Cases, float64 references, per-entry scales and bounds of ``mrl_gemm`` (csrc/gemm.hip), the
tiled GEMM under every layered net: tests/test_gemm_host.py on the CPU, tests/test_gpu_gemm.py
on the device.  Nothing here reads a device result.

Dispatch.  ``slab_chunk``, ``slab_splits``, ``tile_n``, ``grid``, ``remapped``, ``vec_a`` /
``vec_b`` and ``blocks`` restate the host code and the kernel's per-block predicates, so the
host test can prove that the case list reaches every branch (``branches``).

Operands.  op(A) [M, K] and op(B) [K, N] are float32 with mantissas in +-[0.5, 1): row i of
op(A) carries 2^e_i, column j of op(B) 2^f_j, e and f integers of [-8, 8]; bias_j has the scale
2^f_j of its column and H lies in (-1, 1).  No term of an entry is small against the others, so
one missing term moves the entry by at least 0.25 / (terms + 2^8) of its scale.  Row 1 of op(A)
is zero where M >= 3: without a bias those entries have scale 0 and must be exact.  ``layout``
places the operands in flat buffers: every leading dimension tight, + 3, or the next multiple of
4 plus 4 (which keeps the 16-byte loads); padding columns, two guard rows past the last valid row
and the float in front of a base shifted by 4 bytes are NaN; C, the slabs and the gaps between
them hold SENT_BITS, compared afterwards as integers.

Reference and scale (``reference``), float64.  pre_ij = sum_k a_ik b_kj over one or two
products (+ bias_j), S_ij = sum_k |a_ik| |b_kj| (+ |bias_j|); for bf16 compute the operands are
rounded to bf16 first (bfr), since that rounding is the mode's contract and not an error of the
kernel.  A float32 evaluation in any order is off by at most terms * u * S, u = 2^-24.  Through
the epilogues:
  STORE, SLAB  scale = S (a slab: S over that slab's k range; the ones-row: sum_k |b_kj|).
  TANH   t = tanh(pre): the error of pre passes through tanh' = 1 - t^2, and tanh_fast adds its
         own: below |x| = 0.125 a polynomial of relative error < 2e-7, else 1 - 2 / (e^2|x| + 1)
         of absolute error < 2e-7 (both asserted in test_mlp_widths_host.py), each with the
         output rounding under 4 u.  scale = S (1 - t^2) + 4 |t| where |pre| < 0.12, + 4 else
         (a pre within 0.005 of the threshold needs S so large that the first term covers it).
  DTANH  out = pre * d, d = 1 - h^2 as one fma: |d's error| <= u / 2, the product rounds once,
         so |error| <= terms u S |d| + 1.5 u |pre|.  scale = S |d| + |pre|.
With these the error of a correct kernel is at most (terms + 2) u in scale units, terms =
K (or the slab's k count) per product + 1 for a bias: ``apriori``.

Bound.  ``restatement`` evaluates a case in numpy float32, one accumulation per k in ascending
order (no BLAS: a blocked sum errs less than a chain): the f32 form, the split form (three
bf16 parts per operand, the six part products i + j <= 2 per 16-deep step, smallest first) and
the bf16 form (rounded operands).  FLOOR[(mode, epilogue)] is its largest distance from the
reference in scale units over CASES, and TOL = 4 x FLOOR: another summation order, FMA
contraction, the device's exp and rcp (the margin of tests/test_gpu_mlp_widths.py).  Below
about 13 terms the a-priori bound is the smaller of the two, so ``tol`` is min(TOL, apriori):
never above what the error analysis allows for the case (a slab: for its own k count)."""
import functools
import itertools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from tests.mlp_width_cases import round_up2, tanh_fast_f32  # noqa: F401  (round_up2: how FLOOR is rounded)
from tests.test_gpu_bf16 import bfr

U = 2.0 ** -24
GBM, GBN, GBK = 128, 128, 32
GUARD = 2                        # NaN / sentinel rows past the last valid row
SENT_BITS = np.uint32(0xC9A5A5A5)  # about -1.36e6: neither a NaN nor near any result
SLAB_GAP = 7
MODES = ("f32", "split", "bf16")
EPIS = ("store", "tanh", "dtanh")
ORIENTS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (a_trans, b_trans): NN, NT, TN, TT
PADS = ("tight", "pad3", "padv")

Case = namedtuple("Case", "m n k at bt mode epi dual bias ones splits pad shift")


def case_id(c):
    return "%dx%dx%d-%s%s-%s-%s-%s%s%s%s-%s%s" % (
        c.m, c.n, c.k, "NT"[c.at], "NT"[c.bt], c.mode, c.epi, "dual" if c.dual else "single",
        "-bias" if c.bias else "", "-ones" if c.ones else "", "-s%d" % c.splits if c.epi == "slab" else "", c.pad,
        "-shift" + c.shift if c.shift else "")


# ------------------------------------------------------------------ the host dispatch, restated
def slab_chunk(K, splits):
    splits = max(1, splits)
    chunk = (-(-K // splits) + GBK - 1) // GBK * GBK
    return max(chunk, GBK)


def slab_splits(K, req):
    """mrl_gemm_slab_splits: the slabs a request for ``req`` splits gives."""
    if K <= 0:
        return 1
    return -(-K // slab_chunk(K, req))


def n_slabs(c):
    return slab_splits(c.k, c.splits) if c.epi == "slab" else 1


def k_ranges(c):
    """[(kbeg, kend)] per blockIdx.z."""
    if c.epi != "slab":
        return [(0, c.k)]
    ch = slab_chunk(c.k, c.splits)
    return [(z * ch, min(c.k, (z + 1) * ch)) for z in range(n_slabs(c))]


def tile_n(c):
    """gemm_tile_n: n <= 32, or fewer than 160 wide blocks, gives the narrow tile."""
    wide_blocks = -(-c.n // GBN) * -(-c.m // GBM) * n_slabs(c)
    return 32 if (c.n <= 32 or wide_blocks < 160) else 128


def grid(c):
    return (-(-c.n // tile_n(c)), -(-c.m // GBM), n_slabs(c))


def remapped(c):
    gx, gy, _ = grid(c)
    return (gx * gy) % 8 == 0


def _ld(ext, pad):
    return {"tight": ext, "pad3": ext + 3, "padv": (ext + 3) // 4 * 4 + 4}[pad]


def dims(c):
    """Rows, extents and leading dimensions of the stored operands, and the float offsets of
    the bases: ldh differs from ldc in the padded forms."""
    mr = c.m - c.ones
    d = SimpleNamespace(mr=mr)
    d.a_rows, d.a_ext = (c.k, mr) if c.at else (mr, c.k)
    d.b_rows, d.b_ext = (c.n, c.k) if c.bt else (c.k, c.n)
    d.lda, d.ldb = _ld(d.a_ext, c.pad), _ld(d.b_ext, c.pad)
    d.ldc = c.n if c.pad == "tight" else c.n + 3
    d.ldh = c.n if c.pad == "tight" else c.n + 5
    d.offa, d.offb = int(c.shift == "a"), int(c.shift == "b")
    d.slab_stride = c.m * d.ldc + SLAB_GAP if c.epi == "slab" else 0
    d.c_size = n_slabs(c) * d.slab_stride + GUARD * d.ldc if c.epi == "slab" else (c.m + GUARD) * d.ldc
    return d


def vec_a(c):
    """va of the kernel: 16-byte loads along k of A; the buffers are 256-byte aligned, so the
    base is aligned unless shifted."""
    d = dims(c)
    return (not c.at) and d.lda % 4 == 0 and d.offa % 4 == 0


def vec_b(c):
    d = dims(c)
    return bool(c.bt) and d.ldb % 4 == 0 and d.offb % 4 == 0


def blocks(c):
    """(interior, full_out, rows, cols) of every (tm, tn) of the grid: the kernel's
    predicates, and how many rows / columns of the tile are in range."""
    bn, mr = tile_n(c), c.m - c.ones
    gx, gy, _ = grid(c)
    out = []
    for tm in range(gy):
        for tn in range(gx):
            m0, n0 = tm * GBM, tn * bn
            out.append((m0 + GBM <= mr and n0 + bn <= c.n, m0 + GBM <= c.m and n0 + bn <= c.n,
                        min(GBM, c.m - m0), min(bn, c.n - n0)))
    return out


def branches(c):
    """The facts of a case the host test counts: tile width, block kinds, remap, load paths,
    K tails, slab situations."""
    b = {"tile%d" % tile_n(c), "remap" if remapped(c) else "noremap", "dual" if c.dual else "single",
         "bias" if c.bias else "nobias"}
    bl = blocks(c)
    ragged = any(not f for _, f, _, _ in bl)
    b.add("ragged" if ragged else "even")
    if remapped(c) and ragged:
        b.add("remap+ragged")
    if not remapped(c) and ragged:
        b.add("noremap+ragged")
    tails = {(e - s) % GBK for s, e in k_ranges(c)}
    full_tiles = any(e - s >= GBK for s, e in k_ranges(c))
    for inter, full, rows, cols in bl:
        b.add("interior" if inter else "edge")
        b.add("full_out" if full else "checked_out")
        if rows < GBM:
            b.add("m_edge%d" % rows)
        if cols < tile_n(c):
            b.add("n_edge%d" % cols)
        if inter and full_tiles:  # the FULL staging path runs
            b.add("full_load")
            if not c.at:
                b.add("full_a_vector" if vec_a(c) else "full_a_scalar")
            if c.bt:
                b.add("full_b_vector" if vec_b(c) else "full_b_scalar")
            b.update("full_then_ktail%d" % t for t in tails if t)
    b.update("ktail%d" % t for t in tails)
    d = dims(c)
    if not c.at:
        b.add("va" if vec_a(c) else "va_off_by_ld" if d.lda % 4 else "va_off_by_alignment")
    if c.bt:
        b.add("vb" if vec_b(c) else "vb_off_by_ld" if d.ldb % 4 else "vb_off_by_alignment")
    if c.epi == "slab":
        S = n_slabs(c)
        b.add("slabs%d" % S)
        if S < min(c.splits, c.k):
            b.add("slab_clamped")
        if c.k % slab_chunk(c.k, c.splits) == 0:
            b.add("slab_exact")
        else:
            b.add("slab_last%d" % (c.k - (S - 1) * slab_chunk(c.k, c.splits)))
        if c.ones:
            b.add("ones_alone" if (c.m - 1) % GBM == 0 else "ones_shared")
    return b


# ------------------------------------------------------------------ the case list
def _case(m, n, k, o, mode, epi, dual=0, bias=0, ones=0, splits=0, pad="tight", shift=""):
    return Case(m, n, k, o[0], o[1], mode, epi, int(dual), int(bias), int(ones), splits, pad, shift)


def _shift_of(o):
    """The operand whose base the shifted variant moves: the one with a vector path (A when it
    is contiguous along k, else B)."""
    return "a" if not o[0] else "b"


# every M, N and K value of the narrow tile at least once; the one-entry shapes avoid TANH,
# whose single entry could saturate
COVER = [(1, 1, 1, "store"), (31, 31, 3, "tanh"), (32, 32, 4, "dtanh"), (33, 33, 5, "store"), (127, 64, 31, "tanh"),
         (128, 65, 32, "dtanh"), (129, 1, 33, "store"), (257, 65, 64, "tanh"), (33, 31, 65, "dtanh"),
         (127, 33, 100, "tanh"), (257, 64, 100, "store"), (1, 65, 33, "dtanh")]
NARROW_COVER = [_case(m, n, k, ORIENTS[i % 4], MODES[i % 3], epi, dual=i % 2, bias=(i // 2) % 2, pad=PADS[(i // 4) % 3])
                for i, (m, n, k, epi) in enumerate(COVER)]
PRODUCT_SHAPES = [(129, 33, 33, "pad3"), (128, 32, 32, "tight")]
NARROW_PRODUCT = [_case(m, n, k, o, mode, epi, dual, bias, pad=pad) for m, n, k, pad in PRODUCT_SHAPES
                  for o, mode, epi, dual, bias in itertools.product(ORIENTS, MODES, EPIS, (0, 1), (0, 1))]
# (m, n, k, pad, shifted): 160 blocks remapped, all N edges; 159 blocks, the narrow side of the
# threshold; 162 blocks with interior ones, K = 33 scalar FULL loads and a K tail of 1; 168
# blocks remapped, interior ones on the vector path at lda = 40, a 1-column edge; the same, shifted
WIDE_SHAPES = [(20353, 70, 40, "pad3", False), (20352, 70, 40, "tight", False), (6785, 300, 33, "tight", False),
               (7117, 257, 36, "padv", False), (7117, 257, 36, "padv", True)]
WIDE = [_case(m, n, k, o, mode, EPIS[(mi + si) % 3], dual=(mi + si + oi) % 2, bias=(si + (mi + oi) // 2) % 2, pad=pad,
              shift=_shift_of(o) if sh else "")
        for si, (m, n, k, pad, sh) in enumerate(WIDE_SHAPES) for oi, o in enumerate(ORIENTS) for mi, mode in enumerate(MODES)]
TN, NN = ORIENTS[2], ORIENTS[0]
SLAB_SHAPES = [(TN, 128, 130, 1287, 41), (TN, 129, 130, 1287, 41),       # + the ones-row: m = 129 and 130
               (TN, 33, 33, 100, 4), (TN, 33, 33, 40, 64), (TN, 33, 33, 96, 3), (TN, 33, 33, 5, 1),
               (NN, 33, 33, 100, 4)]
SLABS = [_case(mr + ones, n, k, o, mode, "slab", ones=ones, splits=s, pad="pad3")
         for o, mr, n, k, s in SLAB_SHAPES for ones in (0, 1) for mode in MODES]
# the wide tile without the ones-row at the row counts the ones-row cases have
SLABS += [_case(m, 130, 1287, TN, mode, "slab", splits=41, pad="pad3") for m in (130,) for mode in MODES]
CASES = NARROW_COVER + NARROW_PRODUCT + WIDE + SLABS


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=12)
def operands(mr, n, k):
    """The logical float32 operands of every case of one shape: op(A), op(B), the second pair,
    bias [n], H [mr, n].  Cases of one shape share them whatever their layout."""
    rng = np.random.default_rng([mr, n, k])

    def mant(*s):
        return rng.uniform(0.5, 1.0, s) * rng.choice([-1.0, 1.0], s)

    e, f = 2.0 ** rng.integers(-8, 9, mr), 2.0 ** rng.integers(-8, 9, n)
    o = SimpleNamespace(A=mant(mr, k) * e[:, None], B=mant(k, n) * f[None, :], A2=mant(mr, k) * e[:, None],
                        B2=mant(k, n) * f[None, :], bias=mant(n) * f, H=rng.uniform(-1.0, 1.0, (mr, n)))
    for name, a in vars(o).items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if mr >= 3 and name in ("A", "A2"):
            a[1] = 0
        a.setflags(write=False)
        setattr(o, name, a)
    return o


def case_operands(c):
    return operands(c.m - c.ones, c.n, c.k)


def _flat(rows, ext, ld, off, data):
    buf = np.full(off + (rows + GUARD) * ld, np.nan, dtype=np.float32)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :ext] = data
    return buf


def layout(c):
    """The flat host buffers a launch of the case reads (NaN outside the valid blocks), with
    ``dims``; a base is ``buffer + off`` floats.  C is c_size floats of SENT_BITS."""
    o, d = case_operands(c), dims(c)
    st = lambda a, t: a.T if t else a  # noqa: E731
    d.A = _flat(d.a_rows, d.a_ext, d.lda, d.offa, st(o.A, c.at))
    d.B = _flat(d.b_rows, d.b_ext, d.ldb, d.offb, st(o.B, c.bt))
    d.A2 = _flat(d.a_rows, d.a_ext, d.lda, d.offa, st(o.A2, c.at)) if c.dual else None
    d.B2 = _flat(d.b_rows, d.b_ext, d.ldb, d.offb, st(o.B2, c.bt)) if c.dual else None
    d.bias = np.concatenate([o.bias, np.full(GUARD, np.nan, dtype=np.float32)]) if c.bias else None
    d.H = _flat(c.m, c.n, d.ldh, 0, o.H) if c.epi == "dtanh" else None
    return d


@functools.lru_cache(maxsize=64)
def _valid_index(m, n, ldc, S, stride):
    return (np.arange(S)[:, None, None] * stride + np.arange(m)[None, :, None] * ldc + np.arange(n)[None, None, :])


def valid_index(c):
    """Flat indices [S, m, n] of the valid entries in the C buffer."""
    d = dims(c)
    return _valid_index(c.m, c.n, d.ldc, n_slabs(c), d.slab_stride)


def embed(c, values):
    """The C buffer after a launch that wrote ``values`` [S, m, n] and nothing else."""
    buf = np.full(dims(c).c_size, SENT_BITS, dtype=np.uint32).view(np.float32)
    buf[valid_index(c)] = np.asarray(values, dtype=np.float32)
    return buf


# ------------------------------------------------------------------ float64 reference and scales
def _rounded(c, a):
    return bfr(a) if c.mode == "bf16" else a.astype(np.float64)


def evaluate(c, A, B, A2, B2, bias, H, ranges=None, ones_ranges=None):
    """(value, scale) [S, m, n] in float64 of logical float64 operands (see the module
    docstring).  ``ranges`` / ``ones_ranges``: the k range of each slab, for the rows read from
    memory and for the ones-row (the wrong twins move them)."""
    ranges = ranges or k_ranges(c)
    ones_ranges = ones_ranges or ranges
    vs, ss = [], []
    for (s, e), (so, eo) in zip(ranges, ones_ranges):
        v, sc = A[:, s:e] @ B[s:e], np.abs(A[:, s:e]) @ np.abs(B[s:e])
        if c.dual:
            v, sc = v + A2[:, s:e] @ B2[s:e], sc + np.abs(A2[:, s:e]) @ np.abs(B2[s:e])
        if c.ones:
            v, sc = np.vstack([v, B[so:eo].sum(0)[None]]), np.vstack([sc, np.abs(B[so:eo]).sum(0)[None]])
        vs.append(v)
        ss.append(sc)
    v, sc = np.stack(vs), np.stack(ss)
    if c.bias:
        v, sc = v + bias, sc + np.abs(bias)
    if c.epi == "tanh":
        t = np.tanh(v)
        sc = sc * (1 - t * t) + 4.0 * np.where(np.abs(v) < 0.12, np.abs(t), 1.0)
        v = t
    elif c.epi == "dtanh":
        d = 1 - H * H
        v, sc = v * d, sc * np.abs(d) + np.abs(v)
    return v, sc


def _f64_operands(c):
    o = case_operands(c)
    return (_rounded(c, o.A), _rounded(c, o.B), _rounded(c, o.A2), _rounded(c, o.B2), o.bias.astype(np.float64),
            o.H.astype(np.float64))


def _ref_key(c):
    return c._replace(at=0, bt=0, pad="tight", shift="", mode="bf16" if c.mode == "bf16" else "f32",
                      splits=n_slabs(c) if c.epi == "slab" else 0)


@functools.lru_cache(maxsize=6)
def _reference(key):
    v, sc = evaluate(key, *_f64_operands(key))
    v.setflags(write=False)
    sc.setflags(write=False)
    return v, sc


def reference(c):
    """(value, scale) [S, m, n]: shared by the cases that differ only in orientation, layout
    and, between f32 and split compute, mode."""
    return _reference(_ref_key(c))


def terms(c):
    """Terms per entry, per slab [S, 1, 1]."""
    return np.array([(e - s) * (2 if c.dual else 1) + c.bias for s, e in k_ranges(c)], dtype=np.float64)[:, None, None]


def apriori(c):
    return (terms(c) + 2) * U


# ------------------------------------------------------------------ float32 restatements
def _parts(a):
    """The exact three-way bf16 split of float32 values (split2 of csrc/mlp_device.h)."""
    p0 = bfr(a).astype(np.float32)
    r = a - p0
    p1 = bfr(r).astype(np.float32)
    return p0, p1, bfr(r - p1).astype(np.float32)


SPLIT_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # smallest products first


def _accumulate(acc, A, B, s, e, mode):
    """acc += A[:, s:e] B[s:e] in float32, one rounded product and one rounded sum per k."""
    if mode == "split":
        pa, pb = _parts(A[:, s:e]), _parts(B[s:e])
        for k0 in range(0, e - s, 16):
            for i, j in SPLIT_ORDER:
                for k in range(k0, min(k0 + 16, e - s)):
                    acc += pa[i][:, k, None] * pb[j][None, k, :]
        return acc
    if mode == "bf16":
        A, B = bfr(A[:, s:e]).astype(np.float32), bfr(B[s:e]).astype(np.float32)
        s, e = 0, e - s
    for k in range(s, e):
        acc += A[:, k, None] * B[None, k, :]
    return acc


@functools.lru_cache(maxsize=6)
def _pre_f32(mr, n, k, dual, ones, mode, ranges):
    o = operands(mr, n, k)
    out = []
    for s, e in ranges:
        acc = np.zeros((mr + ones, n), dtype=np.float32)
        A = np.vstack([o.A, np.ones((1, k), dtype=np.float32)]) if ones else o.A
        _accumulate(acc, A, o.B, s, e, mode)
        if dual:
            _accumulate(acc, o.A2, o.B2, s, e, mode)
        out.append(acc)
    out = np.stack(out)
    out.setflags(write=False)
    return out


def restatement(c):
    """The case in numpy float32 [S, m, n]: sequential accumulation per k (f32, split or bf16
    operands), the bias, ``tanh_fast_f32``, or 1 - h * h in the shape of the kernel's fma."""
    o = case_operands(c)
    v = _pre_f32(c.m - c.ones, c.n, c.k, c.dual, c.ones, c.mode, tuple(k_ranges(c)))
    if c.bias:
        v = v + o.bias
    if c.epi == "tanh":
        with np.errstate(over="ignore"):  # the polynomial branch of a saturated entry, not taken
            v = tanh_fast_f32(v)
    elif c.epi == "dtanh":
        d = (1.0 - o.H.astype(np.float64) ** 2).astype(np.float32)  # fmaf(-h, h, 1): one rounding
        v = v * d
    return np.asarray(v, dtype=np.float32)


# ------------------------------------------------------------------ distances and bounds
def distance(got, want, scale):
    """Per slab [S, 1, 1]: the largest |got - want| / scale; inf where an entry of scale 0 is
    not exact or a value is not finite."""
    got = np.asarray(got, dtype=np.float64)
    out = np.zeros((want.shape[0], 1, 1))
    if got.shape != want.shape:
        return out + math.inf
    for z in range(want.shape[0]):
        g, w, s = got[z], want[z], scale[z]
        if not np.isfinite(g).all():
            out[z] = math.inf
            continue
        err, pos = np.abs(g - w), s > 0
        if np.any(err[~pos] != 0):
            out[z] = math.inf
        elif pos.any():
            out[z] = np.max(err[pos] / s[pos])
    return out


def measure_floors(visit=None):
    """FLOOR recomputed: the restatements against the float64 reference over CASES, in an order
    that lets the cases of one shape share their operands; ``visit(case, restatement)`` sees
    each on the way."""
    worst = {}
    for c in sorted(CASES, key=lambda c: (c.m, c.n, c.k, c.ones, c.dual, c.mode)):
        r = restatement(c)
        if visit is not None:
            visit(c, r)
        d = float(distance(r, *reference(c)).max())
        key = (c.mode, c.epi)
        worst[key] = max(worst.get(key, 0.0), d)
    return worst


# measure_floors() on the CPU, rounded up to two digits (numpy 2.2)
FLOOR = {
    ("f32", "store"): 2.7e-07, ("f32", "tanh"): 1.2e-07, ("f32", "dtanh"): 1.6e-07, ("f32", "slab"): 2.5e-07,
    # six rounded part products per k where the f32 chain has one
    ("split", "store"): 5.7e-07, ("split", "tanh"): 3.5e-07, ("split", "dtanh"): 4.4e-07, ("split", "slab"): 4.0e-07,
    # products of two 8-bit mantissas have 16 bits, and a few dozen of one entry's common scale
    # sum without rounding in float32: what is left is the bias and the epilogue, and a slab
    # (neither) is exact in any summation order
    ("bf16", "store"): 5.8e-08, ("bf16", "tanh"): 3.6e-08, ("bf16", "dtanh"): 6.9e-08, ("bf16", "slab"): 0.0,
}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}


def tol(c):
    """The case's bound in scale units, per slab [S, 1, 1]: TOL, or the a-priori bound of the
    case's term count where that is the smaller (fewer than about 13 terms)."""
    return np.minimum(TOL[(c.mode, c.epi)], apriori(c))


def within(c, buf):
    """[] or what is wrong with the flat C buffer ``buf`` after a launch of the case: a
    disturbed sentinel (padding columns, guard rows, slab gaps), a NaN among the valid
    entries, a slab whose distance from the reference exceeds ``tol``."""
    buf = np.asarray(buf, dtype=np.float32).reshape(-1)
    d, bad = dims(c), []
    if buf.size != d.c_size:
        return [("size", buf.size, d.c_size)]
    idx = valid_index(c)
    outside = np.ones(buf.size, dtype=bool)
    outside[idx.reshape(-1)] = False
    moved = np.flatnonzero(outside & (buf.view(np.uint32) != SENT_BITS))
    if moved.size:
        bad.append(("sentinel", int(moved.size), int(moved[0])))
    got = buf[idx]
    if np.isnan(got).any():
        bad.append(("nan", int(np.isnan(got).sum()), None))
    dist, t = distance(got, *reference(c)), tol(c)
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
    ev = lambda *a, **kw: evaluate(c, *a, **kw)[0]  # noqa: E731
    _, S = evaluate(c._replace(epi="slab" if c.epi == "slab" else "store"), A, B, A2, B2, bias, H)

    def removed(term, z=slice(None)):
        """the smallest |term| / S over the entries the twin changes (pre-activation scale)"""
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

    # the last k dropped (of the last slab)
    term = A[:, K - 1, None] * B[None, K - 1, :]
    if c.ones:
        term = np.vstack([term, B[None, K - 1, :]])
    yield ("last k dropped", ev(zeroed(A, cols=K - 1), zeroed(B, rows=K - 1), zeroed(A2, cols=K - 1), B2, bias, H),
           removed(term[None], slice(len(ranges) - 1, None)))
    yield "last row of op(A) dropped", ev(zeroed(A, rows=mr - 1), B, zeroed(A2, rows=mr - 1), B2, bias, H), None
    yield "last column of op(B) dropped", ev(A, zeroed(B, cols=N - 1), A2, zeroed(B2, cols=N - 1), bias, H), None
    if c.dual:
        k0 = (-(-K // GBK) - 1) * GBK
        term = A2[:, K - 1, None] * B2[None, K - 1, :]
        yield ("second product missing on the last K tile", ev(A, B, zeroed(A2, cols=slice(k0, K)), B2, bias, H),
               removed(term[None]))
    if c.bias and N >= 2:
        yield "bias shifted by one column", ev(A, B, A2, B2, np.roll(bias, 1), H), None
    d = dims(c)
    if c.epi == "dtanh" and d.ldh != d.ldc and c.m >= 2:
        flat = np.nan_to_num(layout(c).H.astype(np.float64))  # the padding it meets read as 0
        Hw = flat[np.arange(c.m)[:, None] * d.ldc + np.arange(N)[None, :]]
        yield "H indexed with ldc", ev(A, B, A2, B2, bias, Hw), None
    if c.epi == "slab" and len(ranges) >= 2:
        if c.ones:
            term = np.vstack([np.zeros((mr, N)), B[None, ranges[0][1], :]])
            yield ("ones-row one k past its slab", ev(A, B, A2, B2, bias, H, ones_ranges=[(s, min(K, e + 1)) for s, e in ranges]),
                   removed(term[None], slice(0, 1)))
        s1 = ranges[1][0]
        term = A[:, s1 - 1, None] * B[None, s1 - 1, :]
        if c.ones:
            term = np.vstack([term, B[None, s1 - 1, :]])
        yield ("a k counted in two adjacent slabs", ev(A, B, A2, B2, bias, H, ranges=[(max(0, s - 1), e) for s, e in ranges],
                                                      ones_ranges=[(max(0, s - 1), e) for s, e in ranges]),
               removed(term[None], slice(1, 2)))
