"""Cases, references and bounds shared by tests/test_scan_host.py and tests/test_gpu_scan.py
(test helper, not collected; numpy only): the blocked time-major scans of csrc/gae.hip
(`mrl_gae`: gae_scan_kernel and the exact-fit gae_full_kernel) and csrc/episode_stats.hip
(`mrl_episode_stats`).

Both kernels give thread (c, e) chunk c (L consecutive rows) of env e, 32 chunks to a
segment and 16 envs to a block; L = chunk_len(T, 32, 32) of csrc/vector_host.h.  The shape
list names the smallest (T, E) that reach every L of each kernel, one, two and three
segments, and the three block geometries; the flag layouts put episode ends on the rows
where the chunk maps, `vnext` and the segment carry meet, one layout per env column.

Every bound here is derived from the arithmetic the kernels promise (fp64 recurrences,
one float32 rounding of each output), never from what the device returns.
"""
import functools
import math

import numpy as np

from oracle import trpo_np as T
from tests import vector_ops_np as V

NC = 32        # chunks per segment (GAE_NC, EPS_NC)
EB = 16        # envs per block (GAE_EB, EPS_EB)
LMAX = 32      # longest chunk
LS = (1, 2, 4, 8, 16, 32)
GUARD = 4096   # bytes of sentinel either side of every device output


# ------------------------------------------------------------------ geometry
def chunk_len(Tn, nc=NC, lmax=LMAX):
    """csrc/vector_host.h chunk_len: the smallest power of two with nc * L >= T, at most lmax."""
    L = 1
    while L < lmax and nc * L < Tn:
        L <<= 1
    return L


def segment_len(Tn):
    return NC * chunk_len(Tn)


def n_segments(Tn):
    S = segment_len(Tn)
    return (Tn + S - 1) // S


def n_blocks(E):
    return (E + EB - 1) // EB


def exact_fit(Tn, E):
    """mrl_gae takes gae_full_kernel (unless MRL_GAE_GENERAL=1)."""
    return Tn == NC * chunk_len(Tn) and E % EB == 0 and Tn * E * 4 < 2 ** 31


def xcd_permuted(E):
    """xcd_segment (csrc/mrl_common.h) is not the identity."""
    return n_blocks(E) % 8 == 0


def geometry(E):
    if not xcd_permuted(E):
        return "plain"
    return "permuted_partial" if E % EB else "permuted_full"


GEOMETRIES = ("plain", "permuted_partial", "permuted_full")


def gae_kernel(Tn, E):
    return "full" if exact_fit(Tn, E) else "general"


def gae_workspace_bytes(E):
    if E <= 0:
        return 128
    return (n_blocks(E) * 16 + 63) // 64 * 64 + 64


def episode_stats_workspace_bytes(E):
    return n_blocks(E) * 64


# ------------------------------------------------------------------ shapes
TS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2049)
ES = (1, 15, 16, 17, 125, 128, 144)

# L:   1: T <= 32   2: 33..64   4: 65..128   8: 129..256   16: 257..512   32: 513 and up
SHAPES = (
    (1, 1), (31, 15), (32, 16), (32, 17),
    (33, 125), (63, 1), (64, 128), (64, 15),
    (65, 17), (127, 125), (128, 144), (128, 125),
    (129, 16), (200, 125), (255, 17), (256, 16), (256, 15),
    (257, 144), (511, 125), (512, 128), (512, 17),
    (513, 16), (1023, 125), (1024, 144), (1024, 1),
    (1025, 125), (1025, 128), (2047, 17), (2049, 144), (2049, 125), (2049, 15),
)
# every shape the exact-fit kernel takes: T = 32 L for the six L, E a multiple of 16 in each geometry
EXACT_FIT_SHAPES = tuple((NC * L, E) for L in LS for E in (16, 128, 144))
# one ragged shape per L (T and E both off the tile; the last block partial) and one exact fit
SENTINEL_SHAPES = ((31, 15), (63, 17), (127, 125), (200, 125), (511, 17), (1025, 125), (2049, 15), (128, 144))

PARAMS = ((0.995, 0.97), (0.99, 0.0), (1.0, 1.0))


def shape_id(s):
    return f"{s[0]}x{s[1]}"


# ------------------------------------------------------------------ flag layouts
TRUNC, TERM = 1, 3  # flags of an episode end: bit 0 = end, bit 1 = terminated


def _ends(Tn, rows, kind):
    f = np.zeros(Tn, dtype=np.uint8)
    f[np.asarray(rows, dtype=np.int64)] = kind
    f[Tn - 1] = kind
    return f


def _lay_none(Tn, L, S, rng, kind):
    return _ends(Tn, [], kind)


def _lay_every(Tn, L, S, rng, kind):
    f = np.where(np.arange(Tn) % 2 == 0, kind, TRUNC + TERM - kind).astype(np.uint8)
    return f


def _lay_chunk_last(Tn, L, S, rng, kind):
    t = np.arange(Tn)
    return _ends(Tn, t[t % L == L - 1], kind)


def _lay_chunk_first(Tn, L, S, rng, kind):
    t = np.arange(Tn)
    return _ends(Tn, t[t % L == 0], kind)


def _lay_seg_edges(Tn, L, S, rng, kind):
    t = np.arange(Tn)
    return _ends(Tn, t[(t % S == S - 1) | ((t % S == 0) & (t > 0))], kind)


def _lay_single(Tn, L, S, rng, kind):
    return _ends(Tn, [Tn - 2] if Tn >= 2 else [], kind)


def _lay_random(Tn, L, S, rng, kind):
    return _ends(Tn, np.nonzero(rng.random(Tn) < 0.08)[0], kind)


def _lay_random_mixed(Tn, L, S, rng, kind):
    f = _lay_random(Tn, L, S, rng, TRUNC)
    f[(f != 0) & (rng.random(Tn) < 0.5)] = TERM
    return f


def _lay_bit1_mid(Tn, L, S, rng, kind):
    """bit 1 without bit 0 on every row that is no end: both kernels ignore it"""
    f = _lay_random_mixed(Tn, L, S, rng, kind)
    f[f == 0] = 2
    return f


def _lay_open_final(Tn, L, S, rng, kind):
    """the final row unflagged: a truncation for mrl_gae, an open run mrl_episode_stats drops"""
    f = _lay_random_mixed(Tn, L, S, rng, kind)
    f[Tn - 1] = 0
    return f


_BASE = (("none", _lay_none), ("every", _lay_every), ("chunk_last", _lay_chunk_last),
         ("chunk_first", _lay_chunk_first), ("seg_edges", _lay_seg_edges), ("single", _lay_single),
         ("random", _lay_random))
# (name, builder, flags of its ends).  17 layouts: coprime to the 16 envs of a block, so over
# the blocks of a launch a layout visits every env slot
LAYOUTS = tuple((f"{n}_{'trunc' if k == TRUNC else 'term'}", fn, k) for n, fn in _BASE for k in (TRUNC, TERM)) + (
    ("random_mixed", _lay_random_mixed, TRUNC), ("bit1_mid", _lay_bit1_mid, TRUNC),
    ("open_final", _lay_open_final, TRUNC))
LAYOUT_NAMES = tuple(n for n, _, _ in LAYOUTS)


def layout_of(Tn, E, e):
    """Index into LAYOUTS of env column e: cycling, from an offset that differs between shapes
    (so the one- and fifteen-column shapes do not all start at the same layout)."""
    return (e + Tn + 3 * E) % len(LAYOUTS)


def make_flags(Tn, E):
    L, S = chunk_len(Tn), segment_len(Tn)
    rng = np.random.default_rng(7919 * Tn + E)
    flags = np.zeros((Tn, E), dtype=np.uint8)
    for e in range(E):
        _, fn, kind = LAYOUTS[layout_of(Tn, E, e)]
        flags[:, e] = fn(Tn, L, S, rng, kind)
    return flags


def closed(flags):
    """The flags the GAE reference sees: bit 0 set on the final row (the mrl_gae contract of
    include/mrl_hip.h: the final row always ends its episode, a truncation unless bit 1 says
    terminated)."""
    f = flags.copy()
    f[-1] |= 1
    return f


# ------------------------------------------------------------------ values
FAMILIES = ("generic", "offset", "exact")


def make_values(Tn, E, family):
    """(rew, v) float32 [T, E].  generic: unit normals; offset: the same with +1000 on every
    reward (returns reach ~1e5 .. 1e6, advantages cancel against them); exact: integers in
    [-8, 8] (with gamma = lam = 1 every fp64 operation of either kernel and of the reference
    is then exact, and so is the float32 cast of every output: test_scan_host checks the
    magnitudes)."""
    rng = np.random.default_rng(104729 * Tn + 31 * E + FAMILIES.index(family))
    if family == "exact":
        return (rng.integers(-8, 9, (Tn, E)).astype(np.float32), rng.integers(-8, 9, (Tn, E)).astype(np.float32))
    rew = rng.standard_normal((Tn, E)).astype(np.float32)
    v = rng.standard_normal((Tn, E)).astype(np.float32)
    if family == "offset":
        rew = (rew + np.float32(1000.0)).astype(np.float32)
    return rew, v


# ------------------------------------------------------------------ GAE reference and bound
def gae_ref(rew, v, flags, gamma, lam):
    """oracle.trpo_np.gae_batched on the float64 casts of the float32 inputs; (adv, ret) float64."""
    f = closed(flags)
    return T.gae_batched(rew.astype(np.float64), v.astype(np.float64), (f & 1) > 0, (f & 2) > 0, gamma, lam)


def gae_magnitudes(rew, v, flags, gamma, lam):
    """The GAE recursion on |delta| and |rew| with the same continuation mask: M_adv[t, e],
    M_ret[t, e] bound every partial sum an evaluation of adv[t, e] / ret[t, e] can form, in
    any association of the affine chunk maps."""
    f = closed(flags)
    last, term = (f & 1) > 0, (f & 2) > 0
    r, b = rew.astype(np.float64), v.astype(np.float64)
    Tn, E = r.shape
    m_adv, m_ret = np.zeros((Tn, E)), np.zeros((Tn, E))
    a_next, r_next, v_next = np.zeros(E), np.zeros(E), np.zeros(E)
    for t in reversed(range(Tn)):
        cont = ~last[t]
        boot = np.where(cont, v_next, np.where(term[t], 0.0, b[t]))
        delta = np.abs(r[t] + gamma * boot - b[t])
        a_next = delta + gamma * lam * np.where(cont, a_next, 0.0)
        r_next = np.abs(r[t]) + gamma * np.where(cont, r_next, 0.0)
        m_adv[t], m_ret[t] = a_next, r_next
        v_next = b[t]
    return m_adv, m_ret


def gae_bound(ref, mag, nseg):
    """Allowed |device - ref| per element: 2^-24 |ref| + (128 + 2 nseg) 2^-53 M.
    First term: the one float32 rounding of the exact value (half a float32 ulp is at most
    2^-24 of the value).  Second: fp64 reassociation slack -- an output composes at most 32
    in-chunk steps, 5 scan levels and one carry per segment, two roundings each (a product
    and a sum): 2 (32 + 5 + nseg) = 74 + 2 nseg roundings, each at most 2^-53 of a partial
    sum that M bounds; 74 is rounded up to 128 for the roundings inside delta and the
    reference's own."""
    return V.U32 * np.abs(ref) + (128 + 2 * nseg) * V.U64 * mag


def gae_per_path(rew, v, flags, gamma, lam):
    """The reference algorithm's own form (oracle.trpo_np.compute_advantage before its
    standardisation): each column split into paths at its flags & 1 rows, per path
    `discount` of the rewards and of the deltas built with the b1 bootstrap."""
    f = closed(flags)
    r, b = rew.astype(np.float64), v.astype(np.float64)
    Tn, E = r.shape
    adv, ret = np.zeros((Tn, E)), np.zeros((Tn, E))
    for e in range(E):
        start = 0
        for t in np.nonzero(f[:, e] & 1)[0]:
            pr, pb = r[start:t + 1, e], b[start:t + 1, e]
            b1 = np.append(pb, 0 if f[t, e] & 2 else pb[-1])
            deltas = pr + gamma * b1[1:] - b1[:-1]
            ret[start:t + 1, e] = T.discount(pr, gamma)
            adv[start:t + 1, e] = T.discount(deltas, gamma * lam)
            start = t + 1
    return adv, ret


@functools.lru_cache(maxsize=16)
def gae_case(Tn, E, family, gamma, lam):
    """Inputs, reference and bounds of one launch; computed once and shared (read-only)."""
    rew, v = make_values(Tn, E, family)
    flags = make_flags(Tn, E)
    adv, ret = gae_ref(rew, v, flags, gamma, lam)
    m_adv, m_ret = gae_magnitudes(rew, v, flags, gamma, lam)
    nseg = n_segments(Tn)
    case = dict(rew=rew, v=v, flags=flags, adv=adv, ret=ret, adv_bound=gae_bound(adv, m_adv, nseg),
                ret_bound=gae_bound(ret, m_ret, nseg), m_adv=m_adv, m_ret=m_ret)
    for a in case.values():
        a.setflags(write=False)
    return case


def adv_moments_ref(adv32):
    """Exact (sum, sum of squares) of float32 rows with their bounds (vector_ops_np's
    moments_ref / moments_bounds): ((s1, s2), (b1, b2))."""
    a = np.ascontiguousarray(adv32, dtype=np.float32).reshape(-1)
    s1, s2, asum, qsum = V.moments_ref(a)
    return (s1, s2), V.moments_bounds(a.size, asum, qsum)


def worst(err, bound, Tn, E, what):
    """Message for an elementwise bound miss: the worst element's (t, e), its chunk and layout."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    t, e = np.unravel_index(int(np.argmax(ratio)), err.shape)
    L, S = chunk_len(Tn), segment_len(Tn)
    return (f"{what}: worst at (t={t}, e={e}) err {err[t, e]:.3e} bound {bound[t, e]:.3e} (x{ratio[t, e]:.3g}); "
            f"segment {t // S} chunk {(t % S) // L} step {t % L} of L={L}, block {e // EB} slot {e % EB}, "
            f"layout {LAYOUT_NAMES[layout_of(Tn, E, e)]}; {int((ratio > 1).sum())} elements over")


# ------------------------------------------------------------------ episode statistics
def episodes(rew, flags):
    """The closed episodes of a batch, per column in time order: (rewards float64, length)."""
    r = rew.astype(np.float64)
    out = []
    for e in range(r.shape[1]):
        start = 0
        for t in np.nonzero(flags[:, e] & 1)[0]:
            out.append(r[start:t + 1, e])
            start = t + 1
    return out


def episode_stats_ref(rew, flags):
    """mrl_episode_stats' six outputs from math.fsum per episode, and the bounds of the three
    inexact ones.  Returns (out[6], bound[6]); the bounds of the count, the length sum and
    the length maximum are 0.

    With R_i = fsum of episode i (len_i rows, A_i = sum |r|):
      sum R: one sum of all N rows of closed episodes in some order: sum_bound(N, sum A_i).
      max R: the device's R_i is a sum of len_i terms in its own order, sum_bound(len_i, A_i)
        =: b_i from R_i, and the maximum moves by at most the largest b_i.
      sum R^2: each device R_i^2 is off by at most 2 |R_i| b_i + b_i^2, then n_ep terms are
        squared (one rounding) and added: sum_bound(n_ep + 1, sum R_i^2); the reference's own
        three roundings (fsum of R_i, the square, the final fsum) take n_ep + 1 to n_ep + 4."""
    eps = episodes(rew, flags)
    if not eps:
        return np.array([0.0, 0.0, 0.0, -np.inf, 0.0, 0.0]), np.zeros(6)
    R = np.array([math.fsum(p) for p in eps])
    A = np.array([math.fsum(np.abs(p)) for p in eps])
    ln = np.array([len(p) for p in eps], dtype=np.float64)
    b = V.sum_bound(ln, A)
    sq = math.fsum(R * R)
    out = np.array([len(eps), math.fsum(R), sq, R.max(), ln.sum(), ln.max()])
    bound = np.array([0.0, V.sum_bound(ln.sum(), math.fsum(A)), V.sum_bound(len(eps) + 4, sq) +
                      math.fsum(2.0 * np.abs(R) * b + b * b), b.max(), 0.0, 0.0])
    return out, bound


@functools.lru_cache(maxsize=16)
def episode_case(Tn, E, family):
    rew, _ = make_values(Tn, E, family)
    flags = make_flags(Tn, E)
    out, bound = episode_stats_ref(rew, flags)
    for a in (rew, flags, out, bound):
        a.setflags(write=False)
    return dict(rew=rew, flags=flags, out=out, bound=bound)
