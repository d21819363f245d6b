"""Operands, float64 references, float32 restatements and wrong twins for the cases of
tests/layered_step_cases.py.

The head bound
--------------
z[e, o] = sum_k h[e, k] w[k, o] + b[o] in float32.  On every route of head_z
(csrc/rollout_layered_kernels.h) a lane accumulates its ceil(nh / 64) units with one fused
multiply-add each, starting from 0 (head_z_runs<KPL>: the KPL = nh / 64 consecutive units
KPL l .. KPL l + KPL - 1; the lane loop: the units l, l + 64, ..); the 64 lane sums then pass
the six additions of the xor butterfly (offsets 32 .. 1, wave_sumf), and the bias is added last.
No term passes more than

    chain(nh) = ceil(nh / 64) + 6 + 1

roundings, each of relative size at most u = 2**-24, so by the usual summation bound
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, for any order of a sum)

    |z - z_exact| <= gamma(chain) * (sum_k |h_k w_k| + |b|),   gamma(d) = d u / (1 - d u)

with h and w the operands as the route multiplies them: rounded to bf16 (round to nearest even)
first in the two bf16 modes.  Nothing in it is fitted: test_layered_step_host.py holds the
float32 restatement of every route inside it and every wrong twin outside it.
Observed on the device, worst |error| / bound per route and mode (test_gpu_layered_step.py
prints them): see HEAD_OBSERVED below.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import rollout_np as RO
from tests import layered_step_cases as C
from tests.gemm_bf16_cases import from_bits16, rne_bits

U = 2.0 ** -24
A = C.A_HEAD

# worst observed |z - reference| / head_bound on an MI355X, per route and operand mode, over the
# head cases (the record of a measurement: the assertion is ratio <= 1)
HEAD_OBSERVED = {  # every z word equalled the float32 restatement of its route, bit for bit
    ("runs8", "f32"): 0.027, ("runs8", "bf"): 0.022, ("runs8", "b16"): 0.022,
    ("runs4", "f32"): 0.041, ("runs4", "bf"): 0.058, ("runs4", "b16"): 0.058,
    ("strided", "f32"): 0.149, ("strided", "bf"): 0.163, ("strided", "b16"): 0.163,
}


def head_chain(nh):
    """Roundings on the longest accumulation chain: the lane's fused multiply-adds, the wave
    reduction's six additions, the bias add."""
    return -(-nh // 64) + 6 + 1


def gamma(d):
    return d * U / (1.0 - d * U)


def rne(x):
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    return from_bits16(rne_bits(x))


def trunc16(x):
    """float32 -> bf16 by dropping the low 16 bits: a wrong twin's rounding."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


# ------------------------------------------------------------------ 1. the fused head
@functools.lru_cache(maxsize=None)
def head_operands(nh, E):
    """Hidden rows uniform in (-1, 1), head kernel N(0, 1) / sqrt(nh), random bias and logstd,
    noise rows for C.HEAD_T steps: one dropped, doubled or mis-indexed unit moves z by about
    0.4 / sqrt(nh), four orders above f32 rounding of a sum of that size."""
    rng = np.random.default_rng([1, nh, E])
    o = SimpleNamespace(
        hid=rng.uniform(-1.0, 1.0, (E, nh)).astype(np.float32),
        w=(rng.standard_normal((nh, A)) / np.sqrt(nh)).astype(np.float32),
        b=(0.5 * rng.standard_normal(A)).astype(np.float32),
        logstd=(-0.5 + 0.3 * rng.standard_normal(A)).astype(np.float32),
        noise=rng.standard_normal((C.HEAD_T * E, A)))
    o.hid16 = rne_bits(o.hid)  # the rows of the bf16 mode, as bits
    for a in vars(o).values():
        a.setflags(write=False)
    return o


def head_inputs(c):
    """(h, w) as float32, as the route multiplies them."""
    o = head_operands(c.nh, c.E)
    if c.mode == "f32":
        return o.hid, o.w
    return (from_bits16(o.hid16) if c.mode == "b16" else rne(o.hid)), rne(o.w)


def head_reference(c):
    """(z [E, 17] float64, bound [E, 17])."""
    o = head_operands(c.nh, c.E)
    h, w = (x.astype(np.float64) for x in head_inputs(c))
    z = h @ w + o.b.astype(np.float64)
    return z, gamma(head_chain(c.nh)) * (np.abs(h) @ np.abs(w) + np.abs(o.b.astype(np.float64)))


def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product of two float32 is exact in float64; the sum is
    rounded to odd in float64 (TwoSum's error term tells inexact sums and their direction), which
    makes the final rounding to float32 the single rounding of the exact a b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def head_restated(c, route):
    """head_z in float32, operation by operation: the per-lane order of ``route`` ("runs8",
    "runs4" or "strided"), the xor butterfly over the 64 lanes, the bias."""
    o = head_operands(c.nh, c.E)
    h, w = head_inputs(c)
    nh, E = c.nh, c.E
    kpl = {"runs8": 8, "runs4": 4}.get(route)
    assert kpl is None or nh == 64 * kpl
    lanes = np.arange(64)
    acc = np.zeros((E, 64, A), dtype=np.float32)
    for j in range(-(-nh // 64)):
        k = kpl * lanes + j if kpl else lanes + 64 * j
        live = k < nh
        kc = np.minimum(k, nh - 1)
        nxt = fma32(h[:, kc][:, :, None], w[kc][None, :, :], acc)
        acc = np.where(live[None, :, None], nxt, acc)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off, :]
    assert acc.dtype == np.float32 and np.array_equal(acc[:, 0], acc[:, 63])
    return acc[:, 0, :] + o.b[None, :]


def head_twins(c):
    """(name, z [E, 17] float64) of the wrong heads that apply to the case."""
    o = head_operands(c.nh, c.E)
    b = o.b.astype(np.float64)
    hq, wq = (x.astype(np.float64) for x in head_inputs(c))
    z = hq @ wq + b
    out = [("last unit dropped", z - np.outer(hq[:, -1], wq[-1])),
           ("a unit counted twice", z + np.outer(hq[:, c.nh // 2], wq[c.nh // 2])),
           ("bias omitted", z - b)]
    if c.nh > 1:
        out.append(("head kernel read as [A, nh]", hq @ wq.reshape(A, c.nh).T + b))
    if c.E > 1:
        out.append(("row E - 1 used for every env", np.broadcast_to(hq[-1] @ wq + b, z.shape)))
    if c.mode != "f32":
        hraw = (from_bits16(o.hid16) if c.mode == "b16" else o.hid).astype(np.float64)
        wraw = o.w.astype(np.float64)
        out.append(("operands not rounded", hraw @ wraw + b))
        htr = from_bits16(o.hid16) if c.mode == "b16" else trunc16(o.hid)
        out.append(("truncation instead of round-to-nearest-even",
                    htr.astype(np.float64) @ trunc16(o.w).astype(np.float64) + b))
        if c.mode == "bf":  # bf16 rows arrive rounded: only the kernel's own rounding can be half done
            out.append(("only the rows rounded", hq @ wraw + b))
            out.append(("only the head kernel rounded", hraw @ wq + b))
    return out


def head_outside(c, z):
    """Whether z misses the bound of the case anywhere."""
    want, bound = head_reference(c)
    return bool(np.any(np.abs(np.asarray(z, dtype=np.float64) - want) > bound))


# ------------------------------------------------------------------ 2. mrl_rollout_obs
STATE_ID = {"empty": 0, "running": 1, "single": 2}
CONST = 0.25  # the constant column's value: every count times it, and their sums, are exact


@functools.lru_cache(maxsize=4)
def obs_operands(c):
    """raw [E, D] (the device holds its transpose), records [2, nb, RS] and filter_state [2, FS]
    of an obs case.  The half the kernel reads (t & 1; the frozen filter reads half 0) holds the
    case's state and records, the other half plausible other values (a wrong parity is a wrong
    answer, not a NaN).  Column means sit at least 1 from zero, so that a relative 1e-12 on the
    merged mean is a bound on the merge and not on a cancellation."""
    O = C.ENVS[c.env][0]
    D, E, nb = O + 1, c.E, C.n_blocks(c.E)
    RS = FS = 2 + 2 * D
    rng = np.random.default_rng([2, list(C.ENVS).index(c.env), E, c.t, STATE_ID[c.state], c.ev])
    scale = 0.5 + rng.random(D)
    shift = (1.0 + 2.0 * rng.random(D)) * rng.choice([-1.0, 1.0], D)
    raw = rng.standard_normal((E, D)) * scale + shift
    kc = C.const_column(c.env)
    raw[0, 0] = shift[0] + 1e3 * scale[0]  # clips at +5
    if E > 1:
        raw[E - 1, 0] = shift[0] - 1e3 * scale[0]  # and at -5
    if kc is not None:
        raw[:, kc] = CONST
        raw[0, kc] = CONST + 2e-8  # two denominators (1e-8) above the mean
        if E > 1:
            raw[1, kc] = CONST - 1e-6  # clips
    rd = 0 if c.ev else c.t & 1
    counts = np.minimum(C.BLOCK, E - C.BLOCK * np.arange(nb)).astype(np.float64)
    rec = np.zeros((2, nb, RS))
    for p in (0, 1):
        rec[p, :, 0] = counts
        rec[p, :, 1] = counts if (p != rd or c.t > 0) else 0.0  # no reward yet at t = 0
        rec[p, :, 2:2 + D] = shift + 0.1 * scale * rng.standard_normal((nb, D))
        rec[p, :, 2 + D:] = counts[:, None] * scale ** 2 * (0.5 + rng.random((nb, D)))
    zb = C.zero_block(E)
    if zb is not None:
        rec[rd, zb, :2] = 0.0
        rec[rd, zb, 2:] = 1e6  # what a block of no rows may hold: never merged
    if kc is not None:
        rec[rd, :, 2 + kc] = CONST
        rec[rd, :, 2 + D + kc] = 0.0
    fs = np.zeros((2, FS))
    fs[1 - rd, :2] = 7.0, 5.0
    fs[1 - rd, 2:2 + D] = -shift
    fs[1 - rd, 2 + D:] = 6.0 * scale ** 2
    if c.state != "empty":
        n0 = 1000.0 if c.state == "running" else 1.0
        fs[rd, :2] = n0, n0 - (100.0 if c.state == "running" else 0.0)
        fs[rd, 2:2 + D] = shift + 0.05 * scale * rng.standard_normal(D)
        fs[rd, 2 + D:] = (n0 - 1.0) * scale ** 2 * (0.8 + 0.4 * rng.random(D))
        if kc is not None:
            fs[rd, 2 + kc], fs[rd, 2 + D + kc] = CONST, 0.0
    o = SimpleNamespace(raw=raw, rec=rec, fs=fs, O=O, D=D, nb=nb, RS=RS, FS=FS, rd=rd)
    for a in (raw, rec, fs):
        a.setflags(write=False)
    return o


def _recs(rec_half, D):
    """A records half as oracle.rollout_np's (n, mean, M2, reward count) tuples."""
    return [(float(r[0]), r[2:2 + D], r[2 + D:2 + 2 * D], float(r[1])) for r in rec_half]


def merge_reference(c, o):
    """The filter state the obs kernel writes: oracle.rollout_np's _batch and _merge over the
    records of the half it reads, as test_filter_matches_oracle uses them."""
    D, O = o.D, o.O
    recs = _recs(o.rec[o.rd], D)
    f0 = o.fs[o.rd]
    bn, bm, bs = RO._batch(recs, lambda v: v, lambda r: r[0])
    bnr, bmr, bsr = RO._batch(recs, lambda v: v[O], lambda r: r[3])
    n, M, S = RO._merge(f0[0], f0[2:2 + O], f0[2 + D:2 + D + O], bn, bm[:O], bs[:O])
    nr, Mr, Sr = RO._merge(f0[1], f0[2 + O], f0[2 + D + O], bnr, bmr, bsr)
    return np.concatenate([[n, nr], M, [Mr], S, [Sr]])


def obs_reference(c, o=None):
    """(filter state written, or None for the frozen filter; obs rows [E, O] float64)."""
    o = o or obs_operands(c)
    D, O = o.D, o.O
    if c.ev:
        fs, n = None, o.fs[0, 0]
        mean, den = np.zeros(O), np.ones(O)
        if n >= 2:
            mean, den = o.fs[0, 2:2 + O], np.sqrt(o.fs[0, 2 + D:2 + D + O] / (n - 1.0)) + 1e-8
    else:
        fs = merge_reference(c, o)
        n, mean = fs[0], fs[2:2 + O]
        var = fs[2 + D:2 + D + O] / (n - 1.0) if n > 1 else mean ** 2
        den = np.sqrt(var) + 1e-8
    x = o.raw[:, :O]
    if c.filt:
        x = np.clip((x - mean) / den, -5.0, 5.0)
    return fs, x


MERGE_TWINS = ("last partial chunk skipped", "zero-count block merged", "obs count for the reward column",
               "wrong parity")


def merge_twin_applies(c, twin):
    nb = C.n_blocks(c.E)
    return {"last partial chunk skipped": nb > C.LREC and nb % C.LREC != 0,
            "zero-count block merged": C.zero_block(c.E) is not None,
            "obs count for the reward column": c.t == 0,
            "wrong parity": True}[twin] and not c.ev


def merge_restated(c, o=None, twin=None):
    """merge_records_column for all D columns at once, in the device's order: the block records
    in chunks of LREC, the sums sequential in block order within and across chunks, two passes,
    then the Chan merge into the state.  ``twin``: one of MERGE_TWINS, the same with one mistake."""
    o = o or obs_operands(c)
    D, nb = o.D, o.nb
    rd = 1 - o.rd if twin == "wrong parity" else o.rd
    rec, f0 = o.rec[rd], o.fs[rd]
    cnt = np.repeat(rec[:, :1], D, axis=1)
    cnt[:, D - 1] = rec[:, 0] if twin == "obs count for the reward column" else rec[:, 1]
    rm, rs = rec[:, 2:2 + D], rec[:, 2 + D:]
    chunks = [range(b0, min(b0 + C.LREC, nb)) for b0 in range(0, nb, C.LREC)]
    if twin == "last partial chunk skipped":
        chunks = chunks[:-1]
    bn, sm, bs = np.zeros(D), np.zeros(D), np.zeros(D)
    for ch in chunks:
        for q in ch:
            bn = bn + cnt[q]
            sm = sm + cnt[q] * rm[q]
    live = bn > 0
    bm = np.where(live, sm / np.where(live, bn, 1.0), 0.0)
    for ch in chunks:
        for q in ch:
            dm = rm[q] - bm
            on = live if twin == "zero-count block merged" else live & (cnt[q] > 0)
            bs = np.where(on, bs + (rs[q] + cnt[q] * dm * dm), bs)
    n0 = np.repeat(f0[:1], D)
    n0[D - 1] = f0[1]
    M0, S0 = f0[2:2 + D], f0[2 + D:]
    nn = n0 + bn
    delta = bm - M0
    M = np.where(live, M0 + (delta * bn) / np.where(live, nn, 1.0), M0)
    S = np.where(live, S0 + bs + delta * (bm - M) * bn, S0)
    n = np.where(live, nn, n0)
    return np.concatenate([[n[0], n[D - 1]], M, S])


def state_close(got, want):
    """test_filter_matches_oracle's bound on the running stat."""
    return bool(np.allclose(got, want, rtol=1e-12, atol=0.0))


# ------------------------------------------------------------------ 3. the records
def block_records(raw, with_rew):
    """The records half the partials kernel writes for the rows raw [E, D]:
    oracle.rollout_np._block_partials at the device's block of 64 rows."""
    old, RO.BLOCK = RO.BLOCK, C.BLOCK
    try:
        parts = RO._block_partials(raw)
    finally:
        RO.BLOCK = old
    D = raw.shape[1]
    out = np.zeros((len(parts), 2 + 2 * D))
    for r, (n, mean, m2) in zip(out, parts):
        r[0], r[1] = n, n if with_rew else 0.0
        r[2:2 + D], r[2 + D:] = mean, m2
    return out


# ------------------------------------------------------------------ 4. the categorical sample
def categorical_action(p, u):
    """The kernel's rule on a stored prob row: the first index whose float32 running sum exceeds
    u, 0 when none does (the reference's argmax of an all-false mask)."""
    cs = np.cumsum(p.astype(np.float32), axis=1, dtype=np.float32).astype(np.float64)
    return np.argmax(cs > np.asarray(u)[:, None], axis=1).astype(np.int32)


def edge_uniforms(p):
    """u [E] that sit on the rule's edges for the prob rows p: one float64 ulp below and above a
    running sum (cycling over the sums), 0, and 1 - 2**-53."""
    cs = np.cumsum(p.astype(np.float32), axis=1, dtype=np.float32).astype(np.float64)
    E, A_ = cs.shape
    u = np.zeros(E)
    for e in range(E):
        kind, q = e % 4, (e // 4) % A_
        u[e] = (np.nextafter(cs[e, q], -np.inf), np.nextafter(cs[e, q], np.inf), 0.0, 1.0 - 2.0 ** -53)[kind]
    return u
