"""Clipped-surrogate PPO on the device: the MRL_EPI_PPOCLIP epilogue per entry point (the
exact-f32 fused rows kernel, the bf16 fused rows kernel, the layered path's head_rows_kernel),
its exact identities, the activation cache, ppo.PpoClipUpdater against its float64 twin, the
agent and resume.  Oracle, restatement and inputs: tests/ppo_clip_np.py.

Bounds (the method of tests/test_gpu_head_rows.py).  Every output is compared in units of a
per-entry scale (that file's ref_rows scales of the SURRGRAD epilogue, whose formulas these
are).  FLOOR is the largest distance, in those units, between the float64 oracle and the
numpy float32 restatement of the same entry on the inputs of this file -- for mrl_head_rows,
which is given z, the epilogue alone; for the fused f32 kernel the float32 forward too --
measured on the CPU (measure(), re-measured by tests/test_ppo_clip_host.py); the kernel is
allowed 4x the floor.  A clipped row's head gradient has scale 0: it must be exactly (+-)0.

The band.  The gradient is discontinuous in r at 1 -+ eps, so a row whose float64 ratio lies
within DELTA of a bound may be clipped by one evaluation and kept by the other: such rows are
left out of the ghead comparison only (they stay in the sums, which are continuous in r).
DELTA is 4x the largest |r_float32 - r_float64| of the same restatement; the host test caps
the band's share of the rows at 1 %.

bf16.  The reference is the oracle at the float64 emulation of the bf16 rounding points
(tests/test_gpu_ppo.py _emu_z), the bounds tests/test_gpu_bf16.py's: 5e-2 of the largest
entry for the ghead rows, 3e-2 relative + 2e-3 absolute for the mean losses.  Its restatement
(for DELTA) is the same rounding points with float32 accumulation.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import trpo_np as T
from tests import ppo_clip_np as C

pytestmark = pytest.mark.gpu

SENT = 777.25
ENTRIES = ("f32", "bf16", "head")
PPOCLIP, SURRGRAD = 8, 2
BF16_GRAD_RTOL, BF16_ORACLE_RTOL, BF16_LOSS_ATOL = 5e-2, 3e-2, 2e-3   # tests/test_gpu_ppo.py, test_gpu_bf16.py

# FLOOR[entry.head.output]: measure()["floor"], numpy 2.2, rounded up to two digits
FLOOR = {
    "head.softmax.ghead": 3.8e-7, "head.softmax.surr": 1.5e-7, "head.softmax.kl": 9.9e-8, "head.softmax.ent": 5.0e-7,
    "head.gauss.ghead": 6.0e-7, "head.gauss.surr": 2.3e-7, "head.gauss.kl": 1.1e-7, "head.gauss.ent": 4.3e-8,
    "f32.softmax.ghead": 2.3e-7, "f32.softmax.surr": 1.5e-7, "f32.softmax.kl": 2.0e-7, "f32.softmax.ent": 5.0e-7,
    "f32.gauss.ghead": 4.6e-7, "f32.gauss.surr": 3.6e-7, "f32.gauss.kl": 1.4e-7, "f32.gauss.ent": 4.3e-8,
}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}
# RATIO_ERR[entry.head]: measure()["ratio"], the largest |r_float32 - r_float64|, rounded up
RATIO_ERR = {"head.softmax": 4.6e-7, "head.gauss": 5.6e-6, "f32.softmax": 5.5e-7, "f32.gauss": 5.6e-6,
             "bf16.softmax": 5.6e-4, "bf16.gauss": 1.6e-3}
DELTA = {k: 4.0 * v for k, v in RATIO_ERR.items()}


# ------------------------------------------------------------------ references per entry (CPU)
def _bfr32(a):
    """Round float32 values to bf16 (RNE), kept as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _emu_z_f32(spec, th, ob):
    """The fused bf16 forward's rounding points (inputs, hidden weights, hidden activations)
    with float32 accumulation; the head layer an f32 one on the rounded activations."""
    Ws, bs, _ = spec.split(th.astype(np.float32))
    h = _bfr32(ob)
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = _bfr32(np.tanh(h @ _bfr32(W) + b))
    return h @ Ws[-1] + bs[-1]


@functools.lru_cache(maxsize=None)
def reference(entry, head, A, n, eps=C.EPS):
    """(case, z given to / assumed for the entry, float64 oracle rows, float32 restatement rows)."""
    from tests.test_gpu_ppo import _emu_z
    c = C.rows_case(head, A, n, C.BF16_GAP if entry == "bf16" else 0.0)
    spec, th, ob = c["spec"], c["theta"], c["ob"]
    logstd = th[-A:] if head == "gauss" else None
    if entry == "head":   # z is an input: the float32 rounding of the float64 forward
        z = T.mlp_forward(spec, th, ob)[0].astype(np.float32).astype(np.float64)
        z32 = z
    elif entry == "f32":
        z, z32 = T.mlp_forward(spec, th, ob)[0], T.mlp_forward(spec, th, ob, dtype=np.float32)[0]
    else:
        z, z32 = _emu_z(spec, th, ob, False), _emu_z_f32(spec, th, ob)
    args = (logstd, c["act"], c["adv"], c["oldprob"], eps, 1.0 / (n + 3))
    return c, z, C.clip_rows(head, z, *args), C.clip_rows_f32(head, z32, *args)


def scales(entry, c, z, ref):
    """(ghead scale [n, gh], term scales [n, 3]) of the oracle rows: ref_rows' SURRGRAD scales,
    0 for a clipped row's ghead, the surrogate term's rescaled from |r A| to the clipped term.
    The fused entries compute z themselves: its rounding reaches an entry through the whole
    row's weight w, also where the entry itself is near 0 (a Gauss mean gradient w u / sd at
    u ~ 0), so there an entry's scale is at least the row's largest."""
    from tests.test_gpu_head_rows import SURRGRAD as SG, ref_rows
    head, A, n = c["head"], c["A"], c["n"]
    d = dict(head=head, A=A, n=n, z=z, dz=np.zeros_like(z), adv=c["adv"], oldprob=c["oldprob"], act=c["act"])
    if head == "gauss":
        d["logstd"] = c["theta"][-A:]
    r = ref_rows(d, SG, inv_ng=1.0 / (n + 3))
    gsc = r["ghead"][1]
    if entry != "head":
        gsc = np.maximum(gsc, gsc.max(axis=1, keepdims=True))
    gsc = np.where(ref["clipped"][:, None], 0.0, gsc)
    tsc = r["tscale"].copy()
    ra = np.abs(ref["ratio"] * c["adv"])
    tsc[:, 0] = np.where(ra > 0, tsc[:, 0] * np.abs(ref["terms"][:, 0]) / np.where(ra > 0, ra, 1.0), 0.0)
    return gsc, tsc


def wave_of_row(entry, n, prow):
    """The partial row a row's terms are added to: head_rows_kernel runs blocks of 256 rows, a
    wave per 64; the fused kernels a 32-row tile per wave, tile t on partial row t mod prow."""
    r = np.arange(n)
    if entry == "head":
        return ((r // 256) % (prow // 4)) * 4 + (r % 256) // 64
    return (r // 32) % prow


def partial_rows_of(entry, n):
    cap = 3072 if entry == "bf16" else 1536   # ROWS_MAX_BLOCKS_B / ROWS_MAX_BLOCKS
    return 4 * min(max((n + 127) // 128, 1), cap)


def units(entry, c, z, ref, ghead, partial=None, terms=None, delta=0.0):
    """{what: distance in scale units} of ghead rows (rows within delta of a bound left out)
    and of the per-wave sums (partial, or terms summed here as partial holds them)."""
    from tests.test_gpu_head_rows import _units
    n = c["n"]
    gsc, tsc = scales(entry, c, z, ref)
    keep = C.bound_distance(ref["ratio"], C.EPS) > delta
    u = {"ghead": _units(ghead[keep], ref["ghead"][keep], gsc[keep]) if keep.any() else 0.0}
    prow = partial_rows_of(entry, n)
    wv = wave_of_row(entry, n, prow)
    for k, what in enumerate(("surr", "kl", "ent")):
        want = np.bincount(wv, weights=ref["terms"][:, k], minlength=prow)
        scale = np.bincount(wv, weights=tsc[:, k], minlength=prow)
        got = partial[:, k] if partial is not None else np.bincount(wv, weights=terms[:, k], minlength=prow)
        u[what] = _units(got, want, scale)
    return u


def measure():
    """{"floor": {entry.head.what: units}, "ratio": {entry.head: |r32 - r64|}, "band": {entry.head:
    the largest share of a case's rows (n >= 64) within 4x that of a bound}} over every case."""
    out = {"floor": {}, "ratio": {}, "band": {}}
    for entry in ENTRIES:
        for head, A, n in C.case_list():
            c, z, ref, f32 = reference(entry, head, A, n)
            key = f"{entry}.{head}"
            out["ratio"][key] = max(out["ratio"].get(key, 0.0), float(np.abs(f32["ratio"] - ref["ratio"]).max()))
    for entry in ENTRIES:
        for head, A, n in C.case_list():
            c, z, ref, f32 = reference(entry, head, A, n)
            key = f"{entry}.{head}"
            d = 4.0 * out["ratio"][key]
            if n >= 64:
                out["band"][key] = max(out["band"].get(key, 0.0), float((C.bound_distance(ref["ratio"], C.EPS) <= d).mean()))
            if entry == "bf16":
                continue
            for what, v in units(entry, c, z, ref, f32["ghead"], terms=f32["terms"], delta=d).items():
                out["floor"][f"{key}.{what}"] = max(out["floor"].get(f"{key}.{what}", 0.0), v)
    return out


# ------------------------------------------------------------------ the kernels
def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _head_id(head):
    from modular_rl_amd import _lib
    return _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX


@functools.lru_cache(maxsize=None)
def _fused_net(head, A, dtype, n_in=C.N_IN):
    from modular_rl_amd.nets import MlpNet
    return MlpNet(n_in, A, _head_id(head), dtype=dtype)


def run_entry(entry, c, z=None, epi=PPOCLIP, eps=C.EPS, skip=0, slack=3, adv=None):
    """One launch of the entry point itself (not through net.rows' routing) into
    sentinel-filled buffers with `slack` rows to spare: (ghead [n + slack, gh], partial [prow + 2, 4])."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    head, A, n = c["head"], c["A"], c["n"]
    gh = 2 * A if head == "gauss" else A
    prow = partial_rows_of(entry, n)
    ghead = torch.full(((n + slack) * gh,), SENT, dtype=torch.float32, device="cuda")
    partial = torch.full(((prow + 2) * 4,), SENT, dtype=torch.float64, device="cuda")
    act = _dev(c["act"], torch.int32 if head == "softmax" else torch.float32)
    advt, op = _dev(c["adv"] if adv is None else adv), _dev(c["oldprob"])
    skipt = torch.tensor([skip], dtype=torch.int32, device="cuda")
    x = None if entry == "head" else _dev(c["ob"])
    io = _lib.RowsIO(ptr(x), None, 1.0, n, 1.0 / (n + 3), ptr(act), ptr(advt), ptr(op), None, None, ptr(ghead),
                     ptr(partial), 0.0, float(eps), 0.0, 0, 0, None, None)
    if entry == "head":
        assert prow == int(_lib.load().mrl_partial_rows(n))
        zt = _dev(z)
        ls = _dev(c["theta"][-A:]) if head == "gauss" else None
        call("mrl_head_rows", _head_id(head), A, epi, ptr(zt), None, ptr(ls), None, ctypes.byref(io), ptr(skipt), stream())
    else:
        net = _fused_net(head, A, "bf16" if entry == "bf16" else "fp32")
        assert prow == net.partial_rows(n)
        net.set_flat(c["theta"])
        call("mrl_mlp_rows" + net._sfx, ctypes.byref(net.desc), epi, ptr(net.theta), ptr(net.image), None, None,
             ctypes.byref(io), ptr(skipt), stream())
    torch.cuda.synchronize()
    return (ghead.cpu().numpy().astype(np.float64).reshape(n + slack, gh),
            partial.cpu().numpy().astype(np.float64).reshape(prow + 2, 4))


def check_case(entry, head, A, n):
    c, z, ref, _ = reference(entry, head, A, n)
    ghead, partial = run_entry(entry, c, z)
    prow = partial_rows_of(entry, n)
    ctx = (entry, head, A, n)
    assert (ghead[n:] == SENT).all() and (partial[prow:] == SENT).all(), ctx   # nothing past the rows
    assert (partial[:prow, 3] == 0.0).all(), ctx
    key = f"{entry}.{head}"
    keep = C.bound_distance(ref["ratio"], C.EPS) > DELTA[key]
    assert (ghead[:n][ref["clipped"] & keep] == 0.0).all(), ctx          # a clipped row: exactly +-0
    if entry == "bf16":
        err = np.abs(ghead[:n][keep] - ref["ghead"][keep]).max() if keep.any() else 0.0
        rel = err / max(np.abs(ref["ghead"]).max(), 1e-30)
        got = partial[:prow, :3].sum(axis=0) / n
        want = ref["terms"].sum(axis=0) / n
        print("ppoclip", ctx, "ghead rel", rel, "mean terms", got, want)
        assert rel < BF16_GRAD_RTOL, (ctx, rel)
        np.testing.assert_allclose(got, want, rtol=BF16_ORACLE_RTOL, atol=BF16_LOSS_ATOL, err_msg=str(ctx))
        return
    u = units(entry, c, z, ref, ghead[:n], partial=partial[:prow], delta=DELTA[key])
    print("ppoclip", ctx, {k: (v, TOL[f"{key}.{k}"]) for k, v in u.items()})
    for k, v in u.items():
        assert v <= TOL[f"{key}.{k}"], (ctx, k, v, TOL[f"{key}.{k}"])
    _, tsc = scales(entry, c, z, ref)
    for k, what in enumerate(("surr", "kl", "ent")):   # the column sums: the float64 sums of the oracle rows
        assert abs(partial[:prow, k].sum() - ref["terms"][:, k].sum()) <= TOL[f"{key}.{what}"] * tsc[:, k].sum(), (ctx, what)


@pytest.mark.parametrize("head,A", C.HEAD_WIDTHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_ppoclip_rows_per_entry(entry, head, A):
    """Partial sums per wave and every ghead row against the oracle at 1, 31, 32, 33, 64, 65
    and 257 rows (a tile, its edges, two tiles, more than one block)."""
    for n in C.ROW_COUNTS:
        check_case(entry, head, A, n)


@pytest.mark.parametrize("head", ["softmax", "gauss"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_ppoclip_rows_grid_stride_second_trip(entry, head):
    """n = 1536 * 256 + 257: past one trip of head_rows_kernel's and of both fused kernels' grids."""
    check_case(entry, head, C.BIG_WIDTH[head], C.BIG_N)


# ------------------------------------------------------------------ exact identities
def identity_adv(ref, c, every_row_clips):
    """The case's advantages with their signs set from the oracle ratio: none clipped (A < 0
    where r > 1, A > 0 where r < 1: min keeps r A whatever eps is) or all clipped (the reverse)."""
    mag = np.abs(c["adv"])
    assert (mag > 0).all()
    up = ref["ratio"] > 1.0
    return np.where(up, mag, -mag) if every_row_clips else np.where(up, -mag, mag)


TINY_EPS = 1e-4   # tests/test_ppo_clip_host.py: no ratio of the identity cases within DELTA of 1 -+ 1e-4


@pytest.mark.parametrize("head,A", [("softmax", 3), ("gauss", 3)])
@pytest.mark.parametrize("entry", ["f32", "head"])
def test_ppoclip_without_clipped_rows_is_surrgrad_bit_for_bit(entry, head, A):
    """eps = 0.999 and advantages under which no row clips: ghead and partial[:, 0:3] are
    SURRGRAD's bit for bit (the mask only selects between w and 0)."""
    c, z, ref, _ = reference(entry, head, A, 257)
    adv = identity_adv(ref, c, False)
    assert not C.clip_rows(head, z, c["theta"][-A:], c["act"], adv, c["oldprob"], 0.999, 1.0)["clipped"].any()
    g1, p1 = run_entry(entry, c, z, PPOCLIP, eps=0.999, adv=adv)
    g2, p2 = run_entry(entry, c, z, SURRGRAD, eps=0.0, adv=adv)
    assert g1.astype(np.float32).tobytes() == g2.astype(np.float32).tobytes()
    assert p1[:, :3].tobytes() == p2[:, :3].tobytes() and (p1[:-2, 3] == 0).all()


@pytest.mark.parametrize("head,A", [("softmax", 3), ("gauss", 3)])
@pytest.mark.parametrize("entry", ["f32", "head"])
def test_ppoclip_with_every_row_clipped_has_zero_gradient(entry, head, A):
    """Every row clipped (eps = 1e-4, the advantage's sign set against the ratio): every ghead
    entry is +-0 and the surrogate column sums to sum clamp(r) A."""
    n = 257
    c, z, ref, _ = reference(entry, head, A, n)
    adv = identity_adv(ref, c, True)
    r = C.clip_rows(head, z, c["theta"][-A:], c["act"], adv, c["oldprob"], TINY_EPS, 1.0 / (n + 3))
    assert r["clipped"].all()
    ghead, partial = run_entry(entry, c, z, PPOCLIP, eps=TINY_EPS, adv=adv)
    assert (ghead[:n] == 0.0).all() and (ghead[n:] == SENT).all()
    lo, hi = C.clip_bounds(TINY_EPS)
    want = np.where(adv > 0, hi, lo) * adv
    prow = partial_rows_of(entry, n)
    assert abs(partial[:prow, 0].sum() - want.sum()) <= TOL[f"{entry}.{head}.surr"] * np.abs(want).sum()


@pytest.mark.parametrize("head", ["softmax", "gauss"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_ppoclip_skip_flag_leaves_every_output_untouched(entry, head):
    c, z, _, _ = reference(entry, head, 3, 65)
    ghead, partial = run_entry(entry, c, z, skip=1)
    assert (ghead == SENT).all() and (partial == SENT).all()


# ------------------------------------------------------------------ the activation cache
@pytest.mark.parametrize("dtype,n_in", [("fp32", 16), ("bf16", 11), ("fp32", 5)])
@pytest.mark.parametrize("head,A", [("gauss", 3), ("softmax", 3)])
def test_ppoclip_activation_cache_is_bitwise_transparent(head, A, dtype, n_in):
    """PPOCLIP with MRL_CACHE_WRITE and the VJP on the cache against the uncached pair: ghead
    and the partial rows bit for bit, and the gradient bit for bit where the cached VJP is the
    same kernel reading the stored activations (bf16; fp32 at n_in % 16 == 0).  At other fp32
    widths the cached VJP is the 16-row kernel, the same sums in another row order
    (tests/test_gpu_mlp.py): its gradient agrees to fp32 rounding."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import MlpNet
    N = 700
    rng = np.random.default_rng([7, n_in, A])
    spec = T.Spec(n_in, [64, 64], A, head)
    th = (T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)).astype(np.float32)
    ob = rng.standard_normal((N, n_in)).astype(np.float32)
    oldprob = T.policy_prob(spec, th.astype(np.float64) + 0.05 * rng.standard_normal(spec.P), ob.astype(np.float64))
    noise = rng.standard_normal((N, A)) if head == "gauss" else rng.random(N)
    act = T.sample(spec, oldprob, noise)
    adv = rng.standard_normal(N)
    outs = []
    for use_cache in (False, True):
        net = MlpNet(n_in, A, _head_id(head), dtype=dtype)
        net.use_cache = use_cache
        net.set_flat(th)
        x, a = _dev(ob), _dev(act, torch.int32 if head == "softmax" else torch.float32)
        partial = torch.zeros(net.partial_rows(N) * 4, dtype=torch.float64, device="cuda")
        ghead = torch.zeros(N * net.gh, dtype=torch.float32, device="cuda")
        g = torch.zeros(net.P, dtype=torch.float32, device="cuda")
        net.rows(_lib.EPI_PPOCLIP, x, N, inv_n_global=1.0 / N, act=a, adv=_dev(adv), oldprob=_dev(oldprob), ghead=ghead,
                 partial=partial, clip=C.EPS)
        assert (net._cache_key is not None) == use_cache
        net.vjp_flat(x, N, ghead, g)
        outs.append([t.cpu().numpy() for t in (ghead, partial, g)])
    assert (outs[0][0] != 0).any() and (outs[0][0].reshape(N, -1) == 0).all(axis=1).any()  # kept and clipped rows
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    if dtype == "bf16" or n_in % 16 == 0:
        assert outs[0][2].tobytes() == outs[1][2].tobytes()
    else:
        assert np.abs(outs[0][2] - outs[1][2]).max() <= 1e-5 * np.abs(outs[0][2]).max()


# ------------------------------------------------------------------ the updater against its twin
UPDATE_CASES = [("gauss", 11, 3), ("softmax", 4, 3)]
# the seeds: the first (from 1) at which no twin row comes within 1e-3 of a clip bound
UPDATE_N, UPDATE_SEED, UPDATE_PERM_SEED = 300, {"gauss": 13, "softmax": 1}, 123
UPDATE_CFG = dict(clip_param=0.2, epochs=2, stepsize=3e-4, minibatch_size=128)


@functools.lru_cache(maxsize=None)
def update_twin(head, nin, nout, seed=None):
    """(spec, theta, ob, act, adv, oldprob, twin result) of an updater case, on the CPU."""
    rng = np.random.default_rng([UPDATE_SEED[head] if seed is None else seed, nin, nout])
    spec = T.Spec(nin, [64, 64], nout, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-nout:] = -0.3 + 0.1 * rng.standard_normal(nout)
    th = C._r32(th)
    ob = C._r32(rng.standard_normal((UPDATE_N, nin)))
    oldprob = C._r32(T.policy_prob(spec, th + 0.05 * rng.standard_normal(spec.P), ob))
    noise = rng.standard_normal((UPDATE_N, nout)) if head == "gauss" else rng.random(UPDATE_N)
    act = T.sample(spec, oldprob, noise)
    if head == "gauss":
        act = C._r32(act)
    adv = C._r32(T.standardize(rng.standard_normal(UPDATE_N)))
    np.random.seed(UPDATE_PERM_SEED)
    perms = [np.random.permutation(UPDATE_N) for _ in range(UPDATE_CFG["epochs"])]
    twin = C.clip_update(spec, th, ob, act, adv, oldprob, perms, UPDATE_CFG["clip_param"], UPDATE_CFG["stepsize"],
                         UPDATE_CFG["minibatch_size"])
    return spec, th, ob, act, adv, oldprob, twin


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("head,nin,nout", UPDATE_CASES)
def test_ppo_clip_update_matches_twin(layered, head, nin, nout):
    """A whole PpoClipUpdater.update (300 rows: minibatches of 128, 128 and 44, two epochs)
    against the float64 twin on the same permutations, to the bounds of
    tests/test_gpu_ppo.py test_ppo_sgd_update_matches_oracle.  No twin row comes within 1e-3
    of a clip bound (tests/test_ppo_clip_host.py), so no row's mask can differ by rounding."""
    from modular_rl_amd import _lib
    from modular_rl_amd.collector import Batch
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import make_net
    from modular_rl_amd.ppo import PpoClipUpdater
    spec, th, ob, act, adv, oldprob, (th_w, info_w, adam_w, margin) = update_twin(head, nin, nout)
    assert margin > 1e-3
    net = make_net(nin, nout, _head_id(head), [64, 64], impl="layered" if layered else "auto")
    net.set_flat(th)
    pol = StochPolicyMLP(net, DiagGauss(nout) if head == "gauss" else Categorical(nout))
    up = PpoClipUpdater(pol, UPDATE_CFG)
    b = Batch(UPDATE_N, _dev(ob), _dev(act, torch.int32 if head == "softmax" else torch.float32), _dev(oldprob))
    b.adv = _dev(adv)
    np.random.seed(UPDATE_PERM_SEED)
    info = up.update(b)
    th1 = pol.get_flat().astype(np.float64)
    step = np.abs(th_w - th).max()
    print("ppo clip update", layered, head, "theta dist / step", np.abs(th1 - th_w).max() / step, info, info_w)
    assert np.abs(th1 - th_w).max() <= 1e-2 * step, (np.abs(th1 - th_w).max(), step)
    for k in ("surr_before", "kl_before", "ent_before", "surr_after", "kl_after", "ent_after"):
        np.testing.assert_allclose(info[k], info_w[k], rtol=2e-3, atol=2e-6, err_msg=k)
    assert info["epochs_run"] == info_w["epochs_run"] == 2 and up.t == adam_w[2] == 6


# ------------------------------------------------------------------ the agent
def _agent_cfg(**kw):
    return dict(dict(n_envs=64, horizon=64, timestep_limit=200, gamma=0.99, lam=0.97, timesteps_per_batch=64 * 64,
                     use_graph=1, seed=3, epochs=2, minibatch_size=1024), **kw)


def _run_agent(env_id, cfg, n_iter, agent=None, callback=None):
    from modular_rl_amd import agentzoo
    from modular_rl_amd.core import run_policy_gradient_algorithm
    from modular_rl_amd.envs import make
    env = make(env_id)
    if agent is None:
        agent = agentzoo.PpoClipAgent(env.observation_space, env.action_space, cfg)
    seen = []

    def cb(st):
        seen.append(dict(st))
        if callback is not None:
            callback(agent, len(seen))
    run_policy_gradient_algorithm(env, agent, callback=cb, usercfg=dict(cfg, n_iter=n_iter))
    return agent, seen


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("impl,hid", [("auto", [64, 64]), ("layered", [96, 80])])
@pytest.mark.parametrize("env_id", ["CartPole-v0", "Hopper-v2"])
def test_ppo_clip_agent_runs_iterations(env_id, impl, hid, dtype):
    cfg = _agent_cfg(mlp_impl=impl, hid_sizes=hid, mlp_dtype=dtype)
    from modular_rl_amd import agentzoo
    from modular_rl_amd.envs import make
    env = make(env_id)
    agent = agentzoo.PpoClipAgent(env.observation_space, env.action_space, cfg)
    assert agent.policy.net.layered == (impl == "layered")
    th0 = agent.policy.get_flat().copy()
    _, seen = _run_agent(env_id, cfg, 3, agent=agent)
    assert len(seen) == 3
    for st in seen:
        assert all(np.isfinite(v) for k, v in st.items() if k.startswith("pol_")), st
        assert st["pol_epochs_run"] == 2
    assert np.isfinite(agent.policy.get_flat()).all() and (agent.policy.get_flat() != th0).any()


def test_ppo_clip_agent_stops_early_on_target_kl():
    _, seen = _run_agent("CartPole-v0", _agent_cfg(target_kl=1e-9), 2)
    assert [st["pol_epochs_run"] for st in seen] == [1, 1]


def test_ppo_clip_resume_continues_bit_identically(tmp_path):
    """A snapshot taken inside the iteration-2 callback and resumed for one iteration ends
    bit-identical to the uninterrupted 3-iteration run (tests/test_checkpoint.py): theta, the
    VF, the Adam moments and step count, the stats."""
    from modular_rl_amd.checkpoint import load_snapshot, save_snapshot
    from modular_rl_amd import agentzoo
    from modular_rl_amd.envs import make
    cfg = _agent_cfg(timestep_limit=1000, gamma=0.995, pipeline=1)
    path = str(tmp_path / "snap.npz")

    def snap(agent, k):
        if k == 2:
            save_snapshot(path, agent, counter=2, env_id="Hopper-v2")
    full, st_full = _run_agent("Hopper-v2", cfg, 3, callback=snap)
    env = make("Hopper-v2")
    resumed = agentzoo.PpoClipAgent(env.observation_space, env.action_space, cfg)
    assert load_snapshot(path, resumed)["counter"] == 2
    _, st_res = _run_agent("Hopper-v2", cfg, 1, agent=resumed)
    assert np.array_equal(resumed.policy.get_flat(), full.policy.get_flat())
    assert np.array_equal(resumed.baseline.net.get_flat(), full.baseline.net.get_flat())
    want = full.updater.state_arrays()
    assert {"adam_m", "adam_v", "adam_t"} <= set(want) and int(want["adam_t"][0]) == 3 * 2 * 4
    for k, v in want.items():
        w = resumed.updater.state_arrays()[k]
        a = v.cpu().numpy() if torch.is_tensor(v) else v
        b = w.cpu().numpy() if torch.is_tensor(w) else w
        assert np.array_equal(a, b), k
    for k in ("EpRewMean", "pol_surr_after", "pol_kl_after", "pol_epochs_run", "vf_EVBefore"):
        if k in st_full[-1]:
            assert st_res[0][k] == st_full[-1][k], k
