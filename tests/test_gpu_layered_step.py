"""The GPU half of the layered rollout's step tests: every case of tests/layered_step_cases.py
drives one C entry -- mrl_rollout_act_head / _bf16, mrl_rollout_obs, mrl_rollout_reset_rows,
mrl_rollout_act -- through ``_lib.call`` on buffers the test wrote itself, and compares what the
entry left with the float64 references of tests/layered_step_np.py.  A Collector on a small
layered policy owns the buffers; no case runs a policy forward or more than two env steps."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import trpo_np as T
from tests import layered_step_cases as C
from tests import layered_step_np as R
from tests.gemm_bf16_cases import rne_bits

pytestmark = pytest.mark.gpu

SENT = -7.25      # float sentinels (exact in every float format used)
SENT_I = -77
SENT_U8 = 0xAB
SENT16 = 0x7FC1   # a bf16 NaN the kernels never produce
A = C.A_HEAD


@functools.lru_cache(maxsize=None)
def _policy(env_id):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.envs import make
    from modular_rl_amd.nets import LayeredMlpNet
    env = make(env_id)
    head = "softmax" if env.discrete else "gauss"
    rng = np.random.default_rng(17)
    spec = T.Spec(env.obs_dim, [32], env.act_dim, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss").astype(np.float32)
    net = LayeredMlpNet(env.obs_dim, env.act_dim, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, [32])
    net.set_flat(th)
    return env, StochPolicyMLP(net, DiagGauss(env.act_dim) if head == "gauss" else Categorical(env.act_dim))


def _collector(env_id, E, Tn, seed, filt=1, bf16=False, ev=False):
    """A Collector's buffers, and where the case needs one the Collector would not build -- bf16
    compute beside f32 hidden rows, evaluation mode -- a desc built as Collector.__init__ does."""
    from modular_rl_amd import _lib
    from modular_rl_amd.collector import Collector
    env, pol = _policy(env_id)
    col = Collector(env, pol, E, Tn, 1000, filter=filt, seed=seed, use_graph=False)
    assert col.layered
    if bf16 or ev:
        compute = (_lib.COMPUTE_BF16 if bf16 else _lib.COMPUTE_F32) | (_lib.ROLLOUT_EVAL if ev else 0)
        col.desc = _lib.RolloutDesc(env.kind, E, Tn, 1000, int(filt), 0, seed, compute, 0)
        col.evaluate = bool(ev)
    return env, col


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _view(values, lead, dtype):
    """``values`` on the device as a view ``lead`` elements into a larger NaN / sentinel tensor
    (a 16-byte aligned base plus lead elements), with the same guard behind."""
    n = values.size
    fill = float("nan") if dtype == torch.float32 else SENT_I
    big = torch.full((n + 64,), fill, dtype=dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[lead:lead + n] = torch.as_tensor(np.ascontiguousarray(values).reshape(-1)).to(dtype).cuda()
    return big, big[lead:lead + n]


def _sent(buf):
    return {torch.float32: SENT, torch.float64: SENT, torch.int32: SENT_I, torch.uint8: SENT_U8}[buf.dtype]


TRAJ = ("act", "prob", "rew", "flags", "ep_t")


def _prefill(col):
    for name in TRAJ + ("obs",):
        buf = getattr(col, name)
        buf.fill_(_sent(buf))


def _assert_rows_only(col, t, E, what):
    """Of the trajectory buffers only the rows t E .. t E + E - 1 were written."""
    for name in TRAJ:
        buf = getattr(col, name)
        rows, sent = buf.view(col.T, E, -1), _sent(buf)
        for tt in range(col.T):
            if tt != t:
                assert bool((rows[tt] == sent).all()), (what, name, "row block", tt)
        assert not bool((rows[t] == sent).all(dim=-1).any()), (what, name, "a row of step t not written")


def _assert_sampled_action(act, noise, sd, z, what):
    """act == float32(float32(noise) * sd) + z, bit for bit, in numpy float32 from the device's
    own z and sd: the reference's two roundings (core.py:432-435).

    Before this test the kernels wrote __fadd_rn(__fmul_rn(noise, sd), z), which the compiler's
    headers define as plain * and + and the default -ffp-contract fuses into one v_fma_f32: a
    single rounding, one ulp off in a fifth to a third of the action words (512-f32-al-1-1-0-1:
    5 of 17; 512-f32-al-3-4-0-1: 16 of 51; every training case of the fused head and every
    Hopper-v2 case of mrl_rollout_act, 106 of this file's 171 cases).  The layered kernels now
    switch the contraction off for that product and sum (mul_then_add, rollout_device.h)."""
    zn = noise.astype(np.float32)
    expect = (zn * sd) + z
    assert expect.dtype == np.float32
    diff = act.view(np.uint32) != expect.view(np.uint32)
    assert not diff.any(), (what, "%d of %d action words differ from the two-rounding value" % (int(diff.sum()), diff.size))


# ------------------------------------------------------------------ 1. the fused head
HEAD_WORST = {}


def _start(c, o, seed, bf16):
    """A collector after mrl_rollout_reset_rows with sentinels everywhere an act call may write."""
    from modular_rl_amd._lib import call, stream
    _, col = _collector("Humanoid-v2", c.E, C.HEAD_T, seed, bf16=bf16, ev=bool(c.ev))
    if not c.ev:
        col.set_noise(o.noise)
    col.records.fill_(SENT)
    col.filter_state.fill_(SENT)
    call("mrl_rollout_reset_rows", ctypes.byref(col.desc), ctypes.byref(col._bufs()), stream())
    _prefill(col)
    torch.cuda.synchronize()
    return col


def _head_call(c, o, col, woff, hoff):
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    if c.mode == "b16":
        keep_h, h = _view(o.hid16.view(np.int16), 8 + hoff // 2, torch.int16)
        assert h.data_ptr() % 16 == hoff
    else:
        keep_h, h = _view(o.hid, 4 + hoff // 4, torch.float32)
        assert h.data_ptr() % 16 == hoff
    keep_w, w = _view(o.w, 4 + woff, torch.float32)
    assert w.data_ptr() % 16 == 4 * woff
    b, logstd = _dev(o.b, torch.float32), _dev(o.logstd, torch.float32)
    fn = "mrl_rollout_act_head_bf16" if c.mode == "b16" else "mrl_rollout_act_head"
    call(fn, ctypes.byref(col.desc), int(_lib.HEAD_GAUSS), A, ptr(h), int(c.nh), ptr(w), ptr(b), ptr(logstd),
         ctypes.byref(col._bufs()), int(c.t), stream())
    torch.cuda.synchronize()
    del keep_h, keep_w


def _head_variant(c, o, name, woff, hoff):
    """One fused call and its assertions; returns the bits of the z rows."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    E, t, what = c.E, c.t, (C.case_id(c), name)
    seed = 1000 + E
    bf16 = c.mode != "f32"
    col = _start(c, o, seed, bf16)
    rec0, fs0 = col.records.clone(), col.filter_state.clone()
    _head_call(c, o, col, woff, hoff)
    prob = col.prob.view(col.T, E, 2 * A)[t].cpu().numpy()
    act = col.act.view(col.T, E, A)[t].cpu().numpy()
    z, sd = prob[:, :A], prob[:, A:]

    # the mean columns against the float64 reference
    want, bound = R.head_reference(c)
    route = C.head_route(c.nh, woff == 0 and hoff == 0)
    ratio = float((np.abs(z.astype(np.float64) - want) / bound).max())
    key = (route, c.mode)
    HEAD_WORST[key] = max(HEAD_WORST.get(key, 0.0), ratio)
    restated = R.head_restated(c, route)
    print("head %s %s: error/bound %.4f (worst of %s so far %.4f); %d of %d words differ from the %s restatement"
          % (C.case_id(c), name, ratio, key, HEAD_WORST[key], int((restated.view(np.uint32) != z.view(np.uint32)).sum()),
             z.size, route))
    assert np.isfinite(z).all() and ratio <= 1.0, (what, ratio, np.unravel_index(
        np.argmax(np.abs(z - want) / bound), z.shape))

    # the std columns: one row for all, exp(logstd) to the layered test's 1e-4
    assert np.array_equal(sd.view(np.uint32), np.broadcast_to(sd[:1], sd.shape).view(np.uint32)), what
    np.testing.assert_allclose(sd[0], np.exp(o.logstd.astype(np.float64)), rtol=1e-4, atol=1e-4)

    # untouched memory
    _assert_rows_only(col, t, E, what)
    assert torch.equal(col.filter_state, fs0), what
    half = col.records.numel() // 2
    wr = (t + 1) & 1
    if c.ev:
        assert torch.equal(col.records, rec0), what
    else:
        assert torch.equal(col.records[(1 - wr) * half:(2 - wr) * half], rec0[(1 - wr) * half:(2 - wr) * half]), what
        assert not bool((col.records[wr * half:(wr + 1) * half] == SENT).any()), what

    # fused == unfused: mrl_rollout_act on the z rows the fused call produced
    ref = _start(c, o, seed, bf16)
    zrows = _dev(z, torch.float32)
    logstd = _dev(o.logstd, torch.float32)
    call("mrl_rollout_act", ctypes.byref(ref.desc), int(_lib.HEAD_GAUSS), A, ptr(zrows), ptr(logstd),
         ctypes.byref(ref._bufs()), int(t), stream())
    torch.cuda.synchronize()
    for name_ in ("env_state", "env_int", "raw_obs", "rew", "flags", "ep_t", "records", "act", "prob", "filter_state"):
        assert torch.equal(getattr(col, name_), getattr(ref, name_)), (what, "fused != unfused", name_)

    # the action, from the device's own z and sd (last: see _assert_sampled_action)
    if c.ev:
        assert np.array_equal(act.view(np.uint32), z.view(np.uint32)), what
    else:
        _assert_sampled_action(act, o.noise.reshape(C.HEAD_T, E, A)[t], sd, z, what)
    return z.view(np.uint32).copy()


@pytest.mark.parametrize("c", C.HEAD, ids=C.case_id)
def test_fused_head(c, monkeypatch):
    monkeypatch.setenv("MRL_HM_WPB", str(c.wpb))
    o = R.head_operands(c.nh, c.E)
    bits = {name: _head_variant(c, o, name, woff, hoff) for name, woff, hoff in C.head_variants(c)}
    if c.align == "mis":
        # both fallbacks take the lane loop: one result, and not the runs' (which sum in another order)
        assert np.array_equal(bits["woff"], bits["hoff"]), C.case_id(c)
        assert not np.array_equal(bits["woff"], bits["al"]), C.case_id(c)
        strided = R.head_restated(c, "strided").view(np.uint32)
        runs = R.head_restated(c, C.head_route(c.nh, True)).view(np.uint32)
        assert int((bits["woff"] != strided).sum()) < int((bits["woff"] != runs).sum()), C.case_id(c)


# ------------------------------------------------------------------ 2. mrl_rollout_obs
@pytest.mark.parametrize("c", C.OBS, ids=C.case_id)
def test_obs(c):
    from modular_rl_amd._lib import call, stream
    o = R.obs_operands(c)
    E, O, D, t = c.E, o.O, o.D, c.t
    _, col = _collector(c.env, E, C.OBS_T, 2000 + E, filt=c.filt, ev=bool(c.ev))
    assert col.FS == o.FS and col.RS == o.RS and col.NB == o.nb
    assert col.records.numel() == o.rec.size and col.raw_obs.numel() == o.raw.size
    col.raw_obs.copy_(_dev(o.raw.T.reshape(-1), torch.float64))
    rec_in, fs_in = _dev(o.rec.reshape(-1), torch.float64), _dev(o.fs.reshape(-1), torch.float64)
    col.records.copy_(rec_in)
    col.filter_state.copy_(fs_in)
    _prefill(col)
    ld = (O + 7) // 8 * 8
    if c.twin:
        col._xb16 = torch.full((E * ld,), SENT16, dtype=torch.int16, device="cuda")
        col.hidden_b16 = True
    call("mrl_rollout_obs", ctypes.byref(col.desc), ctypes.byref(col._bufs()), int(t), stream())
    torch.cuda.synchronize()
    what = C.case_id(c)

    fs_want, rows_want = R.obs_reference(c, o)
    fs = col.filter_state.cpu().numpy().reshape(2, o.FS)
    if c.ev:
        assert torch.equal(col.filter_state, fs_in), what
    else:
        wr = 1 - o.rd
        assert wr == (t + 1) & 1
        assert fs[wr, 0] == fs_want[0] and fs[wr, 1] == fs_want[1], what
        np.testing.assert_allclose(fs[wr], fs_want, rtol=1e-12, atol=0, err_msg=what)
        assert np.array_equal(fs[o.rd].view(np.uint64), o.fs[o.rd].view(np.uint64)), what
    assert torch.equal(col.records, rec_in), what

    obs = col.obs.view(col.T, E, O)
    rows = obs[t].cpu().numpy()
    np.testing.assert_allclose(rows, rows_want, rtol=1e-6, atol=1e-6, err_msg=what)
    for tt in range(col.T):
        if tt != t:
            assert bool((obs[tt] == SENT).all()), (what, "obs rows of step", tt)
    for name in TRAJ:
        assert bool((getattr(col, name) == _sent(getattr(col, name))).all()), (what, name)
    if c.twin:
        twin = col._xb16.view(E, ld).cpu().numpy().view(np.uint16)
        assert np.array_equal(twin[:, :O], rne_bits(rows)), what
        assert np.all(twin[:, O:] == SENT16), what


# ------------------------------------------------------------------ 3. the records
def _close_records(got, raw, with_rew, what):
    """A records half against oracle.rollout_np._block_partials over the device's own columns.
    Counts exact.  The device sums a block's 64 rows as eight strided partial sums, the oracle in
    row order, so a mean carries an error relative to the column's largest value, not to the
    mean (which may cancel), and an M2 one relative to n max|v|^2: 1e-12 of those scales beside
    the relative 1e-12."""
    D = raw.shape[1]
    want = R.block_records(raw, with_rew)
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, :2], want[:, :2]), what
    for b in range(len(want)):
        v = raw[C.BLOCK * b:C.BLOCK * (b + 1)]
        big = np.abs(v).max(axis=0)
        assert np.all(np.abs(got[b, 2:2 + D] - want[b, 2:2 + D]) <= 1e-12 * (np.abs(want[b, 2:2 + D]) + big)), (what, b)
        assert np.all(np.abs(got[b, 2 + D:] - want[b, 2 + D:]) <= 1e-12 * (want[b, 2 + D:] + len(v) * big ** 2)), (what, b)


@pytest.mark.parametrize("c", C.REC, ids=C.case_id)
def test_records(c):
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    E = c.E
    env, col = _collector(c.env, E, 2, 3000 + E)
    O, Aenv = env.obs_dim, env.act_dim
    D, nb, RS = O + 1, C.n_blocks(E), col.RS
    assert RS == 2 + 2 * D and col.NB == nb
    half = nb * RS
    col.records = torch.full((2 * half + RS,), SENT, dtype=torch.float64, device="cuda")  # a record's room behind
    rng = np.random.default_rng(E)
    col.set_noise(rng.random(2 * E) if env.discrete else rng.standard_normal((2 * E, Aenv)))
    d = ctypes.byref(col.desc)
    call("mrl_rollout_reset_rows", d, ctypes.byref(col._bufs()), stream())
    torch.cuda.synchronize()
    what = C.case_id(c)
    rec = col.records.cpu().numpy()
    raw = col.raw_obs.view(D, E).cpu().numpy().T
    assert np.all(raw[:, O] == 0.0)
    _close_records(rec[:half].reshape(nb, RS), raw, False, what)
    assert np.all(rec[half:] == SENT), what
    if E == 1:  # one row: the mean is the row, M2 exactly 0
        assert np.array_equal(rec[2:2 + D], raw[0]) and np.all(rec[2 + D:2 + 2 * D] == 0.0), what
    if not c.act:
        return
    z = _dev(0.3 * rng.standard_normal((E, Aenv)), torch.float32)
    logstd = None if env.discrete else _dev(-0.5 * np.ones(Aenv), torch.float32)
    head = _lib.HEAD_SOFTMAX if env.discrete else _lib.HEAD_GAUSS
    call("mrl_rollout_act", d, int(head), Aenv, ptr(z), ptr(logstd), ctypes.byref(col._bufs()), 0, stream())
    torch.cuda.synchronize()
    rec1 = col.records.cpu().numpy()
    raw1 = col.raw_obs.view(D, E).cpu().numpy().T
    assert not np.array_equal(raw1, raw) and np.any(raw1[:, O] != 0.0)
    _close_records(rec1[half:2 * half].reshape(nb, RS), raw1, True, what)
    assert np.array_equal(rec1[:half].view(np.uint64), rec[:half].view(np.uint64)), what
    assert np.all(rec1[2 * half:] == SENT), what


# ------------------------------------------------------------------ 4. mrl_rollout_act, a thread per env
@pytest.mark.parametrize("c", C.ACT, ids=C.case_id)
def test_act_thread_per_env(c):
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    E, Tn = c.E, 2
    env, col = _collector(c.env, E, Tn, 4000 + E)
    Aenv = env.act_dim
    rng = np.random.default_rng(E)
    d = ctypes.byref(col.desc)
    z = (0.8 * rng.standard_normal((E, Aenv))).astype(np.float32)
    zrows = _dev(z, torch.float32)
    what = C.case_id(c)

    def step(noise, logstd=None):
        col.set_noise(noise)
        call("mrl_rollout_reset_rows", d, ctypes.byref(col._bufs()), stream())
        _prefill(col)
        head = _lib.HEAD_SOFTMAX if env.discrete else _lib.HEAD_GAUSS
        call("mrl_rollout_act", d, int(head), Aenv, ptr(zrows), ptr(logstd), ctypes.byref(col._bufs()), 0, stream())
        torch.cuda.synchronize()
        _assert_rows_only(col, 0, E, what)
        return col.act.view(Tn, E, -1)[0].cpu().numpy(), col.prob.view(Tn, E, -1)[0].cpu().numpy()

    if not env.discrete:
        noise = rng.standard_normal((Tn * E, Aenv))
        ls = (-0.5 + 0.3 * rng.standard_normal(Aenv)).astype(np.float32)
        act, prob = step(noise, _dev(ls, torch.float32))
        zd, sd = prob[:, :Aenv], prob[:, Aenv:]
        assert np.array_equal(zd.view(np.uint32), z.view(np.uint32)), what
        assert np.array_equal(sd.view(np.uint32), np.broadcast_to(sd[:1], sd.shape).view(np.uint32)), what
        np.testing.assert_allclose(sd[0], np.exp(ls.astype(np.float64)), rtol=1e-4, atol=1e-4)
        _assert_sampled_action(act, noise[:E], sd, zd, what)
        return
    u0 = np.full(Tn * E, 0.5)
    act0, p = step(u0)
    z64 = z.astype(np.float64)
    soft = np.exp(z64 - z64.max(axis=1, keepdims=True))
    np.testing.assert_allclose(p, soft / soft.sum(axis=1, keepdims=True), rtol=1e-6, atol=0, err_msg=what)
    assert np.array_equal(act0.view(np.int32).reshape(E), R.categorical_action(p, u0[:E])), what
    u = np.concatenate([R.edge_uniforms(p), np.full(E, 0.5)])
    act1, p1 = step(u)
    assert np.array_equal(p1.view(np.uint32), p.view(np.uint32)), what
    assert np.array_equal(act1.view(np.int32).reshape(E), R.categorical_action(p, u[:E])), what
