"""Host-side checks of the rollout's evaluation mode (MRL_ROLLOUT_EVAL): the float64 helper
(tests/eval_np.py) against oracle.rollout_np.collect, the arg-max tie rule, the C ABI's refusals
(they precede any HIP call), the agent's collector cache key and sim_agent.py's command line."""
import ctypes
import types

import numpy as np
import pytest

from oracle import rollout_np as RO
from oracle import trpo_np as T
from tests import eval_np
from tests import halfcheetah_cases as HCC
from tests.halfcheetah_np import HALFCHEETAH, TreeEnvs

E_ARG = -1


def _hopper_policy(seed):
    rng = np.random.default_rng(seed)
    spec = T.Spec(11, [64, 64], 3, "gauss")
    th = T.mlp_init(rng, spec.shapes, True) + 0.1 * rng.standard_normal(spec.P)
    th[-3:] = -0.5
    return spec, th.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("kind", ["hopper", "halfcheetah"])
def test_helper_equals_collect_with_zero_noise_and_no_filter(kind):
    """collect has no hook that holds its filter fixed, so the two are compared with the filter
    off, where they must agree exactly: with zero injected noise collect's Gauss sample is its
    mean, bit for bit (0 * sd + z), and the bookkeeping is the same code path.  Two iterations:
    the reset stream goes on.  (A softmax sample at u = 0 is the first action, not the mode; the
    discrete head's mode is checked below and on the device.)"""
    E, Tn, limit = 7, 24, 9
    if kind == "hopper":
        spec, th = _hopper_policy(3)
        a, b = RO.Envs(RO.HOPPER, E, 21), RO.Envs(RO.HOPPER, E, 21)
    else:
        spec, th = HCC.policy_theta([64, 64], 3)
        a, b = TreeEnvs(HALFCHEETAH, E, 21), TreeEnvs(HALFCHEETAH, E, 21)
    fs = RO.FilterState(a.O + 1)
    for it in range(2):
        want, _ = RO.collect(a, RO.FilterState(a.O + 1), spec, th, Tn, limit, it, filt=False,
                             noise=np.zeros((Tn, E, a.A)))
        got = eval_np.collect_eval(b, fs, spec, th, Tn, limit, filt=False)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert (want["flags"][:-1] & 1).any()  # the limit cut episodes inside the horizon
    assert fs.n == 0.0 and not fs.M.any() and not fs.S.any()
    np.testing.assert_array_equal(a.ep_count, b.ep_count)
    np.testing.assert_array_equal(a.state, b.state)


def test_frozen_filter_formula_and_the_clip_only_state():
    rng = np.random.default_rng(0)
    fs = RO.FilterState(4)
    o = 10.0 * rng.standard_normal((5, 3))
    np.testing.assert_array_equal(eval_np.frozen_filter(fs, o), np.clip(o, -5, 5))  # count 0
    fs.n, fs.M[:], fs.S[:] = 1.0, 3.0, 2.0
    np.testing.assert_array_equal(eval_np.frozen_filter(fs, o), np.clip(o, -5, 5))  # count 1: still clip only
    fs.n = 9.0
    want = np.clip((o - 3.0) / (np.sqrt(2.0 / 8.0) + 1e-8), -5, 5)
    np.testing.assert_array_equal(eval_np.frozen_filter(fs, o), want)
    keep = fs.copy()
    eval_np.frozen_filter(fs, o)
    assert (fs.n, fs.nr) == (keep.n, keep.nr) and (fs.M == keep.M).all() and (fs.S == keep.S).all()


def test_argmax_ties_take_the_lowest_index():
    spec = types.SimpleNamespace(head="softmax")
    z = np.array([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0], [-1.0, -2.0, -1.0], [0.0, 0.5, 1.0]])
    np.testing.assert_array_equal(eval_np.mode_action(spec, z), [0, 1, 0, 0, 2])
    from modular_rl_amd.core import Categorical
    np.testing.assert_array_equal(Categorical(3).maxprob(T.softmax(z)), [0, 1, 0, 0, 2])


def _fused_call(lib, _lib, entry, desc, bufs, pol):
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the checks precede the launch
    if entry == "mrl_rollout_step":
        return lib.mrl_rollout_step(ctypes.byref(desc), ctypes.byref(pol), fake, fake, ctypes.byref(bufs), 0, None)
    return lib.mrl_rollout_run(ctypes.byref(desc), ctypes.byref(pol), fake, fake, ctypes.byref(bufs), fake, 1, None)


@pytest.mark.parametrize("compute", [0, 1])
@pytest.mark.parametrize("entry", ["mrl_rollout_step", "mrl_rollout_run"])
def test_abi_eval_desc_refuses_noise(entry, compute):
    """MRL_ROLLOUT_EVAL with noise rows is MRL_E_ARG before any launch; without them the call
    goes on to the next check (a policy of the wrong shape stops it there, still before the
    launch).  A training desc keeps asking for its noise rows."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    names = ("env_state", "env_int", "filter_state", "records", "iteration", "obs", "act", "prob", "rew", "flags",
             "ep_t")
    wrong = _lib.MlpDesc(4, 2, _lib.HEAD_SOFTMAX, 64, 2)  # CartPole's net on Hopper
    ev = _lib.RolloutDesc(_lib.ENV_HOPPER, 10, 7, 200, 1, 0, 0, compute | _lib.ROLLOUT_EVAL, 0)
    bufs = _lib.RolloutBufs(noise=fake, **{k: fake for k in names})
    assert _fused_call(lib, _lib, entry, ev, bufs, wrong) == E_ARG
    assert b"bufs.noise" in lib.mrl_last_error() and b"MRL_ROLLOUT_EVAL" in lib.mrl_last_error()
    bufs = _lib.RolloutBufs(**{k: fake for k in names})
    assert _fused_call(lib, _lib, entry, ev, bufs, wrong) == E_ARG
    assert b"policy shape" in lib.mrl_last_error()
    train = _lib.RolloutDesc(_lib.ENV_HOPPER, 10, 7, 200, 1, 0, 0, compute, 0)
    assert _fused_call(lib, _lib, entry, train, bufs, wrong) == E_ARG
    assert b"bufs.noise" in lib.mrl_last_error() and b"required" in lib.mrl_last_error()


def test_abi_eval_desc_refuses_noise_on_the_layered_act():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    names = ("env_state", "env_int", "filter_state", "records", "iteration", "obs", "act", "prob", "rew", "flags",
             "ep_t", "raw_obs")
    ev = _lib.RolloutDesc(_lib.ENV_HOPPER, 10, 7, 200, 1, 0, 0, _lib.ROLLOUT_EVAL, 0)
    bufs = _lib.RolloutBufs(noise=fake, **{k: fake for k in names})
    rc = lib.mrl_rollout_act(ctypes.byref(ev), _lib.HEAD_GAUSS, 3, fake, fake, ctypes.byref(bufs), 0, None)
    assert rc == E_ARG and b"MRL_ROLLOUT_EVAL" in lib.mrl_last_error()
    bufs = _lib.RolloutBufs(**{k: fake for k in names})
    rc = lib.mrl_rollout_act(ctypes.byref(ev), _lib.HEAD_SOFTMAX, 3, fake, fake, ctypes.byref(bufs), 0, None)
    assert rc == E_ARG and b"policy head" in lib.mrl_last_error()  # past the noise check


def test_abi_eval_desc_draws_no_noise_and_bad_compute_is_still_refused():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for kind, cols in ((_lib.ENV_CARTPOLE, 1), (_lib.ENV_HOPPER, 3), (_lib.ENV_HUMANOID, 17)):
        d = _lib.RolloutDesc(kind, 10, 7, 200, 1, 0, 0, 0, 0)
        assert lib.mrl_rollout_noise_doubles(ctypes.byref(d)) == 7 * 10 * cols
        for compute in (0, 1):
            d.compute = compute | _lib.ROLLOUT_EVAL
            assert lib.mrl_rollout_noise_doubles(ctypes.byref(d)) == 0
    d = _lib.RolloutDesc(_lib.ENV_HOPPER, 0, 7, 200, 1, 0, 0, _lib.ROLLOUT_EVAL, 0)
    assert lib.mrl_rollout_noise_doubles(ctypes.byref(d)) == -1  # n_envs = 0 is still a bad desc
    bufs = _lib.RolloutBufs(**{k: fake for k in ("env_state", "env_int", "filter_state", "records", "iteration")})
    d = _lib.RolloutDesc(_lib.ENV_HOPPER, 10, 7, 200, 1, 0, 0, _lib.ROLLOUT_EVAL, 0)
    assert lib.mrl_rollout_noise(ctypes.byref(d), ctypes.byref(bufs), fake, None) == E_ARG
    assert b"MRL_ROLLOUT_EVAL" in lib.mrl_last_error()
    for bad in (2, 2 | _lib.ROLLOUT_EVAL, 0x200, -1):  # the flag makes no other value acceptable
        d.compute = bad
        assert lib.mrl_rollout_reset(ctypes.byref(d), ctypes.byref(bufs), None) == E_ARG
        assert b"compute" in lib.mrl_last_error()
    d.compute = _lib.ROLLOUT_EVAL
    d.n_envs = 0
    assert lib.mrl_rollout_reset(ctypes.byref(d), ctypes.byref(bufs), None) == E_ARG
    assert b"sizes" in lib.mrl_last_error()


def test_header_and_binding_agree_on_the_flag():
    import os
    import re
    from modular_rl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mrl_hip.h")).read()
    assert int(re.search(r"#define MRL_ROLLOUT_EVAL (\w+)", text).group(1), 0) == _lib.ROLLOUT_EVAL
    assert _lib.ROLLOUT_EVAL & (_lib.COMPUTE_F32 | _lib.COMPUTE_BF16 | _lib.COMPUTE_SPLIT) == 0


class _StubCollector:
    made = []

    def __init__(self, env, policy, E, T, limit, **kw):
        self.E, self.T, self.limit, self.kw = E, T, limit, kw
        self.evaluate = kw["evaluate"]
        self.filter_state = object()
        _StubCollector.made.append(self)


def test_make_collector_cache_key_separates_the_modes(monkeypatch):
    from modular_rl_amd import agentzoo
    monkeypatch.setattr(agentzoo, "Collector", _StubCollector)
    _StubCollector.made = []
    agent = agentzoo.TrpoAgent.__new__(agentzoo.TrpoAgent)
    agent.cfg = {"filter": 1, "timestep_limit": 50, "n_envs": 8, "horizon": 16, "use_graph": 0}
    agent.seed, agent.comm, agent.policy, agent.stochastic = 5, None, None, True
    agent._collectors, agent._pending_state = {}, None
    env = types.SimpleNamespace(spec=types.SimpleNamespace(id="Hopper-v2", max_episode_steps=1000))
    train = agent.make_collector(env)
    assert not train.evaluate and train.kw["seed"] == 5
    assert agent.make_collector(env) is train and agent.make_collector(env, evaluate=False) is train
    ev = agent.make_collector(env, evaluate=True)
    assert ev is not train and ev.evaluate and (ev.E, ev.T, ev.limit) == (train.E, train.T, train.limit)
    assert ev.kw["seed"] == 6  # its own reset stream
    assert ev.filter_state is train.filter_state  # the agent's one filter state
    assert agent.make_collector(env, evaluate=True) is ev
    agent.set_stochastic(False)  # None follows agent.stochastic
    assert agent.make_collector(env) is ev
    agent.set_stochastic(True)
    assert agent.make_collector(env) is train
    assert len(_StubCollector.made) == 2 and len(agent._collectors) == 2
    assert agent._filter_owner() is train  # snapshots read the training collector's counters
    key = agentzoo.TrpoAgent.collector_key
    assert key("Hopper-v2", 8, 16, 50, False) != key("Hopper-v2", 8, 16, 50, True)
    assert key("Hopper-v2", 8, 16, 50, False) == ("Hopper-v2", 8, 16, 50)


def test_evaluation_collector_created_first_takes_only_the_filter_of_a_snapshot():
    import torch
    from modular_rl_amd.checkpoint import apply_collector_state
    col = types.SimpleNamespace(evaluate=True, FS=6, E=3, filter_state=torch.zeros(12, dtype=torch.float64),
                                iteration=torch.zeros(1, dtype=torch.int64),
                                env_int=torch.zeros(6, dtype=torch.int32))
    st = {"filter/state": np.arange(6.0), "rng/iteration": np.array([4]), "rng/episodes": np.arange(8)}
    rest = apply_collector_state(col, st)
    assert sorted(rest) == ["rng/episodes", "rng/iteration"]  # 8 envs' counters: not this collector's
    np.testing.assert_array_equal(col.filter_state[:6].numpy(), np.arange(6.0))
    assert int(col.iteration) == 0 and not col.env_int.any()
    train = types.SimpleNamespace(FS=6, E=8, filter_state=col.filter_state, iteration=torch.zeros(1, dtype=torch.int64),
                                  env_int=torch.zeros(16, dtype=torch.int32))
    assert apply_collector_state(train, rest) is None
    assert int(train.iteration) == 4 and train.env_int[8:].tolist() == list(range(8))


def test_sim_agent_parser_takes_the_reference_flags():
    import sim_agent
    p = sim_agent.make_parser()
    a = p.parse_args(["run.h5"])
    assert a.hdf == "run.h5" and a.timestep_limit is None and a.snapname is None
    assert a.n_envs > 0 and a.episodes == 1 and not a.json
    a = p.parse_args(["run.h5", "--timestep_limit", "250", "--snapname", "0020", "--n_envs", "16", "--episodes", "3",
                      "--json"])
    assert (a.timestep_limit, a.snapname, a.n_envs, a.episodes, a.json) == (250, "0020", 16, 3, True)
    assert "rendering" in sim_agent.__doc__ and "press enter" in sim_agent.__doc__


def test_sim_agent_picks_a_run_logs_snapshot_by_name(tmp_path):
    import json
    import sim_agent
    meta = np.frombuffer(json.dumps({"version": 2}).encode(), dtype=np.uint8)
    arrays = {}
    for name, v in (("0001", 1.0), ("0002", 2.0)):
        arrays[f"agent_snapshots__{name}__policy__theta"] = np.full(3, v, np.float32)
        arrays[f"agent_snapshots__{name}__meta"] = meta
    log = str(tmp_path / "run.npz")
    np.savez(log, params=np.zeros(1, np.uint8), **arrays)
    for snapname, want in ((None, 2.0), ("0001", 1.0)):
        out = sim_agent.snapshot_file(log, snapname, str(tmp_path))
        with np.load(out) as z:
            assert sorted(z.files) == ["meta", "policy__theta"] and z["policy__theta"][0] == want
    with pytest.raises(ValueError):
        sim_agent.snapshot_file(log, "0003", str(tmp_path))
    single = str(tmp_path / "one.npz")
    np.savez(single, meta=meta, policy__theta=np.zeros(3, np.float32))
    assert sim_agent.snapshot_file(single, None, str(tmp_path)) == single
