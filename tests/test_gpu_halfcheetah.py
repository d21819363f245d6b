"""HalfCheetah-v2 on the device, through every layer that steps an env: VecEnv against the numpy
twin (tests/halfcheetah_np.py), written states in the floor, past every hinge stop and sliding
on a foot, the fused rollout (step launches and the persistent launch; 18 filter columns, so the
second column pass of rollout_kernels.h) and the layered rollout against oracle.rollout_np.collect on
the twin, the population rollout (both kernels) replayed through a VecEnv, and run_pg.py /
run_cem_algorithm end to end.  Sizes and tolerances are tests/test_gpu_planar_chains.py's."""
import json

import numpy as np
import pytest
import torch

from tests import cem_small_np
from tests import halfcheetah_cases as HCC
from tests import halfcheetah_np as H

pytestmark = pytest.mark.gpu
ENV_ID = HCC.ENV_ID


def _close(got, want, what, rew=False):
    tol = 1e-4 if rew else 1e-5  # test_rollout_matches_oracle's bounds
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=what)


def _state(vec):
    return vec.env_state[:HCC.NS * vec.E].view(HCC.NS, vec.E).cpu().numpy().T


# ------------------------------------------------------------------ 1. step against the twin
@pytest.mark.parametrize("E,Tn,limit", HCC.STEP_CASES)
def test_step_matches_twin(E, Tn, limit):
    from modular_rl_amd.envs import VecEnv
    vec = VecEnv(ENV_ID, E, seed=HCC.step_seed(E), timestep_limit=limit)
    actions = HCC.step_actions(E, Tn)
    assert (np.abs(actions) > 1.0).any()  # the control clamp is hit
    (obs0, state0), steps = HCC.reference_steps(E, Tn, limit)
    _close(vec.reset().cpu().numpy(), obs0, "reset obs")
    _close(_state(vec), state0, "reset state")
    resets = 0
    for t, w in enumerate(steps):
        o, r, done, info = vec.step(actions[t])
        np.testing.assert_array_equal(info["ep_t"].cpu().numpy(), w["ep_t"], err_msg=f"ep_t {t}")
        np.testing.assert_array_equal(info["flags"].cpu().numpy(),
                                      w["last"].astype(np.uint8) | (w["term"].astype(np.uint8) << 1), err_msg=f"flags {t}")
        np.testing.assert_array_equal(done.cpu().numpy(), w["last"])
        np.testing.assert_array_equal(info["terminated"].cpu().numpy(), w["term"])
        _close(r.cpu().numpy(), w["rew"], f"rew {t}", rew=True)
        if len(w["idx"]):
            _close(info["final_obs"].cpu().numpy()[w["idx"]], w["final_obs"], f"final obs {t}")
            resets += len(w["idx"])
        _close(o.cpu().numpy(), w["obs"], f"obs {t}")
        _close(_state(vec), w["state"], f"state {t}")
        np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), w["ep_count"])
    assert resets > 0


# ------------------------------------------------------------------ 2. written states, one step
# rows in both 64-env blocks (E = 70)
FLOOR_ROWS = [5, 65]    # the back foot's lower sphere 0.02 m into the floor
SLIDE_ROWS = [12, 67]   # the same, sliding at 2 m/s: the friction clamp is active
# every hinge 0.03 rad past each of its stops; four of the twelve also in the second block
STOP_ROWS = {(b, side): [20 + 2 * b + (side > 0)] for b in range(1, 7) for side in (1, -1)}
for _key, _row in (((1, 1), 64), ((3, -1), 66), ((4, 1), 68), ((6, -1), 69)):
    STOP_ROWS[_key].append(_row)


def test_written_states_step_as_the_twin():
    from modular_rl_amd.envs import VecEnv
    E = 70
    vec = VecEnv(ENV_ID, E, seed=19, auto_reset=False)
    vec.reset()
    st = vec.env_state.view(HCC.NS, E)
    act = (0.3 * np.random.default_rng(2).standard_normal((E, 6))).astype(np.float32)
    rest = np.zeros((1, 18))
    _, pen = H.tree_normal_forces(rest, H.HC)
    low = int(np.argmax(pen[0]))
    assert H.HC.spheres[low][0] == 3  # the back foot reaches lowest in the rest pose
    touched = []
    for rows, speed in ((FLOOR_ROWS, 0.0), (SLIDE_ROWS, 2.0)):
        for r in rows:
            st[:, r] = 0.0
            st[1, r] = float(pen[0, low]) - 0.02
            st[9, r] = speed
        touched += rows
    for (b, side), rows in STOP_ROWS.items():
        stop = H.HC.hi[b] if side > 0 else H.HC.lo[b]
        for r in rows:
            st[2 + b, r] = stop + side * 0.03
        touched += rows
    act[touched] = 0.0
    before = _state(vec).copy()
    fn, depth = H.tree_normal_forces(before, H.HC)
    np.testing.assert_allclose(depth[FLOOR_ROWS + SLIDE_ROWS].max(axis=1), 0.02, atol=1e-12)
    lim = 0.4 * fn[SLIDE_ROWS].max(axis=1)
    assert (lim > 0).all() and (H.CF * 2.0 > lim).all()  # the viscous friction is clamped to mu f_n
    after, rew, done = H.hc_step(before, act)
    assert not done.any()
    o, r, d, info = vec.step(act)
    state = _state(vec)
    np.testing.assert_array_equal(info["flags"].cpu().numpy(), np.zeros(E, np.uint8))
    np.testing.assert_allclose(state, after, rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.cpu().numpy(), rew, rtol=0, atol=1e-8)
    np.testing.assert_allclose(o.cpu().numpy(), H.hc_obs(after), rtol=0, atol=1e-8)
    assert (state != before).any(axis=1).all()
    assert (state[SLIDE_ROWS] != state[FLOOR_ROWS]).any(axis=1).all()  # the sliding rows went another way


# ------------------------------------------------------------------ 3. rollout against the oracle's collect
def _fused_policy(th, dtype="fp32"):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import MlpNet
    net = MlpNet(HCC.OBS, HCC.ACT, _lib.HEAD_GAUSS, dtype=dtype)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(HCC.ACT))


def _layered_policy(hid, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import LayeredMlpNet
    net = LayeredMlpNet(HCC.OBS, HCC.ACT, _lib.HEAD_GAUSS, hid)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(HCC.ACT))


def _check_against_collect(pol, E, Tn, limit, its, layered):
    """test_rollout_matches_oracle's assertions and tolerances, over two iterations."""
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    col = Collector(make(ENV_ID), pol, E, Tn, limit, filter=1, seed=HCC.rollout_seeds(E)[1], use_graph=False)
    assert col.layered == layered
    resets = 0
    for want, fs, noise in its:
        if noise is not None:
            col.set_noise(noise.reshape(Tn * E, -1))
        b = col.collect()
        np.testing.assert_array_equal(b.flags.cpu().numpy().reshape(Tn, E), want["flags"])
        np.testing.assert_array_equal(b.ep_t.cpu().numpy().reshape(Tn, E), want["ep_t"])
        np.testing.assert_allclose(b.obs.cpu().numpy().reshape(Tn, E, -1), want["obs"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(b.act.cpu().numpy().reshape(Tn, E, -1), want["act"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(b.prob.cpu().numpy().reshape(Tn, E, -1), want["prob"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(b.rew.cpu().numpy().reshape(Tn, E), want["rew"], rtol=1e-4, atol=1e-4)
        (n, m, var), (nr, mr, vr) = col.filter_stats()
        assert n == fs.n and nr == fs.nr
        np.testing.assert_allclose(m, fs.M[:-1], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(mr, fs.M[-1], rtol=1e-5, atol=1e-6)
        resets += int((want["flags"][:-1] & 1).sum())
    return resets


@pytest.mark.parametrize("E,Tn,limit,inject", HCC.ROLLOUT_CASES)
def test_rollout_matches_twin_collect(E, Tn, limit, inject):
    """The fused rollout (64-64 policy, filter on) against oracle.rollout_np.collect on the
    twin, two iterations, with and without injected noise."""
    _, th, its = HCC.reference_rollout([64, 64], E, Tn, limit, inject)
    resets = _check_against_collect(_fused_policy(th), E, Tn, limit, its, layered=False)
    assert resets > 0 or min(limit, HCC.LIMIT) >= Tn


def test_layered_rollout_matches_twin_collect():
    hid, E, Tn, limit = HCC.LAYERED_CASE
    _, th, its = HCC.reference_rollout(hid, E, Tn, limit, False)
    assert _check_against_collect(_layered_policy(hid, th), E, Tn, limit, its, layered=True) > 0


# ------------------------------------------------------------------ 4. persistent launch = step launches
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("E,Tn,limit", HCC.PERSISTENT_CASES)
def test_persistent_rollout_equals_step_launches(E, Tn, limit, dtype):
    """Two iterations, bit-identical; bf16 runs the bf16 forward's instantiations of both fused
    kernels over the 18 columns."""
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(ENV_ID)
    _, th = HCC.policy_theta([64, 64], 17)
    pol = _fused_policy(th, dtype)
    assert pol.net.dtype == dtype
    outs = []
    for persistent in (False, True):
        col = Collector(env, pol, E, Tn, limit, seed=31, use_graph=False)
        col.persistent = persistent
        got = []
        for _ in range(2):
            b = col.collect()
            if persistent:
                col.check()
            got += [t.clone() for t in (b.obs, b.act, b.prob, b.rew, b.flags, b.ep_t)]
        got += [col.filter_state[:col.FS].clone(), col.env_state.clone(), col.env_int.clone(), col.iteration.clone()]
        outs.append(got)
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), i
    assert int((outs[0][4].view(Tn, E)[:-1] & 1).sum()) > 0  # episodes ended and restarted


# ------------------------------------------------------------------ 5. population rollout
def _replay(n, seed, limit, out):
    """The traced actions through a VecEnv (same seed, no auto-reset): (ret, len, flags)."""
    from modular_rl_amd.envs import VecEnv
    env = VecEnv(ENV_ID, n, seed=seed, auto_reset=False)
    obs = env.reset().cpu().numpy().copy()
    ret = np.zeros(n)
    for t in range(limit):
        np.testing.assert_allclose(obs, out["trace_obs"][t], rtol=1e-5, atol=1e-5, err_msg=f"obs {t}")
        ob, rew, done, info = env.step(torch.as_tensor(out["trace_act"][t]).cuda())
        assert not info["terminated"].any()
        obs = ob.cpu().numpy().copy()
        ret += rew.cpu().numpy()
    return ret


def _run_population(n, seed, limit, thetas, hid=(64, 64)):
    from modular_rl_amd.envs import PopulationRollout
    pop = PopulationRollout(ENV_ID, n, seed=seed, timestep_limit=limit, hid_sizes=hid)
    assert (pop.pol is not None) == (tuple(hid) == (64, 64)) and pop.P == thetas.shape[1]
    out = pop(torch.as_tensor(thetas).cuda(), trace_steps=pop.limit)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def test_population_rollout_replays_through_a_vecenv():
    n, limit, seed = HCC.POP_N, HCC.POP_LIMIT, HCC.POP_SEED
    out = _run_population(n, seed, limit, HCC.population(n, seed))
    ret = _replay(n, seed, limit, out)
    np.testing.assert_array_equal(out["ret"], ret)
    np.testing.assert_array_equal(out["len"], np.full(n, limit, np.int32))
    np.testing.assert_array_equal(out["flags"], np.ones(n, np.uint8))  # never ends by itself: all cut at 25


def test_small_net_kernel_is_bit_identical_to_the_64_64_kernel():
    """A 10-5 net through mrl_pop_rollout_mlp, and zero-padded to 64-64 through
    mrl_pop_rollout: every output and trace (tests/test_gpu_cem_small.py's comparison)."""
    n, limit, seed = HCC.POP_N, HCC.POP_LIMIT, HCC.POP_SEED
    th = HCC.population(n, seed, hid=HCC.SMALL_HID)
    small = _run_population(n, seed, limit, th, hid=HCC.SMALL_HID)
    pad = np.stack([cem_small_np.pad_to_64_64(t, HCC.OBS, HCC.SMALL_HID, HCC.ACT, True) for t in th])
    big = _run_population(n, seed, limit, pad)
    assert (small["len"] == limit).all() and np.abs(small["trace_act"]).max() > 0.0
    for k in ("ret", "len", "flags", "stat", "trace_obs", "trace_act", "trace_rew"):
        assert np.array_equal(big[k], small[k]), k


# ------------------------------------------------------------------ 6. end to end
def test_run_pg_cli_two_iterations(capsys):
    import run_pg
    run_pg.main(["--env", ENV_ID, "--n_iter", "2", "--n_envs", "256", "--horizon", "64", "--json",
                 "--gamma", "0.995", "--lam", "0.97", "--max_kl", "0.01"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for st in lines:
        assert all(np.isfinite(v) for v in st.values()), st
        assert round(st["NumEpBatch"] * st["EpLenMean"]) == 256 * 64
        # 0 < KL <= 2 max_kl: the update moved the policy (theta changed)
        assert 0.0 < st["pol_kl_after"] <= 2 * 0.01 and "pol_surr_after" in st


def test_run_cem_algorithm_two_generations():
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make(ENV_ID)
    cfg = dict(batch_size=64, n_iter=2, elite_frac=0.25, filter=1, seed=5, timestep_limit=40)
    agent = DeterministicAgent(env.observation_space, env.action_space, cfg)
    th0 = agent.get_flat().copy()
    infos = []
    run_cem_algorithm(env, agent, usercfg=cfg, callback=lambda info: infos.append(dict(info)))
    assert len(infos) == 2
    for info in infos:
        assert info["ys"].shape == (64,) and np.isfinite(info["ys"]).all() and np.isfinite(info["th"]).all()
        assert np.isfinite(info["std"]).all() and np.isfinite(info["ymean"])
        assert (info["len"] == 40).all()  # HalfCheetah never ends by itself
    assert np.isfinite(agent.filter_state.cpu().numpy()).all()
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
    assert (agent.get_flat() != th0).any()  # theta changed
