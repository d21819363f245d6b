"""Reacher-v2 and Swimmer-v2 on the device, through every layer that steps an env: VecEnv
against the numpy twin (tests/planar_chains_np.py), written states at the hinge stops and in
the fluid, Reacher's own TimeLimit and its goal across resets, the fused rollout (step launches
and the persistent launch) and the layered rollout against oracle.rollout_np.collect on the
twin, the population rollout (both kernels) replayed through a VecEnv, and run_pg.py /
run_cem_algorithm end to end.  tests/test_planar_chains_host.py proves that every goal
candidate drawn on these seeds keeps 1e-6 clear of the disc's edge, so the device picks the
twin's goals.  Sizes and tolerances are tests/test_gpu_mujoco_chains.py's."""
import json

import numpy as np
import pytest
import torch

from tests import cem_small_np
from tests import planar_cases as PC
from tests import planar_chains_np as PL

pytestmark = pytest.mark.gpu

OBS_FN = {"Reacher-v2": PL.rc_obs, "Swimmer-v2": PL.sw_obs}
STEP_FN = {"Reacher-v2": PL.rc_step, "Swimmer-v2": PL.sw_step}


def _close(got, want, what, rew=False):
    tol = 1e-4 if rew else 1e-5  # test_rollout_matches_oracle's bounds
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=what)


def _state(vec, ns):
    return vec.env_state[:ns * vec.E].view(ns, vec.E).cpu().numpy().T


# ------------------------------------------------------------------ 1. step against the twin
@pytest.mark.parametrize("env_id,E,Tn,limit", PC.ALL_STEP_CASES)
def test_step_matches_twin(env_id, E, Tn, limit):
    from modular_rl_amd.envs import VecEnv
    vec = VecEnv(env_id, E, seed=PC.step_seed(E), timestep_limit=limit)
    ns = PC.NS[env_id]
    actions = PC.step_actions(env_id, E, Tn)
    assert (np.abs(actions) > PC.ACT_HIGH[env_id]).any()  # the control clamp is hit
    (obs0, state0), steps, _ = PC.reference_steps(env_id, E, Tn, limit)
    _close(vec.reset().cpu().numpy(), obs0, "reset obs")
    _close(_state(vec, ns), state0, "reset state")
    resets = 0
    goals = [_state(vec, ns)[:, 4:6].copy()] if env_id == "Reacher-v2" else None
    for t, w in enumerate(steps):
        o, r, done, info = vec.step(actions[t])
        np.testing.assert_array_equal(info["ep_t"].cpu().numpy(), w["ep_t"], err_msg=f"ep_t {t}")
        flags = info["flags"].cpu().numpy()
        np.testing.assert_array_equal(flags, w["last"].astype(np.uint8) | (w["term"].astype(np.uint8) << 1),
                                      err_msg=f"flags {t}")
        np.testing.assert_array_equal(done.cpu().numpy(), w["last"])
        np.testing.assert_array_equal(info["terminated"].cpu().numpy(), w["term"])
        _close(r.cpu().numpy(), w["rew"], f"rew {t}", rew=True)
        if len(w["idx"]):
            _close(info["final_obs"].cpu().numpy()[w["idx"]], w["final_obs"], f"final obs {t}")
            resets += len(w["idx"])
        _close(o.cpu().numpy(), w["obs"], f"obs {t}")
        _close(_state(vec, ns), w["state"], f"state {t}")
        np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), w["ep_count"])
        if goals is not None:  # the goal never moves inside an episode
            now = _state(vec, ns)[:, 4:6].copy()
            kept = np.ones(E, dtype=bool)
            kept[w["idx"]] = False
            np.testing.assert_array_equal(now[kept], goals[-1][kept])
            if len(w["idx"]):
                goals.append(now)
        if limit is None:  # Reacher's own TimeLimit: every row ends at ep_t == 49, terminated
            if t % 50 == 49:
                assert (w["ep_t"] == 49).all()
                np.testing.assert_array_equal(flags, np.full(E, 3, np.uint8))
            else:
                np.testing.assert_array_equal(flags, np.zeros(E, np.uint8))
    assert resets > 0
    if limit is None:
        assert len(goals) == 2 and (goals[0] != goals[1]).all()  # the second episode's goal differs
        np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.full(E, 2))


# ------------------------------------------------------------------ 2. written states, one step
# rows in both 64-env blocks (E = 70): a limited hinge 0.03 rad past its stop, either side, and
# Swimmer rows drifting sideways at 2 m/s (the quadratic drag across the capsules)
STOP_ROWS = {1: [3, 64], -1: [30, 69]}
SIDE_ROWS = [10, 66]


def _written_setup(env_id, auto_reset, limit):
    from modular_rl_amd.envs import VecEnv
    E, seed = 70, 19
    vec = VecEnv(env_id, E, seed=seed, auto_reset=auto_reset, timestep_limit=limit)
    vec.reset()
    ns = PC.NS[env_id]
    model = PL.RC if env_id == "Reacher-v2" else PL.SW
    hinge = 1 if env_id == "Reacher-v2" else 3
    st = vec.env_state.view(ns, E)
    act = (0.3 * np.random.default_rng(2).standard_normal((E, 2))).astype(np.float32)
    for side, rows in STOP_ROWS.items():
        st[hinge, rows] = side * (model.hlim + 0.03)
    touched = sum(STOP_ROWS.values(), [])
    if env_id == "Swimmer-v2":
        st[6, SIDE_ROWS] = 2.0
        touched = touched + SIDE_ROWS
    act[touched] = 0.0
    before = _state(vec, ns).copy()
    after, rew, done = STEP_FN[env_id](before, act)
    assert not done.any()
    # the stop pushes back: the written hinges move towards their range
    for side, rows in STOP_ROWS.items():
        assert (side * after[rows, hinge] < model.hlim + 0.03).all()
    return vec, act, ns, before, after, rew, seed, touched


@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_written_states_step_as_the_twin(env_id):
    vec, act, ns, before, after, rew, _, touched = _written_setup(env_id, auto_reset=False, limit=None)
    o, r, done, info = vec.step(act)
    state = _state(vec, ns)
    np.testing.assert_array_equal(info["flags"].cpu().numpy(), np.zeros(vec.E, np.uint8))
    np.testing.assert_allclose(state, after, rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.cpu().numpy(), rew, rtol=0, atol=1e-8)
    np.testing.assert_allclose(o.cpu().numpy(), OBS_FN[env_id](after), rtol=0, atol=1e-8)
    rest = np.ones(vec.E, dtype=bool)
    rest[touched] = False
    moving = slice(0, 4) if env_id == "Reacher-v2" else slice(0, 10)
    assert (state[rest, moving] != before[rest, moving]).any(axis=1).all()  # the other rows stepped on
    if env_id == "Reacher-v2":
        np.testing.assert_array_equal(state[:, 4:], before[:, 4:])  # the goals stayed
    else:  # the drag slowed the sideways rows: 2 m/s across three capsules, 1 / (1 + 0.87) in 0.04 s
        assert (state[SIDE_ROWS, 6] < 1.5).all() and (state[SIDE_ROWS, 6] > 0.5).all()


@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_rows_ended_by_the_limit_come_back_as_fresh_episodes(env_id):
    vec, act, ns, before, after, rew, seed, _ = _written_setup(env_id, auto_reset=True, limit=1)
    o, r, done, info = vec.step(act)
    np.testing.assert_array_equal(info["flags"].cpu().numpy(), np.ones(vec.E, np.uint8))  # cut, not terminated
    twin = PL.PlanarEnvs(env_id, vec.E, seed)
    twin.reset(np.arange(vec.E))
    first = twin.state.copy()
    twin.reset(np.arange(vec.E))  # the rows' second episodes
    # a reset state is a multiply-add of a Philox uniform (Reacher's goal: a select among four)
    np.testing.assert_allclose(_state(vec, ns), twin.state, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(o.cpu().numpy(), twin.obs(), rtol=1e-12, atol=1e-15)
    if env_id == "Reacher-v2":
        assert (twin.state[:, 4:] != first[:, 4:]).all()  # a new goal
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.full(vec.E, 2))
    np.testing.assert_array_equal(vec.env_int[:vec.E].cpu().numpy(), np.zeros(vec.E, np.int32))
    np.testing.assert_allclose(info["final_obs"].cpu().numpy(), OBS_FN[env_id](after), rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.cpu().numpy(), rew, rtol=0, atol=1e-8)


# ------------------------------------------------------------------ 3. rollout against the oracle's collect
def _fused_policy(env_id, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import MlpNet
    O, A, _, _ = PC.SHAPES[env_id]
    net = MlpNet(O, A, _lib.HEAD_GAUSS)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(A))


def _layered_policy(env_id, hid, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import LayeredMlpNet
    O, A, _, _ = PC.SHAPES[env_id]
    net = LayeredMlpNet(O, A, _lib.HEAD_GAUSS, hid)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(A))


def _check_against_collect(env_id, pol, E, Tn, limit, its, layered):
    """test_rollout_matches_oracle's assertions and tolerances, over two iterations."""
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(env_id)
    col = Collector(env, pol, E, Tn, limit, filter=1, seed=PC.rollout_seeds(E)[1], use_graph=False)
    assert col.layered == layered
    resets = 0
    for want, fs, noise, _ in its:
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


@pytest.mark.parametrize("E,Tn,limit,inject", PC.ROLLOUT_CASES)
@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_rollout_matches_twin_collect(env_id, E, Tn, limit, inject):
    """The fused rollout (64-64 policy, filter on) against oracle.rollout_np.collect on the
    twin, two iterations, with and without injected noise."""
    _, th, its = PC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    resets = _check_against_collect(env_id, _fused_policy(env_id, th), E, Tn, limit, its, layered=False)
    assert resets > 0 or min(limit, PC.SHAPES[env_id][3]) >= Tn


def test_layered_rollout_matches_twin_collect():
    env_id, hid, E, Tn, limit = PC.LAYERED_CASE
    _, th, its = PC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert _check_against_collect(env_id, _layered_policy(env_id, hid, th), E, Tn, limit, its, layered=True) > 0


# ------------------------------------------------------------------ 4. persistent launch = step launches
@pytest.mark.parametrize("E,Tn,limit", PC.PERSISTENT_CASES)
@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_persistent_rollout_equals_step_launches(env_id, E, Tn, limit):
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(env_id)
    _, th = PC.policy_theta(env_id, [64, 64], 17)
    pol = _fused_policy(env_id, th)
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
def _replay(env_id, n, seed, limit, out):
    """The traced actions through a VecEnv (same seed, no auto-reset): (ret, len, flags)."""
    from modular_rl_amd.envs import VecEnv
    env = VecEnv(env_id, n, seed=seed, auto_reset=False)
    obs = env.reset().cpu().numpy().copy()
    alive = np.ones(n, dtype=bool)
    ret, length, flags = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    for t in range(limit):
        if not alive.any():
            break
        np.testing.assert_allclose(obs[alive], out["trace_obs"][t][alive], rtol=1e-5, atol=1e-5, err_msg=f"obs {t}")
        ob, rew, done, info = env.step(torch.as_tensor(out["trace_act"][t]).cuda())
        obs, rew, term = ob.cpu().numpy().copy(), rew.cpu().numpy(), info["terminated"].cpu().numpy()
        ret[alive] += rew[alive]
        ended = alive & (term | (t + 1 >= limit))
        length[ended] = t + 1
        flags[ended] = 1 | (term[ended].astype(np.uint8) << 1)
        alive &= ~ended
    assert not alive.any()
    return ret, length, flags


def _run_population(env_id, n, seed, limit, thetas, hid=(64, 64)):
    from modular_rl_amd.envs import PopulationRollout
    pop = PopulationRollout(env_id, n, seed=seed, timestep_limit=limit, hid_sizes=hid)
    assert (pop.pol is not None) == (tuple(hid) == (64, 64)) and pop.P == thetas.shape[1]
    out = pop(torch.as_tensor(thetas).cuda(), trace_steps=pop.limit)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}, pop


@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_population_rollout_replays_through_a_vecenv(env_id):
    n, limit, seed = PC.POP_N, PC.POP_LIMIT, PC.POP_SEEDS[env_id]
    out, _ = _run_population(env_id, n, seed, limit, PC.population(env_id, n, seed))
    ret, length, flags = _replay(env_id, n, seed, limit, out)
    np.testing.assert_array_equal(out["ret"], ret)
    np.testing.assert_array_equal(out["len"], length)
    np.testing.assert_array_equal(out["flags"], flags)
    np.testing.assert_array_equal(flags, np.ones(n, np.uint8))  # neither env ends by itself: all cut at 25
    assert (length == limit).all()


def test_population_rollout_runs_reacher_to_its_own_timelimit():
    env_id, n, seed = "Reacher-v2", PC.POP_N, PC.POP_SEEDS["Reacher-v2"]
    out, pop = _run_population(env_id, n, seed, None, PC.population(env_id, n, seed))
    assert pop.limit == 50
    ret, length, flags = _replay(env_id, n, seed, 50, out)
    np.testing.assert_array_equal(out["len"], np.full(n, 50, np.int32))
    np.testing.assert_array_equal(out["flags"], np.full(n, 3, np.uint8))
    np.testing.assert_array_equal(out["ret"], ret)
    np.testing.assert_array_equal(length, out["len"])
    np.testing.assert_array_equal(flags, out["flags"])


@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_small_net_kernel_is_bit_identical_to_the_64_64_kernel(env_id):
    """A 10-5 net through mrl_pop_rollout_mlp, and zero-padded to 64-64 through
    mrl_pop_rollout: every output and trace (tests/test_gpu_cem_small.py's comparison)."""
    O, A, _, _ = PC.SHAPES[env_id]
    n, limit, seed = PC.POP_N, PC.POP_LIMIT, PC.POP_SEEDS[env_id]
    th = PC.population(env_id, n, seed, hid=PC.SMALL_HID)
    small, _ = _run_population(env_id, n, seed, limit, th, hid=PC.SMALL_HID)
    pad = np.stack([cem_small_np.pad_to_64_64(t, O, PC.SMALL_HID, A, True) for t in th])
    big, _ = _run_population(env_id, n, seed, limit, pad)
    assert (small["len"] == limit).all() and np.abs(small["trace_act"]).max() > 0.0
    for k in ("ret", "len", "flags", "stat", "trace_obs", "trace_act", "trace_rew"):
        assert np.array_equal(big[k], small[k]), k


# ------------------------------------------------------------------ 6. end to end
def test_run_pg_cli_reacher_two_iterations(capsys):
    import run_pg
    run_pg.main(["--env", "Reacher-v2", "--n_iter", "2", "--n_envs", "256", "--horizon", "64", "--json",
                 "--gamma", "0.995", "--lam", "0.97", "--max_kl", "0.01"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for st in lines:
        assert all(np.isfinite(v) for v in st.values()), st
        assert round(st["NumEpBatch"] * st["EpLenMean"]) == 256 * 64
        assert st["EpLenMean"] <= 50
        assert 0.0 <= st["pol_kl_after"] <= 2 * 0.01 and "pol_surr_after" in st  # KL <= 2 max_kl
        assert st["EpRewMean"] < 0.0  # every step's reward is negative


def test_run_cem_algorithm_swimmer_two_generations():
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make("Swimmer-v2")
    cfg = dict(batch_size=64, n_iter=2, elite_frac=0.25, filter=1, seed=5, timestep_limit=40)
    agent = DeterministicAgent(env.observation_space, env.action_space, cfg)
    infos, ns = [], []

    def callback(info):
        infos.append(dict(info))
        ns.append(float(agent.filter_state[0]))

    run_cem_algorithm(env, agent, usercfg=cfg, callback=callback)
    assert len(infos) == 2
    total = 0
    for it, info in enumerate(infos):
        assert info["ys"].shape == (64,) and np.isfinite(info["ys"]).all() and np.isfinite(info["th"]).all()
        assert np.isfinite(info["std"]).all() and np.isfinite(info["ymean"])
        assert (info["len"] == 40).all()  # Swimmer never ends by itself
        total += int(info["len"].sum())
        assert ns[it] == total  # the filter count equals the steps taken
    assert np.isfinite(agent.filter_state.cpu().numpy()).all()
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
