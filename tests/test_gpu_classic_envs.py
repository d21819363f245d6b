"""Pendulum-v0, MountainCar-v0 and Acrobot-v1 on the device, through every layer that
steps an env: VecEnv against the numpy twin (tests/classic_envs_np.py), the envs' own
terminations, the fused rollout (step launches and the persistent launch) and the layered
rollout against oracle.rollout_np.collect on the twin, the population rollout replayed
through a VecEnv, and run_pg.py / run_cem_algorithm end to end."""
import json

import numpy as np
import pytest
import torch

from tests import cem_np
from tests import classic_cases as CC
from tests import classic_envs_np as CE

pytestmark = pytest.mark.gpu


def _close(got, want, what, rew=False):
    tol = 1e-4 if rew else 1e-5  # test_rollout_matches_oracle's bounds
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=what)


def _state(vec, ns):
    return vec.env_state[:ns * vec.E].view(ns, vec.E).cpu().numpy().T


# ------------------------------------------------------------------ 1. step against the twin
# E = 7: one partial block; 150: three blocks, the last partial; the limits force auto-resets
@pytest.mark.parametrize("E,Tn,limit", [(7, 30, 12), (150, 24, 9)])
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_step_matches_twin(env_id, E, Tn, limit):
    from modular_rl_amd.envs import VecEnv
    seed = 4242 + E
    vec = VecEnv(env_id, E, seed=seed, timestep_limit=limit)
    envs = CE.ClassicEnvs(env_id, E, seed)
    ns, A = envs.ns, envs.A
    rng = np.random.default_rng(E)
    if vec.env.discrete:
        actions = rng.integers(0, 3, size=(Tn, E)).astype(np.int32)
        assert set(np.unique(actions)) == {0, 1, 2}
    else:
        actions = (3.0 * rng.standard_normal((Tn, E, A))).astype(np.float32)
        assert (np.abs(actions) > 2.0).any()  # the torque clamp is hit
    envs.reset(np.arange(E))
    _close(vec.reset().cpu().numpy(), envs.obs(), "reset obs")
    _close(_state(vec, ns), envs.state, "reset state")
    resets = 0
    for t in range(Tn):
        o, r, done, info = vec.step(actions[t])
        rew, dn = envs.step(actions[t])
        ept = envs.ep_t.copy()
        term = dn | (ept + 1 >= envs.max_steps)
        last = term | (ept + 1 >= limit)
        np.testing.assert_array_equal(info["ep_t"].cpu().numpy(), ept, err_msg=f"ep_t {t}")
        np.testing.assert_array_equal(info["flags"].cpu().numpy(), last.astype(np.uint8) | (term.astype(np.uint8) << 1),
                                      err_msg=f"flags {t}")
        np.testing.assert_array_equal(done.cpu().numpy(), last)
        np.testing.assert_array_equal(info["terminated"].cpu().numpy(), term)
        _close(r.cpu().numpy(), rew, f"rew {t}", rew=True)
        envs.ep_t = ept + 1
        if last.any():
            idx = np.nonzero(last)[0]
            _close(info["final_obs"].cpu().numpy()[idx], envs.obs()[idx], f"final obs {t}")
            envs.reset(idx)
            resets += len(idx)
        _close(o.cpu().numpy(), envs.obs(), f"obs {t}")
        _close(_state(vec, ns), envs.state, f"state {t}")
        np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), envs.ep_count)
    assert resets > 0


# ------------------------------------------------------------------ 2. the envs' own terminations
# random play almost never ends a MountainCar or Acrobot episode: states one step from the
# end are written into env_state (rows in both 64-env blocks), beside untouched rows
TERMINAL = {
    # env -> (rows, state, action, state after, obs after)
    "MountainCar-v0": ([3, 64, 69], [0.49, 0.06], 2, [0.55074844, 0.06074844], [0.55074844, 0.06074844]),
    "Acrobot-v1": ([0, 63, 68], [3.0, 0.0, 0.0, 0.0], 1, [2.98205784, 0.01400267, -0.18343727, 0.14511761], None),
}
WALL_ROWS, WALL_STATE = [5, 66], [-1.19, -0.07]  # MountainCar: stopped at the left wall, not done


def _terminal_setup(env_id, auto_reset):
    from modular_rl_amd.envs import VecEnv
    E, seed = 70, 19
    rows, s0, a, s1, _ = TERMINAL[env_id]
    vec = VecEnv(env_id, E, seed=seed, auto_reset=auto_reset)
    vec.reset()
    ns = len(s0)
    st = vec.env_state.view(ns, E)
    st[:, rows] = torch.tensor(s0, dtype=torch.float64, device="cuda")[:, None]
    act = np.random.default_rng(2).integers(0, 3, size=E).astype(np.int32)
    act[rows] = a
    if env_id == "MountainCar-v0":
        st[:, WALL_ROWS] = torch.tensor(WALL_STATE, dtype=torch.float64, device="cuda")[:, None]
        act[WALL_ROWS] = 0
    hit = np.zeros(E, dtype=bool)
    hit[rows] = True
    return vec, act, hit, ns, np.array(s1), seed


@pytest.mark.parametrize("env_id", ["MountainCar-v0", "Acrobot-v1"])
def test_env_termination_is_flagged_for_exactly_the_ending_rows(env_id):
    vec, act, hit, ns, s1, _ = _terminal_setup(env_id, auto_reset=False)
    before = _state(vec, ns).copy()
    o, r, done, info = vec.step(act)
    flags, rew, state = info["flags"].cpu().numpy(), r.cpu().numpy(), _state(vec, ns)
    np.testing.assert_array_equal(flags, np.where(hit, 3, 0).astype(np.uint8))
    np.testing.assert_array_equal(done.cpu().numpy(), hit)
    np.testing.assert_array_equal(rew, np.where(hit & (env_id == "Acrobot-v1"), 0.0, -1.0))
    np.testing.assert_allclose(state[hit], np.tile(s1, (hit.sum(), 1)), rtol=0, atol=1e-8)
    np.testing.assert_array_equal(info["final_obs"].cpu().numpy()[hit], o.cpu().numpy()[hit])
    assert (state[~hit] != before[~hit]).any(axis=1).all()  # the other rows stepped on
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.ones(vec.E, dtype=np.int32))
    if env_id == "MountainCar-v0":
        np.testing.assert_array_equal(state[WALL_ROWS], np.tile([-1.2, 0.0], (2, 1)))
        np.testing.assert_array_equal(o.cpu().numpy(), state)
    else:
        t1, t2 = s1[0], s1[1]
        np.testing.assert_allclose(o.cpu().numpy()[hit][0], [np.cos(t1), np.sin(t1), np.cos(t2), np.sin(t2), s1[2], s1[3]],
                                   rtol=0, atol=1e-8)


@pytest.mark.parametrize("env_id", ["MountainCar-v0", "Acrobot-v1"])
def test_terminated_rows_come_back_as_fresh_episodes(env_id):
    vec, act, hit, ns, s1, seed = _terminal_setup(env_id, auto_reset=True)
    o, r, done, info = vec.step(act)
    np.testing.assert_array_equal(info["flags"].cpu().numpy(), np.where(hit, 3, 0).astype(np.uint8))
    twin = CE.ClassicEnvs(env_id, vec.E, seed)
    twin.reset(np.arange(vec.E))
    twin.reset(np.nonzero(hit)[0])  # the rows' second episodes
    # the reset state is one multiply-add of a Philox uniform: equal up to its contraction
    np.testing.assert_allclose(_state(vec, ns)[hit], twin.state[hit], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(o.cpu().numpy()[hit], twin.obs()[hit], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.where(hit, 2, 1))
    np.testing.assert_array_equal(vec.env_int[:vec.E].cpu().numpy(), np.where(hit, 0, 1))
    fin = info["final_obs"].cpu().numpy()[hit]
    if env_id == "MountainCar-v0":
        np.testing.assert_allclose(fin, np.tile(s1, (hit.sum(), 1)), rtol=0, atol=1e-8)
    else:
        np.testing.assert_allclose(fin[:, 4:], np.tile(s1[2:], (hit.sum(), 1)), rtol=0, atol=1e-8)
    np.testing.assert_array_equal(r.cpu().numpy(), np.where(hit & (env_id == "Acrobot-v1"), 0.0, -1.0))


def test_pendulum_ends_only_at_its_time_limit():
    from modular_rl_amd.envs import VecEnv
    E = 5
    vec = VecEnv("Pendulum-v0", E, seed=8, timestep_limit=None)
    vec.reset()
    rng = np.random.default_rng(4)
    for t in range(200):
        _, r, done, info = vec.step((3.0 * rng.standard_normal((E, 1))).astype(np.float32))
        want = 3 if t == 199 else 0  # step 200: ended and terminated (TimeLimit)
        assert (info["flags"].cpu().numpy() == want).all(), t
        assert (info["ep_t"].cpu().numpy() == t).all()
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.full(E, 2))


# ------------------------------------------------------------------ 3. rollout against the oracle's collect
def _fused_policy(env_id, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import MlpNet
    O, A, disc, _ = CC.SHAPES[env_id]
    net = MlpNet(O, A, _lib.HEAD_SOFTMAX if disc else _lib.HEAD_GAUSS)
    net.set_flat(th)
    return StochPolicyMLP(net, Categorical(A) if disc else DiagGauss(A))


def _layered_policy(env_id, hid, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import LayeredMlpNet
    O, A, disc, _ = CC.SHAPES[env_id]
    net = LayeredMlpNet(O, A, _lib.HEAD_SOFTMAX if disc else _lib.HEAD_GAUSS, hid)
    net.set_flat(th)
    return StochPolicyMLP(net, Categorical(A) if disc else DiagGauss(A))


def _check_against_collect(env_id, pol, E, Tn, limit, its, layered):
    """test_rollout_matches_oracle's assertions and tolerances, over two iterations."""
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(env_id)
    col = Collector(env, pol, E, Tn, limit, filter=1, seed=CC.rollout_seeds(E)[1], use_graph=False)
    assert col.layered == layered
    resets = 0
    for want, fs, noise, _ in its:
        if noise is not None:
            col.set_noise(noise.reshape(Tn * E, -1) if not env.discrete else noise.reshape(-1))
        b = col.collect()
        np.testing.assert_array_equal(b.flags.cpu().numpy().reshape(Tn, E), want["flags"])
        np.testing.assert_array_equal(b.ep_t.cpu().numpy().reshape(Tn, E), want["ep_t"])
        np.testing.assert_allclose(b.obs.cpu().numpy().reshape(Tn, E, -1), want["obs"], rtol=1e-5, atol=1e-5)
        if env.discrete:
            np.testing.assert_array_equal(b.act.cpu().numpy().reshape(Tn, E), want["act"])
        else:
            np.testing.assert_allclose(b.act.cpu().numpy().reshape(Tn, E, -1), want["act"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(b.prob.cpu().numpy().reshape(Tn, E, -1), want["prob"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(b.rew.cpu().numpy().reshape(Tn, E), want["rew"], rtol=1e-4, atol=1e-4)
        (n, m, var), (nr, mr, vr) = col.filter_stats()
        assert n == fs.n and nr == fs.nr
        np.testing.assert_allclose(m, fs.M[:-1], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(mr, fs.M[-1], rtol=1e-5, atol=1e-6)
        resets += int((want["flags"][:-1] & 1).sum())
    return resets


@pytest.mark.parametrize("E,Tn,limit,inject", CC.ROLLOUT_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_rollout_matches_twin_collect(env_id, E, Tn, limit, inject):
    """The fused rollout (64-64 policy, filter on) against oracle.rollout_np.collect on the
    twin; the discrete actions exactly (tests/test_classic_envs_host.py keeps these seeds
    clear of sampling ties)."""
    _, th, its = CC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    resets = _check_against_collect(env_id, _fused_policy(env_id, th), E, Tn, limit, its, layered=False)
    assert resets > 0 or limit >= Tn


def test_layered_rollout_matches_twin_collect():
    env_id, hid, E, Tn, limit = CC.LAYERED_CASE
    _, th, its = CC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert _check_against_collect(env_id, _layered_policy(env_id, hid, th), E, Tn, limit, its, layered=True) > 0


# ------------------------------------------------------------------ 4. persistent launch = step launches
# the limits cut inside the horizon, so both take the auto-reset path; E = 8256 (129 blocks)
# takes the multi-round record merge
@pytest.mark.parametrize("env_id,E,Tn,limit", [
    ("Pendulum-v0", 100, 60, 25), ("MountainCar-v0", 100, 60, 25), ("Acrobot-v1", 100, 60, 25),
    ("Acrobot-v1", 8256, 8, 5)])
def test_persistent_rollout_equals_step_launches(env_id, E, Tn, limit):
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(env_id)
    _, th = CC.policy_theta(env_id, [64, 64], 17)
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
    assert int((outs[0][4].view(Tn, E)[:-1] & 1).sum()) > 0  # episodes were cut and restarted


# ------------------------------------------------------------------ 5. population rollout
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_population_rollout_replays_through_a_vecenv(env_id):
    from modular_rl_amd.envs import PopulationRollout, VecEnv
    O, A, disc, _ = CC.SHAPES[env_id]
    n, limit, seed = CC.POP_N, CC.POP_LIMIT, CC.POP_SEEDS[env_id]
    thetas = CC.population(env_id, n, seed)
    pop = PopulationRollout(env_id, n, seed=seed, timestep_limit=limit)
    out = pop(torch.as_tensor(thetas).cuda(), trace_steps=limit)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    env = VecEnv(env_id, n, seed=seed, auto_reset=False)
    obs = env.reset().cpu().numpy().copy()
    alive = np.ones(n, dtype=bool)
    ret, length, flags = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    rows = clear = 0
    for t in range(limit):
        if not alive.any():
            break
        np.testing.assert_allclose(obs[alive], out["trace_obs"][t][alive], rtol=1e-5, atol=1e-5, err_msg=f"obs {t}")
        if disc:  # the traced action is the float64 arg-max wherever the top two logits are apart
            z = cem_np.forward_64_64(thetas.astype(np.float64)[alive], cem_np.filter_obs(out["trace_obs"][t][alive]), A)
            srt = np.sort(z, axis=1)
            ok = (srt[:, -1] - srt[:, -2]) > 1e-4
            rows, clear = rows + len(z), clear + int(ok.sum())
            assert np.array_equal(out["trace_act"][t][alive][ok], np.argmax(z, axis=1)[ok]), t
        ob, rew, done, info = env.step(torch.as_tensor(out["trace_act"][t]).cuda())
        obs, rew, term = ob.cpu().numpy().copy(), rew.cpu().numpy(), info["terminated"].cpu().numpy()
        ret[alive] += rew[alive]
        ended = alive & (term | (t + 1 >= limit))
        length[ended] = t + 1
        flags[ended] = 1 | (term[ended].astype(np.uint8) << 1)
        alive &= ~ended
    assert not alive.any()
    np.testing.assert_array_equal(out["ret"], ret)
    np.testing.assert_array_equal(out["len"], length)
    np.testing.assert_array_equal(out["flags"], flags)
    if disc:
        assert {0, 1, 2} <= set(np.unique(out["trace_act"]).tolist())
        assert clear >= 0.95 * rows, (clear, rows)


# ------------------------------------------------------------------ 6. end to end
def test_run_pg_cli_pendulum_two_iterations(capsys):
    import run_pg
    run_pg.main(["--env", "Pendulum-v0", "--n_iter", "2", "--n_envs", "256", "--horizon", "64", "--json",
                 "--gamma", "0.995", "--lam", "0.97"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for st in lines:
        assert all(np.isfinite(v) for v in st.values()), st
        assert round(st["NumEpBatch"] * st["EpLenMean"]) == 256 * 64
        assert st["EpRewMean"] < 0.0  # Pendulum's reward is a cost


def test_run_cem_algorithm_acrobot_two_generations():
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make("Acrobot-v1")
    cfg = dict(batch_size=64, n_iter=2, elite_frac=0.25, filter=1, seed=5)
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
        assert info["len"].min() >= 1 and info["len"].max() <= 500
        assert (info["ys"] <= 0.0).all() and (info["ys"] >= -info["len"]).all()  # -1 a step, 0 for the last
        total += int(info["len"].sum())
        assert ns[it] == total  # every step's observation went into the filter
    assert np.isfinite(agent.filter_state.cpu().numpy()).all()
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
