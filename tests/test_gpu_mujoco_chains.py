"""InvertedPendulum-v2 and InvertedDoublePendulum-v2 on the device, through every layer that
steps an env: VecEnv against the numpy twin (tests/mujoco_chains_np.py), the envs' own
terminations and the observed limit force, the fused rollout (step launches and the
persistent launch) and the layered rollout against oracle.rollout_np.collect on the twin, the
population rollout replayed through a VecEnv, and run_pg.py / run_cem_algorithm end to end.
tests/test_mujoco_chains_host.py proves that every compared state keeps 1e-6 clear of a
termination threshold, so the flags are held exactly."""
import json

import numpy as np
import pytest
import torch

from tests import chain_cases as CC
from tests import mujoco_chains_np as MC

pytestmark = pytest.mark.gpu


def _close(got, want, what, rew=False):
    tol = 1e-4 if rew else 1e-5  # test_rollout_matches_oracle's bounds
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=what)


def _state(vec, ns):
    return vec.env_state[:ns * vec.E].view(ns, vec.E).cpu().numpy().T


# ------------------------------------------------------------------ 1. step against the twin
@pytest.mark.parametrize("E,Tn,limit", CC.STEP_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_step_matches_twin(env_id, E, Tn, limit):
    from modular_rl_amd.envs import VecEnv
    vec = VecEnv(env_id, E, seed=CC.step_seed(E), timestep_limit=limit)
    ns = CC.NS[env_id]
    actions = CC.step_actions(env_id, E, Tn)
    assert (np.abs(actions) > CC.ACT_HIGH[env_id]).any()  # the control clamp is hit
    (obs0, state0), steps, _ = CC.reference_steps(env_id, E, Tn, limit)
    _close(vec.reset().cpu().numpy(), obs0, "reset obs")
    _close(_state(vec, ns), state0, "reset state")
    resets = 0
    for t, w in enumerate(steps):
        o, r, done, info = vec.step(actions[t])
        np.testing.assert_array_equal(info["ep_t"].cpu().numpy(), w["ep_t"], err_msg=f"ep_t {t}")
        np.testing.assert_array_equal(info["flags"].cpu().numpy(),
                                      w["last"].astype(np.uint8) | (w["term"].astype(np.uint8) << 1),
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
    assert resets > 0


# ------------------------------------------------------------------ 2. the envs' own terminations
# states one step short of the threshold, written into env_state (rows in both 64-env blocks)
# beside untouched rows: the pendulum at 0.19 rad and tipping, the double pendulum's tip at
# 1.017 and dropping
TERMINAL = {
    "InvertedPendulum-v2": ([3, 64, 69], [0.1, 0.19, 0.0, 1.0]),
    "InvertedDoublePendulum-v2": ([0, 63, 68], [0.1, 0.56, 0.0, 0.0, 1.5, 0.0]),
}
STOP_ROWS, STOP_STATE = [5, 66], [1.03, 0.0, 0.0, 0.0, 0.0, 0.0]  # double pendulum: 3 cm into the slider stop


def _terminal_setup(env_id, auto_reset):
    from modular_rl_amd.envs import VecEnv
    E, seed = 70, 19
    rows, s0 = TERMINAL[env_id]
    vec = VecEnv(env_id, E, seed=seed, auto_reset=auto_reset)
    vec.reset()
    ns = len(s0)
    st = vec.env_state.view(ns, E)
    st[:, rows] = torch.tensor(s0, dtype=torch.float64, device="cuda")[:, None]
    act = (0.3 * np.random.default_rng(2).standard_normal((E, 1))).astype(np.float32)
    act[rows] = 0.0
    if env_id == "InvertedDoublePendulum-v2":
        st[:, STOP_ROWS] = torch.tensor(STOP_STATE, dtype=torch.float64, device="cuda")[:, None]
        act[STOP_ROWS] = 1.0  # full control into the stop
    hit = np.zeros(E, dtype=bool)
    hit[rows] = True
    # the twin from the very same states: it ends exactly the written rows, clear of the threshold
    before = _state(vec, ns).copy()
    step = MC.ip_step if ns == 4 else MC.dp_step
    after, rew, done = step(before, act)
    assert np.array_equal(done, hit) and MC.margin(env_id, after).min() > CC.MARGIN
    assert not step(before, act, (MC.IP if ns == 4 else MC.DP).replace(frame_skip=0))[2].any()  # not ended before
    return vec, act, hit, ns, before, after, rew, seed


@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_env_termination_is_flagged_for_exactly_the_ending_rows(env_id):
    vec, act, hit, ns, before, after, rew, _ = _terminal_setup(env_id, auto_reset=False)
    o, r, done, info = vec.step(act)
    flags, state = info["flags"].cpu().numpy(), _state(vec, ns)
    np.testing.assert_array_equal(flags, np.where(hit, 3, 0).astype(np.uint8))
    np.testing.assert_array_equal(done.cpu().numpy(), hit)
    np.testing.assert_allclose(state, after, rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.cpu().numpy(), rew, rtol=0, atol=1e-8)
    want_obs = (MC.ip_obs if ns == 4 else MC.dp_obs)(after)
    np.testing.assert_allclose(o.cpu().numpy(), want_obs, rtol=0, atol=1e-8)
    np.testing.assert_array_equal(info["final_obs"].cpu().numpy()[hit], o.cpu().numpy()[hit])
    assert (state[~hit] != before[~hit]).any(axis=1).all()  # the other rows stepped on
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.ones(vec.E, dtype=np.int32))
    if ns == 6:  # the rows at the slider stop observe its force, clipped; every other row observes none
        got = o.cpu().numpy()
        assert (want_obs[STOP_ROWS, 8] == -10.0).all() and (state[STOP_ROWS, 0] > 1.0).all()
        np.testing.assert_array_equal(got[STOP_ROWS, 8], np.full(2, -10.0))
        rest = np.ones(vec.E, dtype=bool)
        rest[STOP_ROWS] = False
        assert (got[rest, 8] == 0.0).all() and (got[:, 9:] == 0.0).all()


@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_terminated_rows_come_back_as_fresh_episodes(env_id):
    vec, act, hit, ns, before, after, rew, seed = _terminal_setup(env_id, auto_reset=True)
    o, r, done, info = vec.step(act)
    np.testing.assert_array_equal(info["flags"].cpu().numpy(), np.where(hit, 3, 0).astype(np.uint8))
    twin = MC.ChainEnvs(env_id, vec.E, seed)
    twin.reset(np.arange(vec.E))
    twin.reset(np.nonzero(hit)[0])  # the rows' second episodes
    # a reset state is a multiply-add of a Philox uniform, or a Box-Muller normal of two:
    # equal up to the device's log / sin / cos
    np.testing.assert_allclose(_state(vec, ns)[hit], twin.state[hit], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(o.cpu().numpy()[hit], twin.obs()[hit], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), np.where(hit, 2, 1))
    np.testing.assert_array_equal(vec.env_int[:vec.E].cpu().numpy(), np.where(hit, 0, 1))
    want_fin = (MC.ip_obs if ns == 4 else MC.dp_obs)(after)[hit]
    np.testing.assert_allclose(info["final_obs"].cpu().numpy()[hit], want_fin, rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.cpu().numpy(), rew, rtol=0, atol=1e-8)


# ------------------------------------------------------------------ 3. rollout against the oracle's collect
def _fused_policy(env_id, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import MlpNet
    O, A, _, _ = CC.SHAPES[env_id]
    net = MlpNet(O, A, _lib.HEAD_GAUSS)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(A))


def _layered_policy(env_id, hid, th):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import LayeredMlpNet
    O, A, _, _ = CC.SHAPES[env_id]
    net = LayeredMlpNet(O, A, _lib.HEAD_GAUSS, hid)
    net.set_flat(th)
    return StochPolicyMLP(net, DiagGauss(A))


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


@pytest.mark.parametrize("E,Tn,limit,inject", CC.ROLLOUT_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_rollout_matches_twin_collect(env_id, E, Tn, limit, inject):
    """The fused rollout (64-64 policy, filter on) against oracle.rollout_np.collect on the
    twin, two iterations, with and without injected noise."""
    _, th, its = CC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    resets = _check_against_collect(env_id, _fused_policy(env_id, th), E, Tn, limit, its, layered=False)
    assert resets > 0 or limit >= Tn


def test_layered_rollout_matches_twin_collect():
    env_id, hid, E, Tn, limit = CC.LAYERED_CASE
    _, th, its = CC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert _check_against_collect(env_id, _layered_policy(env_id, hid, th), E, Tn, limit, its, layered=True) > 0


# ------------------------------------------------------------------ 4. persistent launch = step launches
# the limits cut inside the horizon and poles drop, so both reset paths are taken
@pytest.mark.parametrize("E,Tn,limit", CC.PERSISTENT_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
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
    assert int((outs[0][4].view(Tn, E)[:-1] & 1).sum()) > 0  # episodes ended and restarted


# ------------------------------------------------------------------ 5. population rollout
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_population_rollout_replays_through_a_vecenv(env_id):
    from modular_rl_amd.envs import PopulationRollout, VecEnv
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
    np.testing.assert_array_equal(out["ret"], ret)
    np.testing.assert_array_equal(out["len"], length)
    np.testing.assert_array_equal(out["flags"], flags)
    assert (flags == 3).any()  # some candidates dropped their pole inside the limit


# ------------------------------------------------------------------ 6. end to end
def test_run_pg_cli_inverted_pendulum_two_iterations(capsys):
    import run_pg
    run_pg.main(["--env", "InvertedPendulum-v2", "--n_iter", "2", "--n_envs", "256", "--horizon", "64", "--json",
                 "--gamma", "0.995", "--lam", "0.97", "--max_kl", "0.01"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for st in lines:
        assert all(np.isfinite(v) for v in st.values()), st
        assert round(st["NumEpBatch"] * st["EpLenMean"]) == 256 * 64
        assert 0.0 <= st["pol_kl_after"] <= 2 * 0.01 and "pol_surr_after" in st  # KL <= 2 max_kl
        assert 1.0 <= st["EpRewMean"] <= 64.0 and st["EpRewMean"] == pytest.approx(st["EpLenMean"])  # reward 1 a step


def test_run_cem_algorithm_double_pendulum_two_generations():
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make("InvertedDoublePendulum-v2")
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
        assert info["len"].min() >= 1 and info["len"].max() <= 1000
        assert (info["ys"] <= 10.0 * info["len"]).all()  # at most 10 a step
        total += int(info["len"].sum())
        assert ns[it] == total  # every step's observation went into the filter
    assert np.isfinite(agent.filter_state.cpu().numpy()).all()
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
