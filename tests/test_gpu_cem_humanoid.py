"""The wave-per-candidate population rollout on Humanoid-v2 (mrl_pop_rollout_wave,
WavePopulationRollout, population_rollout): replayed step by step through a VecEnv, its actions
against a float64 forward within a derived f32 bound, shared theta / strides / repeat calls /
small populations, the public refusals, and run_cem_algorithm end to end at the reference
battery's hid_sizes 10,5.

A block holds four candidates (waves), so N = 70 leaves two dead waves in the last block; the
kernel has one path for every shape, the first layer apart (lane-spread inputs and a wave sum),
which every shape takes."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cem_humanoid_np as HN
from tests import cem_np, pop_cases
from tests.pop_cases import KEYS

pytestmark = pytest.mark.gpu

ENV = HN.ENV_ID
# seed 46, limit 24: the float64 twin on the CPU oracle envs (cem_humanoid_np.twin_episodes:
# oracle/rollout_np.Envs, the float64 forward on the clipped observations, population spread 0.1)
# ends 36 episodes by itself (lengths 14 .. 24) and cuts 34 at the limit; of seeds 40 .. 51 the
# one (with 44) furthest from the floor of 5 on both sides
HM_SEED, HM_N, HM_LIMIT, HM_SPREAD = 46, 70, 24, 0.1


def run_traced(hid, n, seed, limit, thetas, filter_state=None, shared=False):
    from modular_rl_amd.envs import WavePopulationRollout
    return pop_cases.run_traced(ENV, hid, n, seed, limit, thetas, filter_state, shared, cls=WavePopulationRollout)


def check_replay(n, seed, out, limit):
    pop_cases.check_replay(ENV, n, seed, out, limit)


def check_actions(hid, thetas, out, filter_state):
    return pop_cases.check_actions_bound(ENV, hid, thetas, out, filter_state)


@pytest.fixture(scope="module")
def hm_run():
    th = HN.population((10, 5), HM_N, HM_SEED, spread=HM_SPREAD)
    out, pop = run_traced((10, 5), HM_N, HM_SEED, HM_LIMIT, th)
    assert pop.P == th.shape[1] == 3944 and pop.limit == HM_LIMIT
    return th, out


@pytest.fixture(scope="module")
def hm_filter(hm_run):
    """A BatchZFilter state after 400 traced observation rows of the 10-5 run."""
    _, raw = hm_run
    rows = pop_cases.traced_rows(raw)
    assert len(rows) >= 300
    return pop_cases.filter_state_for(ENV, rows)


def test_replay(hm_run):
    _, out = hm_run
    term = (out["flags"] & 2) != 0
    print("humanoid 10-5: ended by themselves", int(term.sum()), "cut at the limit", int((~term).sum()),
          "len", out["len"].tolist())
    assert term.sum() >= 5 and (~term).sum() >= 5
    assert np.all(out["len"][~term] == HM_LIMIT)
    check_replay(HM_N, HM_SEED, out, HM_LIMIT)


@pytest.mark.parametrize("hid", [(10, 5), (), (64, 64), (7, 3, 5)])
def test_actions_against_float64(hid, hm_run, hm_filter):
    if hid == (10, 5):
        n, seed, limit = HM_N, HM_SEED, HM_LIMIT
        th, raw = hm_run
    else:
        n, seed, limit = 6, 31, 8
        th = HN.population(hid, n, seed, spread=HM_SPREAD)
        raw, pop = run_traced(hid, n, seed, limit, th)
        assert pop.P == th.shape[1]
    assert check_actions(hid, th, raw, None) >= n  # the pass-through branch (filter_state None)
    out, _ = run_traced(hid, n, seed, limit, th, filter_state=hm_filter)
    check_actions(hid, th, out, hm_filter)
    assert not np.array_equal(out["trace_act"], raw["trace_act"])  # the filter is live
    if hid != (10, 5):
        check_replay(n, seed, out, limit)


def test_shared_theta_equals_copies():
    n = 9
    th = HN.population((10, 5), 1, 11, spread=HM_SPREAD)[0]
    a, _ = run_traced((10, 5), n, 4, 12, th, shared=True)
    b, _ = run_traced((10, 5), n, 4, 12, np.repeat(th[None, :], n, axis=0))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert len(set(a["ret"].tolist())) > 1  # the envs' resets differ: the episodes are not one episode


def test_two_calls_give_the_same_bits():
    from modular_rl_amd.envs import WavePopulationRollout
    th = torch.as_tensor(HN.population((10, 5), 10, 2, spread=HM_SPREAD)).cuda()
    pop = WavePopulationRollout(ENV, 10, seed=9, timestep_limit=16)
    first = {k: v.clone() for k, v in pop(th).items()}
    assert int(pop.episodes_started.min()) == 1 and int(pop.episodes_started.max()) == 1
    pop.episodes_started.zero_()  # both calls draw the same resets
    second = pop(th)
    for k in ("ret", "len", "flags", "stat"):
        assert torch.equal(first[k], second[k]), k
    third = pop(th)  # the counter moved on: other resets
    assert int(pop.episodes_started.min()) == 2
    assert not torch.equal(first["stat"], third["stat"])


def test_row_stride_through_the_c_entry(hm_run):
    """A [N, P + 3] buffer viewed as [:, :P], ld_theta = P + 3, the pad NaN, equals the contiguous call."""
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import WavePopulationRollout
    th, want = hm_run
    N, P = th.shape
    buf = torch.full((N, P + 3), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :P] = torch.as_tensor(th).cuda()
    view = buf[:, :P]
    assert view.stride(0) == P + 3 and view.data_ptr() == buf.data_ptr()
    pop = WavePopulationRollout(ENV, N, seed=HM_SEED, timestep_limit=HM_LIMIT, hid_sizes=(10, 5))
    tobs, tact, trew = pop._trace_bufs(pop.limit)
    p = _lib.ptr
    io = _lib.PopIO(p(pop.ret), p(pop.len), p(pop.flags), p(pop.stat), pop.limit, p(tobs), p(tact), p(trew))
    hid = (ctypes.c_int32 * 2)(10, 5)
    _lib.call("mrl_pop_rollout_wave", ctypes.byref(pop.desc), ctypes.byref(pop._bufs), hid, 2, p(view), P + 3, None,
              ctypes.byref(io), _lib.stream())
    torch.cuda.synchronize()
    got = dict(ret=pop.ret, len=pop.len, flags=pop.flags, stat=pop.stat, trace_obs=tobs, trace_act=tact, trace_rew=trew)
    for k in KEYS:  # both trace buffers started as zeros: rows beyond len are equal too
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("n", [1, 5])
def test_small_populations_run_and_replay(n):
    th = HN.population((10, 5), n, 3, spread=HM_SPREAD)
    out, _ = run_traced((10, 5), n, 6, 12, th)
    check_replay(n, 6, out, 12)
    check_actions((10, 5), th, out, None)


def test_public_interface_and_refusals():
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import PopulationRollout, WavePopulationRollout, population_rollout
    with pytest.raises(_lib.MrlError, match="population_rollout"):
        PopulationRollout(ENV, 4, hid_sizes=(10, 5))
    pop = population_rollout(ENV, 4)
    assert type(pop) is WavePopulationRollout and pop.P == 3944 and pop.hid_sizes == (10, 5)
    assert isinstance(pop, PopulationRollout)
    hop = population_rollout("Hopper-v2", 4, hid_sizes=(10, 5))
    assert type(hop) is PopulationRollout and hop.P == 196
    assert population_rollout("Hopper-v2", 4).hid_sizes == (64, 64)
    with pytest.raises(_lib.MrlError):
        WavePopulationRollout(ENV, 4, hid_sizes=(65,))
    with pytest.raises(_lib.MrlError):
        WavePopulationRollout("Hopper-v2", 4, hid_sizes=(10, 5))


def run_cem_once(seed):
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make(ENV)
    cfg = dict(batch_size=16, n_iter=2, elite_frac=0.25, filter=1, seed=seed, hid_sizes=[10, 5], timestep_limit=20)
    agent = DeterministicAgent(env.observation_space, env.action_space, cfg)
    th0 = agent.get_flat().astype(np.float64)
    assert th0.size == 3944
    infos, ns = [], []

    def callback(info):
        infos.append(dict(info))
        ns.append(float(agent.filter_state[0]))

    run_cem_algorithm(env, agent, usercfg=cfg, callback=callback)
    return th0, infos, ns, agent


def test_run_cem_algorithm_end_to_end():
    from modular_rl_amd.cem import sample_population
    seed = 17
    th0, infos, ns, agent = run_cem_once(seed)
    assert len(infos) == 2
    mean, th_std, total = th0, np.ones(th0.size), 0
    for it, info in enumerate(infos):
        # std_decay_time = n_iter / 2; extra_std 0: the schedule is sqrt(elite variance)
        np.testing.assert_allclose(info["std"], cem_np.sample_std_of(th_std, 0.0, it, 1.0), rtol=1e-12, atol=0)
        pop = sample_population(mean, info["std"], 16, seed, it).cpu().numpy()  # the generation's own population
        assert pop.shape == (16, 3944)
        wm, wv, _ = cem_np.refit(pop, info["ys"], 4)
        np.testing.assert_allclose(info["th"], wm, rtol=1e-12, atol=1e-12 * np.abs(pop).max())
        mean, th_std = info["th"], wv
        assert info["len"].min() >= 1 and info["len"].max() <= 20 and np.all(np.isfinite(info["ys"]))
        total += int(info["len"].sum())
        assert ns[it] == total
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
    print("Humanoid-v2 CEM 10-5 ymean per generation:", [float(i["ymean"]) for i in infos])
    _, again, ns2, _ = run_cem_once(seed)
    for a, b in zip(infos, again):
        assert np.array_equal(a["th"], b["th"]) and np.array_equal(a["ys"], b["ys"])
    assert ns == ns2
