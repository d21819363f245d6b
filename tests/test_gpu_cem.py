"""The cross-entropy method on the device: the population rollout replayed step by step
through a VecEnv, its actions against a float64 forward, the sampling and refit kernels
against numpy, and run_cem_algorithm end to end against the float64 twin."""
import numpy as np
import pytest
import torch

from tests import cem_np, pop_cases

pytestmark = pytest.mark.gpu

HID = (64, 64)  # mrl_pop_rollout
# seed 24: the float64 twin on the CPU oracle envs ends 61 episodes early and cuts 9 at the limit
HOPPER_SEED, HOPPER_N, HOPPER_LIMIT = 24, 70, 40
CARTPOLE_SEED, CARTPOLE_N = 5, 7


def population(env_id, n, seed, spread=0.5):
    return cem_np.population(env_id, HID, n, seed, spread)


def run_traced(env_id, n, seed, limit, thetas, filter_state=None, shared=False):
    return pop_cases.run_traced(env_id, HID, n, seed, limit, thetas, filter_state, shared)


@pytest.fixture(scope="module")
def hopper_run():
    th = population("Hopper-v2", HOPPER_N, HOPPER_SEED)
    out, _ = run_traced("Hopper-v2", HOPPER_N, HOPPER_SEED, HOPPER_LIMIT, th)
    return th, out


@pytest.fixture(scope="module")
def cartpole_run():
    th = population("CartPole-v0", CARTPOLE_N, CARTPOLE_SEED)
    out, _ = run_traced("CartPole-v0", CARTPOLE_N, CARTPOLE_SEED, 0, th)
    return th, out


def test_hopper_replay(hopper_run):
    _, out = hopper_run
    term = (out["flags"] & 2) != 0
    print("hopper: terminated", int(term.sum()), "cut at the limit", int((~term).sum()), "len", out["len"].tolist())
    assert term.sum() >= 5 and (~term).sum() >= 5
    assert np.all(out["len"][~term] == HOPPER_LIMIT)
    pop_cases.check_replay("Hopper-v2", HOPPER_N, HOPPER_SEED, out, HOPPER_LIMIT)


def test_cartpole_replay(cartpole_run):
    _, out = cartpole_run
    pop_cases.check_replay("CartPole-v0", CARTPOLE_N, CARTPOLE_SEED, out, 200)
    assert np.array_equal(out["ret"], out["len"].astype(np.float64))


def check_actions(env_id, thetas, out, filter_state):
    return pop_cases.check_actions(env_id, HID, thetas, out, filter_state)


@pytest.mark.parametrize("env_id", ["Hopper-v2", "CartPole-v0"])
def test_actions_against_float64(env_id, hopper_run, cartpole_run):
    hopper = env_id == "Hopper-v2"
    th, raw = hopper_run if hopper else cartpole_run
    n, seed, limit = (HOPPER_N, HOPPER_SEED, HOPPER_LIMIT) if hopper else (CARTPOLE_N, CARTPOLE_SEED, 0)
    # the pass-through branch (filter_state None): the fixtures' runs
    check_actions(env_id, th, raw, None)
    src = raw
    if not hopper:  # seven random CartPole policies give a few dozen rows: take them from a wider run
        src, _ = run_traced(env_id, 64, CARTPOLE_SEED + 1, 0, population(env_id, 64, CARTPOLE_SEED + 1))
    rows = pop_cases.traced_rows(src)
    assert len(rows) >= 300
    fs = pop_cases.filter_state_for(env_id, rows)
    out, _ = run_traced(env_id, n, seed, limit, th, filter_state=fs)
    # rows skipped for near-tied logits when this was written: CartPole 0 of 67 raw and 0 of 135 filtered
    check_actions(env_id, th, out, fs)
    assert not np.array_equal(out["trace_act"], raw["trace_act"])  # the filter is live


@pytest.mark.parametrize("env_id", ["Hopper-v2", "CartPole-v0"])
def test_shared_theta_equals_copies(env_id):
    n = 70
    th = population(env_id, 1, 11, spread=0.1)[0]
    a, _ = run_traced(env_id, n, 4, 25, th, shared=True)
    b, _ = run_traced(env_id, n, 4, 25, np.repeat(th[None, :], n, axis=0))
    for k in pop_cases.KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_two_calls_give_the_same_bits():
    from modular_rl_amd.envs import PopulationRollout
    th = torch.as_tensor(population("Hopper-v2", 70, 2)).cuda()
    pop = PopulationRollout("Hopper-v2", 70, seed=9, timestep_limit=30)
    first = {k: v.clone() for k, v in pop(th).items()}
    assert int(pop.episodes_started.min()) == 1
    pop.episodes_started.zero_()  # both calls draw the same resets
    second = pop(th)
    for k in ("ret", "len", "stat"):
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("P", [7, 4998])
def test_cem_sample_matches_philox_box_muller(P):
    from modular_rl_amd.cem import sample_population
    from oracle import philox
    N, seed, gen = 5, 1234, 3
    rng = np.random.default_rng(P)
    mean, std = rng.standard_normal(P), 0.1 + rng.random(P)
    got = sample_population(mean, std, N, seed, gen).cpu().numpy()
    z = philox.normals(seed, 2, np.arange(N, dtype=np.uint64), np.uint64(gen), P)
    want = (mean[None, :] + std[None, :] * z).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2 * ulp)
    other_gen = sample_population(mean, std, N, seed, gen + 1).cpu().numpy()
    other_seed = sample_population(mean, std, N, seed + 1, gen).cpu().numpy()
    assert not np.array_equal(got, other_gen) and not np.array_equal(got, other_seed)
    assert np.array_equal(got, sample_population(mean, std, N, seed, gen).cpu().numpy())


def test_cem_refit_matches_the_twin_on_the_golden_populations():
    import os
    from modular_rl_amd.cem import refit
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "cem.npz")) as z:
        g = {k: z[k] for k in z.files}
    for tag in ("a", "b"):
        for it in range(6):
            pop32 = g[f"{tag}_pops"][it].astype(np.float32)
            ys = g[f"{tag}_ys"][it]
            mean, var, idx = refit(torch.as_tensor(pop32).cuda(), ys, 6)
            wm, wv, widx = cem_np.refit(pop32, ys, 6)
            atol = 1e-12 * np.abs(pop32).max()
            assert np.array_equal(idx.cpu().numpy(), widx)
            assert np.array_equal(widx, np.argsort(ys)[-6:])  # no ties: the reference's order
            np.testing.assert_allclose(mean.cpu().numpy(), wm, rtol=1e-12, atol=atol)
            np.testing.assert_allclose(var.cpu().numpy(), wv, rtol=1e-12, atol=atol)


def test_cem_refit_ties_nan_and_stride():
    from modular_rl_amd.cem import refit
    rng = np.random.default_rng(0)
    N, P, ld = 9, 5, 8
    buf = torch.as_tensor(rng.standard_normal((N, ld)).astype(np.float32)).cuda()
    view = buf[:, :P]  # ld_theta = 8 > P
    #            0    1    2       3    4    5    6    7    8
    ys = np.array([3.0, 1.0, np.nan, 2.0, 2.0, 0.5, 5.0, 2.0, -1.0])
    # ascending in (y, index), NaN lowest: 2, 8, 5, 1, 3, 4, 7, 0, 6
    for n_elite, want in ((3, [7, 0, 6]), (4, [4, 7, 0, 6]), (5, [3, 4, 7, 0, 6]), (9, [2, 8, 5, 1, 3, 4, 7, 0, 6])):
        mean, var, idx = refit(view, ys, n_elite)
        assert idx.cpu().numpy().tolist() == want
        assert cem_np.elite_order(ys, n_elite).tolist() == want
        el = buf.cpu().numpy()[want, :P].astype(np.float64)
        np.testing.assert_allclose(mean.cpu().numpy(), el.mean(axis=0), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(var.cpu().numpy(), el.var(axis=0), rtol=1e-12, atol=1e-12)


def run_cem_once(seed):
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import run_cem_algorithm
    from modular_rl_amd.envs import make
    env = make("CartPole-v0")
    cfg = dict(batch_size=64, n_iter=3, elite_frac=0.25, filter=1, seed=seed)
    agent = DeterministicAgent(env.observation_space, env.action_space, cfg)
    th0 = agent.get_flat().astype(np.float64)
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
    assert len(infos) == 3
    mean, th_std, total = th0, np.ones(th0.size), 0
    for it, info in enumerate(infos):
        # std_decay_time = n_iter / 2; extra_std 0: the schedule is sqrt(elite variance)
        np.testing.assert_allclose(info["std"], cem_np.sample_std_of(th_std, 0.0, it, 1.5), rtol=1e-12, atol=0)
        pop = sample_population(mean, info["std"], 64, seed, it).cpu().numpy()  # the generation's own population
        wm, wv, _ = cem_np.refit(pop, info["ys"], 16)
        np.testing.assert_allclose(info["th"], wm, rtol=1e-12, atol=1e-12 * np.abs(pop).max())
        mean, th_std = info["th"], wv
        assert info["ys"].max() <= 200 and info["ys"].min() >= 1
        assert np.array_equal(info["ys"], info["len"].astype(np.float64))
        total += int(info["len"].sum())
        assert ns[it] == total
    np.testing.assert_array_equal(agent.get_flat(), infos[-1]["th"].astype(np.float32))
    print("CartPole-v0 CEM ymean per generation:", [float(i["ymean"]) for i in infos])
    _, again, ns2, _ = run_cem_once(seed)
    for a, b in zip(infos, again):
        assert np.array_equal(a["th"], b["th"]) and np.array_equal(a["ys"], b["ys"])
    assert ns == ns2


def test_negative_std_decay_time_from_the_command_line_means_half_the_iterations():
    """run_cem.py hands over every option, std_decay_time = -1.0 (its default) included: the
    extra variance must decay over n_iter / 2 generations.  Each generation's std is the
    schedule applied to the device refit of the generation before (the same kernel on the
    same inputs: the same bits; case 7 pins that refit to the twin)."""
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.cem import refit, run_cem_algorithm, sample_population
    from modular_rl_amd.envs import make
    env = make("CartPole-v0")
    cfg = dict(batch_size=64, n_iter=4, elite_frac=0.25, initial_std=1.0, extra_std=0.5, std_decay_time=-1.0,
               timestep_limit=0, parallel=0, filter=1, seed=3)
    agent = DeterministicAgent(env.observation_space, env.action_space, cfg)
    mean = agent.get_flat().astype(np.float64)
    infos = []
    run_cem_algorithm(env, agent, usercfg=cfg, callback=lambda info: infos.append(dict(info)))
    assert len(infos) == 4
    th_std = np.ones(mean.size)
    for it, info in enumerate(infos):
        want = cem_np.sample_std_of(th_std, 0.5, it, 4 / 2)
        assert np.array_equal(info["std"], want), it
        pop = sample_population(mean, info["std"], 64, 3, it)
        m, v, _ = refit(pop, info["ys"], 16)
        assert np.array_equal(m.cpu().numpy(), info["th"])
        mean, th_std = info["th"], v.cpu().numpy()
    # the schedule itself: 0.25 * (1, 1/2, 0, 0) added to the variance
    assert np.allclose(infos[0]["std"], np.sqrt(1.25)) and np.all(infos[1]["std"] > np.sqrt(0.125))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_cem_generator_on_the_golden_populations(tag):
    """cem(thetas=...) fed the reference's own populations and ys reproduces its th / std /
    ymean.  The populations enter as float32 (relative rounding eps = 2^-24 per entry), so
    th (a mean of entries) is off by at most eps max|theta|, the elite variance by at most
    2 |d| eps max|theta| <= 4 eps max|theta|^2 (|d| <= 2 max|theta|), and std = sqrt(var +
    extra) by that over 2 std; fp64 rounding is far below.  ymean passes through in fp64."""
    import os
    from modular_rl_amd.cem import cem
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "cem.npz")) as z:
        g = {k[2:]: z[k] for k in z.files if k.startswith(tag + "_")}
    batch, n_iter, elite_frac, initial_std, extra_std, decay = g["cfg"]
    calls = []

    def f(pop):
        assert tuple(pop.shape) == (24, 7) and pop.is_cuda and pop.dtype == torch.float32
        calls.append(len(calls))
        return torch.as_tensor(g["ys"][calls[-1]])

    infos = list(cem(f, g["th0"], int(batch), int(n_iter), elite_frac, initial_std, extra_std, decay,
                     thetas=g["pops"]))
    assert len(infos) == 6
    eps = 2.0 ** -24
    for it, info in enumerate(infos):
        top = np.abs(g["pops"][it]).max()
        np.testing.assert_array_equal(info["ys"], g["ys"][it])
        np.testing.assert_allclose(info["ymean"], g["ymean"][it], rtol=1e-12, atol=0)
        np.testing.assert_allclose(info["th"], g["th"][it], rtol=0, atol=1.01 * eps * top)
        prev = np.abs(g["pops"][it - 1]).max() if it else 0.0
        np.testing.assert_allclose(info["std"], g["std"][it], rtol=1e-12,
                                   atol=1.01 * 4 * eps * prev ** 2 / (2 * g["std"][it].min()))


def test_deterministic_agent_acts_filters_and_snapshots(tmp_path):
    from modular_rl_amd.agentzoo import DeterministicAgent
    from modular_rl_amd.checkpoint import load_snapshot, save_snapshot
    from modular_rl_amd.envs import make
    env = make("Hopper-v2")
    agent = DeterministicAgent(env.observation_space, env.action_space, dict(seed=1))
    rng = np.random.default_rng(0)
    ob = rng.standard_normal(11) * 3
    assert np.array_equal(agent.obfilt(ob), np.clip(ob, -5, 5))  # empty filter: clipped only
    fs = np.concatenate([[50.0, 0.0], rng.standard_normal(12), 50 * (0.5 + rng.random(12))])
    agent.filter_state.copy_(torch.as_tensor(fs))
    x = agent.obfilt(ob)
    np.testing.assert_allclose(x, cem_np.filter_obs(ob[None], fs)[0], rtol=1e-6, atol=1e-7)  # the twin rounds to f32
    act, info = agent.act(x)
    z = cem_np.forward_64_64(agent.get_flat(), x.astype(np.float32)[None], 3)[0]
    np.testing.assert_allclose(act, z, rtol=1e-4, atol=1e-5)
    assert agent.rewfilt(2.5) == 2.5
    path = save_snapshot(str(tmp_path / "det.npz"), agent, 7, "Hopper-v2")
    other = DeterministicAgent(env.observation_space, env.action_space, dict(seed=2))
    assert not np.array_equal(other.get_flat(), agent.get_flat())
    meta = load_snapshot(path, other)
    assert meta["counter"] == 7
    assert np.array_equal(other.get_flat(), agent.get_flat())
    assert torch.equal(other.filter_state, agent.filter_state)
    nofilter = DeterministicAgent(env.observation_space, env.action_space, dict(seed=2, filter=0))
    with pytest.raises(ValueError):
        load_snapshot(path, nofilter)
