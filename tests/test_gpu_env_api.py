"""GPU tests of the stand-alone env stepper (VecEnv on mrl_env_reset / mrl_env_step) and
obs filter (BatchZFilter on mrl_obfilter_update_apply): bit-for-bit replay of a layered
Collector's rollout, parity with the float64 oracle, masked reset, auto_reset=False,
the filter alone, and the gym-shaped single env."""
import numpy as np
import pytest
import torch

from oracle import rollout_np as RO
from oracle import trpo_np as T

pytestmark = pytest.mark.gpu

KINDS = {"CartPole-v0": RO.CARTPOLE, "Hopper-v2": RO.HOPPER, "Humanoid-v2": RO.HUMANOID}


def _layered_policy(head, nin, nout, hid, seed, logstd0=-0.5):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import LayeredMlpNet
    rng = np.random.default_rng(seed)
    spec = T.Spec(nin, hid, nout, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.02 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-nout:] = logstd0 + 0.1 * rng.standard_normal(nout)
    th = th.astype(np.float32).astype(np.float64)
    net = LayeredMlpNet(nin, nout, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, hid)
    net.set_flat(th)
    pt = DiagGauss(nout) if head == "gauss" else Categorical(nout)
    return StochPolicyMLP(net, pt)


def _collector(env_id, hid, E, Tn, limit, seed):
    from modular_rl_amd.collector import Collector
    from modular_rl_amd.envs import make
    env = make(env_id)
    pol = _layered_policy("softmax" if env.discrete else "gauss", env.obs_dim, env.act_dim, hid, seed=E)
    col = Collector(env, pol, E, Tn, limit, filter=1, seed=seed, use_graph=False)
    assert col.layered
    return env, col


def _eq(got, want, what):
    assert torch.equal(got, want), what


# ------------------------------------------------------------------ 1. replay
# E = 7: one partial block; 150: three blocks, the last partial; 130: not a multiple of 4
# (the WPB = 4 tail waves); limits 12 / 6 cut episodes, CartPole also terminates.  The two
# wide cases are the C3 / C5 env counts (64 and 16 filter blocks, every CU busy) with a
# limit that cuts inside the short horizon.
@pytest.mark.parametrize("env_id,hid,E,Tn,limit", [
    ("Hopper-v2", [64, 64], 150, 24, 1000),
    ("CartPole-v0", [32], 7, 30, 12),
    ("Humanoid-v2", [64, 64], 130, 30, 6),
    ("Hopper-v2", [64, 64], 4096, 12, 5),
    ("Humanoid-v2", [64, 64], 1024, 12, 5),
])
def test_replay_equals_layered_rollout(env_id, hid, E, Tn, limit):
    """A VecEnv + BatchZFilter driven with a layered Collector's recorded actions gives the
    Collector's rows back bit for bit: filtered observations, rewards, episode counters,
    flags (the Collector's horizon cut at T-1 aside) and the running stat."""
    from modular_rl_amd.envs import VecEnv
    from modular_rl_amd.filters import BatchZFilter
    seed = 777 + E
    env, col = _collector(env_id, hid, E, Tn, limit, seed)
    col.collect()
    O = env.obs_dim
    obs = col.obs.view(Tn, E, O)
    act = col.act.view(Tn, E) if env.discrete else col.act.view(Tn, E, env.act_dim)
    rew, flags, ep_t = col.rew.view(Tn, E), col.flags.view(Tn, E), col.ep_t.view(Tn, E)

    vec = VecEnv(env_id, E, seed=seed, timestep_limit=limit)
    filt = BatchZFilter(O, E)
    _eq(filt(vec.reset()), obs[0], "obs 0")
    resets = 0
    for t in range(Tn):
        o, r, done, info = vec.step(act[t])
        _eq(r.float(), rew[t], f"rew {t}")
        _eq(info["ep_t"], ep_t[t], f"ep_t {t}")
        if t < Tn - 1:
            _eq(info["flags"], flags[t], f"flags {t}")
            _eq(done, (flags[t] & 1) != 0, f"done {t}")
            resets += int(done.sum())
            _eq(filt(o), obs[t + 1], f"obs {t + 1}")
        else:
            _eq(info["flags"] & 2, flags[t] & 2, f"terminated {t}")
    assert resets > 0  # the auto-reset path ran
    # the running stat as far as the Collector has merged it: the obs of steps 0 .. T-1
    FS, D = col.FS, O + 1
    want = col.filter_state[:FS]
    _eq(filt.state[0], want[0], "n")
    _eq(filt.state[2:2 + O], want[2:2 + O], "M")
    _eq(filt.state[2 + D:2 + D + O], want[2 + D:2 + D + O], "S")
    assert filt.n == Tn * E


# ------------------------------------------------------------------ 2. oracle
def _close(env_id, got, want, what, rew=False):
    if env_id == "Humanoid-v2":  # test_humanoid_step_matches_oracle_twin's measure and bound
        rel = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-6)).max())
        assert rel <= 1e-7, (what, rel)
    else:  # test_rollout_matches_oracle's
        tol = 1e-4 if rew else 1e-5
        np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=what)


@pytest.mark.parametrize("env_id,E,Tn,limit", [
    ("Humanoid-v2", 96, 40, 1000), ("Hopper-v2", 150, 24, 9), ("CartPole-v0", 7, 30, 12)])
def test_step_matches_oracle(env_id, E, Tn, limit):
    """VecEnv against oracle.rollout_np.Envs on the same random actions: episode counters
    and flags exact; state, observation, final observation and reward within the bounds
    the rollout kernels are held to."""
    from modular_rl_amd.envs import VecEnv
    seed = 4242 + E
    vec = VecEnv(env_id, E, seed=seed, timestep_limit=limit)
    envs = RO.Envs(KINDS[env_id], E, seed)
    ns, A = envs.ns, envs.A
    rng = np.random.default_rng(E)
    if vec.env.discrete:
        actions = rng.integers(0, 2, size=(Tn, E)).astype(np.int32)
    else:
        actions = (0.4 * rng.standard_normal((Tn, E, A))).astype(np.float32)

    def state():
        return vec.env_state[:ns * E].view(ns, E).cpu().numpy().T

    envs.reset(np.arange(E))
    _close(env_id, vec.reset().cpu().numpy(), envs.obs(), "reset obs")
    _close(env_id, state(), envs.state, "reset state")
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
        _close(env_id, r.cpu().numpy(), rew, f"rew {t}", rew=True)
        envs.ep_t = ept + 1
        if last.any():
            idx = np.nonzero(last)[0]
            _close(env_id, info["final_obs"].cpu().numpy()[idx], envs.obs()[idx], f"final obs {t}")
            envs.reset(idx)
            resets += len(idx)
        _close(env_id, o.cpu().numpy(), envs.obs(), f"obs {t}")
        _close(env_id, state(), envs.state, f"state {t}")
        np.testing.assert_array_equal(vec.episodes_started.cpu().numpy(), envs.ep_count)
    assert resets > 0


# ------------------------------------------------------------------ 3. masked reset, auto_reset=False
def test_masked_reset_touches_only_the_masked_envs():
    from modular_rl_amd.envs import VecEnv
    E, seed = 70, 91
    vec = VecEnv("CartPole-v0", E, seed=seed)
    envs = RO.Envs(RO.CARTPOLE, E, seed)
    envs.reset(np.arange(E))
    vec.reset()
    rng = np.random.default_rng(3)
    for _ in range(5):
        a = rng.integers(0, 2, size=E)
        _, _, done, _ = vec.step(a)
        envs.step(a)
        envs.ep_t += 1
        assert not bool(done.any())
    mask = np.arange(E) % 3 == 0
    state0 = vec.env_state.view(4, E).clone()
    obs0, int0 = vec.obs.clone(), vec.env_int.view(2, E).clone()
    obs = vec.reset(torch.as_tensor(mask))
    state1, int1 = vec.env_state.view(4, E), vec.env_int.view(2, E)
    m = torch.as_tensor(mask).cuda()
    # unmasked envs: state rows, obs rows and counters bit-unchanged
    _eq(state1[:, ~m], state0[:, ~m], "unmasked state")
    _eq(obs[~m], obs0[~m], "unmasked obs")
    _eq(int1[:, ~m], int0[:, ~m], "unmasked counters")
    # masked envs: a new episode each
    assert bool((state1[:, m] != state0[:, m]).any(dim=0).all())
    assert bool((obs[m] != obs0[m]).any(dim=1).all())
    _eq(int1[0, m], torch.zeros_like(int0[0, m]), "masked ep_t")
    _eq(int1[1, m], int0[1, m] + 1, "masked episode counter")
    idx = np.nonzero(mask)[0]
    envs.reset(idx)
    # the reset state is one multiply-add of a Philox uniform: equal up to its contraction
    np.testing.assert_allclose(obs.cpu().numpy()[idx], envs.obs()[idx], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(int1.cpu().numpy(), np.stack([envs.ep_t, envs.ep_count]))
    with pytest.raises(ValueError):
        vec.reset(np.ones(E + 1, dtype=bool))


def test_auto_reset_off_leaves_ended_envs_alone():
    """Twin envs on the same actions, one with auto_reset: until an env's first episode end
    they agree bit for bit; at that step the twin without auto_reset returns the ending
    observation (the other's final_obs), keeps its episode counter and goes on counting."""
    from modular_rl_amd.envs import VecEnv
    E, seed, limit, Tn = 70, 17, 12, 14
    a_env = VecEnv("CartPole-v0", E, seed=seed, timestep_limit=limit, auto_reset=True)
    b_env = VecEnv("CartPole-v0", E, seed=seed, timestep_limit=limit, auto_reset=False)
    _eq(a_env.reset(), b_env.reset(), "reset")
    rng = np.random.default_rng(5)
    # half the envs push one way until the pole falls (terminated), the others balance at random
    push = torch.as_tensor(np.arange(E) % 2 == 0).cuda()
    alive = torch.ones(E, dtype=torch.bool, device="cuda")
    seen_term = seen_cut = 0
    for t in range(Tn):
        act = torch.where(push, 1, torch.as_tensor(rng.integers(0, 2, size=E)).cuda()).int()
        oa, ra, da, ia = a_env.step(act)
        ob, rb, db, ib = b_env.step(act)
        _eq(ib["ep_t"], torch.full_like(ib["ep_t"], t), f"b never restarts {t}")
        _eq(b_env.episodes_started, torch.ones_like(b_env.episodes_started), f"b's episode counter {t}")
        _eq(ia["flags"][alive], ib["flags"][alive], f"flags {t}")
        _eq(ra[alive], rb[alive], f"rew {t}")
        first = alive & db
        _eq(ia["final_obs"][first], ob[first], f"final obs {t}")
        _eq(ib["final_obs"][first], ob[first], f"b's own final obs {t}")
        if bool(first.any()):
            assert bool((oa[first] != ob[first]).any(dim=1).all())  # a's rows are the new episodes'
            _eq(a_env.episodes_started[first], torch.full_like(a_env.episodes_started[first], 2), f"a reset {t}")
        seen_term += int((first & ib["terminated"]).sum())
        seen_cut += int((first & ~ib["terminated"]).sum())
        alive = alive & ~db
        _eq(oa[alive], ob[alive], f"obs {t}")
    assert seen_term > 0 and seen_cut > 0 and not bool(alive.any())


def test_step_rejects_wrong_actions():
    from modular_rl_amd.envs import VecEnv
    cp, hp = VecEnv("CartPole-v0", 5), VecEnv("Hopper-v2", 5)
    cp.reset(), hp.reset()
    for bad in (np.zeros(4, dtype=np.int64), np.zeros((5, 1), dtype=np.int64), np.zeros(5, dtype=np.float32)):
        with pytest.raises(ValueError):
            cp.step(bad)
    for bad in (np.zeros((5, 2), dtype=np.float32), np.zeros(5, dtype=np.float32), np.zeros((5, 3), dtype=np.int64)):
        with pytest.raises(ValueError):
            hp.step(bad)
    cp.step([0, 1, 0, 1, 1])
    hp.step(np.zeros((5, 3)))


# ------------------------------------------------------------------ 4. the filter alone
@pytest.mark.parametrize("dim,n", [(376, 130), (4, 7)])
def test_filter_matches_oracle(dim, n, monkeypatch):
    from modular_rl_amd.filters import BatchZFilter
    monkeypatch.setattr(RO, "BLOCK", 64)  # the device's block of rows
    rng = np.random.default_rng(dim + n)
    scale, shift = 0.5 + rng.random(dim), 3.0 * rng.standard_normal(dim)
    filt = BatchZFilter(dim, n)
    fn, fM, fS = 0.0, np.zeros(dim), np.zeros(dim)
    for it in range(3):
        x = rng.standard_normal((n, dim)) * scale + shift
        x[:, dim - 1] = 0.25  # a constant column: variance 0
        if it == 2:
            x = x[:n - 3]  # a shorter batch than n_rows
        recs = RO._block_partials(x)
        bn, bm, bs = RO._batch(recs, lambda v: v, lambda r: r[0])
        fn, fM, fS = RO._merge(fn, fM, fS, bn, bm, bs)
        var = fS / (fn - 1) if fn > 1 else fM ** 2
        want = np.clip((x - fM) / (np.sqrt(var) + 1e-8), -5.0, 5.0).astype(np.float32)
        got = filt(torch.as_tensor(x).cuda()).cpu().numpy()
        assert filt.n == fn
        np.testing.assert_allclose(filt.mean, fM, rtol=1e-12, atol=0)
        np.testing.assert_allclose(filt.state[2 + dim + 1:2 + dim + 1 + dim].cpu().numpy(), fS, rtol=1e-12, atol=0)
        np.testing.assert_allclose(filt.var, var, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    # update=False: the state bit-unchanged, the same normalisation
    before = filt.state.clone()
    x = rng.standard_normal((n, dim)) * scale + shift
    got = filt(torch.as_tensor(x).cuda(), update=False).cpu().numpy()
    _eq(filt.state, before, "state after update=False")
    want = np.clip((x - fM) / (np.sqrt(var) + 1e-8), -5.0, 5.0).astype(np.float32)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        filt(torch.zeros(n + 1, dim, dtype=torch.float64))


def test_filter_from_collector_state():
    """A BatchZFilter started from a Collector's filter_state (cloned: the Collector's is
    not disturbed) normalises the next iteration's step-0 rows as the Collector does."""
    from modular_rl_amd.envs import VecEnv
    from modular_rl_amd.filters import BatchZFilter
    env_id, E, Tn, seed = "Hopper-v2", 150, 3, 55
    env, col = _collector(env_id, [64, 64], E, Tn, 1000, seed)
    col.collect()
    torch.cuda.synchronize()
    src = col.filter_state[:col.FS]
    src0 = src.clone()
    filt = BatchZFilter(env.obs_dim, E, state=src)
    assert filt.n == Tn * E
    # the rows the Collector's next reset draws: same seed, same episode counters
    vec = VecEnv(env_id, E, seed=seed)
    vec.env_int.copy_(col.env_int)
    raw = vec.reset().clone()
    frozen = filt(raw, update=False).clone()
    _eq(filt.state, src0, "update=False")
    got = filt(raw).clone()
    _eq(col.filter_state[:col.FS], src0, "the Collector's state")
    col.collect()
    want = col.obs[:E]
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-6)
    _eq(got, want, "same rows, same order: the same bits")
    # without the merge the normalisation is the previous iteration's
    assert not torch.equal(frozen, want)


# ------------------------------------------------------------------ 5. gym-shaped single env
def test_single_env_is_gym_shaped():
    from modular_rl_amd.envs import make
    seed = 31
    env = make("CartPole-v0")
    env.seed(seed)
    envs = RO.Envs(RO.CARTPOLE, 1, seed)
    envs.reset(np.arange(1))
    ob = env.reset()
    assert isinstance(ob, np.ndarray) and ob.shape == (4,) and ob.dtype == np.float64
    np.testing.assert_allclose(ob, envs.obs()[0], rtol=1e-5, atol=1e-5)
    ob0 = ob.copy()
    for t in range(12):
        a = 1 if t % 3 != 1 else 0
        ob, r, d, info = env.step(a)
        assert isinstance(ob, np.ndarray) and ob.shape == (4,)
        assert isinstance(r, float) and isinstance(d, bool) and info == {}
        rew, done = envs.step(np.array([a]))
        np.testing.assert_allclose(ob, envs.obs()[0], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(r, rew[0], rtol=1e-4, atol=1e-4)
        assert d == bool(done[0])
    # vec(): the batched twin; its env 0 starts where the single env did
    batch = env.vec(3, seed=seed)
    assert tuple(batch.reset().shape) == (3, 4)
    np.testing.assert_array_equal(batch.obs[0].cpu().numpy(), ob0)
