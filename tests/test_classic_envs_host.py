"""Pendulum-v0, MountainCar-v0 and Acrobot-v1 without a GPU: the registry and the C ABI know
them, the numpy twin (tests/classic_envs_np.py) reproduces values worked out from the
equations by hand, its invariants hold, and the seeds the GPU tests use keep clear of
float-rounding ties."""
import ctypes

import numpy as np
import pytest

from tests import classic_cases as CC
from tests import classic_envs_np as CE

E_ARG, E_UNSUPPORTED = -1, -2


# ------------------------------------------------------------------ registry and ABI
@pytest.mark.parametrize("env_id,kind,obs,space,limit", [
    ("Pendulum-v0", 4, 3, ("box", 1, 2.0), 200), ("MountainCar-v0", 5, 2, ("discrete", 3), 200),
    ("Acrobot-v1", 6, 6, ("discrete", 3), 500)])
def test_registry_describes_the_env(env_id, kind, obs, space, limit):
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import Box, Discrete, make
    env = make(env_id)
    assert env.kind == kind == {4: _lib.ENV_PENDULUM, 5: _lib.ENV_MOUNTAINCAR, 6: _lib.ENV_ACROBOT}[kind]
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (obs,)
    assert env.obs_dim == obs and env.spec.max_episode_steps == limit and env.spec.id == env_id
    if space[0] == "box":
        assert isinstance(env.action_space, Box) and env.action_space.shape == (space[1],)
        np.testing.assert_array_equal(env.action_space.high, np.full(space[1], space[2], np.float32))
        np.testing.assert_array_equal(env.action_space.low, np.full(space[1], -space[2], np.float32))
        assert not env.discrete and env.act_dim == space[1]
    else:
        assert isinstance(env.action_space, Discrete) and env.action_space.n == space[1]
        assert env.discrete and env.act_dim == space[1]
    assert CC.SHAPES[env_id] == (obs, env.act_dim, env.discrete, limit)


@pytest.mark.parametrize("kind,ns,obs,noise_cols", [(4, 2, 3, 1), (5, 2, 2, 1), (6, 4, 6, 1)])
def test_abi_sizes(kind, ns, obs, noise_cols):
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert lib.mrl_env_state_doubles(kind) == ns
    assert lib.mrl_filter_doubles(kind) == 2 + 2 * (obs + 1)
    assert lib.mrl_record_doubles(kind) == 2 + 2 * (obs + 1)
    desc = _lib.RolloutDesc(kind, 10, 7, 200, 0, 0, 0, 0, 0)
    assert lib.mrl_rollout_noise_doubles(ctypes.byref(desc)) == 7 * 10 * noise_cols
    assert lib.mrl_rollout_sync_bytes(ctypes.byref(desc)) == 256 + 2 * (obs + 1) * 1 * 16


@pytest.mark.parametrize("entry", ["mrl_env_reset", "mrl_env_step"])
def test_env_entries_take_the_new_ids(entry):
    """env_id 4 passes the id check: with n_envs = 0 the complaint is about n_envs (the
    checks run before any HIP call); 3 and 7 are still no envs."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bufs = _lib.RolloutBufs(env_state=p, env_int=p)
    io = _lib.EnvIO(p, None, p, p, p, p, None)
    tail = (None,) if entry == "mrl_env_reset" else (1, None)
    for env_id, needle in ((4, "n_envs"), (5, "n_envs"), (6, "n_envs"), (3, "env_id"), (7, "env_id")):
        desc = _lib.RolloutDesc(env_id, 0, 1, 200, 0, 0, 0, 0, 0)
        rc = getattr(lib, entry)(ctypes.byref(desc), ctypes.byref(bufs), ctypes.byref(io), *tail)
        msg = lib.mrl_last_error().decode()
        assert rc == E_ARG and needle in msg, (env_id, rc, msg)
        assert needle == "env_id" or "env_id" not in msg, (env_id, msg)


def test_pop_rollout_wants_the_envs_own_net():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the check precedes the launch
    d = _lib.RolloutDesc(_lib.ENV_ACROBOT, 4, 1, 0, 0, 0, 0, 0, 0)
    b = _lib.RolloutBufs(env_state=fake, env_int=fake)
    io = _lib.PopIO(fake, fake, fake, fake)
    for pol in (_lib.MlpDesc(4, 2, _lib.HEAD_SOFTMAX, 64, 2),   # CartPole's net
                _lib.MlpDesc(6, 3, _lib.HEAD_GAUSS, 64, 2),     # the wrong head
                _lib.MlpDesc(6, 3, _lib.HEAD_SOFTMAX, 32, 1)):  # hid_sizes=[32]
        rc = lib.mrl_pop_rollout(ctypes.byref(d), ctypes.byref(b), ctypes.byref(pol), fake, 0, None, ctypes.byref(io),
                                 None)
        assert rc == E_UNSUPPORTED and b"mrl_pop_rollout" in lib.mrl_last_error()
    d.env_id = 3
    pol = _lib.MlpDesc(6, 3, _lib.HEAD_SOFTMAX, 64, 2)
    rc = lib.mrl_pop_rollout(ctypes.byref(d), ctypes.byref(b), ctypes.byref(pol), fake, 0, None, ctypes.byref(io), None)
    assert rc == E_ARG and b"env_id" in lib.mrl_last_error()


# ------------------------------------------------------------------ anchors
# worked out from the equations of the envs, outside the code under test
def test_pendulum_anchor():
    s, rew, done = CE.pendulum_step(np.array([[0.0, 0.0]]), np.array([[2.0]], dtype=np.float32))
    np.testing.assert_allclose(s[0], [0.015, 0.3], rtol=0, atol=1e-8)
    np.testing.assert_allclose(rew[0], -0.004, rtol=0, atol=1e-8)
    assert not done[0]


def test_mountaincar_anchors():
    s, rew, done = CE.mountaincar_step(np.array([[0.49, 0.06], [-1.19, -0.07]]), np.array([2, 0]))
    np.testing.assert_allclose(s[0], [0.55074844, 0.06074844], rtol=0, atol=1e-8)
    assert s[1, 0] == -1.2 and s[1, 1] == 0.0  # stopped at the left wall
    assert done.tolist() == [True, False] and rew.tolist() == [-1.0, -1.0]


def test_acrobot_anchor():
    s, rew, done = CE.acrobot_step(np.array([[3.0, 0.0, 0.0, 0.0]]), np.array([1]))
    np.testing.assert_allclose(s[0], [2.98205784, 0.01400267, -0.18343727, 0.14511761], rtol=0, atol=1e-8)
    assert done[0] and rew[0] == 0.0


# ------------------------------------------------------------------ invariants
def test_pendulum_reward_and_speed_stay_bounded():
    E, Tn = 1000, 200
    envs = CE.ClassicEnvs(CE.PENDULUM, E, 3)
    envs.reset(np.arange(E))
    assert (np.abs(envs.state[:, 0]) <= np.pi).all() and (np.abs(envs.state[:, 1]) <= 1.0).all()
    rng = np.random.default_rng(0)
    lo = -(np.pi ** 2 + 6.4 + 0.004)
    clipped = 0
    for _ in range(Tn):
        act = (2.0 * rng.standard_normal((E, 1))).astype(np.float32)
        clipped += int((np.abs(act) > 2.0).sum())
        rew, done = envs.step(act)
        assert not done.any()
        assert (rew <= 0.0).all() and (rew >= lo).all(), (rew.min(), rew.max())
        assert (np.abs(envs.state[:, 1]) <= 8.0).all()
        o = envs.obs()
        np.testing.assert_allclose(o[:, 0] ** 2 + o[:, 1] ** 2, 1.0, rtol=0, atol=1e-12)
    assert clipped > 0 and (np.abs(envs.state[:, 1]) == 8.0).any()  # both clamps were reached


def test_acrobot_hangs_still_without_torque():
    s = np.zeros((3, 4))
    for _ in range(500):
        s, rew, done = CE.acrobot_step(s, np.array([1, 1, 1]))
        assert not done.any() and (rew == -1.0).all()
    assert (s == 0.0).all()
    np.testing.assert_array_equal(CE.acrobot_obs(s), np.tile([1.0, 0.0, 1.0, 0.0, 0.0, 0.0], (3, 1)))


def test_mountaincar_stays_in_its_box_and_acrobot_in_its_limits():
    E = 200
    rng = np.random.default_rng(1)
    mc, ac = CE.ClassicEnvs(CE.MOUNTAINCAR, E, 5), CE.ClassicEnvs(CE.ACROBOT, E, 5)
    mc.reset(np.arange(E)), ac.reset(np.arange(E))
    assert (mc.state[:, 1] == 0.0).all() and (mc.state[:, 0] >= -0.6).all() and (mc.state[:, 0] < -0.4).all()
    assert (np.abs(ac.state) <= 0.1).all()
    for _ in range(200):
        mc.step(rng.integers(0, 3, E)), ac.step(rng.integers(0, 3, E))
        assert (mc.state[:, 0] >= -1.2).all() and (mc.state[:, 0] <= 0.6).all() and (np.abs(mc.state[:, 1]) <= 0.07).all()
        assert (np.abs(ac.state[:, :2]) <= np.pi).all()
        assert (np.abs(ac.state[:, 2]) <= 4 * np.pi).all() and (np.abs(ac.state[:, 3]) <= 9 * np.pi).all()


def test_twin_has_the_oracle_envs_duck_type():
    from oracle import rollout_np as RO
    ref = RO.Envs(RO.CARTPOLE, 3, 0)
    for kind in (CE.PENDULUM, CE.MOUNTAINCAR, CE.ACROBOT):
        e = CE.ClassicEnvs(kind, 3, 0, env_offset=2)
        for name in ("kind", "E", "seed", "gid", "ns", "O", "A", "max_steps", "nu", "state", "ep_t", "ep_count"):
            assert type(getattr(e, name)) is type(getattr(ref, name)), name
        assert e.nu % 2 == 0 and e.gid.tolist() == [2, 3, 4]
        e.reset(np.arange(3))
        assert e.obs().shape == (3, e.O) and e.state.shape == (3, e.ns) and e.ep_count.tolist() == [1, 1, 1]


# ------------------------------------------------------------------ the GPU tests' seeds
@pytest.mark.parametrize("env_id", ["MountainCar-v0", "Acrobot-v1"])
@pytest.mark.parametrize("E,Tn,limit,inject", CC.ROLLOUT_CASES)
def test_rollout_seeds_keep_clear_of_sampling_ties(env_id, E, Tn, limit, inject):
    """The GPU rollout test asks for the twin's exact discrete actions: on its seeds no
    cumulative probability lies within 1e-6 of the uniform it is compared with, and all
    three actions are drawn."""
    _, _, its = CC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    seen = set()
    for want, _, _, margin in its:
        assert margin.min() > 1e-6, margin.min()
        seen |= set(np.unique(want["act"]).tolist())
    assert seen == {0, 1, 2}


def test_layered_seed_keeps_clear_of_sampling_ties():
    env_id, hid, E, Tn, limit = CC.LAYERED_CASE
    _, _, its = CC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert min(m.min() for _, _, _, m in its) > 1e-6
    assert any((w["flags"][:-1] & 1).any() for w, _, _, _ in its)  # the limit cuts inside the horizon


@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_population_seed_has_clear_arg_max_rows(env_id):
    rows, clear = CC.reference_population(env_id)
    assert rows >= CC.POP_N * 5 and clear >= 0.95 * rows, (rows, clear)
