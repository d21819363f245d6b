"""Env registry for the device env steppers (replaces ``gym.envs.make``, run_pg.py:85).

The dynamics live in ``csrc/envs.h`` / ``csrc/envs_classic.h`` / ``csrc/envs_chains.h`` / ``csrc/envs_planar.h`` / ``csrc/envs_tree.h`` / ``csrc/humanoid.h`` and run inside the rollout
kernels; this module describes them with gym-compatible spaces / spec so that
``TrpoAgent(env.observation_space, env.action_space, cfg)`` and
``env.spec.max_episode_steps`` (run_pg.py:103-108) work unchanged, and ``VecEnv`` steps
them with the caller's own actions (``mrl_env_reset`` / ``mrl_env_step``).

* ``CartPole-v0`` -- gym's classic-control CartPole equations, TimeLimit 200.
* ``Hopper-v2``   -- gym's hopper.xml as articulated rigid-body dynamics (obs 11, act 3, TimeLimit 1000);
  MuJoCo is not available, so its dynamics are a stand-in.
* ``Humanoid-v2`` -- Humanoid-v2-SHAPED surrogate (obs 376, act 17 in [-0.4, 0.4],
  TimeLimit 1000); its 376-d obs needs the layered rollout (collector.py).
* ``Pendulum-v0``, ``MountainCar-v0``, ``Acrobot-v1`` -- gym's classic-control equations
  (``csrc/envs_classic.h``): a 1-d torque in [-2, 2] (TimeLimit 200, never done by itself),
  three discrete actions (TimeLimit 200) and three discrete torques (TimeLimit 500).
* ``InvertedPendulum-v2``, ``InvertedDoublePendulum-v2`` -- gym's cart-and-pole XML models as
  2- / 3-dof rigid-body chains (``csrc/envs_chains.h``: RK4, penalty joint limits): obs 4 / 11,
  one slider force in [-3, 3] / [-1, 1], TimeLimit 1000; done at |angle| > 0.2 / tip height <= 1.
  MuJoCo is not available, so their dynamics are a stand-in like Hopper's.
* ``Reacher-v2``, ``Swimmer-v2`` -- gym's planar chains without contact (``csrc/envs_planar.h``):
  a two-link arm with a goal drawn at reset and kept in the env state (obs 11, two torques in
  [-1, 1], TimeLimit 50, never done by itself), and a free-floating three-link chain in a fluid
  (obs 8, two torques in [-1, 1], TimeLimit 1000, never done by itself); stand-ins like the above.
* ``HalfCheetah-v2`` -- gym's planar tree of seven bodies, two legs on one torso, with Hopper's
  compliant ground contact and passive joint springs (``csrc/envs_tree.h``: the dynamics over a
  model table with a parent index per body): obs 17, six torques in [-1, 1], TimeLimit 1000,
  never done by itself; a stand-in like the above.
"""
import ctypes

import numpy as np
import torch

from . import _lib


class Box:
    def __init__(self, low, high, shape):
        self.shape = tuple(shape)
        self.low = np.full(self.shape, low, dtype=np.float32)
        self.high = np.full(self.shape, high, dtype=np.float32)

    def __repr__(self):
        return f"Box{self.shape}"


class Discrete:
    def __init__(self, n):
        self.n = int(n)
        self.shape = ()

    def __repr__(self):
        return f"Discrete({self.n})"


class EnvSpec:
    def __init__(self, env_id, max_episode_steps):
        self.id = env_id
        self.max_episode_steps = max_episode_steps


REGISTRY = {
    "CartPole-v0": dict(kind=_lib.ENV_CARTPOLE, obs=4, act=2, discrete=True, max_steps=200, obs_high=np.inf),
    "Hopper-v2": dict(kind=_lib.ENV_HOPPER, obs=11, act=3, discrete=False, max_steps=1000, obs_high=np.inf),
    "Humanoid-v2": dict(kind=_lib.ENV_HUMANOID, obs=376, act=17, discrete=False, max_steps=1000, obs_high=np.inf,
                        act_high=0.4),
    "Pendulum-v0": dict(kind=_lib.ENV_PENDULUM, obs=3, act=1, discrete=False, max_steps=200, obs_high=np.inf,
                        act_high=2.0),
    "MountainCar-v0": dict(kind=_lib.ENV_MOUNTAINCAR, obs=2, act=3, discrete=True, max_steps=200, obs_high=np.inf),
    "Acrobot-v1": dict(kind=_lib.ENV_ACROBOT, obs=6, act=3, discrete=True, max_steps=500, obs_high=np.inf),
    "InvertedPendulum-v2": dict(kind=_lib.ENV_INVPENDULUM, obs=4, act=1, discrete=False, max_steps=1000,
                                obs_high=np.inf, act_high=3.0),
    "InvertedDoublePendulum-v2": dict(kind=_lib.ENV_INVDOUBLEPENDULUM, obs=11, act=1, discrete=False, max_steps=1000,
                                      obs_high=np.inf, act_high=1.0),
    "Reacher-v2": dict(kind=_lib.ENV_REACHER, obs=11, act=2, discrete=False, max_steps=50, obs_high=np.inf,
                       act_high=1.0),
    "Swimmer-v2": dict(kind=_lib.ENV_SWIMMER, obs=8, act=2, discrete=False, max_steps=1000, obs_high=np.inf,
                       act_high=1.0),
    "HalfCheetah-v2": dict(kind=_lib.ENV_HALFCHEETAH, obs=17, act=6, discrete=False, max_steps=1000,
                           obs_high=np.inf, act_high=1.0),
}


class DeviceEnv:
    """Description of a batched device env (a Collector or a ``VecEnv`` holds the state).

    ``reset()`` / ``step(a)`` make it a gym-shaped single env, so the reference's serial
    ``rollout(env, agent, limit)`` loop (core.py:186-204) runs as written: they drive a
    lazily created one-env ``VecEnv`` without auto-reset and return numpy values.  Every
    step is one kernel launch and one device-to-host copy -- a convenience for evaluation
    and debugging; ``vec(n_envs)`` is the batched interface.
    """

    def __init__(self, env_id):
        if env_id not in REGISTRY:
            raise ValueError(f"unknown env {env_id!r}; available: {sorted(REGISTRY)}")
        r = REGISTRY[env_id]
        self.kind = r["kind"]
        self.obs_dim = r["obs"]
        self.observation_space = Box(-r["obs_high"], r["obs_high"], (r["obs"],))
        ah = r.get("act_high", 1.0)
        self.action_space = Discrete(r["act"]) if r["discrete"] else Box(-ah, ah, (r["act"],))
        self.discrete = r["discrete"]
        self.act_dim = r["act"]
        self.spec = EnvSpec(env_id, r["max_steps"])
        self._seed = 0
        self._single = None

    def close(self):
        self._single = None

    def vec(self, n_envs, **kw):
        """A ``VecEnv`` of ``n_envs`` copies of this env."""
        return VecEnv(self, n_envs, **kw)

    def seed(self, seed=0):
        """Seed of the reset-noise stream of ``reset()`` / ``step()`` (restarts the env)."""
        self._seed = int(seed)
        self._single = None
        return [self._seed]

    def reset(self):
        if self._single is None:
            self._single = VecEnv(self, 1, seed=self._seed, auto_reset=False)
        return self._single.reset()[0].cpu().numpy()

    def step(self, action):
        if self._single is None:
            raise RuntimeError("step() before reset()")
        a = np.asarray(action)
        ob, rew, done, _ = self._single.step(a.reshape((1,) if self.discrete else (1, self.act_dim)))
        return ob[0].cpu().numpy(), float(rew[0]), bool(done[0]), {}


class VecEnv:
    """``n_envs`` device envs stepped in lock-step with the caller's actions (gym's
    vector-env shape), on the same HIP dynamics and reset streams as the rollout.

    ``reset(mask=None)`` returns ``obs``, the raw float64 ``[E, obs_dim]`` observations;
    ``step(actions)`` returns ``(obs, rew, done, info)`` with ``done = flags & 1`` and
    ``info = {"flags", "terminated", "ep_t", "final_obs"}`` (flags bit 0: episode ended,
    bit 1: terminated by the env or its TimeLimit; ``ep_t``: the step's index in its
    episode).  With ``auto_reset`` an ended env is reset inside the same call: its ``obs``
    row is the new episode's first observation and ``info["final_obs"]`` holds the
    observation that ended the old one (rows of other envs there are stale).  Without it
    nothing resets; stepping an ended env goes on integrating, as in gym.

    The returned tensors belong to the env and are overwritten by the next call; clone
    what must be kept.  ``timestep_limit=None`` is the env's own ``max_episode_steps``.
    """

    def __init__(self, env_id, n_envs, seed=0, timestep_limit=None, auto_reset=True, env_offset=0, device="cuda"):
        env = env_id if isinstance(env_id, DeviceEnv) else DeviceEnv(env_id)
        if int(n_envs) <= 0:
            raise ValueError(f"n_envs must be positive, got {n_envs}")
        lib = _lib.load(require_gpu=True)
        self.env, self.E = env, int(n_envs)
        self.observation_space, self.action_space, self.spec = env.observation_space, env.action_space, env.spec
        self.auto_reset = bool(auto_reset)
        self.dev = torch.device(device)
        limit = env.spec.max_episode_steps if timestep_limit is None else int(timestep_limit)
        self.desc = _lib.RolloutDesc(env.kind, self.E, 1, limit, 0, int(env_offset), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     _lib.COMPUTE_F32, 0)
        E, O, A = self.E, env.obs_dim, env.act_dim
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.env_state = torch.zeros(int(lib.mrl_env_state_doubles(env.kind)) * E, **f64)
        self.env_int = torch.zeros(2 * E, dtype=torch.int32, device=self.dev)
        self.obs = torch.zeros(E, O, **f64)
        self.final_obs = torch.zeros(E, O, **f64)
        self.rew = torch.zeros(E, **f64)
        self.flags = torch.zeros(E, dtype=torch.uint8, device=self.dev)
        self.ep_t = torch.zeros(E, dtype=torch.int32, device=self.dev)
        self._act = (torch.zeros(E, dtype=torch.int32, device=self.dev) if env.discrete
                     else torch.zeros(E, A, dtype=torch.float32, device=self.dev))
        self._mask = torch.zeros(E, dtype=torch.uint8, device=self.dev)
        self._bufs = _lib.RolloutBufs(env_state=_lib.ptr(self.env_state), env_int=_lib.ptr(self.env_int))

    @property
    def episodes_started(self):
        """int32 [E]: resets of every env so far (the reset-noise stream's counter)."""
        return self.env_int[self.E:]

    def _io(self, mask=None):
        p = _lib.ptr
        return _lib.EnvIO(p(self._act), p(mask), p(self.obs), p(self.rew), p(self.flags), p(self.ep_t),
                          p(self.final_obs))

    def reset(self, mask=None):
        """Reset every env, or those where ``mask`` ([E], non-zero / True) is set."""
        m = None
        if mask is not None:
            mk = torch.as_tensor(mask)
            if tuple(mk.shape) != (self.E,):
                raise ValueError(f"mask must have shape ({self.E},), got {tuple(mk.shape)}")
            self._mask.copy_(mk != 0)
            m = self._mask
        _lib.call("mrl_env_reset", ctypes.byref(self.desc), ctypes.byref(self._bufs), ctypes.byref(self._io(m)),
                  _lib.stream())
        return self.obs

    def step(self, actions):
        a = torch.as_tensor(actions)
        want = tuple(self._act.shape)
        if tuple(a.shape) != want:
            raise ValueError(f"actions must have shape {want}, got {tuple(a.shape)}")
        integral = not (a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool)
        if self.env.discrete and not integral:
            raise ValueError(f"a discrete env takes integer action indices, got {a.dtype}")
        if not self.env.discrete and not a.dtype.is_floating_point:
            raise ValueError(f"a continuous env takes floating-point actions, got {a.dtype}")
        self._act.copy_(a)
        _lib.call("mrl_env_step", ctypes.byref(self.desc), ctypes.byref(self._bufs), ctypes.byref(self._io()),
                  int(self.auto_reset), _lib.stream())
        info = dict(flags=self.flags, terminated=(self.flags & 2) != 0, ep_t=self.ep_t, final_obs=self.final_obs)
        return self.obs, self.rew, (self.flags & 1) != 0, info


def make(env_id):
    return DeviceEnv(env_id)


class PopulationRollout:
    """``n`` whole episodes in one launch, env ``i`` driven by parameter vector ``i``
    (``mrl_pop_rollout``): the objective of the cross-entropy method (cem.py:64-68, one
    ``rollout(env, agent, limit)["reward"].sum()`` per candidate) under the deterministic
    policy (the Gauss head's mean / the arg-max logit).

    ``pop(thetas, filter_state=None, trace_steps=0)`` takes float32 ``[n, P]`` device rows
    (flat Keras-order theta of the env's policy net, ``pop.P`` floats) and returns a dict of tensors the
    object owns: ``ret`` (float64 sum of raw rewards), ``len``, ``flags`` (bit 1:
    terminated), ``stat`` (``[n, 1 + 2 obs_dim]`` Welford count / mean / M2 of the raw
    observations each policy was fed) and, with ``trace_steps > 0``, ``trace_obs`` /
    ``trace_act`` / ``trace_rew`` (rows beyond ``len[i]`` are left as they were).
    ``filter_state`` is a ``BatchZFilter.state`` / Collector ``filter_state[:FS]``, frozen for
    the call; ``None`` (or fewer than two observations in it) feeds the raw observation,
    clipped to +-5.  ``evaluate(theta, ...)`` runs one theta in all ``n`` envs.

    Every call starts a new episode in every env: the reset stream is the ``VecEnv``'s
    (seed, env, episodes started), so a ``VecEnv`` with the same seed replays a traced call.

    ``hid_sizes``: the hidden widths of the tanh policy net.  The default ``(64, 64)`` is the
    env's 64-64 net (``mrl_pop_rollout``, theta streamed from memory every step).  Any other
    shape -- ``(10, 5)`` of the reference's CEM battery, ``()`` for the linear policy -- runs on
    ``mrl_pop_rollout_mlp``, which keeps a block's 64 candidates in LDS for the whole episode:
    up to three hidden layers of 1 .. 64 units whose population tile fits one block's LDS
    (``mrl_pop_rollout_mlp_fits``); a shape that does not raises ``MrlError`` here, and so
    does ``Humanoid-v2``, which a wave steps, not a thread: ``WavePopulationRollout`` below is
    its class and ``population_rollout(env, n, ...)`` picks the class that serves an env.
    """

    DEFAULT_HID = (64, 64)

    def __init__(self, env_id, n, seed=0, timestep_limit=None, env_offset=0, device="cuda", hid_sizes=None):
        env = env_id if isinstance(env_id, DeviceEnv) else DeviceEnv(env_id)
        if int(n) <= 0:
            raise ValueError(f"n must be positive, got {n}")
        lib = _lib.load(require_gpu=True)
        self.env, self.N = env, int(n)
        self.dev = torch.device(device)
        limit = env.spec.max_episode_steps if not timestep_limit else int(timestep_limit)
        self.limit = min(limit, env.spec.max_episode_steps)
        self.desc = _lib.RolloutDesc(env.kind, self.N, 1, self.limit, 0, int(env_offset),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.COMPUTE_F32, 0)
        self.hid_sizes = tuple(int(h) for h in (self.DEFAULT_HID if hid_sizes is None else hid_sizes))
        self._hid = (ctypes.c_int32 * max(len(self.hid_sizes), 1))(*self.hid_sizes)
        self._bind(lib)
        N, O = self.N, env.obs_dim
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.env_state = torch.zeros(int(lib.mrl_env_state_doubles(env.kind)) * N, **f64)
        self.env_int = torch.zeros(2 * N, dtype=torch.int32, device=self.dev)
        self.ret = torch.zeros(N, **f64)
        self.len = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.flags = torch.zeros(N, dtype=torch.uint8, device=self.dev)
        self.stat = torch.zeros(N, 1 + 2 * O, **f64)
        self._trace = None
        self._bufs = _lib.RolloutBufs(env_state=_lib.ptr(self.env_state), env_int=_lib.ptr(self.env_int))

    # the entry point that takes hid_sizes, its predicate, and what a shape it turns away is told
    # (and whether hid_sizes (64, 64) goes to mrl_pop_rollout, the kernel of that one shape)
    ENTRY, FITS, HAS_64_64 = "mrl_pop_rollout_mlp", "mrl_pop_rollout_mlp_fits", True
    REFUSAL = ("PopulationRollout: hid_sizes={hid} on {env} is neither "
               "the 64-64 net nor a net mrl_pop_rollout_mlp takes (the thread-per-env envs, at "
               "most 3 hidden layers of 1..64 units, 64 candidates' parameters within one "
               "block's LDS); envs.population_rollout(env, n, ...) picks the class that serves "
               "an env, WavePopulationRollout for Humanoid-v2")

    def _bind(self, lib):
        """The entry point that takes ``hid_sizes`` on this env, and ``P``; ``MrlError`` if none does."""
        env = self.env
        if self.HAS_64_64 and self.hid_sizes == (64, 64) and env.kind != _lib.ENV_HUMANOID:
            head = _lib.HEAD_SOFTMAX if env.discrete else _lib.HEAD_GAUSS
            self.pol = _lib.MlpDesc(env.obs_dim, env.act_dim, head, 64, 2)
            self.P = int(lib.mrl_mlp_num_params(ctypes.byref(self.pol)))
            return
        self.pol = None
        fits = int(getattr(lib, self.FITS)(env.kind, self._hid, len(self.hid_sizes)))
        _lib.check(min(fits, 0), self.FITS)
        if fits != 1:
            raise _lib.MrlError(self.REFUSAL.format(hid=list(self.hid_sizes), env=env.spec.id))
        self.P = int(lib.mrl_pop_mlp_num_params(env.kind, self._hid, len(self.hid_sizes)))
        _lib.check(min(self.P, 0), "mrl_pop_mlp_num_params")

    def _launch(self, thetas, ld, fs, io):
        entry, net = ("mrl_pop_rollout", (ctypes.byref(self.pol),)) if self.pol is not None else (
            self.ENTRY, (self._hid, len(self.hid_sizes)))
        _lib.call(entry, ctypes.byref(self.desc), ctypes.byref(self._bufs), *net, thetas, ld, fs, ctypes.byref(io),
                  _lib.stream())

    @property
    def episodes_started(self):
        """int32 [n]: episodes every env has started (the reset-noise stream's counter)."""
        return self.env_int[self.N:]

    def _trace_bufs(self, steps):
        if self._trace is None or self._trace[0].shape[0] < steps:
            N, O, A = self.N, self.env.obs_dim, self.env.act_dim
            act = (torch.zeros(steps, N, dtype=torch.int32, device=self.dev) if self.env.discrete
                   else torch.zeros(steps, N, A, dtype=torch.float32, device=self.dev))
            self._trace = (torch.zeros(steps, N, O, dtype=torch.float64, device=self.dev), act,
                           torch.zeros(steps, N, dtype=torch.float64, device=self.dev))
        return tuple(t[:steps] for t in self._trace)

    def _run(self, thetas, ld, filter_state, trace_steps):
        p = _lib.ptr
        fs = None
        if filter_state is not None:
            fs = torch.as_tensor(filter_state, dtype=torch.float64).to(self.dev).contiguous()
            if fs.numel() < 2 + 2 * (self.env.obs_dim + 1):
                raise ValueError("filter_state must hold n_obs, n_rew, M[obs_dim + 1], S[obs_dim + 1]")
        out = dict(ret=self.ret, len=self.len, flags=self.flags, stat=self.stat)
        io = _lib.PopIO(p(self.ret), p(self.len), p(self.flags), p(self.stat))
        if int(trace_steps) > 0:
            tobs, tact, trew = self._trace_bufs(int(trace_steps))
            io.trace_steps, io.trace_obs, io.trace_act, io.trace_rew = int(trace_steps), p(tobs), p(tact), p(trew)
            out.update(trace_obs=tobs, trace_act=tact, trace_rew=trew)
        self._launch(p(thetas), ld, p(fs), io)
        return out

    def _theta(self, th, shape):
        th = torch.as_tensor(th)
        if tuple(th.shape) != shape:
            raise ValueError(f"expected parameters of shape {shape}, got {tuple(th.shape)}")
        return th.to(device=self.dev, dtype=torch.float32).contiguous()

    def __call__(self, thetas, filter_state=None, trace_steps=0):
        return self._run(self._theta(thetas, (self.N, self.P)), self.P, filter_state, trace_steps)

    def evaluate(self, theta, filter_state=None, trace_steps=0):
        """The same ``theta`` in all ``n`` envs: a trained policy's return over ``n`` episodes."""
        return self._run(self._theta(theta, (self.P,)), 0, filter_state, trace_steps)


class WavePopulationRollout(PopulationRollout):
    """``PopulationRollout`` for the wave-per-env envs -- ``Humanoid-v2`` -- on
    ``mrl_pop_rollout_wave``: one wave per candidate keeps its env's state in LDS for the whole
    episode and reads theta from memory every step.  The interface is ``PopulationRollout``'s
    (``__call__``, ``evaluate``, ``episodes_started``, ``P``, ``limit``, ``trace_steps``); a
    ``VecEnv`` of the same seed replays a traced call bit for bit.  ``hid_sizes`` defaults to
    ``(10, 5)``, the reference's CEM battery: at most three hidden layers of 1 .. 64 units
    (``mrl_pop_rollout_wave_fits``); any other shape, or a thread-per-env env, raises
    ``MrlError`` here."""

    DEFAULT_HID = (10, 5)
    ENTRY, FITS, HAS_64_64 = "mrl_pop_rollout_wave", "mrl_pop_rollout_wave_fits", False
    REFUSAL = ("WavePopulationRollout: hid_sizes={hid} on {env} is not "
               "a net mrl_pop_rollout_wave takes (Humanoid-v2, at most 3 hidden layers of 1..64 "
               "units); envs.population_rollout(env, n, ...) picks the class that serves an env")


def population_rollout(env, n, *, hid_sizes=None, **kw):
    """The population rollout that serves ``env`` (an id or a ``DeviceEnv``): a
    ``WavePopulationRollout`` for the wave-per-env envs (Humanoid-v2), a ``PopulationRollout``
    for the thread-per-env ones.  ``hid_sizes=None`` is the class's default: ``(10, 5)`` for
    Humanoid, ``(64, 64)`` otherwise.  ``kw``: ``seed``, ``timestep_limit``, ``env_offset``,
    ``device``."""
    env = env if isinstance(env, DeviceEnv) else DeviceEnv(env)
    cls = WavePopulationRollout if env.kind == _lib.ENV_HUMANOID else PopulationRollout
    return cls(env, n, hid_sizes=hid_sizes, **kw)
