"""float64 numpy twin of the classic-control device envs (test helper, not collected):
Pendulum-v0, MountainCar-v0 and Acrobot-v1 in the operation order of
``modular_rl_amd/csrc/envs_classic.h``, and ``ClassicEnvs``, which has the duck type of
``oracle.rollout_np.Envs`` so that ``oracle.rollout_np.collect`` and the VecEnv comparison
loop run on it unchanged."""
import numpy as np

from oracle import philox

PENDULUM, MOUNTAINCAR, ACROBOT = 4, 5, 6
KINDS = {"Pendulum-v0": PENDULUM, "MountainCar-v0": MOUNTAINCAR, "Acrobot-v1": ACROBOT}
PI = 3.141592653589793
TWO_PI = 2.0 * PI


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


# ---------------------------------------------------------------- Pendulum-v0
PD_MAX_SPEED, PD_MAX_TORQUE, PD_DT, PD_G, PD_M, PD_L = 8.0, 2.0, 0.05, 10.0, 1.0, 1.0


def pendulum_reset(u):
    """u [..., 2] uniforms -> (th, thdot) in [-pi, pi) x [-1, 1)."""
    return np.stack([u[..., 0] * TWO_PI - PI, u[..., 1] * 2.0 - 1.0], axis=-1)


def pendulum_obs(s):
    return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]], axis=1)


def pendulum_step(s, a):
    """s [E, 2] float64, a [E, 1] (float32 values) -> (s', reward, done)."""
    th, thdot = s[:, 0], s[:, 1]
    u = _clamp(np.asarray(a, dtype=np.float32).reshape(len(s)).astype(np.float64), -PD_MAX_TORQUE, PD_MAX_TORQUE)
    md = np.fmod(th + PI, TWO_PI)
    md = np.where(md < 0.0, md + TWO_PI, md)
    an = md - PI
    cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    nthd = thdot + (-3.0 * PD_G / (2.0 * PD_L) * np.sin(th + PI) + 3.0 / (PD_M * (PD_L * PD_L)) * u) * PD_DT
    nth = th + nthd * PD_DT
    nthd = _clamp(nthd, -PD_MAX_SPEED, PD_MAX_SPEED)
    return np.stack([nth, nthd], axis=1), -cost, np.zeros(len(s), dtype=bool)


# ---------------------------------------------------------------- MountainCar-v0
MC_MIN_POS, MC_MAX_POS, MC_MAX_SPEED, MC_GOAL = -1.2, 0.6, 0.07, 0.5


def mountaincar_reset(u):
    return np.stack([u[..., 0] * 0.2 - 0.6, np.zeros_like(u[..., 0])], axis=-1)


def mountaincar_obs(s):
    return s.copy()


def mountaincar_step(s, a):
    p, v = s[:, 0], s[:, 1]
    a = np.asarray(a).astype(np.int64)
    v = v + ((a - 1).astype(np.float64) * 0.001 + np.cos(3.0 * p) * (-0.0025))
    v = _clamp(v, -MC_MAX_SPEED, MC_MAX_SPEED)
    p = p + v
    p = _clamp(p, MC_MIN_POS, MC_MAX_POS)
    v = np.where((p == MC_MIN_POS) & (v < 0.0), 0.0, v)
    return np.stack([p, v], axis=1), -np.ones(len(s)), p >= MC_GOAL


# ---------------------------------------------------------------- Acrobot-v1
AC_DT, AC_M1, AC_M2, AC_L1, AC_LC1, AC_LC2, AC_I1, AC_I2, AC_G = 0.2, 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 9.8
AC_MAX_W1, AC_MAX_W2 = 4.0 * PI, 9.0 * PI
AC_WRAP_MAX = 8


def acrobot_reset(u):
    return u * 0.2 - 0.1


def acrobot_obs(s):
    return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]], axis=1)


def acrobot_dsdt(y, tau):
    """The "book" equations; cos(x - pi/2) as sin x, as the kernel takes it."""
    t1, t2, w1, w2 = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
    c2, s2 = np.cos(t2), np.sin(t2)
    d1 = AC_M1 * (AC_LC1 * AC_LC1) + AC_M2 * (AC_L1 * AC_L1 + AC_LC2 * AC_LC2 + 2.0 * AC_L1 * AC_LC2 * c2) + AC_I1 + AC_I2
    d2 = AC_M2 * (AC_LC2 * AC_LC2 + AC_L1 * AC_LC2 * c2) + AC_I2
    phi2 = AC_M2 * AC_LC2 * AC_G * np.sin(t1 + t2)
    phi1 = (-AC_M2 * AC_L1 * AC_LC2 * (w2 * w2) * s2 - 2.0 * AC_M2 * AC_L1 * AC_LC2 * w2 * w1 * s2
            + (AC_M1 * AC_LC1 + AC_M2 * AC_L1) * AC_G * np.sin(t1) + phi2)
    dw2 = ((tau + d2 / d1 * phi1 - AC_M2 * AC_L1 * AC_LC2 * (w1 * w1) * s2 - phi2)
           / (AC_M2 * (AC_LC2 * AC_LC2) + AC_I2 - d2 * d2 / d1))
    dw1 = -(d2 * dw2 + phi1) / d1
    return np.stack([w1, w2, dw1, dw2], axis=1)


def acrobot_wrap(x):
    x = x.copy()
    for _ in range(AC_WRAP_MAX):
        x = np.where(x > PI, x - TWO_PI, x)
    for _ in range(AC_WRAP_MAX):
        x = np.where(x < -PI, x + TWO_PI, x)
    return x


def acrobot_step(s, a):
    tau = (np.asarray(a).astype(np.int64) - 1).astype(np.float64)
    k1 = acrobot_dsdt(s, tau)
    k2 = acrobot_dsdt(s + (AC_DT / 2.0) * k1, tau)
    k3 = acrobot_dsdt(s + (AC_DT / 2.0) * k2, tau)
    k4 = acrobot_dsdt(s + AC_DT * k3, tau)
    y = s + (AC_DT / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    t1, t2 = acrobot_wrap(y[:, 0]), acrobot_wrap(y[:, 1])
    w1, w2 = _clamp(y[:, 2], -AC_MAX_W1, AC_MAX_W1), _clamp(y[:, 3], -AC_MAX_W2, AC_MAX_W2)
    done = -np.cos(t1) - np.cos(t2 + t1) > 1.0
    return np.stack([t1, t2, w1, w2], axis=1), np.where(done, 0.0, -1.0), done


# kind -> (state doubles, obs, actions, TimeLimit, reset uniforms, reset, obs, step)
_TABLE = {
    PENDULUM: (2, 3, 1, 200, 2, pendulum_reset, pendulum_obs, pendulum_step),
    MOUNTAINCAR: (2, 2, 3, 200, 2, mountaincar_reset, mountaincar_obs, mountaincar_step),
    ACROBOT: (4, 6, 3, 500, 4, acrobot_reset, acrobot_obs, acrobot_step),
}


class ClassicEnvs:
    """``oracle.rollout_np.Envs`` for the three classic-control kinds: the same reset stream
    (Philox domain 1 of (seed, env, episodes started)) and the same bookkeeping."""

    def __init__(self, kind, E, seed, env_offset=0):
        kind = KINDS.get(kind, kind)
        self.kind, self.E, self.seed = kind, E, seed
        self.gid = np.arange(E, dtype=np.uint64) + np.uint64(env_offset)
        self.ns, self.O, self.A, self.max_steps, self.nu, self._reset, self._obs, self._step = _TABLE[kind]
        self.discrete = kind != PENDULUM
        self.state = np.zeros((E, self.ns))
        self.ep_t = np.zeros(E, dtype=np.int64)
        self.ep_count = np.zeros(E, dtype=np.int64)

    def reset(self, idx):
        u = philox.uniforms(self.seed, 1, self.gid[idx], self.ep_count[idx].astype(np.uint64), self.nu)
        self.state[idx] = self._reset(u)
        self.ep_count[idx] += 1
        self.ep_t[idx] = 0

    def obs(self):
        return self._obs(self.state)

    def step(self, act):
        self.state, rew, done = self._step(self.state, act)
        return rew, done
