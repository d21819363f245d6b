"""float64 numpy twin of the cart-and-pole device envs (test helper, not collected):
InvertedPendulum-v2 and InvertedDoublePendulum-v2 in the operation order of
``modular_rl_amd/csrc/envs_chains.h`` (which documents the model and its constants), and
``ChainEnvs``, which has the duck type of ``oracle.rollout_np.Envs`` so that
``oracle.rollout_np.collect`` and the VecEnv comparison loop run on it unchanged.

The step size, the joint damping and the limit constants are fields of a ``Model`` (``IP`` and
``DP`` hold the envs' own); the physics tests step copies with other values
(``IP.replace(damp=0.0)``)."""
import numpy as np

from oracle import philox

INVPENDULUM, INVDOUBLEPENDULUM = 8, 9
KINDS = {"InvertedPendulum-v2": INVPENDULUM, "InvertedDoublePendulum-v2": INVDOUBLEPENDULUM}
PI = 3.141592653589793
RHO = 1000.0
CART_R, CART_L, POLE_L = 0.1, 0.2, 0.6


def cyl_mass(r, l):
    return RHO * (PI * (r * r) * l)


def sph_mass(r):
    return RHO * (4.0 / 3.0 * PI * (r * r * r))


def capsule_mass(r, l):
    return cyl_mass(r, l) + sph_mass(r)


def capsule_inertia(r, l):
    return (cyl_mass(r, l) * (r * r / 4.0 + l * l / 12.0)
            + sph_mass(r) * (2.0 * (r * r) / 5.0 + l * l / 4.0 + 3.0 * l * r / 8.0))


MC = capsule_mass(CART_R, CART_L)


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def limit(q, v, lim, k, c):
    """One-sided penalty stop of a joint at +-lim (Hopper's form)."""
    cv = c * v
    flo, fhi = k * (-lim - q) - cv, k * (lim - q) - cv
    return np.where(q < -lim, flo, np.where(q > lim, fhi, 0.0))


class Model:
    """The constants of one env; ``replace`` returns a copy with some of them changed."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def replace(self, **kw):
        return Model(**{**self.__dict__, **kw})


def rk4(s, h, dsdt):
    """s' = s + h/6 (((k1 + 2 k2) + 2 k3) + k4), stage by stage as ch_rk4."""
    y, acc = s, np.zeros_like(s)
    for st in range(4):
        k = dsdt(y)
        w = 2.0 if st in (1, 2) else 1.0
        hs = h if st == 2 else h * 0.5
        acc = acc + w * k
        y = s + hs * k
    return s + (h / 6.0) * acc


# ---------------------------------------------------------------- InvertedPendulum-v2
_IP_R = 0.049
IP = Model(ns=4, dt=0.02, frame_skip=2, gear=100.0, ctrl=3.0, damp=1.0, gx=0.0, gz=-9.81, xlim=1.0, hlim=PI / 2.0,
           ks=20000.0, cs=400.0, kh=2000.0, ch=50.0, th_done=0.2,
           m1=capsule_mass(_IP_R, POLE_L), i1=capsule_inertia(_IP_R, POLE_L), lc=POLE_L / 2.0)
IP.mt = MC + IP.m1
IP.b = IP.m1 * IP.lc
IP.j = IP.i1 + IP.m1 * (IP.lc * IP.lc)


def ip_reset(u):
    return u[..., :4] * 0.02 - 0.01


def ip_obs(s):
    return s.copy()


def ip_terms(s, p=IP):
    """(M [E, 2, 2], c [E, 2], g [E, 2]) of M qdd = B u - c - g - D qd + tau_lim."""
    th, thd = s[:, 1], s[:, 3]
    sn, cs = np.sin(th), np.cos(th)
    m01 = p.b * cs
    c0 = -(p.b * sn) * (thd * thd)
    g1 = p.b * p.gz * sn
    z = np.zeros_like(th)
    M = np.stack([np.stack([z + p.mt, m01], axis=1), np.stack([m01, z + p.j], axis=1)], axis=1)
    return M, np.stack([c0, z], axis=1), np.stack([z, g1], axis=1)


def ip_dsdt(y, fu, p=IP):
    x, th, xd, thd = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
    sn, cs = np.sin(th), np.cos(th)
    m01 = p.b * cs
    c0 = -(p.b * sn) * (thd * thd)
    g1 = p.b * p.gz * sn
    r0 = fu - c0 - p.damp * xd + limit(x, xd, p.xlim, p.ks, p.cs)
    r1 = -g1 - p.damp * thd + limit(th, thd, p.hlim, p.kh, p.ch)
    l10 = m01 / p.mt
    d1 = p.j - l10 * l10 * p.mt
    y1 = r1 - l10 * r0
    a1 = y1 / d1
    a0 = r0 / p.mt - l10 * a1
    return np.stack([xd, thd, a0, a1], axis=1)


def _control(a, n, p):
    return p.gear * _clamp(np.asarray(a, dtype=np.float32).reshape(n).astype(np.float64), -p.ctrl, p.ctrl)


def ip_step(s, a, p=IP):
    """s [E, 4] float64, a [E, 1] (float32 values) -> (s', reward, done)."""
    fu = _control(a, len(s), p)
    for _ in range(p.frame_skip):
        s = rk4(s, p.dt, lambda y: ip_dsdt(y, fu, p))
    ok = np.isfinite(s).all(axis=1) & (np.abs(s[:, 1]) <= p.th_done)
    return s, np.ones(len(s)), ~ok


def ip_energy(s, p=IP):
    """Kinetic + gravitational + limit-spring energy."""
    M, _, _ = ip_terms(s, p)
    v = s[:, 2:]
    pen_x = np.maximum(np.abs(s[:, 0]) - p.xlim, 0.0)
    pen_h = np.maximum(np.abs(s[:, 1]) - p.hlim, 0.0)
    return (0.5 * np.einsum("ei,eij,ej->e", v, M, v) - p.m1 * p.gz * (p.lc * np.cos(s[:, 1]))
            + 0.5 * p.ks * pen_x ** 2 + 0.5 * p.kh * pen_h ** 2)


# ---------------------------------------------------------------- InvertedDoublePendulum-v2
_DP_R = 0.045
DP = Model(ns=6, dt=0.01, frame_skip=5, gear=500.0, ctrl=1.0, damp=0.05, gx=1e-5, gz=-9.81, xlim=1.0,
           ks=20000.0, cs=400.0, m=capsule_mass(_DP_R, POLE_L), i=capsule_inertia(_DP_R, POLE_L), l=POLE_L,
           lc=POLE_L / 2.0)
DP.mt = MC + DP.m + DP.m
DP.a1 = DP.m * DP.lc + DP.m * DP.l
DP.a2 = DP.m * DP.lc
DP.j1 = DP.i + DP.m * (DP.lc * DP.lc) + DP.m * (DP.l * DP.l)
DP.j2 = DP.i + DP.m * (DP.lc * DP.lc)
DP.h = DP.m * DP.l * DP.lc


def dp_reset(u):
    """u [..., 8] uniforms: u0..u2 -> q, the pairs (u4, u5), (u6, u7) -> Box-Muller normals
    (oracle/philox.py's transform), three of them -> qd."""
    q = u[..., :3] * 0.2 - 0.1
    r0, r1 = np.sqrt(-2.0 * np.log(1.0 - u[..., 4])), np.sqrt(-2.0 * np.log(1.0 - u[..., 6]))
    a0, a1 = 2.0 * PI * u[..., 5], 2.0 * PI * u[..., 7]
    v = np.stack([0.1 * (r0 * np.cos(a0)), 0.1 * (r0 * np.sin(a0)), 0.1 * (r1 * np.cos(a1))], axis=-1)
    return np.concatenate([q, v], axis=-1)


def _dp_parts(y, p):
    t1, t2, t1d, t2d = y[:, 1], y[:, 2], y[:, 4], y[:, 5]
    s1, c1 = np.sin(t1), np.cos(t1)
    s12, c12 = np.sin(t1 + t2), np.cos(t1 + t2)
    s2, c2 = np.sin(t2), np.cos(t2)
    w1, w2 = t1d, t1d + t2d
    w1s, w2s = w1 * w1, w2 * w2
    a01, a02, a12 = p.a1 * c1, p.a2 * c12, p.h * c2
    m01, m02, m11, m12 = a01 + a02, a02, (p.j1 + p.j2) + 2.0 * a12, a12 + p.j2
    c0 = -(p.a1 * s1) * w1s - (p.a2 * s12) * w2s
    hs = p.h * s2
    ca1, ca2 = -hs * w2s, hs * w1s
    ga1, ga2 = -p.a1 * (p.gx * c1 - p.gz * s1), -p.a2 * (p.gx * c12 - p.gz * s12)
    return m01, m02, m11, m12, c0, ca1, ca2, ga1, ga2


def dp_terms(s, p=DP):
    """(M [E, 3, 3], c [E, 3], g [E, 3]) of M qdd = B u - c - g - D qd + tau_lim."""
    m01, m02, m11, m12, c0, ca1, ca2, ga1, ga2 = _dp_parts(s, p)
    z = np.zeros_like(m01)
    M = np.stack([np.stack([z + p.mt, m01, m02], axis=1), np.stack([m01, m11, m12], axis=1),
                  np.stack([m02, m12, z + p.j2], axis=1)], axis=1)
    return M, np.stack([c0, ca1 + ca2, ca2], axis=1), np.stack([z - p.mt * p.gx, ga1 + ga2, ga2], axis=1)


def dp_dsdt(y, fu, p=DP):
    x, xd, t1d, t2d = y[:, 0], y[:, 3], y[:, 4], y[:, 5]
    m01, m02, m11, m12, c0, ca1, ca2, ga1, ga2 = _dp_parts(y, p)
    r0 = fu - c0 + p.mt * p.gx - p.damp * xd + limit(x, xd, p.xlim, p.ks, p.cs)
    r1 = -(ca1 + ca2) - (ga1 + ga2) - p.damp * t1d
    r2 = -ca2 - ga2 - p.damp * t2d
    l10, l20 = m01 / p.mt, m02 / p.mt
    d1 = m11 - l10 * l10 * p.mt
    l21 = (m12 - l20 * l10 * p.mt) / d1
    d2 = p.j2 - l20 * l20 * p.mt - l21 * l21 * d1
    y1 = r1 - l10 * r0
    y2 = r2 - l20 * r0 - l21 * y1
    a2 = y2 / d2
    a1 = y1 / d1 - l21 * a2
    a0 = r0 / p.mt - l10 * a1 - l20 * a2
    return np.stack([xd, t1d, t2d, a0, a1, a2], axis=1)


def dp_tip(s, p=DP):
    s1, c1 = np.sin(s[:, 1]), np.cos(s[:, 1])
    s12, c12 = np.sin(s[:, 1] + s[:, 2]), np.cos(s[:, 1] + s[:, 2])
    return s[:, 0] + p.l * s1 + p.l * s12, p.l * c1 + p.l * c12


def dp_step(s, a, p=DP):
    fu = _control(a, len(s), p)
    for _ in range(p.frame_skip):
        s = rk4(s, p.dt, lambda y: dp_dsdt(y, fu, p))
    xt, yt = dp_tip(s, p)
    dist = 0.01 * (xt * xt) + (yt - 2.0) * (yt - 2.0)
    vel = 1e-3 * (s[:, 4] * s[:, 4]) + 5e-3 * (s[:, 5] * s[:, 5])
    return s, 10.0 - dist - vel, yt <= 1.0


def dp_obs(s, p=DP):
    z = np.zeros(len(s))
    v = _clamp(s[:, 3:6], -10.0, 10.0)
    f = _clamp(limit(s[:, 0], s[:, 3], p.xlim, p.ks, p.cs), -10.0, 10.0)
    return np.stack([s[:, 0], np.sin(s[:, 1]), np.sin(s[:, 2]), np.cos(s[:, 1]), np.cos(s[:, 2]),
                     v[:, 0], v[:, 1], v[:, 2], f, z, z], axis=1)


def dp_energy(s, p=DP):
    """Kinetic + gravitational (both components of g) + limit-spring energy."""
    M, _, _ = dp_terms(s, p)
    v = s[:, 3:]
    x, t1, t12 = s[:, 0], s[:, 1], s[:, 1] + s[:, 2]
    x1, z1 = x + p.lc * np.sin(t1), p.lc * np.cos(t1)
    x2, z2 = x + p.l * np.sin(t1) + p.lc * np.sin(t12), p.l * np.cos(t1) + p.lc * np.cos(t12)
    pot = -(MC * p.gx * x + p.m * (p.gx * x1 + p.gz * z1) + p.m * (p.gx * x2 + p.gz * z2))
    pen_x = np.maximum(np.abs(x) - p.xlim, 0.0)
    return 0.5 * np.einsum("ei,eij,ej->e", v, M, v) + pot + 0.5 * p.ks * pen_x ** 2


# kind -> (model, obs, actions, TimeLimit, reset uniforms, reset, obs, step)
_TABLE = {
    INVPENDULUM: (IP, 4, 1, 1000, 4, ip_reset, ip_obs, ip_step),
    INVDOUBLEPENDULUM: (DP, 11, 1, 1000, 8, dp_reset, dp_obs, dp_step),
}


def margin(kind, s):
    """Distance of the states s [E, ns] to the env's termination threshold."""
    if KINDS.get(kind, kind) == INVPENDULUM:
        return np.abs(np.abs(s[:, 1]) - IP.th_done)
    return np.abs(dp_tip(s)[1] - 1.0)


class ChainEnvs:
    """``oracle.rollout_np.Envs`` for the two chain kinds: the same reset stream (Philox
    domain 1 of (seed, env, episodes started)) and the same bookkeeping.  ``min_margin`` is
    the least distance to the termination threshold over every state stepped to so far."""

    def __init__(self, kind, E, seed, env_offset=0):
        kind = KINDS.get(kind, kind)
        self.kind, self.E, self.seed = kind, E, seed
        self.gid = np.arange(E, dtype=np.uint64) + np.uint64(env_offset)
        self.model, self.O, self.A, self.max_steps, self.nu, self._reset, self._obs, self._step = _TABLE[kind]
        self.ns = self.model.ns
        self.discrete = False
        self.state = np.zeros((E, self.ns))
        self.ep_t = np.zeros(E, dtype=np.int64)
        self.ep_count = np.zeros(E, dtype=np.int64)
        self.min_margin = np.inf

    def reset(self, idx):
        u = philox.uniforms(self.seed, 1, self.gid[idx], self.ep_count[idx].astype(np.uint64), self.nu)
        self.state[idx] = self._reset(u)
        self.ep_count[idx] += 1
        self.ep_t[idx] = 0

    def obs(self):
        return self._obs(self.state)

    def step(self, act):
        self.state, rew, done = self._step(self.state, act)
        self.min_margin = min(self.min_margin, float(margin(self.kind, self.state).min()))
        return rew, done
