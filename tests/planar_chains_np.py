"""float64 numpy twin of the planar device envs without contact (test helper, not collected):
Reacher-v2 and Swimmer-v2 in the operation order of ``modular_rl_amd/csrc/envs_planar.h``
(which documents the models and their constants), and ``PlanarEnvs``, which has the duck type
of ``oracle.rollout_np.Envs`` so that ``oracle.rollout_np.collect`` and the VecEnv comparison
loop run on it unchanged.

The step size, the damping, the limit and the fluid constants are fields of a ``Model``
(``RC`` and ``SW`` hold the envs' own); the physics tests step copies with other values
(``SW.replace(rho=0.0, beta=0.0)``)."""
import dataclasses

import numpy as np

from oracle import philox
from tests.mujoco_chains_np import PI, RHO, _clamp, capsule_inertia, capsule_mass, cyl_mass, limit, rk4, sph_mass

REACHER, SWIMMER = 12, 11
KINDS = {"Reacher-v2": REACHER, "Swimmer-v2": SWIMMER}
KH, CH = 2000.0, 50.0  # the hinge stop: N m/rad, N m s/rad


def capsule_axial(r, l):
    return cyl_mass(r, l) * (r * r / 2.0) + sph_mass(r) * (2.0 * (r * r) / 5.0)


def csqrt(v):
    """pl_sqrt: 40 Newton steps from 1."""
    x = 1.0
    for _ in range(40):
        x = 0.5 * (x + v / x)
    return x


@dataclasses.dataclass
class Model:
    """The constants of one env; ``replace`` returns a copy with some of them changed (the
    derived ones are worked out again)."""
    ns: int
    nq: int
    dt: float
    frame_skip: int
    gear: float
    ctrl: float
    arm: float
    hlim: float
    damp: float = 0.0
    kh: float = KH
    ch: float = CH
    rho: float = 0.0   # the medium's density
    beta: float = 0.0  # and viscosity
    r: float = 0.0     # capsule radius, length, density over 1000
    l: float = 0.0
    dens: float = 1.0
    tip: float = 0.0   # Reacher: the fingertip's distance along link 2

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    def __post_init__(self):
        p = self
        p.m, p.i = p.dens * capsule_mass(p.r, p.l), p.dens * capsule_inertia(p.r, p.l)
        if p.nq == 2:  # Reacher
            p.lc = p.l / 2.0
            p.ms = p.dens * sph_mass(p.r)
            p.i_s = p.ms * (2.0 * (p.r * p.r) / 5.0)
            p.a11 = p.i + p.m * (p.lc * p.lc) + (p.m + p.ms) * (p.l * p.l)
            p.h = p.l * (p.m * p.lc + p.ms * p.tip)
            p.a22 = p.i + p.m * (p.lc * p.lc) + p.i_s + p.ms * (p.tip * p.tip)
        else:  # Swimmer
            p.ia = capsule_axial(p.r, p.l)
            p.mt = 3.0 * p.m + p.arm
            p.s0, p.s1, p.s2 = p.m * 2.0, p.m * -1.5, p.m * -0.5
            p.c01, p.c02, p.c12 = p.m * -0.75, p.m * -0.25, p.m * 0.5
            p.j0, p.j1, p.j2 = p.m * 1.5 + p.i, p.m * 1.25 + p.i, p.m * 0.25 + p.i
            p.bx, p.by = csqrt(6.0 * (p.i + p.i - p.ia) / p.m), csqrt(6.0 * p.ia / p.m)
            p.bd = (p.bx + p.by + p.by) / 3.0
            p.vis_f, p.vis_t = 3.0 * PI * p.beta * p.bd, PI * p.beta * (p.bd * p.bd * p.bd)
            p.ql = 0.5 * p.rho * (p.by * p.by)
            p.qn = 0.5 * p.rho * (p.bx * p.by)
            p.qt = p.rho * p.by * ((p.bx * p.bx) * (p.bx * p.bx) + (p.by * p.by) * (p.by * p.by)) / 64.0


def _control(a, p):
    """a [E, 2] (float32 values) -> (the unclipped actions as float64, the hinge torques)."""
    a = np.asarray(a, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    return a, p.gear * _clamp(a, -p.ctrl, p.ctrl)


# ---------------------------------------------------------------- Reacher-v2
RC = Model(ns=6, nq=2, dt=0.01, frame_skip=2, gear=200.0, ctrl=1.0, arm=1.0, hlim=3.0, damp=1.0,
           r=0.01, l=0.1, dens=300.0 / RHO, tip=0.11)
RC_GOAL2 = 0.04


def rc_candidates(u):
    """The four goal candidates of a reset, [..., 4, 2]."""
    return np.stack([np.stack([u[..., 4 + 2 * c] * 0.4 - 0.2, u[..., 5 + 2 * c] * 0.4 - 0.2], axis=-1)
                     for c in range(4)], axis=-2)


def rc_reset(u):
    """u [..., 12] uniforms -> th, thd and the goal: the first candidate inside the disc, or
    the fourth halved."""
    th = u[..., 0:2] * 0.2 - 0.1
    thd = u[..., 2:4] * 0.01 - 0.005
    gx, gy = 0.5 * (u[..., 10] * 0.4 - 0.2), 0.5 * (u[..., 11] * 0.4 - 0.2)
    for c in (3, 2, 1, 0):
        cx, cy = u[..., 4 + 2 * c] * 0.4 - 0.2, u[..., 5 + 2 * c] * 0.4 - 0.2
        inside = cx * cx + cy * cy < RC_GOAL2
        gx, gy = np.where(inside, cx, gx), np.where(inside, cy, gy)
    return np.concatenate([th, thd, np.stack([gx, gy], axis=-1)], axis=-1)


def rc_fallback(u):
    """True where no candidate lies inside the disc."""
    g = rc_candidates(u)
    return ~((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) < RC_GOAL2).any(axis=-1)


def _rc_parts(y, p):
    q2, q1d, q2d = y[:, 1], y[:, 2], y[:, 3]
    s2, c2 = np.sin(q2), np.cos(q2)
    w1, w2 = q1d, q1d + q2d
    w1s, w2s = w1 * w1, w2 * w2
    a12 = p.h * c2
    m00, m01, m11 = (p.a11 + p.a22) + 2.0 * a12 + p.arm, a12 + p.a22, p.a22 + p.arm
    hs = p.h * s2
    ca1, ca2 = -hs * w2s, hs * w1s
    return m00, m01, m11, ca1, ca2


def rc_terms(s, p=RC):
    """(M [E, 2, 2], c [E, 2]) of M qdd = B u - c - D qd + tau_lim."""
    m00, m01, m11, ca1, ca2 = _rc_parts(s, p)
    z = np.zeros_like(m00)
    M = np.stack([np.stack([m00, m01], axis=1), np.stack([m01, z + m11], axis=1)], axis=1)
    return M, np.stack([ca1 + ca2, ca2], axis=1)


def rc_dsdt(y, tq, p=RC):
    """y [E, 4] = (th1, th2, th1d, th2d), tq [E, 2] the hinge torques."""
    q2, q1d, q2d = y[:, 1], y[:, 2], y[:, 3]
    m00, m01, m11, ca1, ca2 = _rc_parts(y, p)
    r0 = tq[:, 0] - (ca1 + ca2) - p.damp * q1d
    r1 = tq[:, 1] - ca2 - p.damp * q2d + limit(q2, q2d, p.hlim, p.kh, p.ch)
    l10 = m01 / m00
    d1 = m11 - l10 * l10 * m00
    y1 = r1 - l10 * r0
    a1 = y1 / d1
    a0 = r0 / m00 - l10 * a1
    return np.stack([q1d, q2d, a0, a1], axis=1)


def rc_tip(s, p=RC):
    """Fingertip minus goal."""
    s1, c1 = np.sin(s[:, 0]), np.cos(s[:, 0])
    s12, c12 = np.sin(s[:, 0] + s[:, 1]), np.cos(s[:, 0] + s[:, 1])
    return (p.l * c1 + p.tip * c12) - s[:, 4], (p.l * s1 + p.tip * s12) - s[:, 5]


def rc_step(s, a, p=RC):
    """s [E, 6] float64, a [E, 2] (float32 values) -> (s', reward, done)."""
    a, tq = _control(a, p)
    dx, dy = rc_tip(s, p)
    rew = -np.sqrt(dx * dx + dy * dy) - (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
    y = s[:, :4]
    for _ in range(p.frame_skip):
        y = rk4(y, p.dt, lambda v: rc_dsdt(v, tq, p))
    return np.concatenate([y, s[:, 4:]], axis=1), rew, np.zeros(len(s), dtype=bool)


def rc_obs(s, p=RC):
    dx, dy = rc_tip(s, p)
    return np.stack([np.cos(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 0]), np.sin(s[:, 1]), s[:, 4], s[:, 5],
                     s[:, 2], s[:, 3], dx, dy, np.zeros(len(s))], axis=1)


# ---------------------------------------------------------------- Swimmer-v2
SW = Model(ns=10, nq=5, dt=0.01, frame_skip=4, gear=150.0, ctrl=1.0, arm=0.1, hlim=100.0 * PI / 180.0,
           rho=4000.0, beta=0.1, r=0.1, l=1.0)
SW_A = ((1.0, 0.0, 0.0), (0.5, -0.5, 0.0), (0.5, -1.0, -0.5))  # v_b = (xd, yd) + sum_k A[b][k] n_k w_k


def sw_reset(u):
    return u[..., :10] * 0.2 - 0.1


def sw_obs(s):
    return s[:, 2:].copy()


def sw_fluid(vl, vn, w, p=SW):
    """The inertia-box fluid force on one body: along the capsule, across it, the z torque."""
    fl = -p.vis_f * vl - p.ql * (np.abs(vl) * vl)
    fn = -p.vis_f * vn - p.qn * (np.abs(vn) * vn)
    tq = -p.vis_t * w - p.qt * (np.abs(w) * w)
    return fl, fn, tq


def _sw_parts(y, p):
    """(M lower triangle as a 5x5 list of [E] arrays, the velocity terms (cx, cy, cp0, cp1,
    cp2) in the absolute rates, sin, cos and rate of the three absolute angles)."""
    phi = [y[:, 2], y[:, 2] + y[:, 3], (y[:, 2] + y[:, 3]) + y[:, 4]]
    w = [y[:, 7], y[:, 7] + y[:, 8], (y[:, 7] + y[:, 8]) + y[:, 9]]
    sn, cs = [np.sin(f) for f in phi], [np.cos(f) for f in phi]
    ws0, ws1, ws2 = w[0] * w[0], w[1] * w[1], w[2] * w[2]
    c01, s01 = cs[0] * cs[1] + sn[0] * sn[1], sn[1] * cs[0] - cs[1] * sn[0]
    c02, s02 = cs[0] * cs[2] + sn[0] * sn[2], sn[2] * cs[0] - cs[2] * sn[0]
    c12, s12 = cs[1] * cs[2] + sn[1] * sn[2], sn[2] * cs[1] - cs[2] * sn[1]
    ax0, ax1, ax2 = -p.s0 * sn[0], -p.s1 * sn[1], -p.s2 * sn[2]
    ay0, ay1, ay2 = p.s0 * cs[0], p.s1 * cs[1], p.s2 * cs[2]
    a01, a02, a12 = p.c01 * c01, p.c02 * c02, p.c12 * c12
    z = np.zeros_like(a01)
    M = [[None] * 5 for _ in range(5)]
    m33 = (p.j1 + p.j2) + 2.0 * a12
    M[0][0] = z + p.mt
    M[1][0] = z
    M[1][1] = z + p.mt
    M[4][0] = ax2
    M[3][0] = ax1 + ax2
    M[2][0] = ax0 + M[3][0]
    M[4][1] = ay2
    M[3][1] = ay1 + ay2
    M[2][1] = ay0 + M[3][1]
    M[4][4] = z + (p.j2 + p.arm)
    M[4][3] = a12 + p.j2
    M[3][3] = m33 + p.arm
    M[4][2] = a02 + M[4][3]
    M[3][2] = (a01 + a02) + m33
    M[2][2] = p.j0 + 2.0 * (a01 + a02) + m33 + p.arm
    cx = -(p.s0 * cs[0]) * ws0 - (p.s1 * cs[1]) * ws1 - (p.s2 * cs[2]) * ws2
    cy = -(p.s0 * sn[0]) * ws0 - (p.s1 * sn[1]) * ws1 - (p.s2 * sn[2]) * ws2
    cp0 = -((p.c01 * s01) * ws1 + (p.c02 * s02) * ws2)
    cp1 = (p.c01 * s01) * ws0 - (p.c12 * s12) * ws2
    cp2 = (p.c02 * s02) * ws0 + (p.c12 * s12) * ws1
    return M, (cx, cy, cp0, cp1, cp2), sn, cs, w


def sw_terms(s, p=SW):
    """(M [E, 5, 5], c [E, 5]) of M qdd = B u - c + Q_fluid + tau_lim."""
    M, (cx, cy, cp0, cp1, cp2), _, _, _ = _sw_parts(s, p)
    full = np.stack([np.stack([M[max(i, j)][min(i, j)] for j in range(5)], axis=1) for i in range(5)], axis=1)
    return full, np.stack([cx, cy, cp0 + (cp1 + cp2), cp1 + cp2, cp2], axis=1)


def sw_dsdt(y, tq, p=SW):
    """y [E, 10] = q ++ qd, tq [E, 2] the hinge torques."""
    xd, yd = y[:, 5], y[:, 6]
    M, (cx, cy, cp0, cp1, cp2), sn, cs, w = _sw_parts(y, p)
    fx, fy = np.zeros(len(y)), np.zeros(len(y))
    fp = [np.zeros(len(y)) for _ in range(3)]
    for b in range(3):
        vx, vy = xd, yd
        for j in range(b + 1):
            vx = vx - (SW_A[b][j] * w[j]) * sn[j]
            vy = vy + (SW_A[b][j] * w[j]) * cs[j]
        vl, vn = vx * cs[b] + vy * sn[b], vy * cs[b] - vx * sn[b]
        fl, fn, tf = sw_fluid(vl, vn, w[b], p)
        bx, by = fl * cs[b] - fn * sn[b], fl * sn[b] + fn * cs[b]
        fx = fx + bx
        fy = fy + by
        for j in range(b + 1):
            fp[j] = fp[j] + SW_A[b][j] * (by * cs[j] - bx * sn[j])
        fp[b] = fp[b] + tf
    r = [fx - cx,
         fy - cy,
         (fp[0] + (fp[1] + fp[2])) - (cp0 + (cp1 + cp2)),
         tq[:, 0] + (fp[1] + fp[2]) - (cp1 + cp2) + limit(y[:, 3], y[:, 8], p.hlim, p.kh, p.ch),
         tq[:, 1] + fp[2] - cp2 + limit(y[:, 4], y[:, 9], p.hlim, p.kh, p.ch)]
    n = 5
    d = [None] * n
    for j in range(n):
        dj = M[j][j]
        for c in range(j):
            dj = dj - M[j][c] * M[j][c] * d[c]
        d[j] = dj
        for i in range(j + 1, n):
            v = M[i][j]
            for c in range(j):
                v = v - M[i][c] * M[j][c] * d[c]
            M[i][j] = v / dj
    for i in range(1, n):
        for c in range(i):
            r[i] = r[i] - M[i][c] * r[c]
    for i in range(n - 1, -1, -1):
        v = r[i] / d[i]
        for c in range(i + 1, n):
            v = v - M[c][i] * r[c]
        r[i] = v
    return np.stack([y[:, 5 + i] for i in range(5)] + r, axis=1)


def sw_step(s, a, p=SW):
    """s [E, 10] float64, a [E, 2] (float32 values) -> (s', reward, done)."""
    a, tq = _control(a, p)
    xb = s[:, 0]
    for _ in range(p.frame_skip):
        s = rk4(s, p.dt, lambda v: sw_dsdt(v, tq, p))
    rew = (s[:, 0] - xb) / (p.dt * p.frame_skip) - 1e-4 * (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
    return s, rew, np.zeros(len(s), dtype=bool)


def sw_momenta(s, p=SW):
    """The generalised momenta p_x = (M qd)_x, p_y = (M qd)_y, the angular momentum about the
    world's origin L = (M qd)_psi + x p_y - y p_x, and the kinetic energy.  (M qd)_psi alone is
    the angular momentum about the root's origin, which moves: x and y are world coordinates,
    so a rotation of the world turns (x, y) together with psi and Noether's invariant carries
    the x p_y - y p_x term.)"""
    M, _ = sw_terms(s, p)
    v = s[:, 5:]
    mv = np.einsum("eij,ej->ei", M, v)
    ang = mv[:, 2] + s[:, 0] * mv[:, 1] - s[:, 1] * mv[:, 0]
    return mv[:, 0], mv[:, 1], ang, 0.5 * np.einsum("ei,ei->e", v, mv)


# kind -> (model, obs, actions, TimeLimit, reset uniforms, reset, obs, step)
_TABLE = {
    REACHER: (RC, 11, 2, 50, 12, rc_reset, rc_obs, rc_step),
    SWIMMER: (SW, 8, 2, 1000, 10, sw_reset, sw_obs, sw_step),
}


def goal_margin(u):
    """Least |g_x^2 + g_y^2 - 0.04| over every goal candidate of the reset uniforms u."""
    g = rc_candidates(u)
    return float(np.abs(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] - RC_GOAL2).min())


class PlanarEnvs:
    """``oracle.rollout_np.Envs`` for the two planar kinds: the same reset stream (Philox
    domain 1 of (seed, env, episodes started)) and the same bookkeeping.  Neither env ends an
    episode by itself; the one select a last-bit difference could flip is Reacher's goal
    choice, and ``min_margin`` is the least distance of a drawn candidate to the disc's edge
    over every reset so far (infinite for Swimmer)."""

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
        self.fallbacks = 0

    def reset(self, idx):
        u = philox.uniforms(self.seed, 1, self.gid[idx], self.ep_count[idx].astype(np.uint64), self.nu)
        self.state[idx] = self._reset(u)
        if self.kind == REACHER and len(u):
            self.min_margin = min(self.min_margin, goal_margin(u))
            self.fallbacks += int(rc_fallback(u).sum())
        self.ep_count[idx] += 1
        self.ep_t[idx] = 0

    def obs(self):
        return self._obs(self.state)

    def step(self, act):
        self.state, rew, done = self._step(self.state, act)
        return rew, done
