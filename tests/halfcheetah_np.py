"""float64 numpy twin of the planar tree env on the device (test helper, not collected):
HalfCheetah-v2 in the operation order of ``modular_rl_amd/csrc/envs_tree.h`` (which documents
the model and its constants), and ``TreeEnvs``, which has the duck type of
``oracle.rollout_np.Envs`` so that ``oracle.rollout_np.collect`` and the VecEnv comparison loop
run on it unchanged.

The dynamics (``tree_substep``) are written once over a ``Model`` table with a parent index per
body; ``HC`` is HalfCheetah's table and ``hopper_model()`` restates ``oracle.envs``' Hopper as a
second one (the CPU tests step it against ``oracle.envs.hopper_step``).  The physics tests step
copies with other values (``HC.replace(floor=False, damp=...)``)."""
import numpy as np

from oracle import philox
from tests.mujoco_chains_np import PI, _clamp, capsule_inertia, capsule_mass

HALFCHEETAH = 14
KINDS = {"HalfCheetah-v2": HALFCHEETAH}
KC, CC, CF = 20000.0, 400.0, 1000.0  # Hopper's contact: N/m, N s/m, N s/m (clipped to mu fn)
KH, CH = 2000.0, 50.0                # the hinge stop: N m/rad, N m s/rad
GRAV = 9.81


def csin(a):
    """tr_sin: the sine's series, 24 terms (the constexpr table takes the same steps)."""
    t, s = a, a
    for k in range(1, 25):
        t = -t * a * a / float((2 * k) * (2 * k + 1))
        s = s + t
    return s


def ccos(a):
    t, s = 1.0, 1.0
    for k in range(1, 25):
        t = -t * a * a / float((2 * k - 1) * (2 * k))
        s = s + t
    return s


class Model:
    """One tree: bodies 0 .. nb-1 with parent[b] < b (body 0 hangs on rootx / rootz / rooty),
    hinge b >= 1 is coordinate 2 + b and takes action b - 1.  ``replace`` returns a copy with
    some fields changed (the derived ones are worked out again)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.derive()

    def replace(self, **kw):
        base = {k: v for k, v in self.__dict__.items() if k not in ("msub", "sax", "saz", "jc", "pairs", "nq")}
        return Model(**{**base, **kw})

    def derive(self):
        p, nb = self, self.nb
        p.nq = nb + 2
        # subtree masses, and per body the constants of its own frame: sa = m c + sum over the
        # children of (their subtree mass) (their hinge), jc = I + m |c|^2 + the same with |hinge|^2
        p.msub = list(p.mass)
        p.sax = [p.mass[b] * p.comx[b] for b in range(nb)]
        p.saz = [p.mass[b] * p.comz[b] for b in range(nb)]
        p.jc = [p.inertia[b] + p.mass[b] * (p.comx[b] * p.comx[b] + p.comz[b] * p.comz[b]) for b in range(nb)]
        for b in range(nb - 1, 0, -1):
            a = p.parent[b]
            p.sax[a] = p.sax[a] + p.msub[b] * p.px[b]
            p.saz[a] = p.saz[a] + p.msub[b] * p.pz[b]
            p.jc[a] = p.jc[a] + p.msub[b] * (p.px[b] * p.px[b] + p.pz[b] * p.pz[b])
            p.msub[a] = p.msub[a] + p.msub[b]
        # (ancestor a, descendant d, a's child on the way to d)
        p.pairs = []
        for d in range(1, nb):
            c, a = d, p.parent[d]
            while True:
                p.pairs.append((a, d, c))
                if a == 0:
                    break
                c, a = a, p.parent[a]


# ---------------------------------------------------------------- HalfCheetah-v2: the table
HC_R = 0.046
# geom: body, half-length, angle about y (None: along x), centre (x, z)
HC_GEOMS = ((0, 0.5, None, 0.0, 0.0), (0, 0.15, 0.87, 0.6, 0.1), (1, 0.145, -3.8, 0.1, -0.13),
            (2, 0.15, -2.03, -0.14, -0.07), (3, 0.094, -0.27, 0.03, -0.097), (4, 0.133, 0.52, -0.07, -0.12),
            (5, 0.106, -0.6, 0.065, -0.09), (6, 0.07, -0.6, 0.045, -0.07))
HC_TOTAL = 14.0


def _hc_table():
    raw_m = [capsule_mass(HC_R, 2.0 * g[1]) for g in HC_GEOMS]
    raw_i = [capsule_inertia(HC_R, 2.0 * g[1]) for g in HC_GEOMS]
    tot = raw_m[0]
    for k in range(1, 8):
        tot = tot + raw_m[k]
    sc = HC_TOTAL / tot
    gm, gi = [m * sc for m in raw_m], [i * sc for i in raw_i]
    # the torso body: its own capsule and the head, by the parallel-axis theorem
    m0 = gm[0] + gm[1]
    cx, cz = (gm[1] * 0.6) / m0, (gm[1] * 0.1) / m0
    i0 = (gi[0] + gi[1]) + (gm[0] * (cx * cx + cz * cz) + gm[1] * ((0.6 - cx) * (0.6 - cx) + (0.1 - cz) * (0.1 - cz)))
    mass, inertia = [m0] + gm[2:], [i0] + gi[2:]
    comx, comz = [cx] + [g[3] for g in HC_GEOMS[2:]], [cz] + [g[4] for g in HC_GEOMS[2:]]
    spheres = []  # (body, u, w, radius, friction): the two ends of each capsule
    for body, hl, ang, x, z in HC_GEOMS:
        ax, az = (1.0, 0.0) if ang is None else (csin(ang), ccos(ang))
        spheres.append((body, x + hl * ax, z + hl * az, HC_R, 0.4))
        spheres.append((body, x - hl * ax, z - hl * az, HC_R, 0.4))
    return mass, inertia, comx, comz, tuple(spheres)


_m, _i, _cx, _cz, _sph = _hc_table()
HC = Model(nb=7, parent=(0, 0, 1, 2, 0, 4, 5), sgn=(1.0,) * 7,
           px=(0.0, -0.5, 0.16, -0.28, 0.5, -0.14, 0.13), pz=(0.0, 0.0, -0.25, -0.14, 0.0, -0.24, -0.18),
           comx=_cx, comz=_cz, mass=_m, inertia=_i, mt=HC_TOTAL, z0=0.7, spheres=_sph,
           arm=(0.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1), stiff=(0.0, 240.0, 180.0, 120.0, 180.0, 120.0, 60.0),
           damp=(0.0, 6.0, 4.5, 3.0, 4.5, 3.0, 1.5), lo=(0.0, -0.52, -0.785, -0.4, -1.0, -1.2, -0.5),
           hi=(0.0, 1.05, 0.785, 0.785, 0.7, 0.87, 0.5), gear=(0.0, 120.0, 90.0, 60.0, 120.0, 60.0, 30.0),
           kl=KH, cl=CH, kc=KC, cc=CC, cf=CF, grav=GRAV, dt=0.00125, nsub=40, floor=True, ctrl=1.0)
HC_NS, HC_OBS, HC_ACT, HC_NU, HC_MAX_STEPS = 18, 17, 6, 20, 1000
HC_STEP = 0.05  # MuJoCo's timestep 0.01 x frame_skip 5


def hopper_model():
    """oracle.envs' Hopper as a table: a chain whose hinges turn the other way (sgn -1)."""
    from oracle import envs as EV
    sph = tuple((k, u, w, EV.HP_RAD[k], EV.HP_MU[k]) for k in range(4) for (u, w) in EV.HP_CAP[k])
    return Model(nb=4, parent=(0, 0, 1, 2), sgn=(1.0, -1.0, -1.0, -1.0), px=(0.0, 0.0, 0.0, 0.0),
                 pz=(0.0, -EV.HP_SEG[0], -EV.HP_SEG[1], -EV.HP_SEG[2]), comx=[c[0] for c in EV.HP_COM],
                 comz=[c[1] for c in EV.HP_COM], mass=list(EV.HP_MASS), inertia=list(EV.HP_INERTIA), mt=EV.HP_MB[0],
                 z0=0.0, spheres=sph, arm=(0.0, EV.HP_ARM, EV.HP_ARM, EV.HP_ARM), stiff=(0.0,) * 4,
                 damp=(0.0, EV.HP_DAMP, EV.HP_DAMP, EV.HP_DAMP), lo=(0.0,) + EV.HP_LO, hi=(0.0,) + EV.HP_HI,
                 gear=(0.0, EV.HP_GEAR, EV.HP_GEAR, EV.HP_GEAR), kl=EV.HP_KL, cl=EV.HP_CL, kc=EV.HP_KC, cc=EV.HP_CC,
                 cf=EV.HP_CF, grav=EV.HP_GRAV, dt=EV.HP_DT, nsub=EV.HP_FRAME_SKIP, floor=True, ctrl=1.0)


# ---------------------------------------------------------------- the tree dynamics
def tree_frames(q, v, p):
    """Absolute angles and rates, their sin / cos, and the world vectors of every body: S (its
    frame's mass moment sa turned), G (its hinge in the parent's frame, turned)."""
    nb = p.nb
    phi, om = [q[2]], [v[2]]
    for b in range(1, nb):
        a = p.parent[b]
        phi.append(phi[a] + p.sgn[b] * q[2 + b])
        om.append(om[a] + p.sgn[b] * v[2 + b])
    sn, cs = [np.sin(f) for f in phi], [np.cos(f) for f in phi]
    Sx = [p.sax[b] * cs[b] + p.saz[b] * sn[b] for b in range(nb)]
    Sz = [p.saz[b] * cs[b] - p.sax[b] * sn[b] for b in range(nb)]
    Gx, Gz = [None] * nb, [None] * nb
    for b in range(1, nb):
        a = p.parent[b]
        Gx[b] = p.px[b] * cs[a] + p.pz[b] * sn[a]
        Gz[b] = p.pz[b] * cs[a] - p.px[b] * sn[a]
    return om, sn, cs, Sx, Sz, Gx, Gz


def tree_contacts(q, v, om, sn, cs, Gx, Gz, p):
    """Per body the contact force sum (x, z) and its moment about the body's hinge, and the
    normal force and depth of every sphere."""
    nb = p.nb
    zero = np.zeros_like(q[0])
    Pz, Vx, Vz = [q[1] + p.z0], [v[0]], [v[1]]
    for b in range(1, nb):
        a = p.parent[b]
        Pz.append(Pz[a] + Gz[b])
        Vx.append(Vx[a] + om[a] * Gz[b])
        Vz.append(Vz[a] - om[a] * Gx[b])
    Fx, Fz, N = [zero] * nb, [zero] * nb, [zero] * nb
    fns, pens = [], []
    if p.floor:
        for (b, u, w, rad, mu) in p.spheres:
            ox = u * cs[b] + w * sn[b]
            oz = (w * cs[b] - u * sn[b]) - rad
            pen = -(Pz[b] + oz)
            vx = Vx[b] + om[b] * oz
            vz = Vz[b] - om[b] * ox
            fnr = p.kc * pen - p.cc * vz
            fn = np.where(pen > 0.0, np.where(fnr > 0.0, fnr, 0.0), 0.0)
            lim = mu * fn
            fv = p.cf * vx
            fl = np.where(fv > -lim, fv, -lim)
            ft = -np.where(fl < lim, fl, lim)
            Fx[b] = Fx[b] + ft
            Fz[b] = Fz[b] + fn
            N[b] = N[b] + (oz * ft - ox * fn)
            fns.append(fn)
            pens.append(pen)
    return Fx, Fz, N, fns, pens


def tree_terms(q, v, p):
    """(rx, rz, Qs, U, SXs, SZs): the translational right-hand sides, the absolute-angle
    generalised forces summed over subtrees (contact + gravity - velocity terms), the
    absolute-angle inertia summed over both subtrees, and the subtree sums of S."""
    nb = p.nb
    om, sn, cs, Sx, Sz, Gx, Gz = tree_frames(q, v, p)
    Fx, Fz, N, _, _ = tree_contacts(q, v, om, sn, cs, Gx, Gz, p)
    zero = np.zeros_like(q[0])
    w2 = [om[b] * om[b] for b in range(nb)]
    Qa = [N[b] + p.grav * Sx[b] for b in range(nb)]
    Fsx, Fsz = list(Fx), list(Fz)
    for b in range(nb - 1, 0, -1):
        a = p.parent[b]
        Qa[a] = Qa[a] + (Gz[b] * Fsx[b] - Gx[b] * Fsz[b])
        Fsx[a] = Fsx[a] + Fsx[b]
        Fsz[a] = Fsz[a] + Fsz[b]
    # the inertia in the absolute angles (only a body and its ancestors couple) and the
    # velocity terms
    U = [[zero] * nb for _ in range(nb)]
    ca = [zero] * nb
    for b in range(nb):
        U[b][b] = zero + p.jc[b]
    for (a, d, c) in p.pairs:
        X = Gx[c] * Sx[d] + Gz[c] * Sz[d]
        Y = Gz[c] * Sx[d] - Gx[c] * Sz[d]
        U[a][d] = X
        U[d][a] = X
        ca[d] = ca[d] + w2[a] * Y
        ca[a] = ca[a] - w2[d] * Y
    cx, cz = zero, zero
    for b in range(nb):
        cx = cx - w2[b] * Sx[b]
        cz = cz - w2[b] * Sz[b]
    rx = Fsx[0] - cx
    rz = (Fsz[0] - cz) - p.mt * p.grav
    Qs = [Qa[b] - ca[b] for b in range(nb)]
    SXs, SZs = list(Sx), list(Sz)
    for b in range(nb - 1, 0, -1):
        a = p.parent[b]
        Qs[a] = Qs[a] + Qs[b]
        SXs[a] = SXs[a] + SXs[b]
        SZs[a] = SZs[a] + SZs[b]
        for j in range(nb):
            U[j][a] = U[j][a] + U[j][b]
    for b in range(nb - 1, 0, -1):
        a = p.parent[b]
        for j in range(nb):
            U[a][j] = U[a][j] + U[b][j]
    return rx, rz, Qs, U, SXs, SZs


def joint_force(q, v, tau, b, p):
    """Motor, spring, damper and the one-sided stops of hinge b."""
    j = 2 + b
    cv = p.cl * v[j]
    flo, fhi = p.kl * (p.lo[b] - q[j]) - cv, p.kl * (p.hi[b] - q[j]) - cv
    lim = np.where(q[j] < p.lo[b], flo, np.where(q[j] > p.hi[b], fhi, 0.0))
    return ((tau[b - 1] - p.stiff[b] * q[j]) - p.damp[b] * v[j]) + lim


def tree_system(q, v, tau, p):
    """The rotational block C (upper triangle, armature added), the coupling rows B0 / B1 and
    the right-hand sides of [[mt I, B], [B^T, C]] qdd = (rx, rz, r)."""
    nb = p.nb
    rx, rz, Qs, U, SXs, SZs = tree_terms(q, v, p)
    r = [Qs[0]] + [p.sgn[b] * Qs[b] + joint_force(q, v, tau, b, p) for b in range(1, nb)]
    C = [[None] * nb for _ in range(nb)]
    for a in range(nb):
        for b in range(a, nb):
            C[a][b] = (p.sgn[a] * p.sgn[b]) * U[a][b]
        C[a][a] = C[a][a] + p.arm[a]
    B0 = [p.sgn[b] * SZs[b] for b in range(nb)]
    B1 = [-(p.sgn[b] * SXs[b]) for b in range(nb)]
    return rx, rz, r, C, B0, B1


def tree_solve(rx, rz, r, C, B0, B1, p):
    """Schur complement of the translational block, LDL^T of the nb x nb rest."""
    n = p.nb
    imt = 1.0 / p.mt
    K = [[None] * n for _ in range(n)]
    for a in range(n):
        for b in range(a, n):
            K[b][a] = C[a][b] - (B0[a] * B0[b] + B1[a] * B1[b]) * imt
    x = [r[a] - (B0[a] * rx + B1[a] * rz) * imt for a in range(n)]
    d = [None] * n
    for j in range(n):
        dj = K[j][j]
        for c in range(j):
            dj = dj - K[j][c] * K[j][c] * d[c]
        d[j] = dj
        for i in range(j + 1, n):
            val = K[i][j]
            for c in range(j):
                val = val - K[i][c] * K[j][c] * d[c]
            K[i][j] = val / dj
    for i in range(1, n):
        for c in range(i):
            x[i] = x[i] - K[i][c] * x[c]
    for i in range(n - 1, -1, -1):
        val = x[i] / d[i]
        for c in range(i + 1, n):
            val = val - K[c][i] * x[c]
        x[i] = val
    tx, tz = rx, rz
    for a in range(n):
        tx = tx - B0[a] * x[a]
        tz = tz - B1[a] * x[a]
    return [tx * imt, tz * imt] + x


def tree_substep(q, v, tau, p):
    """One dt, semi-implicit Euler.  q, v: lists of nq arrays [E]; tau: list of nb - 1."""
    qdd = tree_solve(*tree_system(q, v, tau, p), p)
    v2 = [v[i] + p.dt * qdd[i] for i in range(p.nq)]
    q2 = [q[i] + p.dt * v2[i] for i in range(p.nq)]
    return q2, v2


def tree_mass_matrix(s, p):
    """M [E, nq, nq] in the joint coordinates, armature included."""
    nq = p.nq
    q, v = [s[:, i] for i in range(nq)], [s[:, nq + i] for i in range(nq)]
    _, _, _, C, B0, B1 = tree_system(q, v, [np.zeros(len(s))] * (p.nb - 1), p)
    M = np.zeros((len(s), nq, nq))
    M[:, 0, 0] = M[:, 1, 1] = p.mt
    for a in range(p.nb):
        M[:, 0, 2 + a] = M[:, 2 + a, 0] = B0[a]
        M[:, 1, 2 + a] = M[:, 2 + a, 1] = B1[a]
        for b in range(a, p.nb):
            M[:, 2 + a, 2 + b] = M[:, 2 + b, 2 + a] = C[a][b]
    return M


def tree_rhs(s, tau, p):
    """The right-hand side [E, nq] of M qdd = rhs."""
    nq = p.nq
    q, v = [s[:, i] for i in range(nq)], [s[:, nq + i] for i in range(nq)]
    rx, rz, r, _, _, _ = tree_system(q, v, tau, p)
    return np.stack([rx, rz] + r, axis=1)


def tree_step(s, tau, p):
    """nsub substeps of the state s [E, 2 nq] under the hinge torques tau (list of [E])."""
    nq = p.nq
    q, v = [s[:, i] for i in range(nq)], [s[:, nq + i] for i in range(nq)]
    with np.errstate(all="ignore"):
        for _ in range(p.nsub):
            q, v = tree_substep(q, v, tau, p)
    return np.stack(q + v, axis=1)


def tree_normal_forces(s, p):
    """(fn [E, spheres], depth [E, spheres]) of the state s."""
    nq = p.nq
    q, v = [s[:, i] for i in range(nq)], [s[:, nq + i] for i in range(nq)]
    om, sn, cs, _, _, Gx, Gz = tree_frames(q, v, p)
    _, _, _, fns, pens = tree_contacts(q, v, om, sn, cs, Gx, Gz, p)
    return np.stack(fns, axis=1), np.stack(pens, axis=1)


# ---------------------------------------------------------------- HalfCheetah-v2: the env
def hc_reset(u):
    """u [..., 20] uniforms: u0..u8 -> q = U(-0.1, 0.1), the pairs (u10, u11) .. (u18, u19) ->
    Box-Muller normals (oracle/philox.py's transform), nine of the ten -> qd = 0.1 N(0, 1)."""
    q = u[..., :9] * 0.2 - 0.1
    z = []
    for k in range(5):
        r = np.sqrt(-2.0 * np.log(1.0 - u[..., 10 + 2 * k]))
        a = 2.0 * PI * u[..., 11 + 2 * k]
        z += [0.1 * (r * np.cos(a)), 0.1 * (r * np.sin(a))]
    return np.concatenate([q, np.stack(z[:9], axis=-1)], axis=-1)


def hc_obs(s):
    return s[:, 1:].copy()


def hc_control(a, p=HC):
    """a [E, 6] (float32 values) -> (the unclipped actions as float64, the hinge torques)."""
    a = np.asarray(a, dtype=np.float32).reshape(-1, p.nb - 1).astype(np.float64)
    ac = _clamp(a, -p.ctrl, p.ctrl)
    return a, [p.gear[b] * ac[:, b - 1] for b in range(1, p.nb)]


def hc_step(s, a, p=HC):
    """s [E, 18] float64, a [E, 6] (float32 values) -> (s', reward, done)."""
    a, tau = hc_control(a, p)
    asq = a[:, 0] * a[:, 0]
    for k in range(1, 6):
        asq = asq + a[:, k] * a[:, k]
    xb = s[:, 0]
    s = tree_step(s, tau, p)
    rew = (s[:, 0] - xb) / HC_STEP - 0.1 * asq
    return s, rew, np.zeros(len(s), dtype=bool)


class TreeEnvs:
    """``oracle.rollout_np.Envs`` for HalfCheetah: the same reset stream (Philox domain 1 of
    (seed, env, episodes started)) and the same bookkeeping.  The env never ends an episode by
    itself, so there is no termination threshold to keep clear of.  The contact and stop forces
    are continuous in position; their dampers switch on at the threshold (f_n jumps by
    -CC v_z where a sphere enters the floor moving down, the stop force by -CH v where a hinge
    passes its stop), so a last-bit difference could still flip a branch there.  The comparisons
    at 1e-5 keep no margin against it: the state would have to sit within an ulp of a threshold."""

    def __init__(self, kind, E, seed, env_offset=0):
        kind = KINDS.get(kind, kind)
        assert kind == HALFCHEETAH
        self.kind, self.E, self.seed = kind, E, seed
        self.gid = np.arange(E, dtype=np.uint64) + np.uint64(env_offset)
        self.model, self.O, self.A, self.max_steps, self.nu = HC, HC_OBS, HC_ACT, HC_MAX_STEPS, HC_NU
        self.ns = HC_NS
        self.discrete = False
        self.state = np.zeros((E, self.ns))
        self.ep_t = np.zeros(E, dtype=np.int64)
        self.ep_count = np.zeros(E, dtype=np.int64)

    def reset(self, idx):
        u = philox.uniforms(self.seed, 1, self.gid[idx], self.ep_count[idx].astype(np.uint64), self.nu)
        self.state[idx] = hc_reset(u)
        self.ep_count[idx] += 1
        self.ep_t[idx] = 0

    def obs(self):
        return hc_obs(self.state)

    def step(self, act):
        self.state, rew, done = hc_step(self.state, act, self.model)
        return rew, done
