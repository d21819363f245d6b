"""HalfCheetah-v2 without a GPU: the numpy twin (tests/halfcheetah_np.py) is checked against
physics instead of MuJoCo output (parity with MuJoCo is unpinned) -- the kinetic energy and the
bias forces by two independent routes (finite differences of a separately written forward
kinematics, a body-by-body assembly from written-out Jacobians), the table-driven tree code on
Hopper's table against oracle.envs.hopper_step, free flight's conserved momenta and its
first-order energy error, the stability conditions that chose HC_DT, the stated figures and the
env's semantics -- and the registry and the C ABI know the env."""
import ctypes

import numpy as np
import pytest

from oracle import envs as EV
from oracle import philox
from tests import halfcheetah_cases as HCC
from tests import halfcheetah_np as H

E_ARG = -1
HC = H.HC
FREE = dict(floor=False, damp=(0.0,) * 7, lo=(-1e9,) * 7, hi=(1e9,) * 7)  # no floor, damping or stops


def _random_states(E, rng, speed=2.0):
    q = np.concatenate([rng.uniform(-1.0, 1.0, (E, 2)), rng.uniform(-np.pi, np.pi, (E, 7))], axis=1)
    return np.concatenate([q, speed * rng.standard_normal((E, 9))], axis=1)


# ------------------------------------------------------------------ an independent forward kinematics
PARENT = {"torso": None, "bthigh": "torso", "bshin": "bthigh", "bfoot": "bshin", "fthigh": "torso",
          "fshin": "fthigh", "ffoot": "fshin"}
FRAME = {"bthigh": (-0.5, 0.0), "bshin": (0.16, -0.25), "bfoot": (-0.28, -0.14), "fthigh": (0.5, 0.0),
         "fshin": (-0.14, -0.24), "ffoot": (0.13, -0.18)}
NAMES = ("torso", "bthigh", "bshin", "bfoot", "fthigh", "fshin", "ffoot")


def _turn(ang, u, w):
    """A positive angle about +y turns +z towards +x."""
    return u * np.cos(ang) + w * np.sin(ang), w * np.cos(ang) - u * np.sin(ang)


def _fk(q):
    """name -> (frame origin x, z, absolute angle) from q [E, 9], written body by body from the
    model table of csrc/envs_tree.h's header comment (not from the twin's)."""
    out = {"torso": (q[:, 0], q[:, 1] + 0.7, q[:, 2])}
    for i, name in enumerate(NAMES[1:]):
        px, pz, pa = out[PARENT[name]]
        dx, dz = _turn(pa, *FRAME[name])
        out[name] = (px + dx, pz + dz, pa + q[:, 3 + i])
    return out


def _coms(q):
    """Centres of mass [E, 7, 2] and absolute angles [E, 7]."""
    fk = _fk(q)
    pos, ang = [], []
    for b, name in enumerate(NAMES):
        x, z, a = fk[name]
        dx, dz = _turn(a, HC.comx[b], HC.comz[b])
        pos.append(np.stack([x + dx, z + dz], axis=1))
        ang.append(a)
    return np.stack(pos, axis=1), np.stack(ang, axis=1)


def _potential(q):
    pos, _ = _coms(q)
    return (np.array(HC.mass) * 9.81 * pos[:, :, 1]).sum(axis=1) + 0.5 * (np.array(HC.stiff[1:]) * q[:, 3:] ** 2).sum(axis=1)


def _no_armature(M):
    return M - np.diag([0.0, 0.0] + list(HC.arm))


# ------------------------------------------------------------------ 1. kinetic energy
def test_kinetic_energy_matches_finite_differences_of_an_independent_kinematics():
    """1/2 qd^T M qd (armature removed) against sum 1/2 m |v|^2 + 1/2 I w^2 with v from central
    differences (step 1e-6) of the centres of mass: 1e-7 relative."""
    rng = np.random.default_rng(11)
    s = _random_states(256, rng)
    q, qd = s[:, :9], s[:, 9:]
    M = _no_armature(H.tree_mass_matrix(s, HC))
    ke = 0.5 * np.einsum("ei,eij,ej->e", qd, M, qd)
    h = 1e-6
    pp, ap = _coms(q + h * qd)
    pm, am = _coms(q - h * qd)
    v, w = (pp - pm) / (2 * h), (ap - am) / (2 * h)
    want = 0.5 * (np.array(HC.mass) * (v ** 2).sum(axis=2)).sum(axis=1) + 0.5 * (np.array(HC.inertia) * w ** 2).sum(axis=1)
    rel = np.abs(ke - want) / want
    print("kinetic energy: largest relative difference", rel.max())
    assert rel.max() < 1e-7


# ------------------------------------------------------------------ 2. bias forces
def test_force_at_rest_is_minus_the_gradient_of_the_potential_energy():
    """Contact, damping, limits and control off, qd = 0: the generalised force equals minus the
    numerical gradient of sum m g z + 1/2 sum k q^2 (central differences, step 1e-6; the bound
    is the difference quotient's error, 1e-7 of the largest component)."""
    rng = np.random.default_rng(12)
    s = _random_states(64, rng, speed=0.0)
    p = HC.replace(**FREE)
    f = H.tree_rhs(s, [np.zeros(64)] * 6, p)
    h = 1e-6
    grad = np.zeros((64, 9))
    for i in range(9):
        d = np.zeros(9)
        d[i] = h
        grad[:, i] = (_potential(s[:, :9] + d) - _potential(s[:, :9] - d)) / (2 * h)
    err = np.abs(f + grad).max(axis=1) / np.abs(grad).max(axis=1)
    print("force at rest + grad V: largest relative difference", err.max())
    assert err.max() < 1e-7


def _jacobians(s):
    """Per body (m, I, jx, jz, jw, ax, az): the centre of mass's Jacobian rows [E, 9], the
    rotation row, and the velocity-product acceleration Jdot qd, from the chain of turned
    offsets root -> body written out here."""
    E = len(s)
    q, qd = s[:, :9], s[:, 9:]
    fk = _fk(q)
    one, zero = np.ones(E), np.zeros(E)
    chains = {"torso": ["torso"]}
    for name in NAMES[1:]:
        chains[name] = chains[PARENT[name]] + [name]
    rate = {"torso": qd[:, 2]}
    for i, name in enumerate(NAMES[1:]):
        rate[name] = rate[PARENT[name]] + qd[:, 3 + i]
    bodies = []
    for b, name in enumerate(NAMES):
        chain = chains[name]
        # the turned offset carried by each body of the chain: its child's frame, or the com
        offs = [_turn(fk[c][2], *FRAME[chain[k + 1]]) for k, c in enumerate(chain[:-1])]
        offs.append(_turn(fk[name][2], HC.comx[b], HC.comz[b]))
        jx, jz, jw = [one, zero] + [zero] * 7, [zero, one] + [zero] * 7, [zero] * 9
        ax, az = zero, zero
        for k, c in enumerate(chain):
            ex, ez = offs[k]
            # d e / d angle = (e_z, -e_x); joint j moves every body of the chain from j on
            for c2 in chain[:k + 1]:
                col = 2 + NAMES.index(c2)
                jx[col] = jx[col] + ez
                jz[col] = jz[col] - ex
            ax = ax - rate[c] ** 2 * ex
            az = az - rate[c] ** 2 * ez
        for c in chain:
            jw[2 + NAMES.index(c)] = one
        bodies.append((HC.mass[b], HC.inertia[b], jx, jz, jw, ax, az))
    return bodies


def test_mass_matrix_and_bias_match_a_body_by_body_assembly():
    """M = sum m (Jx^T Jx + Jz^T Jz) + I Jw^T Jw + armature, the velocity terms
    c = sum m (Jx^T ax + Jz^T az), gravity sum m g Jz^T: test_hopper_physics.py's bound (1e-11 of
    the largest entry), M symmetric positive definite, and the Schur + LDL^T solve against
    numpy's."""
    E = 256
    s = _random_states(E, np.random.default_rng(3))
    Mw, cw = np.zeros((E, 9, 9)), np.zeros((E, 9))
    for m, inertia, jx, jz, jw, ax, az in _jacobians(s):
        jx, jz, jw = np.stack(jx, axis=1), np.stack(jz, axis=1), np.stack(jw, axis=1)
        Mw += m * (jx[:, :, None] * jx[:, None, :] + jz[:, :, None] * jz[:, None, :])
        Mw += inertia * jw[:, :, None] * jw[:, None, :]
        cw += m * (jx * ax[:, None] + jz * (az[:, None] + 9.81))
    Mw = Mw + np.diag([0.0, 0.0] + list(HC.arm))
    cw[:, 3:] += np.array(HC.stiff[1:]) * s[:, 3:9]
    p = HC.replace(**FREE)
    M = H.tree_mass_matrix(s, p)
    f = H.tree_rhs(s, [np.zeros(E)] * 6, p)
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert (np.linalg.eigvalsh(M) > 0).all()
    assert (np.abs(M - Mw).max(axis=(1, 2)) / np.abs(Mw).max(axis=(1, 2))).max() < 1e-11
    assert (np.abs(f + cw).max(axis=1) / np.abs(cw).max(axis=1)).max() < 1e-11
    q, v = [s[:, i] for i in range(9)], [s[:, 9 + i] for i in range(9)]
    qdd = np.stack(H.tree_solve(*H.tree_system(q, v, [np.zeros(E)] * 6, p), p), axis=1)
    want = np.linalg.solve(Mw, -cw[:, :, None])[:, :, 0]
    assert (np.abs(qdd - want).max(axis=1) / np.abs(want).max(axis=1)).max() < 1e-10


# ------------------------------------------------------------------ 3. the tree code on Hopper's chain
HOPPER_MEASURED = 4.0e-15  # largest |difference| over the 256 states, as measured (this test prints it)


def test_tree_code_steps_hoppers_table_as_the_oracle_does():
    """The table-driven dynamics on oracle.envs' Hopper (hinges of the other sign through the
    table) against oracle.envs.hopper_step, one env step from 256 sampled states.  Both are
    fp64 evaluations of the same equations in a different operation order; the bound is 100
    times the largest difference measured (far below 1e-8: rounding, not formulation)."""
    hp = H.hopper_model()
    rng = np.random.default_rng(0)
    E = 256
    q = np.zeros((E, 6))
    q[:, 0] = rng.uniform(-1.0, 1.0, E)
    q[:, 1] = rng.uniform(0.85, 1.3, E)
    q[:, 2] = rng.uniform(-0.3, 0.3, E)
    q[:, 3:5] = rng.uniform(-1.5, 0.1, (E, 2))   # past the upper stop at 0 for some
    q[:, 5] = rng.uniform(-0.9, 0.9, E)          # past either stop (+-0.785) for some
    v = rng.standard_normal((E, 6))
    s = np.concatenate([q, v], axis=1)
    _, pen = H.tree_normal_forces(s, hp)
    in_floor = (pen > 0).any(axis=1)
    past = (q[:, 3:] < np.array(EV.HP_LO)).any(axis=1) | (q[:, 3:] > np.array(EV.HP_HI)).any(axis=1)
    assert in_floor.mean() >= 0.25 and past.sum() >= 16 and (~in_floor).sum() >= 16
    a = (1.5 * rng.standard_normal((E, 3))).astype(np.float32)
    q2, v2, _, _ = EV.hopper_step(q, v, a)
    tau = [EV.HP_GEAR * np.clip(a[:, k].astype(np.float64), -1.0, 1.0) for k in range(3)]
    got = H.tree_step(s, tau, hp)
    diff = np.abs(got - np.concatenate([q2, v2], axis=1)).max()
    print("tree code on Hopper's table: largest difference", diff, "in the floor", in_floor.mean(),
          "past a stop", int(past.sum()))
    assert diff <= 100 * HOPPER_MEASURED


# ------------------------------------------------------------------ 4. free flight
def _momenta(s, p, t):
    M = H.tree_mass_matrix(s, p)
    mv = np.einsum("eij,ej->ei", M, s[:, 9:])
    energy = 0.5 * np.einsum("ei,ei->e", s[:, 9:], mv) + _potential(s[:, :9])
    return mv[:, 0], mv[:, 1] + p.mt * p.grav * t, energy


def test_free_flight_conserves_momentum_and_energy_up_to_the_integrators_first_order():
    """No floor, damping, limits or control; the joint springs stay on.  p_x = (M qd)_x,
    p_z + M g t and the energy (kinetic with the armature, gravity, springs) are invariants of
    the equations of motion: their time derivative along (qd, qdd) vanishes to the central
    difference quotient's own error.  That error is rounding: each quantity is a sum of some 50
    rounded products of its scale, so two evaluations differ by up to 50 eps scale and the
    quotient over 2h, h = 1e-6, by 50 eps scale / h = 1.1e-8 scale per second (the truncation
    term, h^2 times a third derivative, is smaller).  The integrator does not conserve the two
    momenta to rounding as well, and cannot: rootx and rootz are the
    torso's coordinates, not the centre of mass's, so semi-implicit Euler -- v += dt qdd with
    M(q_old), then q += dt v -- leaves M(q_new) v_new off M(q_old) v_new by O(dt), exactly as
    it does the energy.  All three deviations over a fixed window halve with the substep:
    ratio in [1.7, 2.3].  Measured: momenta 1.995 to 2.016, energy 1.976 to 1.993."""
    rng = np.random.default_rng(5)
    E = 8
    s0 = np.concatenate([rng.uniform(-0.3, 0.3, (E, 9)), rng.uniform(-1.0, 1.0, (E, 9))], axis=1)
    zero = [np.zeros(E)] * 6
    free = HC.replace(**FREE)
    q, v = [s0[:, i] for i in range(9)], [s0[:, 9 + i] for i in range(9)]
    qdd = np.stack(H.tree_solve(*H.tree_system(q, v, zero, free), free), axis=1)
    h = 1e-6
    fwd = _momenta(np.concatenate([s0[:, :9] + h * s0[:, 9:], s0[:, 9:] + h * qdd], axis=1), free, h)
    bwd = _momenta(np.concatenate([s0[:, :9] - h * s0[:, 9:], s0[:, 9:] - h * qdd], axis=1), free, -h)
    rate = np.abs(np.stack(fwd) - np.stack(bwd)) / (2 * h)
    scale = np.abs(np.stack(_momenta(s0, free, 0.0))).max(axis=1, keepdims=True)
    print("free flight: d/dt of p_x, p_z + M g t, E", rate.max(axis=1), "scale", scale[:, 0])
    assert (rate < 50 * np.finfo(np.float64).eps * scale / h).all()
    dev = []
    for halvings in (0, 1):
        p = HC.replace(dt=HC.dt / 2 ** halvings, nsub=HC.nsub * 2 ** halvings, **FREE)
        first = np.stack(_momenta(s0, p, 0.0))
        s, worst = s0.copy(), np.zeros((3, E))
        for k in range(4):  # 0.2 s
            s = H.tree_step(s, zero, p)
            worst = np.maximum(worst, np.abs(np.stack(_momenta(s, p, 0.05 * (k + 1))) - first))
        dev.append(worst)
    ratio = dev[0] / dev[1]
    for name, d0, r in zip(("p_x", "p_z + M g t", "E"), dev[0], ratio):
        print("free flight", name, "deviation", d0, "ratio", r)
    assert (dev[0] > 1e-6).all()  # above rounding: the ratio means something
    assert (dev[0] < 0.1 * scale).all()
    assert ((ratio > 1.7) & (ratio < 2.3)).all(), ratio


# ------------------------------------------------------------------ 5. stability: what chose HC_DT
MG = 14.0 * 9.81


@pytest.fixture(scope="module")
def long_run():
    """1000 steps from reset of 64 envs under each of: zero actions, 3-sigma normal actions,
    actions held at +-1 (one batch of 192 rows), and as row 192 a cheetah set down at rest with
    zero action: the step at which it reached static equilibrium."""
    E = 64
    envs = H.TreeEnvs("HalfCheetah-v2", E, 7)
    envs.reset(np.arange(E))
    rest = np.zeros((1, 18))
    _, pen = H.tree_normal_forces(rest, HC)
    rest[0, 1] = pen.max()  # lifted until its lowest sphere touches the floor
    s = np.concatenate([envs.state] * 3 + [rest], axis=0)
    rng = np.random.default_rng(1)
    held = np.sign(rng.standard_normal((E, 6)))
    finite, settled = True, None
    for t in range(2000):
        if t >= 1000 and settled is not None:
            break
        if t < 1000:
            a = np.concatenate([np.zeros((E, 6)), 3.0 * rng.standard_normal((E, 6)), held, np.zeros((1, 6))], axis=0)
            s, _, done = H.hc_step(s, a.astype(np.float32))
            finite = finite and bool(np.isfinite(s).all()) and not done.any()
            last = s
        else:  # only the set-down row goes on
            s, _, _ = H.hc_step(s[-1:], np.zeros((1, 6), np.float32))
        fn, pen = H.tree_normal_forces(s[-1:], HC)
        if settled is None and abs(fn.sum() / MG - 1.0) < 1e-6 and np.abs(s[-1, 9:]).max() < 1e-6:
            settled = (t + 1, fn.sum(), pen.max(), s[-1].copy())
    return finite, last, settled, (fn.sum(), pen.max(), np.abs(s[-1, 9:]).max())


def test_states_stay_finite_for_1000_steps_under_zero_noisy_and_held_actions(long_run):
    finite, last, _, _ = long_run
    print("after 1000 steps: largest |state| under zero / 3-sigma / held actions",
          [float(np.abs(last[64 * k:64 * (k + 1)]).max()) for k in range(3)])
    assert finite and np.isfinite(last).all()


def test_cheetah_set_down_at_rest_reaches_static_equilibrium(long_run):
    """sum f_n = M g to 1e-6 relative and no sphere deeper than M g / HP_KC (6.9 mm: one sphere
    carrying the whole weight).  Observed at HC_DT = 0.01 / 8: settled after 744 steps (37 s:
    the slow mode is the passive legs creeping on their springs against the friction), depth
    3.6 mm.  At 0.01 / 4 and 0.01 / 5 the contacts chatter and it never settles, which is what
    ruled those substeps out."""
    _, _, settled, final = long_run
    print("set down at rest: settled (step, sum fn, depth)", None if settled is None else settled[:3], "final", final)
    assert settled is not None, final
    steps, fsum, depth, _ = settled
    assert steps <= 2000 and abs(fsum / MG - 1.0) < 1e-6 and 0.0 < depth < MG / H.KC


# ------------------------------------------------------------------ 6. figures and semantics
def test_masses_and_inertias_match_the_stated_figures():
    assert HC.mt == 14.0 and abs(sum(HC.mass) - 14.0) < 1e-14 * 14.0
    want_m = (6.2502, 1.5435, 1.5874, 1.0954, 1.4381, 1.2008, 0.88452)
    want_i = (0.89712, 0.016844, 0.018267, 0.0063524, 0.013740, 0.0082221, 0.0035291)
    for b in range(7):
        assert abs(HC.mass[b] / want_m[b] - 1.0) < 1e-4 and abs(HC.inertia[b] / want_i[b] - 1.0) < 1e-4, b
    assert round(HC.comx[0], 4) == 0.1524 and round(HC.comz[0], 4) == 0.0254
    # the torso by hand: two capsules of radius 0.046, lengths 1.0 and 0.3, at the same density
    r = 0.046
    vol = [np.pi * r * r * 2 * h + 4.0 / 3.0 * np.pi * r ** 3 for h in (0.5, 0.15, 0.145, 0.15, 0.094, 0.133, 0.106, 0.07)]
    np.testing.assert_allclose(HC.mass[0], 14.0 * (vol[0] + vol[1]) / sum(vol), rtol=1e-13)
    np.testing.assert_allclose(HC.mass[6], 14.0 * vol[7] / sum(vol), rtol=1e-13)
    for a in (0.87, -3.8, -2.03, -0.27, 0.52, -0.6):  # the constexpr series are the functions
        assert abs(H.csin(a) - np.sin(a)) < 4e-16 and abs(H.ccos(a) - np.cos(a)) < 4e-16
    assert len(HC.spheres) == 16 and len(HC.pairs) == 12 and HC.dt * HC.nsub == 0.05


def test_every_hinge_stop_settles_on_its_static_deflection():
    """Floating without gravity or floor and with the joint springs off (against its own spring
    no motor reaches its stop: 240 N m/rad x 1.05 rad > 120 N m), each hinge in turn starts at
    rest on a stop and its motor pushes it in at full control.  It settles where the stop's
    spring balances the motor, gear / k_l past the stop, on both sides of every hinge (the
    ranges are asymmetric).  The stop's damper (50 N m s/rad on less than 1 kg m^2) has died
    out long before 5 s: 1e-6 relative."""
    p = HC.replace(floor=False, grav=0.0, stiff=(0.0,) * 7)
    s = np.zeros((12, 18))
    a = np.zeros((12, 6), dtype=np.float32)
    want = np.zeros(12)
    for b in range(1, 7):
        for k, (side, stop) in enumerate(((1.0, p.hi[b]), (-1.0, p.lo[b]))):
            row = 2 * (b - 1) + k
            s[row, 2 + b] = stop
            a[row, b - 1] = 2.0 * side
            want[row] = p.gear[b] / p.kl
    for _ in range(100):
        s, _, _ = H.hc_step(s, a, p)
    got = np.array([(s[2 * (b - 1) + k, 2 + b] - stop) * side for b in range(1, 7)
                    for k, (side, stop) in enumerate(((1.0, p.hi[b]), (-1.0, p.lo[b])))])
    print("hinge stops: deflection / static", got / want)
    assert (want > 0).all() and np.abs(got / want - 1.0).max() < 1e-6
    assert np.abs(s[:, 12:]).max() < 1e-6  # the hinges are at rest (the floating root drifts at O(dt))


def test_reward_uses_the_unclipped_action_and_the_displacement_and_done_is_never_set():
    rng = np.random.default_rng(2)
    s = _random_states(16, rng, speed=1.0)
    s[:, 1] = 0.5
    a = (3.0 * rng.standard_normal((16, 6))).astype(np.float32)
    s1, rew, done = H.hc_step(s, a)
    a64 = a.astype(np.float64)
    np.testing.assert_allclose(rew, (s1[:, 0] - s[:, 0]) / 0.05 - 0.1 * (a64 ** 2).sum(axis=1), rtol=1e-13, atol=1e-13)
    assert not done.any() and (np.abs(a) > 1.0).any()
    np.testing.assert_array_equal(H.hc_step(s, np.clip(a, -1.0, 1.0))[0], s1)  # the clamp: same motion
    np.testing.assert_array_equal(H.hc_obs(s1), s1[:, 1:])
    bad = s.copy()
    bad[0, 3] = np.nan
    assert not H.hc_step(bad, a)[2].any()


def test_reset_draws_the_stated_distributions():
    n = 100000
    u = philox.uniforms(3, 1, np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), 20)
    s = H.hc_reset(u)
    assert s.shape == (n, 18)
    q, v = s[:, :9], s[:, 9:]
    assert (np.abs(q) <= 0.1).all() and np.abs(q).max() > 0.0999
    np.testing.assert_allclose(q.std(axis=0), 0.2 / np.sqrt(12.0), rtol=0.02)
    np.testing.assert_allclose(v.std(axis=0), 0.1, rtol=0.02)
    assert np.abs(v.mean(axis=0)).max() < 0.002 and np.abs(q.mean(axis=0)).max() < 0.001
    assert np.abs(np.corrcoef(s.T) - np.eye(18)).max() < 0.02
    np.testing.assert_array_equal(q, u[:, :9] * 0.2 - 0.1)
    r = np.sqrt(-2.0 * np.log(1.0 - u[:, 10]))
    np.testing.assert_array_equal(v[:, 0], 0.1 * (r * np.cos(2.0 * H.PI * u[:, 11])))
    np.testing.assert_array_equal(v[:, 1], 0.1 * (r * np.sin(2.0 * H.PI * u[:, 11])))
    e = H.TreeEnvs("HalfCheetah-v2", 64, 3)
    e.reset(np.arange(64))
    np.testing.assert_array_equal(e.state, s[:64])


def test_twin_has_the_oracle_envs_duck_type():
    from oracle import rollout_np as RO
    ref = RO.Envs(RO.CARTPOLE, 3, 0)
    e = H.TreeEnvs(H.HALFCHEETAH, 3, 0, env_offset=2)
    for name in ("kind", "E", "seed", "gid", "ns", "O", "A", "max_steps", "nu", "state", "ep_t", "ep_count"):
        assert type(getattr(e, name)) is type(getattr(ref, name)), name
    assert e.nu % 2 == 0 and e.gid.tolist() == [2, 3, 4] and (e.ns, e.O, e.A, e.nu) == (18, 17, 6, 20)
    e.reset(np.arange(3))
    assert e.obs().shape == (3, 17) and e.state.shape == (3, 18) and e.ep_count.tolist() == [1, 1, 1]
    rew, done = e.step(np.zeros((3, 6), np.float32))
    assert rew.shape == (3,) and done.dtype == bool and not done.any()


# ------------------------------------------------------------------ 7. registry and ABI
def test_registry_describes_the_env():
    """HalfCheetah is id 14: tests/test_planar_chains_host.py holds 13 to be no env, and
    existing tests stay as they are."""
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import Box, make
    env = make("HalfCheetah-v2")
    assert env.kind == 14 == _lib.ENV_HALFCHEETAH == H.KINDS["HalfCheetah-v2"]
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (17,)
    assert env.obs_dim == 17 and env.spec.max_episode_steps == 1000 and env.spec.id == "HalfCheetah-v2"
    assert isinstance(env.action_space, Box) and env.action_space.shape == (6,)
    np.testing.assert_array_equal(env.action_space.high, np.full(6, 1.0, np.float32))
    np.testing.assert_array_equal(env.action_space.low, np.full(6, -1.0, np.float32))
    assert not env.discrete and env.act_dim == 6
    assert (HCC.OBS, HCC.ACT, HCC.NS, HCC.LIMIT) == (17, 6, 18, 1000)


def test_abi_sizes():
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert lib.mrl_env_state_doubles(14) == 18
    assert lib.mrl_filter_doubles(14) == 2 + 2 * 18
    assert lib.mrl_record_doubles(14) == 2 + 2 * 18
    desc = _lib.RolloutDesc(14, 10, 7, 200, 0, 0, 0, 0, 0)
    assert lib.mrl_rollout_noise_doubles(ctypes.byref(desc)) == 7 * 10 * 6
    assert lib.mrl_rollout_sync_bytes(ctypes.byref(desc)) == 256 + 2 * 18 * 1 * 16


@pytest.mark.parametrize("entry", ["mrl_env_reset", "mrl_env_step"])
def test_env_entries_take_the_new_id(entry):
    """env_id 14 passes the argument checks that env_id 3 fails: with n_envs = 0 the complaint
    is about n_envs (the checks run before any HIP call); 3, 7, 10, 13 and 15 are no envs."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bufs = _lib.RolloutBufs(env_state=p, env_int=p)
    io = _lib.EnvIO(p, None, p, p, p, p, None)
    tail = (None,) if entry == "mrl_env_reset" else (1, None)
    for env_id, needle in ((14, "n_envs"), (3, "env_id"), (7, "env_id"), (10, "env_id"), (13, "env_id"),
                           (15, "env_id")):
        desc = _lib.RolloutDesc(env_id, 0, 1, 200, 0, 0, 0, 0, 0)
        rc = getattr(lib, entry)(ctypes.byref(desc), ctypes.byref(bufs), ctypes.byref(io), *tail)
        msg = lib.mrl_last_error().decode()
        assert rc == E_ARG and needle in msg, (env_id, rc, msg)
        assert needle == "env_id" or "env_id" not in msg, (env_id, msg)


def test_small_population_net_fits():
    from modular_rl_amd import _lib
    lib = _lib.load()
    hid = (ctypes.c_int32 * 2)(10, 5)
    assert lib.mrl_pop_rollout_mlp_fits(14, hid, 2) == 1
    assert lib.mrl_pop_mlp_num_params(14, hid, 2) == 17 * 10 + 10 + 10 * 5 + 5 + 5 * 6 + 6 + 6
    for bad in (3, 7, 10, 13):
        assert lib.mrl_pop_rollout_mlp_fits(bad, hid, 2) == E_ARG
