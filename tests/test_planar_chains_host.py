"""Reacher-v2 and Swimmer-v2 without a GPU: the registry and the C ABI know them, and the numpy
twin (tests/planar_chains_np.py) is checked against physics instead of MuJoCo output (parity
with MuJoCo is unpinned): a mass matrix and bias forces assembled body by body from written-out
Jacobians, hand-worked accelerations and fluid forces, the free swimmer's conserved momenta and
energy at RK4's order, the hinge stops' static deflection, Reacher's bounded goal draw, and the
distance every GPU comparison keeps from the goal disc's edge."""
import ctypes

import numpy as np
import pytest

from oracle import philox
from tests import planar_cases as PC
from tests import planar_chains_np as PL

E_ARG = -1


# ------------------------------------------------------------------ M and the bias forces
def _jacobians(kind, s):
    """Per body (mass, inertia, jx, jy, jw, ax, ay) in the relative joint coordinates: the
    centre of mass's position Jacobian rows jx, jy [E, n], the rotation row jw, and the
    velocity-product acceleration (ax, ay) = Jdot qd, each written out by hand."""
    E = len(s)
    one, zero = np.ones(E), np.zeros(E)
    if kind == PL.REACHER:
        p = PL.RC
        t1, t12, w1, w12 = s[:, 0], s[:, 0] + s[:, 1], s[:, 2], s[:, 2] + s[:, 3]

        def point(r2):  # a point r2 along link 2 (link 1's tip is at 0.1)
            return ([-0.1 * np.sin(t1) - r2 * np.sin(t12), -r2 * np.sin(t12)],
                    [0.1 * np.cos(t1) + r2 * np.cos(t12), r2 * np.cos(t12)],
                    -0.1 * np.cos(t1) * w1 ** 2 - r2 * np.cos(t12) * w12 ** 2,
                    -0.1 * np.sin(t1) * w1 ** 2 - r2 * np.sin(t12) * w12 ** 2)

        bodies = [(p.m, p.i, [-0.05 * np.sin(t1), zero], [0.05 * np.cos(t1), zero], [one, zero],
                   -0.05 * np.cos(t1) * w1 ** 2, -0.05 * np.sin(t1) * w1 ** 2)]
        for m, inertia, r2 in ((p.m, p.i, 0.05), (p.ms, p.i_s, 0.11)):
            jx, jy, ax, ay = point(r2)
            bodies.append((m, inertia, jx, jy, [one, one], ax, ay))
        return bodies, 2, p.arm
    p = PL.SW
    f0, f1, f2 = s[:, 2], s[:, 2] + s[:, 3], s[:, 2] + s[:, 3] + s[:, 4]
    w0, w1, w2 = s[:, 7], s[:, 7] + s[:, 8], s[:, 7] + s[:, 8] + s[:, 9]
    bodies = []
    # torso: r + 1.0 e0; mid: r + 0.5 e0 - 0.5 e1; back: r + 0.5 e0 - 1.0 e1 - 0.5 e2
    for k0, k1, k2, jw in ((1.0, 0.0, 0.0, [zero, zero, one, zero, zero]),
                           (0.5, -0.5, 0.0, [zero, zero, one, one, zero]),
                           (0.5, -1.0, -0.5, [zero, zero, one, one, one])):
        dx = [-k0 * np.sin(f0), -k1 * np.sin(f1), -k2 * np.sin(f2)]  # d pos_x / d phi_k
        dy = [k0 * np.cos(f0), k1 * np.cos(f1), k2 * np.cos(f2)]
        jx = [one, zero, dx[0] + dx[1] + dx[2], dx[1] + dx[2], dx[2]]
        jy = [zero, one, dy[0] + dy[1] + dy[2], dy[1] + dy[2], dy[2]]
        ax = -k0 * np.cos(f0) * w0 ** 2 - k1 * np.cos(f1) * w1 ** 2 - k2 * np.cos(f2) * w2 ** 2
        ay = -k0 * np.sin(f0) * w0 ** 2 - k1 * np.sin(f1) * w1 ** 2 - k2 * np.sin(f2) * w2 ** 2
        bodies.append((p.m, p.i, jx, jy, jw, ax, ay))
    return bodies, 5, p.arm


def _per_body(kind, s):
    """M = sum m (Jx^T Jx + Jy^T Jy) + I Jw^T Jw + armature, c = sum m (Jx^T ax + Jy^T ay)."""
    bodies, n, arm = _jacobians(kind, s)
    E = len(s)
    M, c = np.zeros((E, n, n)), np.zeros((E, n))
    for m, inertia, jx, jy, jw, ax, ay in bodies:
        jx, jy, jw = np.stack(jx, axis=1), np.stack(jy, axis=1), np.stack(jw, axis=1)
        M += m * (jx[:, :, None] * jx[:, None, :] + jy[:, :, None] * jy[:, None, :])
        M += inertia * jw[:, :, None] * jw[:, None, :]
        c += m * (jx * ax[:, None] + jy * ay[:, None])
    return M + arm * np.eye(n), c


def _random_states(kind, E, rng):
    if kind == PL.REACHER:
        return np.concatenate([rng.uniform(-np.pi, np.pi, (E, 2)), 2.0 * rng.standard_normal((E, 2)),
                               rng.uniform(-0.2, 0.2, (E, 2))], axis=1)
    return np.concatenate([rng.uniform(-np.pi, np.pi, (E, 5)), 2.0 * rng.standard_normal((E, 5))], axis=1)


@pytest.mark.parametrize("kind", [PL.REACHER, PL.SWIMMER])
def test_mass_matrix_and_bias_match_a_body_by_body_assembly(kind):
    """test_hopper_physics.py's bound (1e-11 of the largest entry), M symmetric positive
    definite at random q, and the LDL^T against numpy's solve with damping, limits, fluid and
    control off."""
    E = 256
    s = _random_states(kind, E, np.random.default_rng(3))
    if kind == PL.REACHER:
        (M, c), n = PL.rc_terms(s), 2
        k = PL.rc_dsdt(s[:, :4], np.zeros((E, 2)), PL.RC.replace(damp=0.0, hlim=1e9))
    else:
        (M, c), n = PL.sw_terms(s), 5
        k = PL.sw_dsdt(s, np.zeros((E, 2)), PL.SW.replace(rho=0.0, beta=0.0, hlim=1e9))
    Mw, cw = _per_body(kind, s)
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert (np.linalg.eigvalsh(M) > 0).all()
    assert (np.abs(M - Mw).max(axis=(1, 2)) / np.abs(Mw).max(axis=(1, 2))).max() < 1e-11
    assert (np.abs(c - cw).max(axis=1) / np.abs(cw).max(axis=1)).max() < 1e-11
    want = np.linalg.solve(Mw, -cw[:, :, None])[:, :, 0]
    assert (np.abs(k[:, n:] - want).max(axis=1) / np.abs(want).max(axis=1)).max() < 1e-11
    np.testing.assert_array_equal(k[:, :n], s[:, n:2 * n])


def test_masses_match_the_stated_figures():
    assert round(PL.RC.m, 4) == 0.0107 and round(PL.RC.ms * 1e3, 2) == 1.26 and round(PL.SW.m, 1) == 35.6
    assert round(PL.SW.bx, 3) == 1.136 and round(PL.SW.by, 3) == 0.171
    for v in (0.03, 1.2, 6.0 * PL.SW.ia / PL.SW.m):  # the constexpr Newton root is the root
        assert abs(PL.csqrt(v) - np.sqrt(v)) <= 2e-16 * np.sqrt(v)


# ------------------------------------------------------------------ Reacher at rest
def test_reacher_at_rest_under_torque_has_the_closed_form_acceleration():
    """At rest every velocity term vanishes; with damping and the stop off, [[a, b], [b, d]]
    (qdd1, qdd2) = (0, tau): qdd1 = -b tau / (a d - b^2), qdd2 = a tau / (a d - b^2), with
    a = A11 + A22 + 2 H cos th2 + 1, b = A22 + H cos th2, d = A22 + 1 worked out here from the
    masses.  tau = gear * clamp(u): u = 0.5 gives 100 N m, u = 7 is clamped to 1 (200 N m)."""
    p = PL.RC.replace(damp=0.0, hlim=1e9)
    m, ms, i, i_s = PL.RC.m, PL.RC.ms, PL.RC.i, PL.RC.i_s
    for th2 in (0.0, 0.7, -2.9):
        h = 0.1 * (m * 0.05 + ms * 0.11) * np.cos(th2)
        d0 = i + m * 0.05 ** 2 + i_s + ms * 0.11 ** 2
        a = i + m * 0.05 ** 2 + (m + ms) * 0.1 ** 2 + d0 + 2.0 * h + 1.0
        b, d = d0 + h, d0 + 1.0
        for u, tau in ((0.5, 100.0), (7.0, 200.0), (-7.0, -200.0)):
            _, tq = PL._control(np.array([[0.0, u]], dtype=np.float32), PL.RC)
            assert tq[0, 0] == 0.0 and tq[0, 1] == tau
            k = PL.rc_dsdt(np.array([[0.3, th2, 0.0, 0.0]]), tq, p)[0]
            det = a * d - b * b
            np.testing.assert_allclose(k, [0.0, 0.0, -b * tau / det, a * tau / det], rtol=1e-12, atol=1e-12)


def test_reacher_at_rest_stays_exactly_at_rest():
    s = np.array([[0.3, -1.2, 0.0, 0.0, 0.1, -0.05], [0.0, 2.5, 0.0, 0.0, -0.1, 0.1]])
    s0 = s.copy()
    for _ in range(50):
        s, rew, done = PL.rc_step(s, np.zeros((2, 2), dtype=np.float32))
        assert not done.any()
        dx, dy = PL.rc_tip(s0)
        np.testing.assert_array_equal(rew, -np.sqrt(dx * dx + dy * dy))
    assert np.array_equal(s, s0)


def test_reacher_reward_uses_the_unclipped_action_and_the_goal_stays():
    s = np.array([[0.1, 0.2, 0.0, 0.0, 0.05, 0.08]])
    a = np.array([[3.0, -2.0]], dtype=np.float32)
    s1, rew, _ = PL.rc_step(s, a)
    dx, dy = PL.rc_tip(s)
    assert rew[0] == -np.sqrt(dx[0] ** 2 + dy[0] ** 2) - 13.0
    np.testing.assert_array_equal(s1[:, 4:], s[:, 4:])
    o = PL.rc_obs(s1)
    assert o.shape == (1, 11) and o[0, 10] == 0.0 and (o[0, 4:6] == s[0, 4:]).all()
    # the clamp: a = 3 moves the arm exactly as a = 1
    np.testing.assert_array_equal(PL.rc_step(s, np.array([[1.0, -1.0]], dtype=np.float32))[0], s1)


# ------------------------------------------------------------------ the free swimmer
def test_swimmer_without_fluid_conserves_momenta_and_energy_at_rk4_order():
    """Fluid and control off, the stops out of reach: translations and rotations of the plane
    are symmetries, so p_x = (M qd)_x, p_y = (M qd)_y and the angular momentum about the
    world's origin L = (M qd)_psi + x p_y - y p_x are conserved, and so is the kinetic energy.
    ((M qd)_psi alone is the angular momentum about the moving root and is not conserved: it
    changes by tens of percent over the window at either step size, ratio 1.0.)  Their largest
    deviation over a fixed window is RK4's global error, O(dt^4): halving dt must cut it by
    more than 8 (16 predicted; 8 is test_mujoco_chains_host.py's margin).  The deviation is the
    window's largest, not the last step's, as there.  Measured: ratios 15.7 to 16.4."""
    rng = np.random.default_rng(5)
    E = 8
    p = PL.SW.replace(rho=0.0, beta=0.0, hlim=1e9)
    s0 = np.concatenate([rng.uniform(-0.5, 0.5, (E, 5)), rng.uniform(-2.0, 2.0, (E, 5))], axis=1)
    q0 = np.stack(PL.sw_momenta(s0, p))
    dev = []
    for halvings in (0, 1):
        ph = p.replace(dt=p.dt / 2 ** halvings, frame_skip=p.frame_skip * 2 ** halvings)
        s, worst = s0.copy(), np.zeros((4, E))
        for _ in range(25):  # 1 s
            s, _, _ = PL.sw_step(s, np.zeros((E, 2), dtype=np.float32), ph)
            worst = np.maximum(worst, np.abs(np.stack(PL.sw_momenta(s, ph)) - q0))
        dev.append(worst)
    ratio = dev[0] / dev[1]
    for name, d0, r in zip(("p_x", "p_y", "L", "T"), dev[0], ratio):
        print("swimmer", name, "deviation", d0, "ratio", r)
    scale = np.abs(q0).max(axis=1, keepdims=True)
    assert (dev[0] > 1e-10).all()  # above rounding (1e-12 here): the ratio means something
    assert (dev[0] < 1e-3 * scale).all()
    assert (ratio > 8.0).all(), ratio


# ------------------------------------------------------------------ the fluid model
def test_fluid_force_on_a_single_body_matches_the_box_formula():
    """Hand-computed from the capsule: m = 1000 (pi r^2 l + 4/3 pi r^3), I_t and I_a of the
    cylinder and the two half-spheres, box sides b = sqrt(6 (I_j + I_k - I_i) / m), then at
    1 m/s sideways f = -(3 pi beta d + 1/2 rho b_x b_z) and at 1 rad/s about z
    tau = -(pi beta d^3 + rho b_z (b_x^4 + b_y^4) / 64)."""
    r, l, rho, beta = 0.1, 1.0, 4000.0, 0.1
    mc, msph = 1000.0 * np.pi * r * r * l, 1000.0 * 4.0 / 3.0 * np.pi * r ** 3
    m = mc + msph
    it = mc * (r * r / 4 + l * l / 12) + msph * (2 * r * r / 5 + l * l / 4 + 3 * l * r / 8)
    ia = mc * r * r / 2 + msph * 2 * r * r / 5
    bx, by = np.sqrt(6 * (2 * it - ia) / m), np.sqrt(6 * ia / m)
    d = (bx + 2 * by) / 3
    one, zero = np.ones(1), np.zeros(1)
    fl, fn, tq = PL.sw_fluid(zero, one, zero)
    np.testing.assert_allclose(fn, -(3 * np.pi * beta * d + 0.5 * rho * bx * by), rtol=1e-12)
    assert fl[0] == 0.0 and tq[0] == 0.0
    fl, fn, tq = PL.sw_fluid(zero, zero, one)
    np.testing.assert_allclose(tq, -(np.pi * beta * d ** 3 + rho * by * (bx ** 4 + by ** 4) / 64), rtol=1e-12)
    assert fl[0] == 0.0 and fn[0] == 0.0
    fl, fn, tq = PL.sw_fluid(-2.0 * one, zero, zero)  # along the capsule, the other way: odd in v
    np.testing.assert_allclose(fl, 2 * 3 * np.pi * beta * d + 0.5 * rho * by * by * 4.0, rtol=1e-12)
    # through the dynamics: the swimmer straight, drifting sideways at 1 m/s, every body feels fn
    s = np.zeros((1, 10))
    s[0, 6] = 1.0
    k = PL.sw_dsdt(s, np.zeros((1, 2)), PL.SW.replace(hlim=1e9))
    f1 = -(3 * np.pi * beta * d + 0.5 * rho * bx * by)
    M, _ = PL.sw_terms(s)
    np.testing.assert_allclose((M[0] @ k[0, 5:])[:2], [0.0, 3 * f1], rtol=1e-12, atol=1e-9)


def test_fluid_dissipates_the_kinetic_energy_monotonically():
    rng = np.random.default_rng(7)
    E = 16
    s = np.concatenate([rng.uniform(-0.5, 0.5, (E, 5)), rng.uniform(-1.0, 1.0, (E, 5))], axis=1)
    p = PL.SW.replace(hlim=1e9)
    t_prev = PL.sw_momenta(s, p)[3]
    t0 = t_prev.copy()
    for _ in range(25):
        s, _, _ = PL.sw_step(s, np.zeros((E, 2), dtype=np.float32), p)
        t = PL.sw_momenta(s, p)[3]
        assert (t < t_prev).all()
        t_prev = t
    print("swimmer kinetic energy after 1 s in the fluid / at the start", t_prev / t0)
    assert (t_prev < 0.5 * t0).all()


# ------------------------------------------------------------------ the hinge stops
@pytest.mark.parametrize("kind,side", [(PL.REACHER, 1), (PL.REACHER, -1), (PL.SWIMMER, 1), (PL.SWIMMER, -1)])
def test_hinge_stop_settles_on_the_static_deflection(kind, side):
    """The limited hinge starts at rest on its stop and its motor pushes it in at full control,
    tau = gear * ctrl.  It settles where the stop's spring balances the motor, tau / k past the
    stop: the settled deflection is asserted within 5 % of tau / k."""
    if kind == PL.REACHER:
        p, step, col = PL.RC, PL.rc_step, 1
        s = np.array([[0.2, side * p.hlim, 0.0, 0.0, 0.1, 0.1]])
        act = np.array([[0.0, side * 2.0]], dtype=np.float32)
        n_steps = 200  # 4 s
    else:
        p, step, col = PL.SW, PL.sw_step, 3
        s = np.zeros((1, 10))
        s[0, 3] = side * p.hlim
        act = np.array([[side * 2.0, 0.0]], dtype=np.float32)
        n_steps = 200  # 8 s
    static = p.gear * p.ctrl / p.kh
    pen = []
    for _ in range(n_steps):
        s, _, _ = step(s, act, p)
        pen.append(side * s[0, col] - p.hlim)
    pen = np.array(pen)
    print(kind, side, "static", static, "max deflection", pen.max(), "overshoot", pen.max() / static - 1.0,
          "final", pen[-1], "final / static", pen[-1] / static)
    assert np.isfinite(s).all()
    assert abs(pen[-1] / static - 1.0) < 0.05
    assert 0.0 < pen.max() <= 2.0 * static  # a spring-damper's step response overshoots less than 2x


# ------------------------------------------------------------------ Reacher's reset
def test_reacher_reset_draws_a_goal_inside_the_disc_with_a_rare_fallback():
    n = 100000
    u = philox.uniforms(3, 1, np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), 12)
    s = PL.rc_reset(u)
    assert s.shape == (n, 6)
    assert (np.abs(s[:, :2]) <= 0.1).all() and np.abs(s[:, :2]).max() > 0.0999
    assert (np.abs(s[:, 2:4]) <= 0.005).all() and np.abs(s[:, 2:4]).max() > 0.00499
    norm = np.sqrt(s[:, 4] ** 2 + s[:, 5] ** 2)
    assert (norm < 0.2).all() and norm.max() > 0.199
    fb = PL.rc_fallback(u)
    print("reacher reset: fallbacks", int(fb.sum()), "of", n, "expected", n * (1 - np.pi / 4) ** 4)
    assert 1 <= fb.sum() <= 0.01 * n
    g = PL.rc_candidates(u)
    inside = (g[..., 0] ** 2 + g[..., 1] ** 2) < 0.04
    first = np.argmax(inside, axis=1)
    rows = np.arange(n)
    np.testing.assert_array_equal(s[~fb, 4:], g[rows, first][~fb])  # the first candidate inside
    np.testing.assert_array_equal(s[fb, 4:], 0.5 * g[fb, 3])  # none inside: the fourth, halved
    assert (first[~fb] > 0).any()  # a later candidate is taken when the first is outside
    # the envs class draws the same state from the same stream
    e = PL.PlanarEnvs(PL.REACHER, 64, 3)
    e.reset(np.arange(64))
    np.testing.assert_array_equal(e.state, s[:64])


def test_swimmer_reset_draws_the_stated_distribution():
    e = PL.PlanarEnvs(PL.SWIMMER, 4000, 3)
    e.reset(np.arange(4000))
    assert e.state.shape == (4000, 10) and (np.abs(e.state) <= 0.1).all() and np.abs(e.state).max() > 0.0999
    assert np.abs(np.corrcoef(e.state.T) - np.eye(10)).max() < 0.08
    np.testing.assert_array_equal(e.obs(), e.state[:, 2:])
    assert e.min_margin == np.inf


def test_swimmer_reward_is_the_displacement_across_the_step():
    s = np.zeros((1, 10))
    s[0, 5] = 0.5
    a = np.array([[2.0, -3.0]], dtype=np.float32)
    s1, rew, done = PL.sw_step(s, a)
    assert rew[0] == (s1[0, 0] - s[0, 0]) / (0.01 * 4) - 1e-4 * 13.0 and not done[0]


def test_twin_has_the_oracle_envs_duck_type():
    from oracle import rollout_np as RO
    ref = RO.Envs(RO.CARTPOLE, 3, 0)
    for kind, ns, O in ((PL.REACHER, 6, 11), (PL.SWIMMER, 10, 8)):
        e = PL.PlanarEnvs(kind, 3, 0, env_offset=2)
        for name in ("kind", "E", "seed", "gid", "ns", "O", "A", "max_steps", "nu", "state", "ep_t", "ep_count"):
            assert type(getattr(e, name)) is type(getattr(ref, name)), name
        assert e.nu % 2 == 0 and e.gid.tolist() == [2, 3, 4] and (e.ns, e.O, e.A) == (ns, O, 2)
        e.reset(np.arange(3))
        assert e.obs().shape == (3, O) and e.state.shape == (3, ns) and e.ep_count.tolist() == [1, 1, 1]


# ------------------------------------------------------------------ the GPU tests' seeds
@pytest.mark.parametrize("env_id,E,Tn,limit", PC.ALL_STEP_CASES)
def test_step_cases_keep_clear_of_the_goal_edge(env_id, E, Tn, limit):
    """The GPU tests ask for the twin's goals: on their seeds no candidate drawn lies within
    1e-6 of the disc's edge (|g_x^2 + g_y^2 - 0.04|), so a last-bit difference cannot pick
    another one; and episodes end inside the run."""
    _, steps, least = PC.reference_steps(env_id, E, Tn, limit)
    assert least > PC.MARGIN, least
    assert sum(len(s["idx"]) for s in steps) > 0
    assert (np.abs(PC.step_actions(env_id, E, Tn)) > PC.ACT_HIGH[env_id]).any()  # the control clamp is hit
    assert all(np.isfinite(s["state"]).all() and np.isfinite(s["rew"]).all() for s in steps)


@pytest.mark.parametrize("E,Tn,limit,inject", PC.ROLLOUT_CASES)
@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_rollout_cases_keep_clear_of_the_goal_edge(env_id, E, Tn, limit, inject):
    _, _, its = PC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    assert min(m for _, _, _, m in its) > PC.MARGIN
    assert all(np.isfinite(w["obs"]).all() and np.isfinite(w["rew"]).all() for w, _, _, _ in its)


def test_layered_case_cuts_inside_the_horizon():
    env_id, hid, E, Tn, limit = PC.LAYERED_CASE
    _, _, its = PC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert min(m for _, _, _, m in its) > PC.MARGIN
    assert any((w["flags"][:-1] & 1).any() for w, _, _, _ in its)


@pytest.mark.parametrize("env_id", PC.ENV_IDS)
def test_population_case_keeps_clear_of_the_goal_edge(env_id):
    rows, ended, least = PC.reference_population(env_id)
    assert rows == PC.POP_N * PC.POP_LIMIT and ended == 0 and least > PC.MARGIN, (rows, ended, least)
    # the seeds of the other GPU cases that reset Reacher: written-state test (19), persistent (31)
    for seed, E, episodes in ((19, 70, 2), (31, 100, 4), (31, 40, 5), (PC.POP_SEEDS[env_id], PC.POP_N, 1)):
        e = PL.PlanarEnvs(env_id, E, seed)
        for _ in range(episodes):
            e.reset(np.arange(E))
        assert e.min_margin > PC.MARGIN


# ------------------------------------------------------------------ registry and ABI
@pytest.mark.parametrize("env_id,kind,obs,limit", [("Reacher-v2", 12, 11, 50), ("Swimmer-v2", 11, 8, 1000)])
def test_registry_describes_the_env(env_id, kind, obs, limit):
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import Box, make
    env = make(env_id)
    assert env.kind == kind == {12: _lib.ENV_REACHER, 11: _lib.ENV_SWIMMER}[kind] == PL.KINDS[env_id]
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (obs,)
    assert env.obs_dim == obs and env.spec.max_episode_steps == limit and env.spec.id == env_id
    assert isinstance(env.action_space, Box) and env.action_space.shape == (2,)
    np.testing.assert_array_equal(env.action_space.high, np.full(2, 1.0, np.float32))
    np.testing.assert_array_equal(env.action_space.low, np.full(2, -1.0, np.float32))
    assert not env.discrete and env.act_dim == 2
    assert PC.SHAPES[env_id] == (obs, 2, False, limit) and PC.KIND_IDS[env_id] == kind and PC.ACT_HIGH[env_id] == 1.0
    assert PL._TABLE[kind][1:5] == (obs, 2, limit, {12: 12, 11: 10}[kind])  # reset uniforms


@pytest.mark.parametrize("kind,ns,obs", [(12, 6, 11), (11, 10, 8)])
def test_abi_sizes(kind, ns, obs):
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert lib.mrl_env_state_doubles(kind) == ns
    assert lib.mrl_filter_doubles(kind) == 2 + 2 * (obs + 1)
    assert lib.mrl_record_doubles(kind) == 2 + 2 * (obs + 1)
    desc = _lib.RolloutDesc(kind, 10, 7, 200, 0, 0, 0, 0, 0)
    assert lib.mrl_rollout_noise_doubles(ctypes.byref(desc)) == 7 * 10 * 2  # two normals a row
    assert lib.mrl_rollout_sync_bytes(ctypes.byref(desc)) == 256 + 2 * (obs + 1) * 1 * 16


@pytest.mark.parametrize("entry", ["mrl_env_reset", "mrl_env_step"])
def test_env_entries_take_the_new_ids(entry):
    """env_id 11 and 12 pass the argument checks that env_id 3 fails: with n_envs = 0 the
    complaint is about n_envs (the checks run before any HIP call); 3, 7, 10 and 13 are no
    envs (tests/test_mujoco_chains_host.py holds 10 to that, so Reacher is 12)."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bufs = _lib.RolloutBufs(env_state=p, env_int=p)
    io = _lib.EnvIO(p, None, p, p, p, p, None)
    tail = (None,) if entry == "mrl_env_reset" else (1, None)
    for env_id, needle in ((11, "n_envs"), (12, "n_envs"), (3, "env_id"), (7, "env_id"), (10, "env_id"),
                           (13, "env_id")):
        desc = _lib.RolloutDesc(env_id, 0, 1, 200, 0, 0, 0, 0, 0)
        rc = getattr(lib, entry)(ctypes.byref(desc), ctypes.byref(bufs), ctypes.byref(io), *tail)
        msg = lib.mrl_last_error().decode()
        assert rc == E_ARG and needle in msg, (env_id, rc, msg)
        assert needle == "env_id" or "env_id" not in msg, (env_id, msg)


def test_small_population_net_fits_for_the_new_ids():
    from modular_rl_amd import _lib
    lib = _lib.load()
    hid = (ctypes.c_int32 * 2)(10, 5)
    for kind, obs in ((12, 11), (11, 8)):
        assert lib.mrl_pop_rollout_mlp_fits(kind, hid, 2) == 1
        assert lib.mrl_pop_mlp_num_params(kind, hid, 2) == obs * 10 + 10 + 10 * 5 + 5 + 5 * 2 + 2 + 2
