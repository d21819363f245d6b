"""InvertedPendulum-v2 and InvertedDoublePendulum-v2 without a GPU: the registry and the C ABI
know them, and the numpy twin (tests/mujoco_chains_np.py) is checked against physics instead
of MuJoCo output (parity with MuJoCo is unpinned): hand-worked accelerations, a mass matrix and
bias forces assembled body by body, RK4's energy-drift order, the slider stop, the envs' own
terminations, and the distance every GPU comparison keeps from a termination threshold."""
import ctypes

import numpy as np
import pytest

from tests import chain_cases as CC
from tests import mujoco_chains_np as MC

E_ARG = -1
FREE = dict(damp=0.0, xlim=1e9)  # no dissipation, the stops out of reach


# ------------------------------------------------------------------ registry and ABI
@pytest.mark.parametrize("env_id,kind,obs,high", [("InvertedPendulum-v2", 8, 4, 3.0),
                                                  ("InvertedDoublePendulum-v2", 9, 11, 1.0)])
def test_registry_describes_the_env(env_id, kind, obs, high):
    from modular_rl_amd import _lib
    from modular_rl_amd.envs import Box, make
    env = make(env_id)
    assert env.kind == kind == {8: _lib.ENV_INVPENDULUM, 9: _lib.ENV_INVDOUBLEPENDULUM}[kind] == MC.KINDS[env_id]
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (obs,)
    assert env.obs_dim == obs and env.spec.max_episode_steps == 1000 and env.spec.id == env_id
    assert isinstance(env.action_space, Box) and env.action_space.shape == (1,)
    np.testing.assert_array_equal(env.action_space.high, np.full(1, high, np.float32))
    np.testing.assert_array_equal(env.action_space.low, np.full(1, -high, np.float32))
    assert not env.discrete and env.act_dim == 1
    assert CC.SHAPES[env_id] == (obs, 1, False, 1000) and CC.KIND_IDS[env_id] == kind and CC.ACT_HIGH[env_id] == high


@pytest.mark.parametrize("kind,ns,obs", [(8, 4, 4), (9, 6, 11)])
def test_abi_sizes(kind, ns, obs):
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert lib.mrl_env_state_doubles(kind) == ns
    assert lib.mrl_filter_doubles(kind) == 2 + 2 * (obs + 1)
    assert lib.mrl_record_doubles(kind) == 2 + 2 * (obs + 1)
    desc = _lib.RolloutDesc(kind, 10, 7, 200, 0, 0, 0, 0, 0)
    assert lib.mrl_rollout_noise_doubles(ctypes.byref(desc)) == 7 * 10
    assert lib.mrl_rollout_sync_bytes(ctypes.byref(desc)) == 256 + 2 * (obs + 1) * 1 * 16


@pytest.mark.parametrize("entry", ["mrl_env_reset", "mrl_env_step"])
def test_env_entries_take_the_new_ids(entry):
    """env_id 8 and 9 pass the id check: with n_envs = 0 the complaint is about n_envs (the
    checks run before any HIP call); 7 and 10 are no envs."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bufs = _lib.RolloutBufs(env_state=p, env_int=p)
    io = _lib.EnvIO(p, None, p, p, p, p, None)
    tail = (None,) if entry == "mrl_env_reset" else (1, None)
    for env_id, needle in ((8, "n_envs"), (9, "n_envs"), (7, "env_id"), (10, "env_id")):
        desc = _lib.RolloutDesc(env_id, 0, 1, 200, 0, 0, 0, 0, 0)
        rc = getattr(lib, entry)(ctypes.byref(desc), ctypes.byref(bufs), ctypes.byref(io), *tail)
        msg = lib.mrl_last_error().decode()
        assert rc == E_ARG and needle in msg, (env_id, rc, msg)
        assert needle == "env_id" or "env_id" not in msg, (env_id, msg)


def test_twin_has_the_oracle_envs_duck_type():
    from oracle import rollout_np as RO
    ref = RO.Envs(RO.CARTPOLE, 3, 0)
    for kind, ns, O in ((MC.INVPENDULUM, 4, 4), (MC.INVDOUBLEPENDULUM, 6, 11)):
        e = MC.ChainEnvs(kind, 3, 0, env_offset=2)
        for name in ("kind", "E", "seed", "gid", "ns", "O", "A", "max_steps", "nu", "state", "ep_t", "ep_count"):
            assert type(getattr(e, name)) is type(getattr(ref, name)), name
        assert e.nu % 2 == 0 and e.gid.tolist() == [2, 3, 4] and (e.ns, e.O, e.A) == (ns, O, 1)
        e.reset(np.arange(3))
        assert e.obs().shape == (3, O) and e.state.shape == (3, ns) and e.ep_count.tolist() == [1, 1, 1]


# ------------------------------------------------------------------ the model's constants
def test_masses_match_the_xml_cross_check():
    for got, want in ((MC.MC, 10.47), (MC.IP.m1, 5.02), (MC.DP.m, 4.20)):
        assert round(got, 2) == want, got  # the stated two decimals: three significant figures or more
    # the capsule's transverse inertia lies between a rod's and a rod's with all mass at the ends
    for m, i in ((MC.IP.m1, MC.IP.i1), (MC.DP.m, MC.DP.i)):
        assert m * 0.6 ** 2 / 12.0 < i < m * (0.6 + 0.1) ** 2 / 4.0


def test_resets_draw_the_stated_distributions():
    ip, dp = MC.ChainEnvs(MC.INVPENDULUM, 4000, 3), MC.ChainEnvs(MC.INVDOUBLEPENDULUM, 4000, 3)
    ip.reset(np.arange(4000)), dp.reset(np.arange(4000))
    assert (np.abs(ip.state) <= 0.01).all() and np.abs(ip.state).max() > 0.0099
    assert (np.abs(dp.state[:, :3]) <= 0.1).all() and np.abs(dp.state[:, :3]).max() > 0.099
    v = dp.state[:, 3:]
    # 12000 draws of 0.1 N(0, 1): mean within 4 sigma / sqrt(n), std within 4 %, no shared pairs
    assert abs(v.mean()) < 4 * 0.1 / np.sqrt(v.size) and abs(v.std() / 0.1 - 1.0) < 0.04
    assert np.abs(np.corrcoef(v.T) - np.eye(3)).max() < 0.08
    # the transform is oracle/philox.py's: calls 2 and 3 of the reset stream
    from oracle import philox
    u = philox.uniforms(3, 1, dp.gid, np.zeros(4000, dtype=np.uint64), 8)
    z = np.sqrt(-2.0 * np.log(1.0 - u[:, 4])) * np.cos(2.0 * np.pi * u[:, 5])
    np.testing.assert_allclose(v[:, 0], 0.1 * z, rtol=1e-15, atol=0)


# ------------------------------------------------------------------ hand anchors
def test_pendulum_upright_under_force_has_the_closed_form_acceleration():
    """Upright (th = 0) and at rest every velocity, gravity and damping term vanishes, so
    [[a, b], [b, d]] (xdd, thdd) = (F, 0) with a = mc + m1, b = m1 l/2, d = I1 + m1 l^2/4:
    thdd = -b xdd / d from the second row, then xdd (a - b^2/d) = F from the first, i.e.
    xdd = F d / (a d - b^2), thdd = -F b / (a d - b^2).  F = gear * clamp(u): u = 2 gives 200 N,
    u = 7 is clamped to 3 (300 N)."""
    a, b, d = MC.MC + MC.IP.m1, MC.IP.m1 * 0.3, MC.IP.i1 + MC.IP.m1 * 0.09
    for u, F in ((2.0, 200.0), (7.0, 300.0), (-7.0, -300.0)):
        fu = MC._control(np.array([[u]], dtype=np.float32), 1, MC.IP)
        assert fu[0] == F
        k = MC.ip_dsdt(np.zeros((1, 4)), fu)[0]
        det = a * d - b * b
        np.testing.assert_allclose(k, [0.0, 0.0, F * d / det, -F * b / det], rtol=1e-12, atol=1e-12)


def test_pendulum_upright_at_rest_is_conserved_exactly():
    s = np.zeros((2, 4))
    for _ in range(50):
        s, rew, done = MC.ip_step(s, np.zeros((2, 1), dtype=np.float32))
        assert (rew == 1.0).all() and not done.any()
    assert (s == 0.0).all()


def test_double_pendulum_hanging_straight_has_no_acceleration():
    p = MC.DP.replace(gx=0.0)
    y = np.array([[0.3, np.pi, 0.0, 0.0, 0.0, 0.0]])
    k = MC.dp_dsdt(y, np.zeros(1), p)
    np.testing.assert_allclose(k, 0.0, rtol=0, atol=1e-12)
    # with the XML's x-gravity the cart alone would accelerate at 1e-5 (all masses share it)
    assert MC.dp_dsdt(y, np.zeros(1))[0, 3] == pytest.approx(1e-5, rel=1e-3)


# ------------------------------------------------------------------ M and the bias forces
def _per_body(kind, s):
    """M and h = c + g assembled body by body: M = sum m Jv^T Jv + I Jw^T Jw, h = sum m Jv^T
    (Jv' qd - gvec) with every body's centre-of-mass Jacobian written out in the relative
    joint coordinates."""
    n = 2 if kind == MC.INVPENDULUM else 3
    p = MC.IP if n == 2 else MC.DP
    q, v = s[:, :n], s[:, n:]
    E = len(s)
    one, zero = np.ones(E), np.zeros(E)
    bodies = [(MC.MC, 0.0, [one] + [zero] * (n - 1), [zero] * n, [zero] * n, zero, zero)]  # the cart
    if n == 2:
        th, w = q[:, 1], v[:, 1]
        bodies.append((p.m1, p.i1, [one, 0.3 * np.cos(th)], [zero, -0.3 * np.sin(th)], [zero, one],
                       -0.3 * np.sin(th) * w ** 2, -0.3 * np.cos(th) * w ** 2))
    else:
        t1, t12, w1, w12 = q[:, 1], q[:, 1] + q[:, 2], v[:, 1], v[:, 1] + v[:, 2]
        bodies.append((p.m, p.i, [one, 0.3 * np.cos(t1), zero], [zero, -0.3 * np.sin(t1), zero], [zero, one, zero],
                       -0.3 * np.sin(t1) * w1 ** 2, -0.3 * np.cos(t1) * w1 ** 2))
        bodies.append((p.m, p.i, [one, 0.6 * np.cos(t1) + 0.3 * np.cos(t12), 0.3 * np.cos(t12)],
                       [zero, -0.6 * np.sin(t1) - 0.3 * np.sin(t12), -0.3 * np.sin(t12)], [zero, one, one],
                       -0.6 * np.sin(t1) * w1 ** 2 - 0.3 * np.sin(t12) * w12 ** 2,
                       -0.6 * np.cos(t1) * w1 ** 2 - 0.3 * np.cos(t12) * w12 ** 2))
    M, h = np.zeros((E, n, n)), np.zeros((E, n))
    for m, inertia, jx, jz, jw, ax, az in bodies:
        jx, jz, jw = np.stack(jx, axis=1), np.stack(jz, axis=1), np.stack(jw, axis=1)
        M += m * (jx[:, :, None] * jx[:, None, :] + jz[:, :, None] * jz[:, None, :])
        M += inertia * jw[:, :, None] * jw[:, None, :]
        h += m * (jx * (ax - p.gx)[:, None] + jz * (az - p.gz)[:, None])
    return M, h


@pytest.mark.parametrize("kind", [MC.INVPENDULUM, MC.INVDOUBLEPENDULUM])
def test_mass_matrix_and_bias_match_a_body_by_body_assembly(kind):
    """test_hopper_physics.py's bound (1e-11 of the largest entry), and M symmetric positive
    definite at random q."""
    rng = np.random.default_rng(3)
    E, n = 256, 2 if kind == MC.INVPENDULUM else 3
    s = np.concatenate([rng.uniform(-np.pi, np.pi, (E, n)), 2.0 * rng.standard_normal((E, n))], axis=1)
    M, c, g = (MC.ip_terms if n == 2 else MC.dp_terms)(s)
    Mw, hw = _per_body(kind, s)
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert (np.linalg.eigvalsh(M) > 0).all()
    assert (np.abs(M - Mw).max(axis=(1, 2)) / np.abs(Mw).max(axis=(1, 2))).max() < 1e-11
    assert (np.abs(c + g - hw).max(axis=1) / np.abs(hw).max(axis=1)).max() < 1e-11
    # the dynamics solve M qdd = -c - g (no control, damping or stops): the LDL^T against numpy's solve
    p = (MC.IP if n == 2 else MC.DP).replace(**FREE, **(dict(hlim=1e9) if n == 2 else {}))
    k = (MC.ip_dsdt if n == 2 else MC.dp_dsdt)(s, np.zeros(E), p)
    want = np.linalg.solve(Mw, -hw[:, :, None])[:, :, 0]
    assert (np.abs(k[:, n:] - want).max(axis=1) / np.abs(want).max(axis=1)).max() < 1e-11


# ------------------------------------------------------------------ the integrator
@pytest.mark.parametrize("kind", [MC.INVPENDULUM, MC.INVDOUBLEPENDULUM])
def test_energy_drift_falls_sixteenfold_when_dt_is_halved(kind):
    """No damping, no control, the stops out of reach: the energy drift over a fixed time is
    RK4's global error, O(dt^4).  Halving dt must cut it by at least 8 (16 predicted; the
    factor of 2 is margin for higher-order terms).  The drift is the largest |E(t) - E(0)|
    over the env steps of the window, not the last step's alone: RK4's energy error is signed
    and oscillates with the poles, so at a single instant it can pass through zero at one of
    the two step sizes (seen on the double pendulum: end-point ratios from 2.7 to 566 on the
    states whose windowed ratios are 13 to 47; the pendulum's windowed ratios are 13.7 to 14.7)."""
    rng = np.random.default_rng(5)
    E = 8
    if kind == MC.INVPENDULUM:
        p, step, energy, n = MC.IP.replace(**FREE, hlim=1e9), MC.ip_step, MC.ip_energy, 2
    else:
        p, step, energy, n = MC.DP.replace(**FREE), MC.dp_step, MC.dp_energy, 3
    s0 = np.concatenate([rng.uniform(-0.5, 0.5, (E, n)), rng.uniform(-1.0, 1.0, (E, n))], axis=1)
    e0 = energy(s0, p)
    drift = []
    for halvings in (0, 1):
        ph = p.replace(dt=p.dt / 2 ** halvings, frame_skip=p.frame_skip * 2 ** halvings)
        s, worst = s0.copy(), np.zeros(E)
        for _ in range(25):  # 1 s (0.04 s a step) / 1.25 s (0.05 s a step)
            s, _, _ = step(s, np.zeros((E, 1), dtype=np.float32), ph)
            worst = np.maximum(worst, np.abs(energy(s, ph) - e0))
        drift.append(worst)
    print(kind, "energy", e0, "drift", drift[0], drift[1], "ratio", drift[0] / drift[1])
    assert (drift[0] > 1e-11).all()  # above rounding: the ratio means something
    assert (drift[0] < 1e-3 * np.abs(e0)).all()
    assert (drift[0] / drift[1] >= 8.0).all(), drift[0] / drift[1]


# ------------------------------------------------------------------ the slider stop
@pytest.mark.parametrize("kind", [MC.INVPENDULUM, MC.INVDOUBLEPENDULUM])
def test_slider_stop_holds_a_cart_driven_into_it(kind):
    """The cart starts at rest at the stop (x = 1) and the motor pushes it in at full control,
    F = gear * ctrl.  A spring-damper's step response overshoots its static deflection F / k
    by less than 2x at any damping, so the penetration stays below 2 F / k, and it settles
    at F / k (within 2x either way: the poles lean on the cart).  The stop only dissipates:
    energy (kinetic + gravity + stop spring) minus the motor's work F (x - x0) never grows."""
    if kind == MC.INVPENDULUM:
        p, step, energy = MC.IP, MC.ip_step, MC.ip_energy
        s = np.array([[1.0, 0.0, 0.0, 0.0]])
    else:
        p, step, energy = MC.DP, MC.dp_step, MC.dp_energy
        s = np.array([[1.0, np.pi, 0.0, 0.0, 0.0, 0.0]])  # the poles hang
    F = p.gear * p.ctrl
    static = F / p.ks
    act = np.full((1, 1), 2.0 * p.ctrl, dtype=np.float32)  # clamped to full control
    x0, e_prev, pen = s[0, 0], energy(s, p)[0], []
    for t in range(200):
        s, _, _ = step(s, act, p)
        e = energy(s, p)[0] - F * (s[0, 0] - x0)
        assert e <= e_prev + 1e-9 * max(1.0, abs(e_prev)), (t, e, e_prev)
        e_prev = e
        pen.append(s[0, 0] - 1.0)
    pen = np.array(pen)
    print(kind, "static", static, "max penetration", pen.max(), "final", pen[-1])
    assert 0.0 < pen.max() <= 2.0 * static
    assert 0.5 * static <= pen[-1] <= 2.0 * static
    if kind == MC.INVDOUBLEPENDULUM:  # the observed limit force: pushing back, clipped
        assert MC.dp_obs(s)[0, 8] == -10.0 and (MC.dp_obs(s)[0, 9:] == 0.0).all()


# ------------------------------------------------------------------ the envs' own terminations
# (shortest, longest) zero-control episode of 32 envs, seed 9, as the twin gives them: a record
# of this model's time scale, not MuJoCo's
IP_ZERO_CONTROL_STEPS = (20, 38)
DP_ZERO_CONTROL_STEPS = (8, 16)


def _zero_control_lengths(kind, E=32, seed=9):
    envs = MC.ChainEnvs(kind, E, seed)
    envs.reset(np.arange(E))
    length = np.zeros(E, dtype=np.int64)
    how = []
    for t in range(1000):
        before = envs.state.copy()
        _, done = envs.step(np.zeros((E, 1), dtype=np.float32))
        new = done & (length == 0)
        length[new] = t + 1
        how.append((new, before, envs.state.copy()))
        if (length > 0).all():
            break
    return length, how


def test_pendulum_falls_past_its_angle_threshold_under_zero_control():
    length, how = _zero_control_lengths(MC.INVPENDULUM)
    print("InvertedPendulum-v2 zero-control episode lengths", sorted(length.tolist()))
    assert (length > 0).all() and (length.min(), length.max()) == IP_ZERO_CONTROL_STEPS
    for new, before, after in how:
        assert (np.abs(before[new, 1]) <= 0.2).all() and (np.abs(after[new, 1]) > 0.2).all()  # the angle test
        assert np.isfinite(after).all() and (np.abs(after[:, 0]) < 1.0).all()  # not the stop, not a blow-up


def test_double_pendulum_drops_below_its_height_threshold_under_zero_control():
    length, how = _zero_control_lengths(MC.INVDOUBLEPENDULUM)
    print("InvertedDoublePendulum-v2 zero-control episode lengths", sorted(length.tolist()))
    assert (length > 0).all() and (length.min(), length.max()) == DP_ZERO_CONTROL_STEPS
    for new, before, after in how:
        assert (MC.dp_tip(before[new])[1] > 1.0).all() and (MC.dp_tip(after[new])[1] <= 1.0).all()  # the height test
        assert np.isfinite(after).all()


# ------------------------------------------------------------------ the GPU tests' seeds
@pytest.mark.parametrize("E,Tn,limit", CC.STEP_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_step_cases_keep_clear_of_the_thresholds(env_id, E, Tn, limit):
    """The GPU tests ask for the twin's exact flags: on their seeds no compared state lies
    within 1e-6 of a termination threshold (|th| - 0.2, y_t - 1), so a last-bit difference
    in the device's sin, cos or log cannot flip one; and episodes end inside the run."""
    _, steps, least = CC.reference_steps(env_id, E, Tn, limit)
    assert least > CC.MARGIN, least
    assert sum(len(s["idx"]) for s in steps) > 0
    assert (np.abs(CC.step_actions(env_id, E, Tn)) > CC.ACT_HIGH[env_id]).any()  # the control clamp is hit


@pytest.mark.parametrize("E,Tn,limit,inject", CC.ROLLOUT_CASES)
@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_rollout_cases_keep_clear_of_the_thresholds(env_id, E, Tn, limit, inject):
    _, _, its = CC.reference_rollout(env_id, [64, 64], E, Tn, limit, inject)
    assert min(m for _, _, _, m in its) > CC.MARGIN
    assert all(np.isfinite(w["obs"]).all() and np.isfinite(w["rew"]).all() for w, _, _, _ in its)


def test_layered_case_keeps_clear_of_the_thresholds():
    env_id, hid, E, Tn, limit = CC.LAYERED_CASE
    _, _, its = CC.reference_rollout(env_id, hid, E, Tn, limit, False)
    assert min(m for _, _, _, m in its) > CC.MARGIN
    assert any((w["flags"][:-1] & 1).any() for w, _, _, _ in its)  # the limit cuts inside the horizon


@pytest.mark.parametrize("env_id", CC.ENV_IDS)
def test_population_case_keeps_clear_of_the_thresholds(env_id):
    rows, ended, least = CC.reference_population(env_id)
    assert rows >= CC.POP_N * 5 and least > CC.MARGIN, (rows, least)
    assert ended > 0  # some candidates drop their pole inside the limit
