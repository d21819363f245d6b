// Planar chains without contact on device beside envs_chains.h's cart-and-pole chains (fp64,
// FMA contraction off), operation-for-operation twins of tests/planar_chains_np.py:
// Reacher-v2 and Swimmer-v2, the "reacher" and "swimmer" tasks of the reference's MuJoCo
// battery.  gym and MuJoCo are absent, so parity with them is unpinned, as Hopper's is; the
// models restate gym's reacher.xml and swimmer.xml and this header is the record of every
// constant.  No multiply-add is fused here (no fmad call): the twin is plain numpy, and only
// sin / cos / sqrt may differ from it in the last bit.
//
// Both chains lie in the horizontal plane, so gravity does not enter.  Every force is explicit
// in RK4 (ch_rk4), one classical step per MuJoCo timestep, frame_skip times per env step; the
// stages and the frames stay rolled loops.  Geoms are capsules along their body's x axis
// (ch_capsule_mass / ch_capsule_inertia at density 1000, scaled to the XML's density);
// pl_capsule_axial is the capsule's inertia about its own axis,
//     I_a = m_cyl r^2/2 + m_sph 2 r^2/5.
//
// Reacher-v2.  Two hinges about z, q = (th1, th2) with th2 relative to link 1.  Links:
// capsules of radius 0.01 and length 0.1, density 300 (0.0107 kg each); a fingertip sphere of
// radius 0.01 (1.26 g, inertia 2/5 m r^2) is welded 0.11 m along link 2.  In the absolute
// angles phi_1 = th1, phi_2 = th1 + th2 the kinetic energy has the matrix
//     A11 = I1 + m1 l^2/4 + (m2 + ms) l^2     A12 = l (m2 l/2 + ms 0.11) cos th2
//     A22 = I2 + m2 l^2/4 + Is + ms 0.11^2
// M = J^T A J + armature; the velocity terms are formed in the absolute rates and mapped by
// J^T.  Armature 1 and damping 1 on both hinges, hinge 1 unlimited, hinge 2 limited to +-3 rad
// by the penalty stop (CH_KH, CH_CH), gear 200 on both, control clamped to [-1, 1], timestep
// 0.01, frame_skip 2.
//     M(q) qdd = B u - c(q, qd) - D qd + tau_lim,   2x2 LDL^T.
// State (6): th1, th2, th1d, th2d, g_x, g_y; the goal never moves inside an episode and is
// not integrated.  obs (11) = cos th1, cos th2, sin th1, sin th2, g_x, g_y, th1d, th2d,
// tip_x - g_x, tip_y - g_y, 0 with tip = l e(phi_1) + 0.11 e(phi_2).  reward =
// -|tip - g| - sum a^2 with the unclipped action and, as gym, the tip of the state the action
// is applied to (before the frames).  done: never; TimeLimit 50.  Reset (NU = 12 uniforms):
// u0, u1 -> th = U(-0.1, 0.1); u2, u3 -> thd = U(-0.005, 0.005); (u4, u5) .. (u10, u11) are
// four goal candidates U(-0.2, 0.2)^2, the goal is the first with g_x^2 + g_y^2 < 0.04 by
// plain selects, and if none qualifies (probability (1 - pi/4)^4 = 0.21 %) the fourth times
// 0.5 (norm below 0.142).
//
// Swimmer-v2.  Three capsules of radius 0.1 and length 1, density 1000 (35.6 kg each),
// q = (x, y, psi, th2, th3): the root slides in x and y and turns about z at its origin, the
// torso runs from 0.5 to 1.5 along the root's x axis, "mid" is hinged at (0.5, 0) and extends
// 1 m along -x, "back" is hinged at mid's far end and extends another 1 m.  With the absolute
// angles phi_0 = psi, phi_1 = psi + th2, phi_2 = psi + th2 + th3, e_k = (cos phi_k, sin phi_k)
// and n_k = (-sin phi_k, cos phi_k) the centres of mass move with
//     v_b = (xd, yd) + sum_k a[b][k] n_k w_k,   a = {{1, 0, 0}, {0.5, -0.5, 0}, {0.5, -1, -0.5}}
// so in (x, y, phi_0, phi_1, phi_2) the kinetic energy has the matrix
//     A_xx = A_yy = 3 m       A_x,k = -m S_k sin phi_k      A_y,k = m S_k cos phi_k
//     A_k,l = m C_kl cos(phi_k - phi_l) + I delta_kl
// with S_k = sum_b a[b][k] = (2, -1.5, -0.5) and C_kl = sum_b a[b][k] a[b][l]
// (C00 = 1.5, C01 = -0.75, C02 = -0.25, C11 = 1.25, C12 = 0.5, C22 = 0.25), and the velocity
// terms c_x = -m sum S_k cos phi_k w_k^2, c_y = -m sum S_k sin phi_k w_k^2,
// c_k = -m sum_l C_kl sin(phi_l - phi_k) w_l^2.  M = J^T A J + armature 0.1 on all five
// joints, no damping, no gravity term; the two relative hinges are limited to +-100 deg by
// the penalty stop, motors of gear 150 act on th2 and th3, control clamped to [-1, 1],
// timestep 0.01, frame_skip 4.  The 5x5 system is solved by an LDL^T.
// Fluid (density 4000, viscosity 0.1): MuJoCo's inertia-box model per body, in the body's
// inertial frame at its centre of mass.  Equivalent box sides b_i = sqrt(6 (I_j + I_k - I_i)
// / m) (along the capsule 1.136 m, across 0.171 m; constexpr, by pl_sqrt's Newton steps),
// mean side d = (b_0 + b_1 + b_2) / 3,
//     f_i = -3 pi beta d v_i - 1/2 rho b_j b_k |v_i| v_i
//     tau_i = -pi beta d^3 w_i - rho b_i (b_j^4 + b_k^4) |w_i| w_i / 64
// of which the two in-plane forces and the z torque survive; they are mapped to generalised
// forces by the bodies' Jacobians (a[b][k] n_k for the force, 1 on phi_b for the torque).
// State (10) = q ++ qd.  obs (8) = q[2:] ++ qd.  reward = (x_after - x_before) / (dt
// frame_skip) - 1e-4 sum a^2, unclipped action.  done: never; TimeLimit 1000.  Reset: q, qd =
// U(-0.1, 0.1), NU = 10.
//
// Deviations from MuJoCo, documented like the cart-and-pole chains':
//  * joint limits are one-sided penalty spring-dampers (Hopper's hinge constants) instead of
//    the constraint solver;
//  * joint damping is integrated explicitly by RK4 (MuJoCo: implicitly);
//  * Reacher's goal draw is bounded: four candidates and a fallback instead of gym's
//    unbounded rejection loop, and the goal is env state, not two slide joints (gym's target
//    joints have their velocity zeroed at reset and nothing acts on them);
//  * Reacher's frictionless plane contact (conaffinity 0 everywhere) is absent.
#pragma once
#include "envs_chains.h"

#pragma clang fp contract(off)

namespace mrl {

constexpr double pl_capsule_axial(double r, double l) {
  return ch_cyl_mass(r, l) * (r * r / 2.0) + ch_sph_mass(r) * (2.0 * (r * r) / 5.0);
}
// sqrt of a constant by 40 Newton steps from 1 (the twin takes the same steps)
constexpr double pl_sqrt(double v) {
  double x = 1.0;
  for (int i = 0; i < 40; ++i) x = 0.5 * (x + v / x);
  return x;
}

// ------------------------------------------------------------------ Reacher-v2
constexpr int RC_NS = 6, RC_NQ = 4, RC_OBS = 11, RC_ACT = 2, RC_NU = 12, RC_FRAME_SKIP = 2, RC_MAX_STEPS = 50;
constexpr double RC_DT = 0.01, RC_GEAR = 200.0, RC_CTRL = 1.0, RC_DAMP = 1.0, RC_ARM = 1.0, RC_HLIM = 3.0;
constexpr double RC_R = 0.01, RC_L = 0.1, RC_LC = RC_L / 2.0, RC_TIP = 0.11, RC_DENS = 300.0 / CH_RHO;
constexpr double RC_GOAL = 0.2, RC_GOAL2 = 0.04;
constexpr double RC_M = RC_DENS * ch_capsule_mass(RC_R, RC_L), RC_I = RC_DENS * ch_capsule_inertia(RC_R, RC_L);
constexpr double RC_MS = RC_DENS * ch_sph_mass(RC_R), RC_IS = RC_MS * (2.0 * (RC_R * RC_R) / 5.0);
constexpr double RC_A11 = RC_I + RC_M * (RC_LC * RC_LC) + (RC_M + RC_MS) * (RC_L * RC_L);
constexpr double RC_H = RC_L * (RC_M * RC_LC + RC_MS * RC_TIP);  // A12 / cos th2
constexpr double RC_A22 = RC_I + RC_M * (RC_LC * RC_LC) + RC_IS + RC_MS * (RC_TIP * RC_TIP);

__device__ inline void reacher_reset(const double* u, double* s) {
  s[0] = u[0] * 0.2 - 0.1;
  s[1] = u[1] * 0.2 - 0.1;
  s[2] = u[2] * 0.01 - 0.005;
  s[3] = u[3] * 0.01 - 0.005;
  // the fourth candidate halved unless an earlier one (the first that does) lies in the disc
  double gx = 0.5 * (u[10] * 0.4 - 0.2), gy = 0.5 * (u[11] * 0.4 - 0.2);
#pragma unroll
  for (int c = 3; c >= 0; --c) {
    const double cx = u[4 + 2 * c] * 0.4 - 0.2, cy = u[5 + 2 * c] * 0.4 - 0.2;
    const bool in = cx * cx + cy * cy < RC_GOAL2;
    gx = in ? cx : gx;
    gy = in ? cy : gy;
  }
  s[4] = gx;
  s[5] = gy;
}

// d/dt of (th1, th2, th1d, th2d) under the hinge torques t1, t2
__device__ inline void reacher_dsdt(const double* y, double t1, double t2, double* k) {
  const double q2 = y[1], q1d = y[2], q2d = y[3];
  double s2, c2;
  sincos(q2, &s2, &c2);
  const double w1 = q1d, w2 = q1d + q2d;  // absolute link rates
  const double w1s = w1 * w1, w2s = w2 * w2;
  const double a12 = RC_H * c2;
  const double m00 = (RC_A11 + RC_A22) + 2.0 * a12 + RC_ARM, m01 = a12 + RC_A22, m11 = RC_A22 + RC_ARM;
  const double hs = RC_H * s2;
  const double ca1 = -hs * w2s, ca2 = hs * w1s;
  const double r0 = t1 - (ca1 + ca2) - RC_DAMP * q1d;
  const double r1 = t2 - ca2 - RC_DAMP * q2d + ch_limit(q2, q2d, RC_HLIM, CH_KH, CH_CH);
  // LDL^T of [[m00, m01], [m01, m11]]
  const double l10 = m01 / m00;
  const double d1 = m11 - l10 * l10 * m00;
  const double y1 = r1 - l10 * r0;
  const double a1 = y1 / d1;
  const double a0 = r0 / m00 - l10 * a1;
  k[0] = q1d;
  k[1] = q2d;
  k[2] = a0;
  k[3] = a1;
}

// fingertip minus goal
__device__ inline void reacher_tip(const double* s, double& dx, double& dy) {
  double s1, c1, s12, c12;
  sincos(s[0], &s1, &c1);
  sincos(s[0] + s[1], &s12, &c12);
  dx = (RC_L * c1 + RC_TIP * c12) - s[4];
  dy = (RC_L * s1 + RC_TIP * s12) - s[5];
}

__device__ inline void reacher_step(double* s, const float* a, double& rew, bool& done) {
  const double a0 = (double)a[0], a1 = (double)a[1];
  const double t1 = RC_GEAR * ch_clamp(a0, -RC_CTRL, RC_CTRL), t2 = RC_GEAR * ch_clamp(a1, -RC_CTRL, RC_CTRL);
  double dx, dy;
  reacher_tip(s, dx, dy);
  rew = -sqrt(dx * dx + dy * dy) - (a0 * a0 + a1 * a1);
#pragma unroll 1
  for (int f = 0; f < RC_FRAME_SKIP; ++f)
    ch_rk4<RC_NQ>(s, RC_DT, [t1, t2](const double* y, double* k) { reacher_dsdt(y, t1, t2, k); });
  done = false;
}

__device__ inline void reacher_obs(const double* s, double* o) {
  double s1, c1, s2, c2, dx, dy;
  sincos(s[0], &s1, &c1);
  sincos(s[1], &s2, &c2);
  reacher_tip(s, dx, dy);
  o[0] = c1;
  o[1] = c2;
  o[2] = s1;
  o[3] = s2;
  o[4] = s[4];
  o[5] = s[5];
  o[6] = s[2];
  o[7] = s[3];
  o[8] = dx;
  o[9] = dy;
  o[10] = 0.0;
}

struct ReacherEnv {
  static constexpr int NS = RC_NS, OBS = RC_OBS, ACT = RC_ACT, DISCRETE = 0, MAX_STEPS = RC_MAX_STEPS, NU = RC_NU;
  __device__ static void reset(const double* u, double* s) { reacher_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { reacher_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) { reacher_step(s, a, rew, done); }
};

// ------------------------------------------------------------------ Swimmer-v2
constexpr int SW_NS = 10, SW_NQ = 5, SW_OBS = 8, SW_ACT = 2, SW_NU = 10, SW_FRAME_SKIP = 4, SW_MAX_STEPS = 1000;
constexpr double SW_DT = 0.01, SW_GEAR = 150.0, SW_CTRL = 1.0, SW_ARM = 0.1;
constexpr double SW_HLIM = 100.0 * CH_PI / 180.0;
constexpr double SW_RHO = 4000.0, SW_BETA = 0.1;  // the medium: density, viscosity
constexpr double SW_R = 0.1, SW_L = 1.0;
constexpr double SW_M = ch_capsule_mass(SW_R, SW_L), SW_I = ch_capsule_inertia(SW_R, SW_L);
constexpr double SW_IA = pl_capsule_axial(SW_R, SW_L);
// v_b = (xd, yd) + sum_k SW_A[b][k] n_k w_k; S_k and C_kl of the header comment, times m
constexpr double SW_A[3][3] = {{1.0, 0.0, 0.0}, {0.5, -0.5, 0.0}, {0.5, -1.0, -0.5}};
constexpr double SW_MT = 3.0 * SW_M + SW_ARM;  // M_xx = M_yy
constexpr double SW_S0 = SW_M * 2.0, SW_S1 = SW_M * -1.5, SW_S2 = SW_M * -0.5;
constexpr double SW_C01 = SW_M * -0.75, SW_C02 = SW_M * -0.25, SW_C12 = SW_M * 0.5;
constexpr double SW_J0 = SW_M * 1.5 + SW_I, SW_J1 = SW_M * 1.25 + SW_I, SW_J2 = SW_M * 0.25 + SW_I;
// the equivalent box: along the capsule, across it (twice), their mean
constexpr double SW_BX = pl_sqrt(6.0 * (SW_I + SW_I - SW_IA) / SW_M), SW_BY = pl_sqrt(6.0 * SW_IA / SW_M);
constexpr double SW_BD = (SW_BX + SW_BY + SW_BY) / 3.0;
constexpr double SW_VIS_F = 3.0 * CH_PI * SW_BETA * SW_BD, SW_VIS_T = CH_PI * SW_BETA * (SW_BD * SW_BD * SW_BD);
constexpr double SW_QL = 0.5 * SW_RHO * (SW_BY * SW_BY);  // drag along the capsule: faces b_y b_z
constexpr double SW_QN = 0.5 * SW_RHO * (SW_BX * SW_BY);  // drag across it: faces b_x b_z
constexpr double SW_QT =
    SW_RHO * SW_BY * ((SW_BX * SW_BX) * (SW_BX * SW_BX) + (SW_BY * SW_BY) * (SW_BY * SW_BY)) / 64.0;

__device__ inline void swimmer_reset(const double* u, double* s) {
  for (int i = 0; i < SW_NS; ++i) s[i] = u[i] * 0.2 - 0.1;
}

// the inertia-box fluid force on one body: along the capsule, across it, and the z torque
__device__ inline void swimmer_fluid(double vl, double vn, double w, double& fl, double& fn, double& tq) {
  fl = -SW_VIS_F * vl - SW_QL * (fabs(vl) * vl);
  fn = -SW_VIS_F * vn - SW_QN * (fabs(vn) * vn);
  tq = -SW_VIS_T * w - SW_QT * (fabs(w) * w);
}

// d/dt of (q, qd) under the hinge torques t2, t3
__device__ inline void swimmer_dsdt(const double* y, double t2, double t3, double* k) {
  const double xd = y[5], yd = y[6];
  const double phi[3] = {y[2], y[2] + y[3], (y[2] + y[3]) + y[4]};
  const double w[3] = {y[7], y[7] + y[8], (y[7] + y[8]) + y[9]};  // absolute body rates
  double sn[3], cs[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) sincos(phi[b], &sn[b], &cs[b]);
  const double ws0 = w[0] * w[0], ws1 = w[1] * w[1], ws2 = w[2] * w[2];
  // cos (phi_k - phi_l) and sin (phi_l - phi_k), k < l
  const double c01 = cs[0] * cs[1] + sn[0] * sn[1], s01 = sn[1] * cs[0] - cs[1] * sn[0];
  const double c02 = cs[0] * cs[2] + sn[0] * sn[2], s02 = sn[2] * cs[0] - cs[2] * sn[0];
  const double c12 = cs[1] * cs[2] + sn[1] * sn[2], s12 = sn[2] * cs[1] - cs[2] * sn[1];
  // A in (x, y, phi_0, phi_1, phi_2)
  const double ax0 = -SW_S0 * sn[0], ax1 = -SW_S1 * sn[1], ax2 = -SW_S2 * sn[2];
  const double ay0 = SW_S0 * cs[0], ay1 = SW_S1 * cs[1], ay2 = SW_S2 * cs[2];
  const double a01 = SW_C01 * c01, a02 = SW_C02 * c02, a12 = SW_C12 * c12;
  // M = J^T A J + armature, lower triangle (row, column): suffix sums over the bodies
  double M[SW_NQ][SW_NQ];
  const double m33 = (SW_J1 + SW_J2) + 2.0 * a12;
  M[0][0] = SW_MT;
  M[1][0] = 0.0;
  M[1][1] = SW_MT;
  M[4][0] = ax2;
  M[3][0] = ax1 + ax2;
  M[2][0] = ax0 + M[3][0];
  M[4][1] = ay2;
  M[3][1] = ay1 + ay2;
  M[2][1] = ay0 + M[3][1];
  M[4][4] = SW_J2 + SW_ARM;
  M[4][3] = a12 + SW_J2;
  M[3][3] = m33 + SW_ARM;
  M[4][2] = a02 + M[4][3];
  M[3][2] = (a01 + a02) + m33;
  M[2][2] = SW_J0 + 2.0 * (a01 + a02) + m33 + SW_ARM;
  // velocity terms in the absolute rates
  const double cx = -(SW_S0 * cs[0]) * ws0 - (SW_S1 * cs[1]) * ws1 - (SW_S2 * cs[2]) * ws2;
  const double cy = -(SW_S0 * sn[0]) * ws0 - (SW_S1 * sn[1]) * ws1 - (SW_S2 * sn[2]) * ws2;
  const double cp0 = -((SW_C01 * s01) * ws1 + (SW_C02 * s02) * ws2);
  const double cp1 = (SW_C01 * s01) * ws0 - (SW_C12 * s12) * ws2;
  const double cp2 = (SW_C02 * s02) * ws0 + (SW_C12 * s12) * ws1;
  // fluid forces body by body, mapped by the bodies' Jacobians
  double fx = 0.0, fy = 0.0, fp[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    double vx = xd, vy = yd;
#pragma unroll
    for (int j = 0; j <= b; ++j) {
      vx = vx - (SW_A[b][j] * w[j]) * sn[j];
      vy = vy + (SW_A[b][j] * w[j]) * cs[j];
    }
    const double vl = vx * cs[b] + vy * sn[b], vn = vy * cs[b] - vx * sn[b];
    double fl, fn, tq;
    swimmer_fluid(vl, vn, w[b], fl, fn, tq);
    const double bx = fl * cs[b] - fn * sn[b], by = fl * sn[b] + fn * cs[b];
    fx = fx + bx;
    fy = fy + by;
#pragma unroll
    for (int j = 0; j <= b; ++j) fp[j] = fp[j] + SW_A[b][j] * (by * cs[j] - bx * sn[j]);
    fp[b] = fp[b] + tq;
  }
  double r[SW_NQ];
  r[0] = fx - cx;
  r[1] = fy - cy;
  r[2] = (fp[0] + (fp[1] + fp[2])) - (cp0 + (cp1 + cp2));
  r[3] = t2 + (fp[1] + fp[2]) - (cp1 + cp2) + ch_limit(y[3], y[8], SW_HLIM, CH_KH, CH_CH);
  r[4] = t3 + fp[2] - cp2 + ch_limit(y[4], y[9], SW_HLIM, CH_KH, CH_CH);
  // LDL^T in place: M's strict lower triangle becomes L, d the pivots
  double d[SW_NQ];
#pragma unroll
  for (int j = 0; j < SW_NQ; ++j) {
    double dj = M[j][j];
#pragma unroll
    for (int c = 0; c < j; ++c) dj = dj - M[j][c] * M[j][c] * d[c];
    d[j] = dj;
#pragma unroll
    for (int i = j + 1; i < SW_NQ; ++i) {
      double v = M[i][j];
#pragma unroll
      for (int c = 0; c < j; ++c) v = v - M[i][c] * M[j][c] * d[c];
      M[i][j] = v / dj;
    }
  }
#pragma unroll
  for (int i = 1; i < SW_NQ; ++i)
#pragma unroll
    for (int c = 0; c < i; ++c) r[i] = r[i] - M[i][c] * r[c];
#pragma unroll
  for (int i = SW_NQ - 1; i >= 0; --i) {
    double v = r[i] / d[i];
#pragma unroll
    for (int c = i + 1; c < SW_NQ; ++c) v = v - M[c][i] * r[c];
    r[i] = v;
  }
#pragma unroll
  for (int i = 0; i < SW_NQ; ++i) {
    k[i] = y[SW_NQ + i];
    k[SW_NQ + i] = r[i];
  }
}

__device__ inline void swimmer_step(double* s, const float* a, double& rew, bool& done) {
  const double a0 = (double)a[0], a1 = (double)a[1];
  const double t2 = SW_GEAR * ch_clamp(a0, -SW_CTRL, SW_CTRL), t3 = SW_GEAR * ch_clamp(a1, -SW_CTRL, SW_CTRL);
  const double xb = s[0];
#pragma unroll 1
  for (int f = 0; f < SW_FRAME_SKIP; ++f)
    ch_rk4<SW_NS>(s, SW_DT, [t2, t3](const double* y, double* k) { swimmer_dsdt(y, t2, t3, k); });
  rew = (s[0] - xb) / (SW_DT * SW_FRAME_SKIP) - 1e-4 * (a0 * a0 + a1 * a1);
  done = false;
}

__device__ inline void swimmer_obs(const double* s, double* o) {
  for (int i = 0; i < SW_OBS; ++i) o[i] = s[2 + i];
}

struct SwimmerEnv {
  static constexpr int NS = SW_NS, OBS = SW_OBS, ACT = SW_ACT, DISCRETE = 0, MAX_STEPS = SW_MAX_STEPS, NU = SW_NU;
  __device__ static void reset(const double* u, double* s) { swimmer_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { swimmer_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) { swimmer_step(s, a, rew, done); }
};

}  // namespace mrl
