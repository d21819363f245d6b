// Cart-and-pole chains on device beside envs.h's Hopper (fp64, FMA contraction off),
// operation-for-operation twins of tests/mujoco_chains_np.py: InvertedPendulum-v2 and
// InvertedDoublePendulum-v2, the "ip" and "idp" tasks of the reference's MuJoCo battery.
// gym and MuJoCo are absent, so parity with them is unpinned, as Hopper's is; the models
// restate gym's inverted_pendulum.xml and inverted_double_pendulum.xml and this header is
// the record of every constant.  No multiply-add is fused here (no fmad call): the twin is
// plain numpy, and only sin / cos / log may differ from it in the last bit.
//
// Model.  A cart on a slider (x) carries a serial chain of one or two poles on hinges about
// y; a positive angle tips a pole towards +x.  Pole k has mass m, length l, its centre of
// mass at l/2, and the capsule's transverse inertia I about it.  In the absolute pole angles
// phi_1 = th1, phi_2 = th1 + th2 the kinetic energy has the matrix
//     A00 = mc + m1 + m2        A01 = (m1 l/2 + m2 l) cos phi_1    A02 = m2 l/2 cos phi_2
//     A11 = I1 + m1 l^2/4 + m2 l^2   A12 = m2 l l/2 cos th2         A22 = I2 + m2 l^2/4
// and M = J^T A J with phi = J q (the second hinge is relative to pole 1).  The velocity
// terms c and the gravity terms g are formed in the absolute angles and mapped by J^T too.
//     M(q) qdd = B u - c(q, qd) - g(q) - D qd + tau_lim
// is solved by a 2x2 / 3x3 LDL^T, and (q, qd) advance by one classical RK4 step per MuJoCo
// timestep with every force explicit, frame_skip times per env step.
//
// Geoms: density 1000, inertia from geom.  A capsule of radius r and cylinder length l has
// the volume pi r^2 l + 4/3 pi r^3 and, about a transverse axis through its centre,
//     I = m_cyl (r^2/4 + l^2/12) + m_sph (2 r^2/5 + l^2/4 + 3 l r/8)
// (m_sph: the two half-spheres together).  The cart is a capsule of radius 0.1 and length
// 0.2 (10.47 kg; it only translates, so its inertia does not enter).
//  * InvertedPendulum-v2: pole radius 0.049, length 0.6 (5.02 kg), lower end at the hinge;
//    joint damping 1 on both joints, armature 0, slider range +-1 m, hinge range +-90 deg,
//    gear 100 on the slider, control clamped to [-3, 3], gravity (0, 0, -9.81), timestep
//    0.02, frame_skip 2.  obs = qpos ++ qvel, reward 1, done = !(all finite && |th| <= 0.2),
//    reset q, qd = uniform(-0.01, 0.01).
//  * InvertedDoublePendulum-v2: two poles of radius 0.045, length 0.6 (4.20 kg each), the
//    second hinged at the tip of the first, hinges unlimited, slider range +-1 m; damping
//    0.05 on all three joints, gear 500, control clamped to [-1, 1], gravity
//    (1e-5, 0, -9.81), timestep 0.01, frame_skip 5.  obs = (x, sin th1, sin th2, cos th1,
//    cos th2, clip(qd, +-10), clip(limit force per dof, +-10)), reward
//    10 - (0.01 x_t^2 + (y_t - 2)^2) - (1e-3 th1d^2 + 5e-3 th2d^2) at the pole tip
//    (x_t, y_t), done = y_t <= 1, reset q = uniform(-0.1, 0.1), qd = 0.1 N(0, 1): the
//    normals by Box-Muller on the reset's own Philox uniforms (NU = 8: u0..u2 -> q, u3
//    unused, the pairs (u4, u5) and (u6, u7) -> three of four normals).
//
// Deviations from MuJoCo, documented like Hopper's:
//  * joint limits are one-sided penalty spring-dampers in Hopper's form instead of the
//    constraint solver: the hinge takes Hopper's 2000 N m/rad and 50 N m s/rad, the slider
//    the contact constants 2e4 N/m and 400 N s/m.  The slider's limit force is also what
//    the double pendulum observes in place of gym's qfrc_constraint columns (its two hinge
//    columns are zero: the hinges have no limit);
//  * joint damping is integrated explicitly by RK4 (MuJoCo: implicitly);
//  * the pendulum's XML puts the pole's upper end 0.001 m off in x; here the pole is
//    straight along its hinge frame's z axis.
#pragma once
#include "mrl_common.h"

#pragma clang fp contract(off)

namespace mrl {

constexpr double CH_PI = 3.141592653589793;
constexpr double CH_RHO = 1000.0;
constexpr double CH_KS = 20000.0, CH_CS = 400.0;  // slider stop: N/m, N s/m
constexpr double CH_KH = 2000.0, CH_CH = 50.0;    // hinge stop: N m/rad, N m s/rad
constexpr double CH_XLIM = 1.0;                   // slider range +-1 m
constexpr double CH_CART_R = 0.1, CH_CART_L = 0.2, CH_POLE_L = 0.6;

constexpr double ch_cyl_mass(double r, double l) { return CH_RHO * (CH_PI * (r * r) * l); }
constexpr double ch_sph_mass(double r) { return CH_RHO * (4.0 / 3.0 * CH_PI * (r * r * r)); }
constexpr double ch_capsule_mass(double r, double l) { return ch_cyl_mass(r, l) + ch_sph_mass(r); }
constexpr double ch_capsule_inertia(double r, double l) {
  return ch_cyl_mass(r, l) * (r * r / 4.0 + l * l / 12.0) +
         ch_sph_mass(r) * (2.0 * (r * r) / 5.0 + l * l / 4.0 + 3.0 * l * r / 8.0);
}
constexpr double CH_MC = ch_capsule_mass(CH_CART_R, CH_CART_L);

__device__ inline double ch_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one-sided penalty stop of a joint at +-lim (Hopper's form): both sides evaluated, the
// active one picked by a plain select
__device__ inline double ch_limit(double q, double v, double lim, double k, double c) {
  const double cv = c * v;
  const double flo = k * (-lim - q) - cv, fhi = k * (lim - q) - cv;
  return q < -lim ? flo : (q > lim ? fhi : 0.0);
}

// y = s + h k and acc += w k of an RK4 stage over N doubles; stage weights 1 2 2 1 and
// steps h/2 h/2 h, so that s' = s + h/6 (((k1 + 2 k2) + 2 k3) + k4).  The stages and the
// frames stay rolled loops: one copy of the dynamics per kernel.
template <int N, class F>
__device__ inline void ch_rk4(double* s, double h, F dsdt) {
  double y[N], acc[N], k[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    y[i] = s[i];
    acc[i] = 0.0;
  }
#pragma unroll 1
  for (int st = 0; st < 4; ++st) {
    dsdt(y, k);
    const bool mid = st == 1 || st == 2;
    const double w = mid ? 2.0 : 1.0;
    const double hs = st == 2 ? h : h * 0.5;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      acc[i] = acc[i] + w * k[i];
      y[i] = s[i] + hs * k[i];
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = s[i] + (h / 6.0) * acc[i];
}

// ------------------------------------------------------------------ InvertedPendulum-v2
constexpr int IP_NS = 4, IP_OBS = 4, IP_ACT = 1, IP_NU = 4, IP_FRAME_SKIP = 2;
constexpr double IP_DT = 0.02, IP_GEAR = 100.0, IP_CTRL = 3.0, IP_DAMP = 1.0, IP_GZ = -9.81;
constexpr double IP_POLE_R = 0.049, IP_HLIM = CH_PI / 2.0, IP_TH_DONE = 0.2;
constexpr double IP_M1 = ch_capsule_mass(IP_POLE_R, CH_POLE_L), IP_I1 = ch_capsule_inertia(IP_POLE_R, CH_POLE_L);
constexpr double IP_LC = CH_POLE_L / 2.0;
constexpr double IP_MT = CH_MC + IP_M1;              // A00
constexpr double IP_B = IP_M1 * IP_LC;               // A01 / cos th
constexpr double IP_J = IP_I1 + IP_M1 * (IP_LC * IP_LC);  // A11

__device__ inline void invpendulum_reset(const double* u, double* s) {
  for (int i = 0; i < 4; ++i) s[i] = u[i] * 0.02 - 0.01;
}

// d/dt of (x, th, xd, thd) under the slider force fu
__device__ inline void invpendulum_dsdt(const double* y, double fu, double* k) {
  const double x = y[0], th = y[1], xd = y[2], thd = y[3];
  double sn, cs;
  sincos(th, &sn, &cs);
  const double m01 = IP_B * cs;
  const double c0 = -(IP_B * sn) * (thd * thd);
  const double g1 = IP_B * IP_GZ * sn;
  const double r0 = fu - c0 - IP_DAMP * xd + ch_limit(x, xd, CH_XLIM, CH_KS, CH_CS);
  const double r1 = -g1 - IP_DAMP * thd + ch_limit(th, thd, IP_HLIM, CH_KH, CH_CH);
  // LDL^T of [[MT, m01], [m01, J]]
  const double l10 = m01 / IP_MT;
  const double d1 = IP_J - l10 * l10 * IP_MT;
  const double y1 = r1 - l10 * r0;
  const double a1 = y1 / d1;
  const double a0 = r0 / IP_MT - l10 * a1;
  k[0] = xd;
  k[1] = thd;
  k[2] = a0;
  k[3] = a1;
}

__device__ inline void invpendulum_step(double* s, const float* a, double& rew, bool& done) {
  const double fu = IP_GEAR * ch_clamp((double)a[0], -IP_CTRL, IP_CTRL);
#pragma unroll 1
  for (int f = 0; f < IP_FRAME_SKIP; ++f)
    ch_rk4<IP_NS>(s, IP_DT, [fu](const double* y, double* k) { invpendulum_dsdt(y, fu, k); });
  const bool ok = isfinite(s[0]) & isfinite(s[1]) & isfinite(s[2]) & isfinite(s[3]) & (fabs(s[1]) <= IP_TH_DONE);
  done = !ok;
  rew = 1.0;
}

__device__ inline void invpendulum_obs(const double* s, double* o) {
  for (int i = 0; i < 4; ++i) o[i] = s[i];
}

struct InvPendulumEnv {
  static constexpr int NS = IP_NS, OBS = IP_OBS, ACT = IP_ACT, DISCRETE = 0, MAX_STEPS = 1000, NU = IP_NU;
  __device__ static void reset(const double* u, double* s) { invpendulum_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { invpendulum_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) { invpendulum_step(s, a, rew, done); }
};

// ------------------------------------------------------------------ InvertedDoublePendulum-v2
constexpr int DP_NS = 6, DP_OBS = 11, DP_ACT = 1, DP_NU = 8, DP_FRAME_SKIP = 5;
constexpr double DP_DT = 0.01, DP_GEAR = 500.0, DP_CTRL = 1.0, DP_DAMP = 0.05, DP_GX = 1e-5, DP_GZ = -9.81;
constexpr double DP_POLE_R = 0.045;
constexpr double DP_M = ch_capsule_mass(DP_POLE_R, CH_POLE_L), DP_I = ch_capsule_inertia(DP_POLE_R, CH_POLE_L);
constexpr double DP_L = CH_POLE_L, DP_LC = CH_POLE_L / 2.0;
constexpr double DP_MT = CH_MC + DP_M + DP_M;                                  // A00
constexpr double DP_A1 = DP_M * DP_LC + DP_M * DP_L;                           // A01 / cos phi_1
constexpr double DP_A2 = DP_M * DP_LC;                                         // A02 / cos phi_2
constexpr double DP_J1 = DP_I + DP_M * (DP_LC * DP_LC) + DP_M * (DP_L * DP_L);  // A11
constexpr double DP_J2 = DP_I + DP_M * (DP_LC * DP_LC);                        // A22
constexpr double DP_H = DP_M * DP_L * DP_LC;                                   // A12 / cos th2

__device__ inline void invdoublependulum_reset(const double* u, double* s) {
  for (int i = 0; i < 3; ++i) s[i] = u[i] * 0.2 - 0.1;
  // Box-Muller of oracle/philox.py on the pairs (u4, u5), (u6, u7)
  const double r0 = sqrt(-2.0 * log(1.0 - u[4])), r1 = sqrt(-2.0 * log(1.0 - u[6]));
  double s0, c0, s1, c1;
  sincos(2.0 * CH_PI * u[5], &s0, &c0);
  sincos(2.0 * CH_PI * u[7], &s1, &c1);
  s[3] = 0.1 * (r0 * c0);
  s[4] = 0.1 * (r0 * s0);
  s[5] = 0.1 * (r1 * c1);
}

// d/dt of (x, th1, th2, xd, th1d, th2d) under the slider force fu
__device__ inline void invdoublependulum_dsdt(const double* y, double fu, double* k) {
  const double x = y[0], t1 = y[1], t2 = y[2], xd = y[3], t1d = y[4], t2d = y[5];
  double s1, c1, s12, c12, s2, c2;
  sincos(t1, &s1, &c1);
  sincos(t1 + t2, &s12, &c12);
  sincos(t2, &s2, &c2);
  const double w1 = t1d, w2 = t1d + t2d;  // absolute pole rates
  const double w1s = w1 * w1, w2s = w2 * w2;
  const double a01 = DP_A1 * c1, a02 = DP_A2 * c12, a12 = DP_H * c2;
  const double m01 = a01 + a02, m02 = a02, m11 = (DP_J1 + DP_J2) + 2.0 * a12, m12 = a12 + DP_J2;
  // velocity and gravity terms in the absolute angles, mapped by J^T
  const double c0 = -(DP_A1 * s1) * w1s - (DP_A2 * s12) * w2s;
  const double hs = DP_H * s2;
  const double ca1 = -hs * w2s, ca2 = hs * w1s;
  const double ga1 = -DP_A1 * (DP_GX * c1 - DP_GZ * s1), ga2 = -DP_A2 * (DP_GX * c12 - DP_GZ * s12);
  const double r0 = fu - c0 + DP_MT * DP_GX - DP_DAMP * xd + ch_limit(x, xd, CH_XLIM, CH_KS, CH_CS);
  const double r1 = -(ca1 + ca2) - (ga1 + ga2) - DP_DAMP * t1d;
  const double r2 = -ca2 - ga2 - DP_DAMP * t2d;
  // LDL^T of [[MT, m01, m02], [m01, m11, m12], [m02, m12, J2]]
  const double l10 = m01 / DP_MT, l20 = m02 / DP_MT;
  const double d1 = m11 - l10 * l10 * DP_MT;
  const double l21 = (m12 - l20 * l10 * DP_MT) / d1;
  const double d2 = DP_J2 - l20 * l20 * DP_MT - l21 * l21 * d1;
  const double y1 = r1 - l10 * r0;
  const double y2 = r2 - l20 * r0 - l21 * y1;
  const double a2 = y2 / d2;
  const double a1 = y1 / d1 - l21 * a2;
  const double a0 = r0 / DP_MT - l10 * a1 - l20 * a2;
  k[0] = xd;
  k[1] = t1d;
  k[2] = t2d;
  k[3] = a0;
  k[4] = a1;
  k[5] = a2;
}

__device__ inline void invdoublependulum_step(double* s, const float* a, double& rew, bool& done) {
  const double fu = DP_GEAR * ch_clamp((double)a[0], -DP_CTRL, DP_CTRL);
#pragma unroll 1
  for (int f = 0; f < DP_FRAME_SKIP; ++f)
    ch_rk4<DP_NS>(s, DP_DT, [fu](const double* y, double* k) { invdoublependulum_dsdt(y, fu, k); });
  double s1, c1, s12, c12;
  sincos(s[1], &s1, &c1);
  sincos(s[1] + s[2], &s12, &c12);
  const double xt = s[0] + DP_L * s1 + DP_L * s12;
  const double yt = DP_L * c1 + DP_L * c12;
  const double dist = 0.01 * (xt * xt) + (yt - 2.0) * (yt - 2.0);
  const double vel = 1e-3 * (s[4] * s[4]) + 5e-3 * (s[5] * s[5]);
  rew = 10.0 - dist - vel;
  done = yt <= 1.0;
}

__device__ inline void invdoublependulum_obs(const double* s, double* o) {
  o[0] = s[0];
  o[1] = sin(s[1]);
  o[2] = sin(s[2]);
  o[3] = cos(s[1]);
  o[4] = cos(s[2]);
  for (int i = 0; i < 3; ++i) o[5 + i] = ch_clamp(s[3 + i], -10.0, 10.0);
  o[8] = ch_clamp(ch_limit(s[0], s[3], CH_XLIM, CH_KS, CH_CS), -10.0, 10.0);
  o[9] = 0.0;
  o[10] = 0.0;
}

struct InvDoublePendulumEnv {
  static constexpr int NS = DP_NS, OBS = DP_OBS, ACT = DP_ACT, DISCRETE = 0, MAX_STEPS = 1000, NU = DP_NU;
  __device__ static void reset(const double* u, double* s) { invdoublependulum_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { invdoublependulum_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) {
    invdoublependulum_step(s, a, rew, done);
  }
};

}  // namespace mrl
