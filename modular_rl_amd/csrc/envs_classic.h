// Classic-control env dynamics on device beside envs.h's CartPole (fp64, FMA contraction
// off), operation-for-operation twins of tests/classic_envs_np.py.  The equations restate
// gym's classic_control sources of the reference's era (its coverage.sh runs Acrobot and
// Pendulum; its "classic" experiment batteries add MountainCar); gym itself is absent, so
// parity with it is unpinned, as CartPole's is.
//
//  * Pendulum-v0: state (th, thdot), obs (cos th, sin th, thdot), one torque in [-2, 2];
//    never done by itself (TimeLimit 200).
//  * MountainCar-v0: state = obs = (position, velocity), three actions (push left, none,
//    right); done at position >= 0.5 (TimeLimit 200).
//  * Acrobot-v1: state (t1, t2, w1, w2), obs (cos t1, sin t1, cos t2, sin t2, w1, w2), three
//    torques -1 / 0 / +1 on the second joint; one RK4 step of dt 0.2 on the "book"
//    equations; done when the tip is above the bar by one link (TimeLimit 500).
#pragma once
#include "mrl_common.h"

#pragma clang fp contract(off)

namespace mrl {

constexpr double CC_PI = 3.141592653589793, CC_2PI = 2.0 * CC_PI;

__device__ inline double cc_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------ Pendulum-v0
constexpr int PD_NS = 2, PD_OBS = 3, PD_ACT = 1;
constexpr double PD_MAX_SPEED = 8.0, PD_MAX_TORQUE = 2.0, PD_DT = 0.05;
constexpr double PD_G = 10.0, PD_M = 1.0, PD_L = 1.0;

__device__ inline void pendulum_reset(const double* u, double* s) {
  s[0] = u[0] * CC_2PI - CC_PI;
  s[1] = u[1] * 2.0 - 1.0;
}

__device__ inline void pendulum_step(double* s, const float* a, double& rew, bool& done) {
  const double th = s[0], thdot = s[1];
  const double u = cc_clamp((double)a[0], -PD_MAX_TORQUE, PD_MAX_TORQUE);
  // angle_normalize: a floored mod by 2 pi (the result in [0, 2 pi)), shifted to [-pi, pi)
  double md = fmod(th + CC_PI, CC_2PI);
  if (md < 0.0) md = md + CC_2PI;
  const double an = md - CC_PI;
  const double cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u);
  double nthd = thdot + (-3.0 * PD_G / (2.0 * PD_L) * sin(th + CC_PI) + 3.0 / (PD_M * (PD_L * PD_L)) * u) * PD_DT;
  s[0] = th + nthd * PD_DT;  // the unclipped speed
  s[1] = cc_clamp(nthd, -PD_MAX_SPEED, PD_MAX_SPEED);
  rew = -cost;
  done = false;
}

__device__ inline void pendulum_obs(const double* s, double* o) {
  o[0] = cos(s[0]);
  o[1] = sin(s[0]);
  o[2] = s[1];
}

struct PendulumEnv {
  static constexpr int NS = PD_NS, OBS = PD_OBS, ACT = PD_ACT, DISCRETE = 0, MAX_STEPS = 200, NU = 2;
  __device__ static void reset(const double* u, double* s) { pendulum_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { pendulum_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) { pendulum_step(s, a, rew, done); }
};

// ------------------------------------------------------------------ MountainCar-v0
constexpr int MC_NS = 2, MC_OBS = 2;
constexpr double MC_MIN_POS = -1.2, MC_MAX_POS = 0.6, MC_MAX_SPEED = 0.07, MC_GOAL = 0.5;

__device__ inline void mountaincar_reset(const double* u, double* s) {
  s[0] = u[0] * 0.2 - 0.6;
  s[1] = 0.0;  // u[1]: the pair's second uniform, unused
}

__device__ inline void mountaincar_step(double* s, int a, double& rew, bool& done) {
  double p = s[0], v = s[1];
  v = v + ((double)(a - 1) * 0.001 + cos(3.0 * p) * (-0.0025));
  v = cc_clamp(v, -MC_MAX_SPEED, MC_MAX_SPEED);
  p = p + v;
  p = cc_clamp(p, MC_MIN_POS, MC_MAX_POS);
  if (p == MC_MIN_POS && v < 0.0) v = 0.0;
  s[0] = p;
  s[1] = v;
  done = p >= MC_GOAL;
  rew = -1.0;
}

__device__ inline void mountaincar_obs(const double* s, double* o) {
  o[0] = s[0];
  o[1] = s[1];
}

struct MountainCarEnv {
  static constexpr int NS = MC_NS, OBS = MC_OBS, ACT = 3, DISCRETE = 1, MAX_STEPS = 200, NU = 2;
  __device__ static void reset(const double* u, double* s) { mountaincar_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { mountaincar_obs(s, o); }
  __device__ static void step(double* s, int a, double& rew, bool& done) { mountaincar_step(s, a, rew, done); }
};

// ------------------------------------------------------------------ Acrobot-v1
constexpr int AC_NS = 4, AC_OBS = 6;
constexpr double AC_DT = 0.2, AC_M1 = 1.0, AC_M2 = 1.0, AC_L1 = 1.0, AC_LC1 = 0.5, AC_LC2 = 0.5;
constexpr double AC_I1 = 1.0, AC_I2 = 1.0, AC_G = 9.8;
constexpr double AC_MAX_W1 = 4.0 * CC_PI, AC_MAX_W2 = 9.0 * CC_PI;
// wrap(): +-2 pi at most this many times.  The speeds are clamped every step, so a stored
// state is never more than a turn or two out; the bound keeps a state written from
// outside (an infinity, 1e300) from spinning a lane forever.
constexpr int AC_WRAP_MAX = 8;

__device__ inline void acrobot_reset(const double* u, double* s) {
  for (int i = 0; i < 4; ++i) s[i] = u[i] * 0.2 - 0.1;
}

// d/dt of (t1, t2, w1, w2) under torque tau ("book" equations).  cos(x - pi/2) is taken as
// sin x: the same function, and exact at the hanging equilibrium, where the rounded pi/2
// would leave a torque of 6e-17.
__device__ inline void acrobot_dsdt(const double* y, double tau, double* k) {
  const double t1 = y[0], t2 = y[1], w1 = y[2], w2 = y[3];
  const double c2 = cos(t2), s2 = sin(t2);
  const double d1 = AC_M1 * (AC_LC1 * AC_LC1) + AC_M2 * (AC_L1 * AC_L1 + AC_LC2 * AC_LC2 + 2.0 * AC_L1 * AC_LC2 * c2) +
                    AC_I1 + AC_I2;
  const double d2 = AC_M2 * (AC_LC2 * AC_LC2 + AC_L1 * AC_LC2 * c2) + AC_I2;
  const double phi2 = AC_M2 * AC_LC2 * AC_G * sin(t1 + t2);
  const double phi1 = -AC_M2 * AC_L1 * AC_LC2 * (w2 * w2) * s2 - 2.0 * AC_M2 * AC_L1 * AC_LC2 * w2 * w1 * s2 +
                      (AC_M1 * AC_LC1 + AC_M2 * AC_L1) * AC_G * sin(t1) + phi2;
  const double dw2 = (tau + d2 / d1 * phi1 - AC_M2 * AC_L1 * AC_LC2 * (w1 * w1) * s2 - phi2) /
                     (AC_M2 * (AC_LC2 * AC_LC2) + AC_I2 - d2 * d2 / d1);
  const double dw1 = -(d2 * dw2 + phi1) / d1;
  k[0] = w1;
  k[1] = w2;
  k[2] = dw1;
  k[3] = dw2;
}

__device__ inline double acrobot_wrap(double x) {
  for (int i = 0; i < AC_WRAP_MAX && x > CC_PI; ++i) x = x - CC_2PI;
  for (int i = 0; i < AC_WRAP_MAX && x < -CC_PI; ++i) x = x + CC_2PI;
  return x;
}

__device__ inline void acrobot_step(double* s, int a, double& rew, bool& done) {
  const double tau = (double)(a - 1);
  double k1[4], k2[4], k3[4], k4[4], y[4];
  acrobot_dsdt(s, tau, k1);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + (AC_DT / 2.0) * k1[i];
  acrobot_dsdt(y, tau, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + (AC_DT / 2.0) * k2[i];
  acrobot_dsdt(y, tau, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + AC_DT * k3[i];
  acrobot_dsdt(y, tau, k4);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + (AC_DT / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  s[0] = acrobot_wrap(y[0]);
  s[1] = acrobot_wrap(y[1]);
  s[2] = cc_clamp(y[2], -AC_MAX_W1, AC_MAX_W1);
  s[3] = cc_clamp(y[3], -AC_MAX_W2, AC_MAX_W2);
  done = -cos(s[0]) - cos(s[1] + s[0]) > 1.0;
  rew = done ? 0.0 : -1.0;
}

__device__ inline void acrobot_obs(const double* s, double* o) {
  o[0] = cos(s[0]);
  o[1] = sin(s[0]);
  o[2] = cos(s[1]);
  o[3] = sin(s[1]);
  o[4] = s[2];
  o[5] = s[3];
}

struct AcrobotEnv {
  static constexpr int NS = AC_NS, OBS = AC_OBS, ACT = 3, DISCRETE = 1, MAX_STEPS = 500, NU = 4;
  __device__ static void reset(const double* u, double* s) { acrobot_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { acrobot_obs(s, o); }
  __device__ static void step(double* s, int a, double& rew, bool& done) { acrobot_step(s, a, rew, done); }
};

}  // namespace mrl
