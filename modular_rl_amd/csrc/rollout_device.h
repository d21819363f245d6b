// Device code shared by the rollout units -- rollout.hip and rollout_eval.hip (the fused 64-64
// path, kernel templates in rollout_kernels.h), rollout_layered.hip and rollout_layered_eval.hip
// (the layered path, rollout_layered_kernels.h), env_api.hip (the stand-alone env stepper and obs
// filter) and pop_rollout*.hip (the population rollouts): the list of the device envs
// (MRL_ENV_LIST) with what is generated from it -- EnvC<>, env_info(), env_known() -- the launch
// arguments RollArgs, env reset / sampling noise / sample-and-step / episode bookkeeping, the
// 16-lane fp64 sums, the Chan merge, the layered path's column partial and record merge, and
// the block set-up of the Humanoid wave-per-env kernels.  An env's dynamics and its traits
// struct are in its own header (envs*.h, humanoid.h).
#pragma once
#include <math.h>

#include <type_traits>

#include "../../include/mrl_hip.h"
#include "envs.h"
#include "envs_chains.h"
#include "envs_classic.h"
#include "envs_planar.h"
#include "envs_tree.h"
#include "mlp_device.h"

namespace mrl {

constexpr int RB = 256;  // threads per block
constexpr int ENVS_PER_BLOCK = 64;  // fused step: 4 waves x 16 envs
constexpr int MAXD = 16;  // obs dims + 1 (reward)
constexpr int MAXD_L = 384;  // obs dims + 1 on the layered path
// Layered-path kernels are parallel over (env block, 32-column chunk): the 376-d obs
// makes every per-column loop long, so no block walks all columns.
constexpr int LCOLS = 32;

// Hopper-v2 in the fused step kernel, where the four 16-lane rows of a wave hold
// the SAME 16 envs: row g evaluates sincos of segment angle g and the contacts of
// capsule g, and the rows exchange the results, so every row continues with the
// identical state.  All lanes must be active.
// the persistent kernel's capsule constants: the row's own six, read from the LDS table
// once per launch and held in registers (the other kernels select them per substep)
struct HopperQuad {
  int g;
  const double* capc;  // the row's capsule {rad, mu, u0, u1, w0, w1}, or null
  __device__ CapsuleC capsule(int) const {
    if (capc != nullptr) return CapsuleC{capc[0], capc[1], capc[2], capc[3], capc[4], capc[5]};
    return capsule_const(g);
  }
  __device__ void sincos4(const double* phi, double* s, double* c, double& so, double& co) const {
    double sx, cx;
    sincos(sel4(g, phi[0], phi[1], phi[2], phi[3]), &sx, &cx);
    quads(sx, s);
    quads(cx, c);
    so = sx;
    co = cx;
  }
  // segment k == g's value: the row's own (sel4(g, quads(x)) is x, bit for bit), with no
  // wait for the row exchange and no select
  __device__ double own(int, const double*, double v) const { return v; }
  template <class F>
  __device__ void contacts(F f, double (*ct)[3]) const {
    double own[3], x[4];
    f(g, own);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      quads(own[i], x);
#pragma unroll
      for (int k = 0; k < 4; ++k) ct[k][i] = x[k];
    }
  }
};

// One line per device env: the MRL_ENV_* id (include/mrl_hip.h) and the traits struct its
// header declares beside its dynamics -- constants NS / OBS / ACT / DISCRETE / MAX_STEPS / NU,
// reset(u, s), obs(s, o) and one step(s, a, rew, done) taking an int action (DISCRETE) or a
// const float* one.  T: an env a thread steps whole; W: Humanoid, stepped by the wave-per-env
// kernels (hm_*_kernel), constants only.  EnvC<>, env_info(), env_known() and rollout_host.h's
// two dispatches are generated from this list and name no env themselves.
#define MRL_ENV_LIST(T, W)                            \
  T(MRL_ENV_CARTPOLE, CartPoleEnv)                    \
  T(MRL_ENV_HOPPER, HopperEnv)                        \
  T(MRL_ENV_PENDULUM, PendulumEnv)                    \
  T(MRL_ENV_MOUNTAINCAR, MountainCarEnv)              \
  T(MRL_ENV_ACROBOT, AcrobotEnv)                      \
  T(MRL_ENV_INVPENDULUM, InvPendulumEnv)              \
  T(MRL_ENV_INVDOUBLEPENDULUM, InvDoublePendulumEnv)  \
  T(MRL_ENV_REACHER, ReacherEnv)                      \
  T(MRL_ENV_SWIMMER, SwimmerEnv)                      \
  T(MRL_ENV_HALFCHEETAH, HalfCheetahEnv)              \
  W(MRL_ENV_HUMANOID, HumanoidEnv)
#define MRL_ENV_NONE(ID, E)

// What the kernels see of an env: its traits E, and over them the obs rows handed to `out`
// and the fused step kernel's step.  A thread steps an env whole, so the four rows of the
// fused step all step it identically; only Hopper splits the work over them (HopperQuad).
template <class E>
struct EnvAdaptor : E {
  __device__ static void step_cont_quad(double* s, const float* a, double& rew, bool& done, int g,
                                        const double* capc) {
    if constexpr (std::is_same_v<E, HopperEnv>) hopper_step(s, a, rew, done, HopperQuad{g, capc});
    else E::step(s, a, rew, done);
  }
  template <class Out>
  __device__ static void obs_out(const double* s, Out out) {
    double o[E::OBS];
    E::obs(s, o);
#pragma unroll
    for (int k = 0; k < E::OBS; ++k) out(k, o[k]);
  }
};
// keyed on the id, so that the kernel templates <int ENV> keep their names
template <int ENV>
struct EnvC;
#define MRL_ENV_BIND(ID, E) \
  template <>               \
  struct EnvC<ID> : EnvAdaptor<E> {};
MRL_ENV_LIST(MRL_ENV_BIND, MRL_ENV_BIND)
#undef MRL_ENV_BIND

struct EnvInfo {
  int ns, obs, act, discrete, max_steps;
};
template <class E>
__host__ __device__ constexpr EnvInfo env_info_of() {
  return EnvInfo{E::NS, E::OBS, E::ACT, E::DISCRETE, E::MAX_STEPS};
}
// an id that is not in the list has Hopper's row
__host__ __device__ inline EnvInfo env_info(int id) {
#define MRL_ENV_ROW(ID, E) \
  if (id == ID) return env_info_of<E>();
  MRL_ENV_LIST(MRL_ENV_ROW, MRL_ENV_ROW)
#undef MRL_ENV_ROW
  return env_info_of<HopperEnv>();
}
// the ids the entry points take (MRL_ENV_*; 3, 7, 10 and 13 are not)
__host__ __device__ inline bool env_known(int id) {
#define MRL_ENV_ROW(ID, E) \
  if (id == ID) return true;
  MRL_ENV_LIST(MRL_ENV_ROW, MRL_ENV_ROW)
#undef MRL_ENV_ROW
  return false;
}
__host__ __device__ inline int filt_doubles(int obs) { return 2 + 2 * (obs + 1); }

struct RollArgs {
  mrl_rollout_desc d;
  mrl_rollout_bufs b;
  int nb;      // blocks
  int FS, RS;  // filter / record doubles
};

template <int ENV>
__device__ inline void reset_env(const RollArgs& a, int e, double* s) {
  const int E = a.d.n_envs;
  const uint32_t gid = (uint32_t)(a.d.env_offset + e);
  const uint64_t w = (uint64_t)(uint32_t)a.b.env_int[E + e];
  double u[EnvC<ENV>::NU];
#pragma unroll
  for (int c = 0; c < EnvC<ENV>::NU / 2; ++c) philox_uniform2(a.d.seed, 1, gid, w, (uint32_t)c, u[2 * c], u[2 * c + 1]);
  EnvC<ENV>::reset(u, s);
  a.b.env_int[E + e] = (int32_t)(w + 1);
  a.b.env_int[e] = 0;
}

// sum over the 16 lanes of an aligned 16-lane row by DPP (no LDS round trips): lane
// pairs i^1, i^2 (quad_perm), then i <-> 7-i (row_half_mirror), i <-> 15-i (row_mirror);
// every add is commutative in its pair, so all 16 lanes end with the same bits
template <int CTRL>
__device__ inline double dpp_d(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// x / n for an env count n >= 0 (a mean of n values): when every active lane's n is a power
// of two -- a full 64-env block, E = 4096 -- the multiply by the exact 2^-k instead, which is
// the same correctly rounded value as the division (x 2^-k and x / 2^k round the same real
// number once), without the division's dependent v_div_scale / v_rcp / fma chain on the
// step's critical path; the branch is wave-uniform (a ballot)
__device__ inline double div_count(double x, double n) {
  int e;
  const double m = frexp(n, &e);
  if (__builtin_amdgcn_ballot_w64(m != 0.5) == 0) return x * ldexp(1.0, 1 - e);
  return x / n;
}

__device__ inline double sum16(double v) {
  v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_d<0x141>(v);  // row_half_mirror
  v += dpp_d<0x140>(v);  // row_mirror
  return v;
}

// Chan merge of (nb, mb, m2b) into (n, M, S); for nb == 1 this is RunningStat.push
__device__ inline void chan_merge(double& n, double& M, double& S, double nb, double mb, double m2b) {
  if (nb <= 0.0) return;
  const double na = n;
  const double nn = na + nb;
  const double delta = mb - M;
  const double newM = M + (delta * nb) / nn;
  S = S + m2b + delta * (mb - newM) * nb;
  M = newM;
  n = nn;
}

// the filter's mean and denominator std + 1e-8 of a column with running stat (n, M, S)
__device__ inline void filter_column(double n, double M, double S, double& mean, double& den) {
  const double var = n > 1.0 ? S / (n - 1.0) : M * M;  // running_stat.py:27
  mean = M;
  den = sqrt(var) + 1e-8;
}

// column k's running stat (n, M, S) into a filter state of D columns; the obs count is column
// 0's, the reward count the reward column's
__device__ inline void store_filter_column(double* fs, int D, int k, double n, double M, double S) {
  if (k == 0) fs[0] = n;
  if (k == D - 1) fs[1] = n;
  fs[2 + k] = M;
  fs[2 + D + k] = S;
}

// Sampling noise of env e at step t is Philox (gid, iteration*T + t) on domain 0:
// Categorical u = first uniform of call 0, Gauss z[2c], z[2c+1] = Box-Muller of call
// c.  A whole iteration's rows are drawn up front by noise_fill_kernel (one thread per
// (row, pair): the transcendental work leaves the step kernels' latency chain), or
// injected by the caller; the step kernels only load zn rows.
template <int ENV>
__device__ inline void load_noise(const RollArgs& a, int64_t row, double* zn) {
  using EC = EnvC<ENV>;
  const double* nz = reinterpret_cast<const double*>(a.b.noise);
  if constexpr (EC::DISCRETE) zn[0] = nz[row];
  else
#pragma unroll
    for (int q = 0; q < EC::ACT; ++q) zn[q] = nz[row * EC::ACT + q];
}

// z + sd * noise in fp32 with the product rounded before the sum (core.py:432-435: numpy's two
// roundings).  __fmul_rn / __fadd_rn do not give that: the compiler's headers define them as
// plain * and +, which the default -ffp-contract fuses into one v_fma_f32 (one rounding), so
// the contraction is switched off for this product and sum.  The layered rollout's kernels
// sample with it (tests/test_gpu_layered_step.py holds their actions to the two roundings bit
// for bit); the fused 64-64 step kernels (QUAD) keep the contracted form they have always
// computed -- at most one ulp of the action away -- because their trajectories are what the fused
// rollout tests and the benchmark were recorded against
__device__ inline float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p + c;
}

// sample the action from the head rows z (core.py:261-267; distributions.py:3-13 /
// core.py:432-435), write act/prob rows, step the env (fp64)
// QUAD: the four 16-lane rows of the wave hold this env (fused step kernel); every
// lane steps it (row h = lane >> 4 of the angle functions), lanes with `store` write
// SD: `logstd` holds the standard deviations exp(logstd) already (the persistent kernel
// forms them once per launch: the same expf, not one per step)
template <int ENV, bool QUAD = false, bool SD = false>
__device__ inline void sample_and_step(const RollArgs& a, int64_t row, const float* z, const float* logstd,
                                       const double* zn, double* s, double& rew, bool& done, bool store = true,
                                       int h = 0, const double* capc = nullptr) {
  using EC = EnvC<ENV>;
  constexpr int A = EC::ACT;
  if constexpr (EC::DISCRETE) {
    float m = z[0];
#pragma unroll
    for (int q = 1; q < A; ++q) m = fmaxf(m, z[q]);
    float p[A], se = 0.f;
#pragma unroll
    for (int q = 0; q < A; ++q) {
      p[q] = expf(z[q] - m);
      se += p[q];
    }
#pragma unroll
    for (int q = 0; q < A; ++q) p[q] = p[q] / se;
    const double u = zn[0];
    int act = 0;
    float cs = 0.f;
    bool found = false;
#pragma unroll
    for (int q = 0; q < A; ++q) {
      cs += p[q];
      if (!found && (double)cs > u) {
        act = q;
        found = true;
      }
    }
    if (store) {
      reinterpret_cast<int32_t*>(a.b.act)[row] = act;
#pragma unroll
      for (int q = 0; q < A; ++q) a.b.prob[row * A + q] = p[q];
    }
    EC::step(s, act, rew, done);
  } else {
    float av[A];
#pragma unroll
    for (int q = 0; q < A; ++q) {
      const float sd = SD ? logstd[q] : expf(logstd[q]);
      av[q] = QUAD ? __fadd_rn(__fmul_rn((float)zn[q], sd), z[q]) : mul_then_add((float)zn[q], sd, z[q]);
      if (store) {
        reinterpret_cast<float*>(a.b.act)[row * A + q] = av[q];
        a.b.prob[row * 2 * A + q] = z[q];
        a.b.prob[row * 2 * A + A + q] = sd;
      }
    }
    if constexpr (QUAD) EC::step_cont_quad(s, av, rew, done, h, capc);
    else EC::step(s, av, rew, done);
  }
}

// ------------------------------------------------------------------ evaluation mode
// MRL_ROLLOUT_EVAL (mrl_hip.h): the kernels' EV instantiations.  Its own text, beside
// sample_and_step rather than folded into it (§3's Box-Muller note: a shared helper has changed
// the existing listings before).
//
// column k of the frozen observation filter: what mrl_pop_rollout feeds its policies -- the
// state's mean and sqrt(S / (n - 1)) + 1e-8, or with fewer than two observations mean 0 and
// denominator 1, which leave the observation bit for bit (the caller clips at +-5)
__device__ inline void frozen_filter_column(const double* fs, int D, int k, double& mean, double& den) {
  const double n = fs[0];
  mean = 0.0;
  den = 1.0;
  if (n >= 2.0) {
    mean = fs[2 + k];
    den = sqrt(fs[2 + D + k] / (n - 1.0)) + 1e-8;
  }
}

// sample_and_step with the head's mode for the action (ProbType.maxprob; core.py:261-267 with
// stochastic = False): the Gauss mean, or the arg-max logit with the lowest index on a tie
// (np.argmax).  No noise row is read; act / prob rows as sample_and_step writes them.
template <int ENV, bool QUAD = false, bool SD = false>
__device__ inline void mode_and_step(const RollArgs& a, int64_t row, const float* z, const float* logstd, double* s,
                                     double& rew, bool& done, bool store = true, int h = 0,
                                     const double* capc = nullptr) {
  using EC = EnvC<ENV>;
  constexpr int A = EC::ACT;
  if constexpr (EC::DISCRETE) {
    float m = z[0];
    int act = 0;
#pragma unroll
    for (int q = 1; q < A; ++q)
      if (z[q] > m) {
        m = z[q];
        act = q;
      }
    float p[A], se = 0.f;
#pragma unroll
    for (int q = 0; q < A; ++q) {
      p[q] = expf(z[q] - m);
      se += p[q];
    }
    if (store) {
      reinterpret_cast<int32_t*>(a.b.act)[row] = act;
#pragma unroll
      for (int q = 0; q < A; ++q) a.b.prob[row * A + q] = p[q] / se;
    }
    EC::step(s, act, rew, done);
  } else {
    float av[A];
#pragma unroll
    for (int q = 0; q < A; ++q) {
      av[q] = z[q];
      if (store) {
        reinterpret_cast<float*>(a.b.act)[row * A + q] = z[q];
        a.b.prob[row * 2 * A + q] = z[q];
        a.b.prob[row * 2 * A + A + q] = SD ? logstd[q] : expf(logstd[q]);
      }
    }
    if constexpr (QUAD) EC::step_cont_quad(s, av, rew, done, h, capc);
    else EC::step(s, av, rew, done);
  }
}

// episode bookkeeping: gym TimeLimit => done (terminated, bootstrap 0); the rollout
// loop limit / horizon cut => not terminated (core.py:190-207, 73); auto-reset; store
template <int ENV>
__device__ inline void finish_env_step(const RollArgs& a, int e, int64_t row, int t, double* s, double rew, bool done) {
  using EC = EnvC<ENV>;
  const int E = a.d.n_envs;
  const int ept = a.b.env_int[e];
  a.b.ep_t[row] = ept;
  const bool term = done || (ept + 1 >= EC::MAX_STEPS);
  const bool last = term || (ept + 1 >= a.d.timestep_limit) || (t == a.d.horizon - 1);
  a.b.rew[row] = (float)rew;
  a.b.flags[row] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
  if (last && t < a.d.horizon - 1) reset_env<ENV>(a, e, s);
  else a.b.env_int[e] = ept + 1;
#pragma unroll
  for (int i = 0; i < EC::NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
}

// episode bookkeeping of finish_env_step without the horizon: TimeLimit => terminated,
// the caller's limit => ended, not terminated
template <int ENV>
__device__ inline void env_step_flags(const RollArgs& a, int ept, bool done, bool& term, bool& last) {
  term = done || (ept + 1 >= EnvC<ENV>::MAX_STEPS);
  last = term || (a.d.timestep_limit > 0 && ept + 1 >= a.d.timestep_limit);
}

// bf16 RNE round trip (the bf16 compute mode's operand rounding on the f32-input MFMA)
__device__ inline float bf16r(float x) { return (float)(__bf16)x; }

// two-pass (mean, M2) of one column over a block's nvalid rows, for the 256 threads of an
// (env block, 32-column chunk) block: thread (c = tid & 31, g = tid >> 5) takes rows g, g + 8,
// ... of column c through load(row), loaded once, all issued together, for both passes; the
// sums stay in row order.  Shared by the layered rollout's partials and the stand-alone
// filter, which must agree bit for bit.  The results are valid in the threads with g == 0.
template <class Load>
__device__ inline void col_partial(Load load, int nvalid, bool kin, double (*red)[LCOLS], int c, int g, double& mean,
                                   double& m2out) {
  constexpr int PR = ENVS_PER_BLOCK / 8;
  double cv[PR];
#pragma unroll
  for (int q = 0; q < PR; ++q) cv[q] = load(min(g + 8 * q, max(nvalid - 1, 0)));  // clamped: in the column
  double sm = 0.0;
  if (kin)
#pragma unroll
    for (int q = 0; q < PR; ++q)
      if (g + 8 * q < nvalid) sm += cv[q];
  red[g][c] = sm;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int q = 0; q < 8; ++q) tot += red[q][c];
  mean = nvalid > 0 ? div_count(tot, (double)nvalid) : 0.0;
  __syncthreads();
  double m2 = 0.0;
  if (kin)
#pragma unroll
    for (int q = 0; q < PR; ++q)
      if (g + 8 * q < nvalid) {
        const double dv = cv[q] - mean;
        m2 += dv * dv;
      }
  red[g][c] = m2;
  __syncthreads();
  double t2 = 0.0;
  if (g == 0 && kin)
#pragma unroll
    for (int q = 0; q < 8; ++q) t2 += red[q][c];
  m2out = t2;
}

// column k of the batch records (block order, two passes: n, mean = sum n_b m_b / n,
// M2 = sum M2_b + n_b (m_b - mean)^2 -- oracle/rollout_np.py _batch) Chan-merged into the
// running stat fs_in -> (n, M, S).  Shared by lrollout_obs_kernel and the stand-alone filter.
__device__ inline void merge_records_column(const double* rec, int nb, int RS, int D, int k, bool isr,
                                            const double* fs_in, double& n, double& M, double& S) {
  // the block records in chunks of LREC: every load of a chunk issued before the
  // chunk's sums (the sums themselves stay sequential in block order, as the oracle's);
  // one dependent global load per block per pass had made this launch ~14 us of waiting
  constexpr int LREC = 16;
  double bn = 0.0, sm = 0.0, bm = 0.0, bs = 0.0;
  // the filter's M2 terms and the fs_in state loaded with the first chunk (one record
  // round trip when nb <= LREC: the second pass reuses the first's loads)
  double rn1[LREC], rm1[LREC], rs1[LREC];
  const double n0 = fs_in[isr ? 1 : 0], M0 = fs_in[2 + k], S0 = fs_in[2 + D + k];
  if (nb <= LREC) {
#pragma unroll
    for (int q = 0; q < LREC; ++q) {
      const double* r = rec + (int64_t)min(q, nb - 1) * RS;
      rn1[q] = r[isr ? 1 : 0];
      rm1[q] = r[2 + k];
      rs1[q] = r[2 + D + k];
    }
#pragma unroll
    for (int q = 0; q < LREC; ++q)
      if (q < nb) {
        bn += rn1[q];
        sm += rn1[q] * rm1[q];
      }
    if (bn > 0.0) {
      bm = sm / bn;
#pragma unroll
      for (int q = 0; q < LREC; ++q)
        if (q < nb && rn1[q] > 0.0) {
          const double dm = rm1[q] - bm;
          bs += rs1[q] + rn1[q] * dm * dm;
        }
    }
  } else {
    for (int b0 = 0; b0 < nb; b0 += LREC) {
      double rn[LREC], rm[LREC];
#pragma unroll
      for (int q = 0; q < LREC; ++q) {
        const double* r = rec + (int64_t)min(b0 + q, nb - 1) * RS;
        rn[q] = r[isr ? 1 : 0];
        rm[q] = r[2 + k];
      }
#pragma unroll
      for (int q = 0; q < LREC; ++q)
        if (b0 + q < nb) {
          bn += rn[q];
          sm += rn[q] * rm[q];
        }
    }
    if (bn > 0.0) {
      bm = sm / bn;
      for (int b0 = 0; b0 < nb; b0 += LREC) {
        double rn[LREC], rm[LREC], rs[LREC];
#pragma unroll
        for (int q = 0; q < LREC; ++q) {
          const double* r = rec + (int64_t)min(b0 + q, nb - 1) * RS;
          rn[q] = r[isr ? 1 : 0];
          rm[q] = r[2 + k];
          rs[q] = r[2 + D + k];
        }
#pragma unroll
        for (int q = 0; q < LREC; ++q)
          if (b0 + q < nb && rn[q] > 0.0) {
            const double dm = rm[q] - bm;
            bs += rs[q] + rn[q] * dm * dm;
          }
      }
    }
  }
  n = n0, M = M0, S = S0;
  chan_merge(n, M, S, bn, bm, bs);
}

// The block of the Humanoid wave-per-env kernels (hm_reset_kernel, hm_act_kernel, hm_env_*_kernel).
// WPB waves (envs) per block: 1 -- a one-wave block per env, padded so that at most four
// share a CU (hm_lds_pad) -- or 4 -- four envs per block sharing one copy of the model
// tables (94 KB of LDS, so one block per CU; the LDS left beside it takes a co-scheduled
// kernel's blocks without displacing an env).  Waves are independent after the tables'
// barrier (a wave's LDS operations complete in issue order).
// The tables and (WPB = 1) the env's state are static LDS objects -- their addresses are
// constants the ds instructions take as offsets; the WPB = 4 states sit in dynamic LDS
// after them, one wave-uniform base each.
template <int WPB>
__device__ inline hm::Wave& hm_block(int& e, int& lane) {
  extern __shared__ __attribute__((aligned(16))) double hm_dyn[];
  lane = threadIdx.x & 63;
  if constexpr (WPB == 1) {
    __shared__ hm::Wave W1;
    e = blockIdx.x;
    return W1;
  } else {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    e = blockIdx.x * WPB + wave;
    return reinterpret_cast<hm::Wave*>(hm_dyn)[wave];
  }
}
template <int WPB>
__device__ inline void hm_load_tables(hm::Shared& S, int lane) {
  if (WPB == 1) {
    hm::load_shared(S, lane);
  } else {  // the block's waves copy disjoint parts, then wait for each other
    const double* src = reinterpret_cast<const double*>(&hm::SHARED);
    double* dst = reinterpret_cast<double*>(&S);
    for (int i = threadIdx.x; i < (int)(sizeof(hm::Shared) / 8); i += 64 * WPB) dst[i] = src[i];
    __syncthreads();
  }
}

}  // namespace mrl
