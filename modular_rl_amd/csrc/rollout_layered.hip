// Layered-policy rollout: the kernels and C entry points.
//
// For policies the fused step kernel does not cover (wide nets, Humanoid's 376-d obs),
// step t is three launches: lrollout_obs (filter merge + normalised obs rows) ->
// the policy's GEMM forward over the E rows (LayeredMlpNet) -> lrollout_act (sample,
// env step, raw next obs + reward as SoA rows [O+1][E] fp64, block partials).
// Shares the env functions, the column partial and the record merge with the other rollout
// units (rollout_device.h).
#include "rollout_host.h"

namespace mrl {

#ifndef MRL_ROLLOUT_EVAL_UNIT
// per-(env block, column chunk) two-pass partial of the SoA rows raw[k][e0 .. e0+nvalid):
// column k = 32*blockIdx.y + (tid & 31); 8 thread groups stride the envs.
__global__ __launch_bounds__(RB) void lrollout_partials_kernel(RollArgs a, int D, int rec_parity, int with_rew) {
  __shared__ double red[8][LCOLS];
  const int E = a.d.n_envs;
  const int e0 = blockIdx.x * ENVS_PER_BLOCK;
  const int nvalid = min(ENVS_PER_BLOCK, E - e0);
  const int c = threadIdx.x & (LCOLS - 1), g = threadIdx.x >> 5;
  const int k = blockIdx.y * LCOLS + c;
  double* r = a.b.records + (int64_t)rec_parity * a.nb * a.RS + (int64_t)blockIdx.x * a.RS;
  const double* col = a.b.raw_obs + (int64_t)(k < D ? k : 0) * E + e0;
  double mean, t2;
  col_partial([&](int row) { return col[row]; }, nvalid, k < D, red, c, g, mean, t2);
  if (g == 0 && k < D) {
    r[2 + k] = mean;
    r[2 + D + k] = t2;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    r[0] = (double)nvalid;
    r[1] = with_rew ? (double)nvalid : 0.0;
  }
}
#endif  // MRL_ROLLOUT_EVAL_UNIT

template <int ENV>
__global__ __launch_bounds__(RB) void lrollout_reset_kernel(RollArgs a) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS;
  const int E = a.d.n_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) {
    double s[EC::NS];
    reset_env<ENV>(a, e, s);
#pragma unroll
    for (int i = 0; i < EC::NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
    double* raw = a.b.raw_obs;
    EC::obs_out(s, [&](int k, double v) { raw[(int64_t)k * E + e] = v; });
    raw[(int64_t)O * E + e] = 0.0;
  }
}

// merge of the batch records (block order, two passes: n, mean = sum n_b m_b / n,
// M2 = sum M2_b + n_b (m_b - mean)^2 -- oracle/rollout_np.py _batch) into the running
// stat, then the normalised obs rows of step t for this (env block, column chunk).
// EV (here, in lrollout_act_kernel and in hm_act_kernel): the evaluation instantiation
// (MRL_ROLLOUT_EVAL, rollout_device.h) -- here the frozen filter: no record is read, nothing
// is merged, the state is not written
template <int ENV, bool EV = false>
__global__ __launch_bounds__(RB) void lrollout_obs_kernel(RollArgs a, int t) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, D = O + 1;
  __shared__ double fmean[LCOLS], fden[LCOLS];
  constexpr int G = RB / ENVS_PER_BLOCK, CPT = LCOLS / G;  // thread groups over columns, columns per thread
  static_assert(RB % ENVS_PER_BLOCK == 0 && LCOLS % G == 0, "tile mapping");
  __shared__ float tile[LCOLS * (ENVS_PER_BLOCK + 1)];
  const int E = a.d.n_envs;
  const double* fs_in = a.b.filter_state + (t & 1) * a.FS;
  double* fs_out = a.b.filter_state + ((t + 1) & 1) * a.FS;
  const double* rec = a.b.records + (int64_t)(t & 1) * a.nb * a.RS;
  const int kbase = blockIdx.y * LCOLS;
  // this block's raw observation values, loaded first: their latency runs under the
  // record loads and the merge below (they do not depend on it)
  const int e0 = blockIdx.x * ENVS_PER_BLOCK;
  const int nvalid = min(ENVS_PER_BLOCK, E - e0);
  const int el = threadIdx.x % ENVS_PER_BLOCK, kb = threadIdx.x / ENVS_PER_BLOCK;
  double v[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int k = kbase + kb + G * q;
    v[q] = (k < O && el < nvalid) ? a.b.raw_obs[(int64_t)k * E + e0 + el] : 0.0;
  }
  if constexpr (EV) {
    if (threadIdx.x < LCOLS && kbase + (int)threadIdx.x < O)
      frozen_filter_column(a.b.filter_state, D, kbase + threadIdx.x, fmean[threadIdx.x], fden[threadIdx.x]);
  } else if (threadIdx.x < LCOLS && kbase + (int)threadIdx.x < D) {
    const int k = kbase + threadIdx.x;
    const bool isr = (k == O);
    double n, M, S;
    merge_records_column(rec, a.nb, a.RS, D, k, isr, fs_in, n, M, S);
    if (blockIdx.x == 0) {
      if (k == 0) fs_out[0] = n;
      if (isr) fs_out[1] = n;
      fs_out[2 + k] = M;
      fs_out[2 + D + k] = S;
    }
    const double var = n > 1.0 ? S / (n - 1.0) : M * M;  // running_stat.py:27
    fmean[threadIdx.x] = M;
    fden[threadIdx.x] = sqrt(var) + 1e-8;
  }
  __syncthreads();
  // normalised obs rows (core.py:191-192): SoA raw -> LDS tile -> row-major fp32 rows
  const int64_t row0 = (int64_t)t * E + e0;
  {
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int kl = kb + G * q;
      double x = v[q];
      if (a.d.filter) {
        x = x - fmean[kl];
        x = x / fden[kl];
        x = x < -5.0 ? -5.0 : (x > 5.0 ? 5.0 : x);
      }
      tile[kl * (ENVS_PER_BLOCK + 1) + el] = (float)x;
    }
  }
  __syncthreads();
  {
    const int el = threadIdx.x / G, part = threadIdx.x % G;
    if (el < nvalid) {
      float* dst = a.b.obs + (row0 + el) * O;
      // the bf16 twin of the row for the first hidden GEMM (mrl_cast_rows_bf16's RNE)
      uint16_t* dsb = a.b.obs_bf16 ? a.b.obs_bf16 + (int64_t)(e0 + el) * ((O + 7) / 8 * 8) : nullptr;
#pragma unroll
      for (int q = 0; q < CPT; ++q) {
        const int k = kbase + part * CPT + q;
        const float v = tile[(part * CPT + q) * (ENVS_PER_BLOCK + 1) + el];
        if (k < O) {
          dst[k] = v;
          if (dsb) dsb[k] = __builtin_bit_cast(uint16_t, (__bf16)v);
        }
      }
    }
  }
}

// sample + env step + raw next obs / reward (SoA) for one env per thread
template <int ENV, bool EV = false>
__global__ __launch_bounds__(RB) void lrollout_act_kernel(RollArgs a, const float* __restrict__ zrows,
                                                          const float* __restrict__ logstd, int t) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, NS = EC::NS, A = EC::ACT;
  const int E = a.d.n_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t row = (int64_t)t * E + e;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = a.b.env_state[(int64_t)i * E + e];
  float z[A];
#pragma unroll
  for (int q = 0; q < A; ++q) z[q] = zrows[(int64_t)e * A + q];
  double zn[A + 1];
  if constexpr (!EV) load_noise<ENV>(a, row, zn);
  double rew = 0.0;
  bool done = false;
  if constexpr (EV) mode_and_step<ENV>(a, row, z, logstd, s, rew, done);
  else sample_and_step<ENV>(a, row, z, logstd, zn, s, rew, done);
  finish_env_step<ENV>(a, e, row, t, s, rew, done);
  double* raw = a.b.raw_obs;
  EC::obs_out(s, [&](int k, double v) { raw[(int64_t)k * E + e] = v; });
  raw[(int64_t)O * E + e] = rew;
}

// Humanoid-v2 on the layered rollout: one wave per env (humanoid.h), its state in LDS.
// hm_reset_kernel = lrollout_reset_kernel, hm_act_kernel = lrollout_act_kernel.
// The block set-up (hm_block, hm_load_tables) is rollout_device.h's.
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_reset_kernel(RollArgs a) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  const int E = a.d.n_envs;
  hm_load_tables<WPB>(S, lane);
  if (e >= E) return;  // after the tables' barrier
  const uint32_t w = (uint32_t)a.b.env_int[E + e];
  hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
  hm::forward(W, S, lane);
  double* raw = a.b.raw_obs;
  hm::observation(W, S, lane, [&](int k, double v) { raw[(int64_t)k * E + e] = v; });
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, a.b.env_state + (int64_t)HM_NS * E + (int64_t)e * HM_KCACHE, lane);
  if (lane == 0) {
    raw[(int64_t)HM_OBS * E + e] = 0.0;
    a.b.env_int[E + e] = (int32_t)(w + 1);
    a.b.env_int[e] = 0;
  }
}

// The policy head fused into the step (HeadRows.hid != nullptr): z = hid[e] . W + b for
// the env's row of the last hidden layer, lane-strided over the hidden units (17
// accumulators per lane) and reduced across the wave in a fixed order -- one launch of
// a 1024 x 512 x 17 GEMM with 8 blocks (33 us per step) removed.  bf: the operands
// rounded to bf16 like the layered bf16 GEMM's (products and sums stay f32).
struct HeadRows {
  const float* hid;  // [E, nh] rows of the last hidden layer, or nullptr: z rows given
  const float* w;    // [nh, A] head kernel (Keras layout)
  const float* b;    // [A]
  int nh, bf;
  const uint16_t* hid16;  // the hidden rows as bf16 bits instead of hid (the bf16 tape's)
};

// lane l takes the KPL consecutive hidden units KPL l .. KPL l + KPL - 1: their head-kernel
// rows are one contiguous, 16-B aligned run of KPL A floats (KPL % 4 == 0), loaded as
// float4s -- a quarter of the strided lane-per-unit loads' instructions (nh = 64 KPL)
template <int KPL>
__device__ inline float head_z_runs(const HeadRows& hr, int e, int lane) {
  constexpr int A = HM_ACT;
  static_assert(KPL % 4 == 0, "16-B aligned runs");
  float acc[A], hv[KPL];
#pragma unroll
  for (int o = 0; o < A; ++o) acc[o] = 0.f;
  if (hr.hid16) {
    const uint4* h = reinterpret_cast<const uint4*>(hr.hid16 + (int64_t)e * hr.nh + KPL * lane);
#pragma unroll
    for (int q = 0; q < KPL / 8; ++q) {
      const uint4 u = h[q];
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hv[8 * q + 2 * r] = __uint_as_float(w[r] << 16);
        hv[8 * q + 2 * r + 1] = __uint_as_float(w[r] & 0xffff0000u);
      }
    }
    if constexpr (KPL % 8 != 0) {
      const uint2 u = reinterpret_cast<const uint2*>(hr.hid16 + (int64_t)e * hr.nh + KPL * lane)[KPL / 4 - 1];
      hv[KPL - 4] = __uint_as_float(u.x << 16);
      hv[KPL - 3] = __uint_as_float(u.x & 0xffff0000u);
      hv[KPL - 2] = __uint_as_float(u.y << 16);
      hv[KPL - 1] = __uint_as_float(u.y & 0xffff0000u);
    }
  } else {
    const float4* h = reinterpret_cast<const float4*>(hr.hid + (int64_t)e * hr.nh + KPL * lane);
#pragma unroll
    for (int q = 0; q < KPL / 4; ++q) {
      const float4 u = h[q];
      hv[4 * q] = hr.bf ? bf16r(u.x) : u.x;
      hv[4 * q + 1] = hr.bf ? bf16r(u.y) : u.y;
      hv[4 * q + 2] = hr.bf ? bf16r(u.z) : u.z;
      hv[4 * q + 3] = hr.bf ? bf16r(u.w) : u.w;
    }
  }
  const float4* w4 = reinterpret_cast<const float4*>(hr.w + (int64_t)KPL * lane * A);
#pragma unroll
  for (int q = 0; q < KPL * A / 4; ++q) {
    const float4 w = w4[q];
    const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 4 * q + r;
      acc[f % A] = fmaf(hv[f / A], hr.bf ? bf16r(ws[r]) : ws[r], acc[f % A]);
    }
  }
  float z = 0.f;
#pragma unroll
  for (int o = 0; o < A; ++o) {
    const float sum = wave_sumf(acc[o]);
    if (lane == o) z = sum + hr.b[o];
  }
  return z;
}

__device__ inline float head_z(const HeadRows& hr, int e, int lane) {
  constexpr int A = HM_ACT;
  const bool al = (reinterpret_cast<uintptr_t>(hr.w) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(hr.hid16 ? (const void*)hr.hid16 : (const void*)hr.hid) & 15) == 0;
  if (al && hr.nh == 512) return head_z_runs<8>(hr, e, lane);
  if (al && hr.nh == 256) return head_z_runs<4>(hr, e, lane);
  float acc[A];
#pragma unroll
  for (int o = 0; o < A; ++o) acc[o] = 0.f;
  const float* hrow = hr.hid + (int64_t)e * hr.nh;
  const uint16_t* hrow16 = hr.hid16 + (int64_t)e * hr.nh;
  for (int k = lane; k < hr.nh; k += 64) {
    const float hv = hr.hid16 ? __uint_as_float((uint32_t)hrow16[k] << 16) : (hr.bf ? bf16r(hrow[k]) : hrow[k]);
    const float* wr = hr.w + (int64_t)k * A;
#pragma unroll
    for (int o = 0; o < A; ++o) acc[o] = fmaf(hv, hr.bf ? bf16r(wr[o]) : wr[o], acc[o]);
  }
  float z = 0.f;
#pragma unroll
  for (int o = 0; o < A; ++o) {
    const float sum = wave_sumf(acc[o]);
    if (lane == o) z = sum + hr.b[o];
  }
  return z;
}

template <int WPB, bool EV = false>
__global__ __launch_bounds__(64 * WPB) void hm_act_kernel(RollArgs a, const float* __restrict__ zrows, HeadRows hr,
                                                          const float* __restrict__ logstd, int t) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  constexpr int A = HM_ACT;
  const int E = a.d.n_envs;
  const bool live = e < E;
  const int ec = live ? e : E - 1;  // a block's waves past E load a valid env, store nothing
  double* const kc = a.b.env_state + (int64_t)HM_NS * E + (int64_t)ec * HM_KCACHE;
  const bool fused = hr.hid != nullptr || hr.hid16 != nullptr;
  float zh = 0.f;
  if constexpr (WPB == 4) {
    // the model tables' global loads first, held in registers while the env's own loads
    // (state, kinematics cache) and the head's dot products run, stored behind them:
    // one load latency for the launch's prologue instead of three in sequence
    constexpr int NW = (int)(sizeof(hm::Shared) / 8), PER = (NW + 64 * WPB - 1) / (64 * WPB);
    const double* src = reinterpret_cast<const double*>(&hm::SHARED);
    double tv[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = (int)threadIdx.x + 64 * WPB * i;
      tv[i] = src[k < NW ? k : 0];
    }
    if (lane < HM_NS) W.s[lane] = a.b.env_state[(int64_t)lane * E + ec];
    hm::load_kcache(W, kc, lane);
    if (fused) zh = head_z(hr, ec, lane);
    double* dst = reinterpret_cast<double*>(&S);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = (int)threadIdx.x + 64 * WPB * i;
      if (k < NW) dst[k] = tv[i];
    }
    __syncthreads();
  } else {
    hm_load_tables<WPB>(S, lane);
    if (lane < HM_NS) W.s[lane] = a.b.env_state[(int64_t)lane * E + ec];
    hm::load_kcache(W, kc, lane);
    if (fused) zh = head_z(hr, ec, lane);
  }
  if (!live) return;  // after the tables' barrier
  const int64_t row = (int64_t)t * E + e;
  WAVE_SYNC();
  // sample (DiagGauss, core.py:432-435): a = z + sd * noise in fp32; the action is the ctrl
  if (lane < A) {
    const float z = fused ? zh : zrows[(int64_t)e * A + lane];
    const float sd = expf(logstd[lane]);
    float av = z;  // EV: the mean, no noise row is read
    if constexpr (!EV) {
      const double zn = reinterpret_cast<const double*>(a.b.noise)[row * A + lane];
      av = __fadd_rn(__fmul_rn((float)zn, sd), z);
    }
    reinterpret_cast<float*>(a.b.act)[row * A + lane] = av;
    a.b.prob[row * 2 * A + lane] = z;
    a.b.prob[row * 2 * A + A + lane] = sd;
    W.s[HM_NQ + HM_NV + lane] = (double)av;
  }
  WAVE_SYNC();
  // one forward site (the kernel's code must fit the instruction cache): passes
  // 0..FRAME_SKIP-1 are the substeps, pass FRAME_SKIP observes the new state, pass
  // FRAME_SKIP + 1 the reset one
  double x_before = 0.0, rew = 0.0;
  // diagnostic stamps of block 0 (cols 0-11: phases of pass 1, 12/15 realtime and
  // 13/14 shader clock at kernel start / end) -- never set in production
  int64_t* st = (a.b.stamps != nullptr && e == 0) ? a.b.stamps + (int64_t)t * 16 : nullptr;
  if (st != nullptr && lane == 0) {
    st[12] = (int64_t)__builtin_amdgcn_s_memrealtime();
    st[13] = (int64_t)__builtin_amdgcn_s_memtime();
  }
  for (int pass = 0;; ++pass) {
    int64_t* sp = pass == 1 ? st : nullptr;
    if (sp != nullptr && lane == 0) sp[0] = (int64_t)__builtin_amdgcn_s_memtime();
    if (pass > 0) hm::forward(W, S, lane, sp);  // pass 0: the kinematics cache
    if (pass < hm::FRAME_SKIP) {
      if (pass == 0) x_before = W.com[0];
      hm::accelerations(W, S, lane, sp);
      hm::integrate(W, lane);
      continue;
    }
    if (pass > hm::FRAME_SKIP) break;
    bool done;
    hm::reward_done(W, lane, x_before, rew, done);
    // episode bookkeeping (finish_env_step): TimeLimit => terminated, limit / horizon cut => not
    const int ept = a.b.env_int[e];
    const bool term = done || (ept + 1 >= EnvC<MRL_ENV_HUMANOID>::MAX_STEPS);
    const bool last = term || (ept + 1 >= a.d.timestep_limit) || (t == a.d.horizon - 1);
    if (lane == 0) {
      a.b.ep_t[row] = ept;
      a.b.rew[row] = (float)rew;
      a.b.flags[row] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
    }
    if (!(last && t < a.d.horizon - 1)) {
      if (lane == 0) a.b.env_int[e] = ept + 1;
      break;
    }
    const uint32_t w = (uint32_t)a.b.env_int[E + e];
    hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
    if (lane == 0) {
      a.b.env_int[E + e] = (int32_t)(w + 1);
      a.b.env_int[e] = 0;
    }
  }
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, kc, lane);  // W holds forward() of the state just stored
  double* raw = a.b.raw_obs;
  hm::observation(W, S, lane, [&](int k, double v) { raw[(int64_t)k * E + e] = v; });
  if (lane == 0) raw[(int64_t)HM_OBS * E + e] = rew;
  if (st != nullptr && lane == 0) {
    st[14] = (int64_t)__builtin_amdgcn_s_memtime();
    st[15] = (int64_t)__builtin_amdgcn_s_memrealtime();
  }
}

// ------------------------------------------------------------------ Humanoid, stand-alone stepper
// The stand-alone env stepper's (env_api.hip) Humanoid kernels: hm_reset_kernel / hm_act_kernel
// with the caller's rows and ctrl.  They are compiled in this unit, beside hm_act_kernel, and
// env_api.hip launches them through launch_hm_env_reset / launch_hm_env_step (rollout_host.h).
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_env_reset_kernel(RollArgs a, mrl_env_io io) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  const int E = a.d.n_envs;
  hm_load_tables<WPB>(S, lane);
  if (e >= E || (io.mask != nullptr && io.mask[e] == 0)) return;  // after the tables' barrier
  const uint32_t w = (uint32_t)a.b.env_int[E + e];
  hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
  hm::forward(W, S, lane);
  double* orow = io.obs + (int64_t)e * HM_OBS;
  hm::observation(W, S, lane, [&](int k, double v) { orow[k] = v; });
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, a.b.env_state + (int64_t)HM_NS * E + (int64_t)e * HM_KCACHE, lane);
  if (lane == 0) {
    a.b.env_int[E + e] = (int32_t)(w + 1);
    a.b.env_int[e] = 0;
  }
}

// hm_act_kernel with the caller's ctrl in place of the sampled one
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_env_step_kernel(RollArgs a, mrl_env_io io, int auto_reset) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  constexpr int A = HM_ACT;
  const int E = a.d.n_envs;
  const bool live = e < E;
  const int ec = live ? e : E - 1;  // a block's waves past E load a valid env, store nothing
  double* const kc = a.b.env_state + (int64_t)HM_NS * E + (int64_t)ec * HM_KCACHE;
  hm_load_tables<WPB>(S, lane);
  if (!live) return;  // after the tables' barrier
  if (lane < HM_NS) W.s[lane] = a.b.env_state[(int64_t)lane * E + e];
  hm::load_kcache(W, kc, lane);
  WAVE_SYNC();
  if (lane < A) W.s[HM_NQ + HM_NV + lane] = (double)reinterpret_cast<const float*>(io.act)[(int64_t)e * A + lane];
  WAVE_SYNC();
  // one forward and one observation site, as in hm_act_kernel: passes 0..FRAME_SKIP-1 are
  // the substeps, pass FRAME_SKIP observes the new state (into final_obs when the env is
  // reset in this call), pass FRAME_SKIP + 1 the reset one
  double x_before = 0.0, rew = 0.0;
  for (int pass = 0;; ++pass) {
    if (pass > 0) hm::forward(W, S, lane);  // pass 0: the kinematics cache
    if (pass < hm::FRAME_SKIP) {
      if (pass == 0) x_before = W.com[0];
      hm::accelerations(W, S, lane);
      hm::integrate(W, lane);
      continue;
    }
    double* orow = io.obs + (int64_t)e * HM_OBS;
    double* orow2 = nullptr;
    bool again = false;
    if (pass == hm::FRAME_SKIP) {
      bool done, term, last;
      hm::reward_done(W, lane, x_before, rew, done);
      const int ept = a.b.env_int[e];
      env_step_flags<MRL_ENV_HUMANOID>(a, ept, done, term, last);
      if (lane == 0) {
        io.ep_t[e] = ept;
        io.rew[e] = rew;
        io.flags[e] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
      }
      again = last && auto_reset;
      if (!again && lane == 0) a.b.env_int[e] = ept + 1;
      double* frow = io.final_obs != nullptr ? io.final_obs + (int64_t)e * HM_OBS : nullptr;
      if (again) orow = frow;  // the obs row waits for the reset state
      else if (last) orow2 = frow;
    }
    if (orow != nullptr)
      hm::observation(W, S, lane, [&](int k, double v) {
        orow[k] = v;
        if (orow2 != nullptr) orow2[k] = v;
      });
    if (!again) break;
    const uint32_t w = (uint32_t)a.b.env_int[E + e];
    hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
    if (lane == 0) {
      a.b.env_int[E + e] = (int32_t)(w + 1);
      a.b.env_int[e] = 0;
    }
  }
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, kc, lane);  // W holds forward() of the state just stored
}

#ifdef MRL_ROLLOUT_EVAL_UNIT
// The evaluation unit (rollout_layered_eval.hip compiles this file with MRL_ROLLOUT_EVAL_UNIT):
// the EV instantiations of lrollout_obs_kernel, lrollout_act_kernel and hm_act_kernel behind
// the launchers the entry points below call -- a unit of their own for rollout.hip's reason
// (its launchers): the training kernels' unit holds the kernels it held before.  No partials
// launch follows an evaluation step: there is nothing to merge.
void launch_lrollout_obs_eval(const RollArgs& a, int t, hipStream_t s) {
  const dim3 grid(a.nb, (env_info(a.d.env_id).obs + 1 + LCOLS - 1) / LCOLS);
  dispatch_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((lrollout_obs_kernel<env(), true>), grid, dim3(RB), 0, s, a, t);
  });
}
void launch_lrollout_act_eval(const RollArgs& a, const float* z, const HeadRows& hr, const float* logstd, int t,
                              hipStream_t s) {
  const int E = a.d.n_envs;
  if (a.d.env_id == MRL_ENV_HUMANOID) {
    const int wpb = hm_wpb();
    const dim3 grid((E + wpb - 1) / wpb), block(64 * wpb);
    const size_t lds = hm_lds_bytes(wpb, E);
    if (wpb == 4) hipLaunchKernelGGL((hm_act_kernel<4, true>), grid, block, lds, s, a, z, hr, logstd, t);
    else hipLaunchKernelGGL((hm_act_kernel<1, true>), grid, block, lds, s, a, z, hr, logstd, t);
    return;
  }
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((lrollout_act_kernel<env(), true>), dim3((E + 63) / 64), dim3(64), 0, s, a, z, logstd, t);
  });
}

}  // namespace mrl
#else
void launch_hm_env_reset(const RollArgs& a, const mrl_env_io& io, hipStream_t s) {
  MRL_LAUNCH_HM(hm_env_reset_kernel, hm_lds_state, a.d.n_envs, s, a, io);
}
void launch_hm_env_step(const RollArgs& a, const mrl_env_io& io, int auto_reset, hipStream_t s) {
  MRL_LAUNCH_HM(hm_env_step_kernel, hm_lds_bytes, a.d.n_envs, s, a, io, auto_reset);
}

}  // namespace mrl

using namespace mrl;

extern "C" {

static int check_rows(const mrl_rollout_desc* d, const mrl_rollout_bufs* b) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (!b->raw_obs) return fail(E_ARG, "the layered rollout needs raw_obs [(obs_dim+1) * n_envs] doubles");
  if (env_info(d->env_id).obs + 1 > MAXD_L) return fail(E_UNSUPPORTED, "obs dim too large");
  return OK;
}

int mrl_rollout_reset_rows(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  RollArgs a = make_args(d, b);
  const int D = env_info(d->env_id).obs + 1;
  // one wave per block: the per-env step is latency-bound, so spread the waves over CUs
  const dim3 genv((d->n_envs + 63) / 64), gpart(a.nb, (D + LCOLS - 1) / LCOLS);
  hipStream_t s = (hipStream_t)stream;
  if (d->env_id == MRL_ENV_HUMANOID) MRL_LAUNCH_HM(hm_reset_kernel, hm_lds_state, d->n_envs, s, a);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, lrollout_reset_kernel, genv, dim3(64), 0, s, a);
  // evaluation: the reset kernels as they are (raw_obs feeds the obs kernel), no partial of obs_0
  if (!roll_eval(d)) hipLaunchKernelGGL(lrollout_partials_kernel, gpart, dim3(RB), 0, s, a, D, 0, 0);
  return hip_check(hipGetLastError(), "mrl_rollout_reset_rows");
}

int mrl_rollout_obs(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  if (!b->obs) return fail(E_ARG, "null obs");
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const dim3 grid(a.nb, (env_info(d->env_id).obs + 1 + LCOLS - 1) / LCOLS);
  if (roll_eval(d)) launch_lrollout_obs_eval(a, t, (hipStream_t)stream);
  else MRL_DISPATCH_ENV(d->env_id, lrollout_obs_kernel, grid, dim3(RB), 0, (hipStream_t)stream, a, t);
  return hip_check(hipGetLastError(), "mrl_rollout_obs");
}

static int rollout_act(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* z, const HeadRows& hr,
                       const float* logstd, const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  if (!b->act || !b->prob || !b->rew || !b->flags || !b->ep_t || (!z && !hr.hid && !hr.hid16))
    return fail(E_ARG, "null trajectory buffer");
  if ((hr.hid || hr.hid16) && d->env_id != MRL_ENV_HUMANOID)
    return fail(E_UNSUPPORTED, "the fused head is the Humanoid step's");
  rc = check_noise(d, b);
  if (rc) return rc;
  EnvInfo ei = env_info(d->env_id);
  const bool gauss = head == MRL_HEAD_GAUSS;
  if (n_out != ei.act || gauss == (bool)ei.discrete || (!gauss && head != MRL_HEAD_SOFTMAX))
    return fail(E_ARG, "policy head does not match the env");
  if (gauss && !logstd) return fail(E_ARG, "DiagGauss needs logstd");
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const int D = ei.obs + 1;
  const dim3 genv((d->n_envs + 63) / 64), gpart(a.nb, (D + LCOLS - 1) / LCOLS);
  hipStream_t s = (hipStream_t)stream;
  if (roll_eval(d)) {
    launch_lrollout_act_eval(a, z, hr, logstd, t, s);
    return hip_check(hipGetLastError(), "mrl_rollout_act");
  }
  if (d->env_id == MRL_ENV_HUMANOID) MRL_LAUNCH_HM(hm_act_kernel, hm_lds_bytes, d->n_envs, s, a, z, hr, logstd, t);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, lrollout_act_kernel, genv, dim3(64), 0, s, a, z, logstd, t);
  hipLaunchKernelGGL(lrollout_partials_kernel, gpart, dim3(RB), 0, s, a, D, (t + 1) & 1, 1);
  return hip_check(hipGetLastError(), "mrl_rollout_act");
}

int mrl_rollout_act(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* z, const float* logstd,
                    const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!z) return fail(E_ARG, "null z rows");
  return rollout_act(d, head, n_out, z, HeadRows{nullptr, nullptr, nullptr, 0, 0, nullptr}, logstd, b, t, stream);
}

int mrl_rollout_act_head(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* hidden,
                         int32_t n_hidden, const float* w_head, const float* b_head, const float* logstd,
                         const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!d || !hidden || !w_head || !b_head || n_hidden <= 0) return fail(E_ARG, "mrl_rollout_act_head: bad arguments");
  if (d->env_id != MRL_ENV_HUMANOID || n_out != HM_ACT)
    return fail(E_UNSUPPORTED, "mrl_rollout_act_head: the fused head is the Humanoid step's (17 outputs)");
  return rollout_act(d, head, n_out, nullptr,
                     HeadRows{hidden, w_head, b_head, n_hidden, (int)(roll_compute(d) == MRL_COMPUTE_BF16), nullptr}, logstd,
                     b, t, stream);
}

int mrl_rollout_act_head_bf16(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const uint16_t* hidden16,
                              int32_t n_hidden, const float* w_head, const float* b_head, const float* logstd,
                              const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!d || !hidden16 || !w_head || !b_head || n_hidden <= 0)
    return fail(E_ARG, "mrl_rollout_act_head_bf16: bad arguments");
  if (d->env_id != MRL_ENV_HUMANOID || n_out != HM_ACT)
    return fail(E_UNSUPPORTED, "mrl_rollout_act_head_bf16: the fused head is the Humanoid step's (17 outputs)");
  if (roll_compute(d) != MRL_COMPUTE_BF16) return fail(E_ARG, "mrl_rollout_act_head_bf16: bf16 hidden rows need MRL_COMPUTE_BF16");
  return rollout_act(d, head, n_out, nullptr, HeadRows{nullptr, w_head, b_head, n_hidden, 1, hidden16}, logstd, b, t,
                     stream);
}

}  // extern "C"
#endif  // MRL_ROLLOUT_EVAL_UNIT
