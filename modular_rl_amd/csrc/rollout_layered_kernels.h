// The layered rollout's kernel templates: the thread-per-env reset, obs and act kernels
// (lrollout_*) and Humanoid's wave-per-env reset and step (hm_reset_kernel, hm_act_kernel, with
// the policy head fused into the step).  rollout_layered.hip instantiates the training kernels,
// rollout_layered_eval.hip the evaluation ones (EV = true): a module each, by the rule at the
// top of rollout_kernels.h.
#pragma once
#include "rollout_device.h"

namespace mrl {

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
    if (blockIdx.x == 0) store_filter_column(fs_out, D, k, n, M, S);
    filter_column(n, M, S, fmean[threadIdx.x], fden[threadIdx.x]);
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
      av = mul_then_add((float)zn, sd, z);
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

}  // namespace mrl
