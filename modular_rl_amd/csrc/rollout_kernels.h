// The fused 64-64 rollout's kernel templates: reset, one step per launch, and the persistent
// kernel (the whole horizon in one launch).  Per launch (step t) every block
//   1. merges the per-block Welford partials of the E raw observations of step t
//      (and rewards of step t-1) -- published by launch t-1 -- into the running
//      stat (every block derives the identical state; block 0 stores it; ping-pong
//      buffers by step parity),
//   2. normalises its envs' observations (x - mean)/(std + 1e-8), clip +-5, stores
//      them as the trajectory rows (fp32) and in LDS,
//   3. runs the policy MLP forward on MFMA (16 envs per wave, rollout_forward.h),
//   4. samples the action (Philox counter stream or injected noise),
//   5. steps the env (fp64), auto-resets finished episodes, writes reward/flags,
//   6. publishes the block's Welford partial of the new raw obs and the reward (rollout_stat.h).
// Kernels are templated on the env so every per-env array has a compile-time size
// (registers, no scratch).
//
// Two units instantiate these templates, and each module holds its own kernels alone:
// rollout.hip the training kernels (EV = false), rollout_eval.hip the evaluation ones
// (EV = true, MRL_ROLLOUT_EVAL; rollout_device.h) behind launch_rollout_*_eval.  Instantiated
// beside the training kernels, the EV kernels changed a training kernel's listing (Swimmer's
// step kernel, a loop branch in its other sense: the envs' step functions gain callers in the
// module).  The same holds for rollout_layered_kernels.h and its two units.
#pragma once
#include "rollout_forward.h"
#include "rollout_stat.h"

namespace mrl {

// EV (here and in the two kernels below): the evaluation instantiation -- the envs' reset
// alone, no partial of obs_0
template <int ENV, bool EV = false>
__global__ __launch_bounds__(RB) void rollout_reset_kernel(RollArgs a) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, D = O + 1;
  static_assert(D <= 2 * COLS, "two column passes");
  const int E = a.d.n_envs;
  const int le = threadIdx.x;
  const int e = blockIdx.x * ENVS_PER_BLOCK + le;
  if constexpr (EV) {
    if (le < ENVS_PER_BLOCK && e < E) {
      double s[EC::NS];
      reset_env<ENV>(a, e, s);
#pragma unroll
      for (int i = 0; i < EC::NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
    }
    return;
  }
  __shared__ double vals[ENVS_PER_BLOCK * col_slots(D)];
  if (le < ENVS_PER_BLOCK && e < E) {
    double s[EC::NS], o[O];
    reset_env<ENV>(a, e, s);
#pragma unroll
    for (int i = 0; i < EC::NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
    EC::obs(s, o);
#pragma unroll
    for (int k = 0; k < O; ++k) vals[le * D + k] = o[k];
    vals[le * D + O] = 0.0;
  }
  __syncthreads();
  const int nvalid = min(ENVS_PER_BLOCK, E - (int)blockIdx.x * ENVS_PER_BLOCK);
  publish_partial(a, vals, nvalid, D, false, a.b.records);
  if constexpr (D > COLS) publish_partial<COLS>(a, vals, nvalid, D, false, a.b.records);
}

// One launch = step t of E envs: 4 waves x 16 envs per block, the four 16-lane rows of
// a wave share the wave's 16 envs (split angle functions / noise / obs columns, the
// MFMA tiles of forward16).
template <int ENV, bool BF, bool EV = false>
__global__ __launch_bounds__(RB) void rollout_step_kernel(RollArgs a, const float* __restrict__ logstd,
                                                          const float* __restrict__ rimg, int t) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, D = O + 1, NS = EC::NS, A = EC::ACT;
  static_assert(D <= 2 * COLS, "two column passes");
  __shared__ double vals[EV ? 1 : ENVS_PER_BLOCK * col_slots(D)];
  __shared__ double fmean[col_slots(D)], fden[col_slots(D)];
  __shared__ float xt[4][16][MAX_IN + 1];  // +1: conflict-free column reads
  // diagnostic phase stamps (100 MHz realtime) of block 0 / thread 0 -- never set in production
#define STAMP(k)                                                                    \
  do {                                                                              \
    if (a.b.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0)               \
      a.b.stamps[(int64_t)t * 16 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); \
  } while (0)
  STAMP(0);
  if (a.b.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0)  // shader clock, for the in-kernel GHz
    a.b.stamps[(int64_t)t * 16 + 14] = (int64_t)__builtin_amdgcn_s_memtime();
  const int E = a.d.n_envs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int le = wave * 16 + j;
  const int e = blockIdx.x * ENVS_PER_BLOCK + le;
  const bool valid = e < E;
  const int64_t row = (int64_t)t * E + e;

  // 0. every global load of the step up front, in the order they are consumed (the
  //    vector-memory counter retires in order): filter records, env state, noise
  //    rows, policy weights
  const double* fs_in = a.b.filter_state + (t & 1) * a.FS;
  double* fs_out = a.b.filter_state + ((t + 1) & 1) * a.FS;
  const double* rec_in = a.b.records + (int64_t)(t & 1) * a.nb * a.RS;
  double* rec_out = a.b.records + (int64_t)((t + 1) & 1) * a.nb * a.RS;
  const int k = threadIdx.x >> 4, jj = threadIdx.x & 15;
  const bool kcol = k < D, isr = (k == O), one_round = a.nb <= 16 * RB_MAX;
  RecRound rr;
  double fn = 0.0, fM = 0.0, fS = 0.0;
  if constexpr (EV) {
    // the frozen filter: thread c < O takes column c's mean and denominator (in fM, fS) from
    // the state, which stays as it is -- no record is read, the 16-lane column groups have
    // nothing to do
    if ((int)threadIdx.x < O) frozen_filter_column(a.b.filter_state, D, threadIdx.x, fM, fS);
  } else if (kcol) {
    if (one_round) rr.load(rec_in, a.nb, a.RS, D, O, k, jj, 0);
    fn = fs_in[isr ? 1 : 0];
    fM = fs_in[2 + k];
    fS = fs_in[2 + D + k];
  }
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = valid ? a.b.env_state[(int64_t)i * E + e] : 0.0;
  double zn[A + 1] = {};
  if constexpr (!EV)
    if (valid) load_noise<ENV>(a, row, zn);
  RollWeights<O, A, BF> wt;
  wt.load(rimg, lane);
  __shared__ bf16x8 w1s_l[BF ? 1 : 3 * 8 * 64];  // fp32 mode: the split W1 fragments (24 KB)
  if constexpr (!BF) {
    constexpr RDims R = rollout_dims(O);
    for (int i = threadIdx.x; i < 3 * 8 * 64; i += RB) w1s_l[i] = reinterpret_cast<const bf16x8*>(rimg + R.bs1)[i];
    wt.w1s = w1s_l;
  }
  float lsd[A];
#pragma unroll
  for (int q = 0; q < A; ++q) lsd[q] = EC::DISCRETE ? 0.f : logstd[q];
  STAMP(1);

  // 2. running-stat merge (filters.py:30-31 push, per step over all envs): the block
  //    partials -> one batch -> one Chan merge; every block derives the same state
  if constexpr (EV) {
    if ((int)threadIdx.x < O) {
      fmean[threadIdx.x] = fM;
      fden[threadIdx.x] = fS;
    }
  } else if (kcol) {
    double bn, bm, bs;
    if (one_round) rr.batch(bn, bm, bs);
    else batch_of_records(rec_in, a.nb, a.RS, D, O, k, jj, bn, bm, bs);
    chan_merge(fn, fM, fS, bn, bm, bs);
    if (jj == 0 && blockIdx.x == 0) store_filter_column(fs_out, D, k, fn, fM, fS);
    if (!isr && jj == 0) filter_column(fn, fM, fS, fmean[k], fden[k]);
  }
  if constexpr (D > COLS && !EV) {  // the columns past the 16 thread groups: a second pass by the first groups
    const int k2 = k + COLS;
    if (k2 < D) {
      const bool isr2 = (k2 == O);
      double fn2 = fs_in[isr2 ? 1 : 0], fM2 = fs_in[2 + k2], fS2 = fs_in[2 + D + k2];
      double bn, bm, bs;
      batch_of_records(rec_in, a.nb, a.RS, D, O, k2, jj, bn, bm, bs);
      chan_merge(fn2, fM2, fS2, bn, bm, bs);
      if (jj == 0 && blockIdx.x == 0) store_filter_column(fs_out, D, k2, fn2, fM2, fS2);
      if (!isr2 && jj == 0) filter_column(fn2, fM2, fS2, fmean[k2], fden[k2]);
    }
  }
  __syncthreads();
  STAMP(2);

  // 3. filtered observation (core.py:191-192); row g takes columns 4i + g
  {
    float vf[(O + 3) / 4];
    filtered_obs<ENV>(s, g, a.d.filter != 0, fmean, fden, vf);
#pragma unroll
    for (int i = 0; i < (O + 3) / 4; ++i) {
      const int kc = 4 * i + g;
      if (kc < O) {
        if (valid) a.b.obs[row * O + kc] = vf[i];
        xt[wave][j][kc] = vf[i];
      }
    }
  }
  WAVE_LDS_ORDER();
  STAMP(3);

  // 4. policy forward (MFMA, 16 envs per wave)
  const XRow<O> xl{&xt[wave][j][0], valid};
  float z[A];
  forward16<O, A, BF>(wt, xl, lane, z,
                  (a.b.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0) ? a.b.stamps + t * 16 : nullptr);
  STAMP(4);

  // 5. sample + env step: every row steps the env (split angle functions), row 0 stores
  double rew = 0.0;
  bool done = false;
  if constexpr (EV) {  // the head's mode; the bookkeeping below is the training step's, no partial follows
    mode_and_step<ENV, true>(a, row, z, lsd, s, rew, done, valid && g == 0, g);
    if (valid && g == 0) finish_env_step<ENV>(a, e, row, t, s, rew, done);
    return;
  }
  sample_and_step<ENV, true>(a, row, z, lsd, zn, s, rew, done, valid && g == 0, g);
  STAMP(5);
  if (valid && g == 0) {
    finish_env_step<ENV>(a, e, row, t, s, rew, done);
    // 6. raw next observation + reward into the block partial
    double o[O];
    EC::obs(s, o);
#pragma unroll
    for (int c = 0; c < O; ++c) vals[le * D + c] = o[c];
    vals[le * D + O] = rew;
  }
  __syncthreads();
  STAMP(6);
  const int nvalid = min(ENVS_PER_BLOCK, E - (int)blockIdx.x * ENVS_PER_BLOCK);
  publish_partial(a, vals, nvalid, D, true, rec_out);
  if constexpr (D > COLS) publish_partial<COLS>(a, vals, nvalid, D, true, rec_out);
  STAMP(7);
  if (a.b.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
    a.b.stamps[(int64_t)t * 16 + 15] = (int64_t)__builtin_amdgcn_s_memtime();
#undef STAMP
}

// initial state of env e's episode number epc (reset_env's Philox draw, domain 1).  Always
// inlined: as a call (the double pendulum's Box-Muller reset is past the inliner's size limit)
// the state it fills would live in scratch.
template <int ENV>
__device__ __attribute__((always_inline)) inline void episode_start_state(const RollArgs& a, int e, uint32_t epc, double* s) {
  const uint32_t gid = (uint32_t)(a.d.env_offset + e);
  double u[EnvC<ENV>::NU];
#pragma unroll
  for (int c = 0; c < EnvC<ENV>::NU / 2; ++c)
    philox_uniform2(a.d.seed, 1, gid, (uint64_t)epc, (uint32_t)c, u[2 * c], u[2 * c + 1]);
  EnvC<ENV>::reset(u, s);
}

// The persistent rollout (rollout_stat.h, the persistent hand-off).
// ST: the diagnostic build with phase stamps (launched only when bufs.stamps is set);
// production launches carry no stamp code, whose uniform pointers / offsets cost SGPRs
// that the compiler then spilled to VGPR lanes (a v_readlane per reload, every step).
// EV: the filter is frozen, so a step has no cross-block dependency left -- the episode
// bookkeeping is each env's own registers.  The evaluation instantiation therefore drops the
// hand-off whole (no granule is published or polled, `sync` is not touched, no block waits
// for another and the grid need not be resident) and with it both per-step barriers: fmean /
// fden are written once before the loop, and a wave reads only its own rows of xt.
template <int ENV, bool BF, bool ST, bool EV = false>
__global__ __launch_bounds__(RB) void rollout_persistent_kernel(RollArgs a, const float* __restrict__ logstd,
                                                                const float* __restrict__ rimg,
                                                                uint32_t* __restrict__ sync) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, D = O + 1, NS = EC::NS, A = EC::ACT;
  static_assert(D <= 2 * COLS, "two column passes");
  static_assert(!(EV && ST), "the phase stamps are the training launch's");
  __shared__ double vals[EV ? 1 : ENVS_PER_BLOCK * col_slots(D)];
  __shared__ double fmean[col_slots(D)], fden[col_slots(D)];
  __shared__ float xt[4][16][MAX_IN + 1];  // +1: conflict-free column reads
  __shared__ int s_fail;
  // HP_CAP: the capsule constants, one LDS read per constant per substep instead of a
  // select chain on the lane's row (rollout 14.30 -> 14.05 ms, profiles/r06d_ab.txt)
  __shared__ double hp_cap[24];
  const int E = a.d.n_envs, T = a.d.horizon, nb = a.nb;
  // diagnostic phase stamps (100 MHz realtime) of block 0 -- never set in production
#define PSTAMP(tt, k)                                                                  \
  do {                                                                                 \
    if (ST && threadIdx.x == 0 && blockIdx.x == 0)                                     \
      a.b.stamps[(int64_t)(tt) * 16 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); \
  } while (0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int le = wave * 16 + j;
  const int e = blockIdx.x * ENVS_PER_BLOCK + le;
  const bool valid = e < E;
  const int ec = valid ? e : E - 1;  // invalid lanes shadow a valid env, store nothing
  const int k = threadIdx.x >> 4, jj = threadIdx.x & 15;
  const bool kcol = !EV && k < D, isr = (k == O);  // EV: no column group has a column to merge
  const int nvalid = min(ENVS_PER_BLOCK, E - (int)blockIdx.x * ENVS_PER_BLOCK);
  const Granules gr(sync, nb, D);
  if (threadIdx.x == 0) s_fail = 0;
  if (threadIdx.x < 24) hp_cap[threadIdx.x] = HP_CAP[threadIdx.x];

  RollWeights<O, A, BF> wt;
  wt.load(rimg, lane);
  __shared__ bf16x8 w1s_l[BF ? 1 : 3 * 8 * 64];  // fp32 mode: the split W1 fragments (24 KB)
  if constexpr (!BF) {
    constexpr RDims R = rollout_dims(O);
    for (int i = threadIdx.x; i < 3 * 8 * 64; i += RB) w1s_l[i] = reinterpret_cast<const bf16x8*>(rimg + R.bs1)[i];
    wt.w1s = w1s_l;
  }
  float lsd[A], sdv[A];
#pragma unroll
  for (int q = 0; q < A; ++q) {
    lsd[q] = EC::DISCRETE ? 0.f : logstd[q];
    sdv[q] = expf(lsd[q]);
  }
  // the running stat at the start of the iteration (every block keeps the same copy)
  double fn = 0.0, fM = 0.0, fS = 0.0;
  if constexpr (EV) {
    // the frozen filter, for all T steps: thread c < O writes column c's mean and denominator
    // (the barrier after the reset below publishes them); the column groups do nothing
    if ((int)threadIdx.x < O) {
      frozen_filter_column(a.b.filter_state, D, threadIdx.x, fM, fS);
      fmean[threadIdx.x] = fM;
      fden[threadIdx.x] = fS;
    }
  } else if (kcol) {
    fn = a.b.filter_state[isr ? 1 : 0];
    fM = a.b.filter_state[2 + k];
    fS = a.b.filter_state[2 + D + k];
  }
  // the columns past the 16 thread groups (D > COLS): a second pass by the first groups
  const int k2 = k + COLS;
  const bool kcol2 = !EV && D > COLS && k2 < D, isr2 = (k2 == O);
  double fn2 = 0.0, fM2 = 0.0, fS2 = 0.0;
  if constexpr (D > COLS && !EV) {
    if (kcol2) {
      fn2 = a.b.filter_state[isr2 ? 1 : 0];
      fM2 = a.b.filter_state[2 + k2];
      fS2 = a.b.filter_state[2 + D + k2];
    }
  }
  // reset every env (core.py:186); all four rows of a wave hold the same env.  sn is
  // the start state of the env's NEXT episode, drawn ahead so an auto-reset is a copy:
  // its Philox draw runs behind the step's publish, under the hand-off latency.
  double s[NS], sn[NS];
  uint32_t epc = (uint32_t)a.b.env_int[E + ec];
  int ept = 0;
  episode_start_state<ENV>(a, ec, epc, s);
  epc += 1u;
  episode_start_state<ENV>(a, ec, epc, sn);
  bool refill = false;
  if constexpr (!EV) {
    if (valid && g == 0) {
      double o[O];
      EC::obs(s, o);
#pragma unroll
      for (int c = 0; c < O; ++c) vals[le * D + c] = o[c];
      vals[le * D + O] = 0.0;
    }
  }
  __syncthreads();
  if constexpr (!EV) {
    publish_granules(gr, vals, nvalid, 0);  // gather step 0's partials
    if constexpr (D > COLS) publish_granules<COLS>(gr, vals, nvalid, 0);
  }
  double capr[6];  // row g's capsule constants
#pragma unroll
  for (int f = 0; f < 6; ++f) capr[f] = hp_cap[4 * f + g];

  for (int t = 0; t < T; ++t) {
    const int64_t row = (int64_t)t * E + e;
    PSTAMP(t, 0);
    if (ST && threadIdx.x == 0 && blockIdx.x == 0)  // shader clock beside the 100 MHz one (in-kernel GHz)
      a.b.stamps[(int64_t)t * 16 + 9] = (int64_t)__builtin_amdgcn_s_memtime();
    double zn[A + 1] = {};
    if constexpr (!EV) load_noise<ENV>(a, (int64_t)t * E + ec, zn);  // independent of the hand-off: issued first
    // the next episode's start state of envs that auto-reset at step t-1: off the step's
    // critical path, under the first poll of the hand-off (or beside it, non-polling waves)
    auto refill_next = [&]() {
      if (refill) {
        episode_start_state<ENV>(a, ec, epc, sn);
        refill = false;
      }
    };
    // running-stat merge of step t's batch (filters.py:30-31), identical in every block
    if (!kcol) refill_next();  // kcol is wave-uniform: waves that do not poll
    if (kcol) {
      double bn, bm, bs;
      RecRound rr;
      bool ok = true;
      if (nb <= 16 * RB_SMALL) {
        RecRoundT<RB_SMALL> r4;
        ok = gather_granules(gr, r4, t, k, jj, 0, E, t > 0, sync, refill_next);
        PSTAMP(t, 7);
        r4.batch(bn, bm, bs);
      } else if (nb <= 16 * RB_MAX) {
        ok = gather_granules(gr, rr, t, k, jj, 0, E, t > 0, sync, refill_next);
        PSTAMP(t, 7);
        rr.batch(bn, bm, bs);
      } else {
        double n = 0.0, sm = 0.0, raw = 0.0;
        for (int b0 = 0; b0 < nb && ok; b0 += 16 * RB_MAX) {
          ok = gather_granules(gr, rr, t, k, jj, b0, E, t > 0, sync, refill_next);
          rr.accumulate(n, sm, raw);
        }
        n = sum16(n);
        sm = sum16(sm);
        bm = n > 0.0 ? div_count(sm, n) : 0.0;
        bn = n;
        bs = sum16(raw) - n * bm * bm;
      }
      if (!ok) s_fail = 1;
      chan_merge(fn, fM, fS, bn, bm, bs);
      // the filter_column and store_filter_column lines are written out in this kernel: as
      // calls they changed HalfCheetah's listings
      if (!isr && jj == 0) {
        const double var = fn > 1.0 ? fS / (fn - 1.0) : fM * fM;  // running_stat.py:27
        fmean[k] = fM;
        fden[k] = sqrt(var) + 1e-8;
      }
    }
    if constexpr (D > COLS && !EV) {
      // kcol2 is uniform in a 16-lane group, not in a wave (it holds for half of wave 0), and so
      // is kcol where D is no multiple of 4: everything below works per 16-lane group
      if (kcol2) {
        double bn, bm, bs;
        RecRound rr;
        bool ok = true;
        if (nb <= 16 * RB_MAX) {
          ok = gather_granules(gr, rr, t, k2, jj, 0, E, t > 0, sync, refill_next);
          rr.batch(bn, bm, bs);
        } else {
          double n = 0.0, sm = 0.0, raw = 0.0;
          for (int b0 = 0; b0 < nb && ok; b0 += 16 * RB_MAX) {
            ok = gather_granules(gr, rr, t, k2, jj, b0, E, t > 0, sync, refill_next);
            rr.accumulate(n, sm, raw);
          }
          n = sum16(n);
          sm = sum16(sm);
          bm = n > 0.0 ? div_count(sm, n) : 0.0;
          bn = n;
          bs = sum16(raw) - n * bm * bm;
        }
        if (!ok) s_fail = 1;
        chan_merge(fn2, fM2, fS2, bn, bm, bs);
        if (!isr2 && jj == 0) {
          const double var = fn2 > 1.0 ? fS2 / (fn2 - 1.0) : fM2 * fM2;
          fmean[k2] = fM2;
          fden[k2] = sqrt(var) + 1e-8;
        }
      }
    }
    PSTAMP(t, 8);
    if constexpr (!EV) {
      __syncthreads();
      if (s_fail) break;  // uniform: a block that gave up leaves the loop whole
    }
    PSTAMP(t, 1);
    // filtered observation (core.py:191-192); row g takes columns 4i + g
    {
      float vf[(O + 3) / 4];
      filtered_obs<ENV>(s, g, a.d.filter != 0, fmean, fden, vf);
#pragma unroll
      for (int i = 0; i < (O + 3) / 4; ++i) {
        const int kc = 4 * i + g;
        if (kc < O) {
          if (valid) a.b.obs[row * O + kc] = vf[i];
          xt[wave][j][kc] = vf[i];
        }
      }
    }
    WAVE_LDS_ORDER();
    PSTAMP(t, 2);
    const XRow<O> xl{&xt[wave][j][0], valid};
    float z[A];
    forward16<O, A, BF>(wt, xl, lane, z);
    PSTAMP(t, 3);
    // sample + env step on every row (split angle functions); row 0 stores
    double rew = 0.0;
    bool done = false;
    if constexpr (EV) mode_and_step<ENV, true, true>(a, row, z, sdv, s, rew, done, valid && g == 0, g, capr);
    else sample_and_step<ENV, true, true>(a, row, z, sdv, zn, s, rew, done, valid && g == 0, g, capr);
    PSTAMP(t, 4);
    // episode bookkeeping on every row, so the rows keep identical env state
    // (finish_env_step: gym TimeLimit => terminated; limit / horizon cut => not)
    {
      const bool term = done || (ept + 1 >= EC::MAX_STEPS);
      const bool last = term || (ept + 1 >= a.d.timestep_limit) || (t == T - 1);
      if (valid && g == 0) {
        a.b.ep_t[row] = ept;
        a.b.rew[row] = (float)rew;
        a.b.flags[row] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
      }
      if (last && t < T - 1) {
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] = sn[i];
        epc += 1u;
        ept = 0;
        refill = true;
      } else {
        ept += 1;
      }
    }
    if constexpr (EV) continue;  // nothing to hand on
    if (valid && g == 0) {
      double o[O];
      EC::obs(s, o);
#pragma unroll
      for (int c = 0; c < O; ++c) vals[le * D + c] = o[c];
      vals[le * D + O] = rew;
    }
    __syncthreads();
    PSTAMP(t, 5);
    if (t + 1 < T) publish_granules(gr, vals, nvalid, t + 1);
    else publish_partial(a, vals, nvalid, D, true, a.b.records + (int64_t)(T & 1) * nb * a.RS);  // for finish
    if constexpr (D > COLS) {
      if (t + 1 < T) publish_granules<COLS>(gr, vals, nvalid, t + 1);
      else publish_partial<COLS>(a, vals, nvalid, D, true, a.b.records + (int64_t)(T & 1) * nb * a.RS);
    }
    PSTAMP(t, 6);
  }
#undef PSTAMP
  // state for the next iteration and the finish kernel: env state / counters, and the
  // running stat where the step kernels leave it (parity T)
  if (valid && g == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
    a.b.env_int[e] = ept;
    a.b.env_int[E + e] = (int32_t)epc;
  }
  if constexpr (EV) return;  // the filter state stays as it was
  if (blockIdx.x == 0 && kcol && jj == 0) {
    double* fs_out = a.b.filter_state + (T & 1) * a.FS;
    if (k == 0) fs_out[0] = fn;
    if (isr) fs_out[1] = fn;
    fs_out[2 + k] = fM;
    fs_out[2 + D + k] = fS;
  }
  if constexpr (D > COLS) {
    if (blockIdx.x == 0 && kcol2 && jj == 0) {
      double* fs_out = a.b.filter_state + (T & 1) * a.FS;
      if (isr2) fs_out[1] = fn2;
      fs_out[2 + k2] = fM2;
      fs_out[2 + D + k2] = fS2;
    }
  }
}

}  // namespace mrl
