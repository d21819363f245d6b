// Batched lock-step rollout: E envs per GPU advance one step per launch.
//
// Replaces the reference's serial per-step loop (core.py:182-221):
//     ob = agent.obfilt(ob)                 ZFilter, filters.py:30-38
//     action, {"prob"} = agent.act(ob)      StochPolicy.act, core.py:261-267
//     ob, rew, done, _ = env.step(action)   gym
//     agent.rewfilt(rew)                    stats only, core.py:198-199
// Per launch (step t) every block
//   1. merges the per-block Welford partials of the E raw observations of step t
//      (and rewards of step t-1) -- published by launch t-1 -- into the running
//      stat (every block derives the identical state; block 0 stores it; ping-pong
//      buffers by step parity),
//   2. normalises its envs' observations (x - mean)/(std + 1e-8), clip +-5, stores
//      them as the trajectory rows (fp32) and in LDS,
//   3. runs the policy MLP forward on MFMA (32 envs per wave, image in LDS),
//   4. samples the action (Philox counter stream or injected noise),
//   5. steps the env (fp64), auto-resets finished episodes, writes reward/flags,
//   6. publishes the block's Welford partial of the new raw obs and the reward.
// Kernels are templated on the env so every per-env array has a compile-time size
// (registers, no scratch).
//
// This unit is the fused 64-64 path: the step kernel above, the persistent kernel (the whole
// horizon in one launch, below), the noise fill, image pack, reset and finish kernels and
// their C entry points.  The layered path is rollout_layered.hip, the stand-alone env stepper
// and obs filter env_api.hip, the population rollout cem.hip; what the units share is
// rollout_device.h (device code) and rollout_host.h (checks, dispatch).
#include "rollout_host.h"

namespace mrl {

// ------------------------------------------------------------------ rollout policy forward
// One wave = 16 envs on v_mfma_f32_16x16x4_f32 (mlp_layout.h, rollout image): the
// step kernel is a latency chain at one wave per SIMD, and 16-row tiles halve both
// the MFMA chain and the tanh work of a 32-row tile.  The weight fragments of the
// wave go straight from global memory (L2-resident rollout image) into registers,
// loaded at kernel entry so their latency hides under the filter merge.
template <int O, int A>
struct RWeights {
  static constexpr RDims R = rollout_dims(O);
  float4 a0[4][R.KS0p / 4];
  const bf16x8* w1s = nullptr;  // the split W1 fragments (image section bs1), staged in LDS
  float4 b0[4], b1[4];
  float4 hv[A][4];
  float hb[A];
  __device__ void load(const float* __restrict__ img, int lane) {
    const int g = lane >> 4;
    const float4* f = reinterpret_cast<const float4*>(img);
#pragma unroll
    for (int mo = 0; mo < 4; ++mo)
#pragma unroll
      for (int s4 = 0; s4 < R.KS0p / 4; ++s4) a0[mo][s4] = f[(R.a0 >> 2) + (mo * (R.KS0p / 4) + s4) * 64 + lane];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      b0[mt] = f[(R.b0 >> 2) + g * 4 + mt];
      b1[mt] = f[(R.b1 >> 2) + g * 4 + mt];
    }
#pragma unroll
    for (int o = 0; o < A; ++o)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) hv[o][mt] = f[(R.hv >> 2) + (g * MAX_OUT + o) * 4 + mt];
#pragma unroll
    for (int o = 0; o < A; ++o) hb[o] = img[R.hb + o];
  }
};

// bf16 compute mode: layer-0 / layer-1 fragments of v_mfma_f32_16x16x32_bf16 (image
// segments ba0 / ba1), biases and the VALU head as in RWeights
template <int O, int A>
struct RWeightsB {
  static constexpr RDims R = rollout_dims(O);
  bf16x8 a0[4];
  bf16x8 a1[4][2];
  float4 b0[4], b1[4];
  float4 hv[A][4];
  float hb[A];
  __device__ void load(const float* __restrict__ img, int lane) {
    const int g = lane >> 4;
    const bf16x8* f0 = reinterpret_cast<const bf16x8*>(img + R.ba0);
    const bf16x8* f1 = reinterpret_cast<const bf16x8*>(img + R.ba1);
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) {
      a0[mo] = f0[mo * 64 + lane];
#pragma unroll
      for (int p = 0; p < 2; ++p) a1[mo][p] = f1[(mo * 2 + p) * 64 + lane];
    }
    const float4* f = reinterpret_cast<const float4*>(img);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      b0[mt] = f[(R.b0 >> 2) + g * 4 + mt];
      b1[mt] = f[(R.b1 >> 2) + g * 4 + mt];
    }
#pragma unroll
    for (int o = 0; o < A; ++o)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) hv[o][mt] = f[(R.hv >> 2) + (g * MAX_OUT + o) * 4 + mt];
#pragma unroll
    for (int o = 0; o < A; ++o) hb[o] = img[R.hb + o];
  }
};

template <int O, int A, bool BF>
using RollWeights = typename std::conditional<BF, RWeightsB<O, A>, RWeights<O, A>>::type;

__device__ inline f32x4 as_f32x4(float4 v) {
  f32x4 r;
  r[0] = v.x;
  r[1] = v.y;
  r[2] = v.z;
  r[3] = v.w;
  return r;
}

__device__ inline void tanh4(f32x4& a) {
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = tanh_fast(a[r]);
}

template <bool BF>
__device__ inline void tanh4r(f32x4& a) {
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    const f32x2 t = tanh_fast2(f32x2{a[r], a[r + 1]});
    a[r] = BF ? bf16r(t.x) : t.x;
    a[r + 1] = BF ? bf16r(t.y) : t.y;
  }
}

// head rows z[o] of the wave's 16 envs (every lane of an env's column ends with all A).
// BF (MRL_COMPUTE_BF16): x, h1, h2 rounded to bf16 (W0, W1 are rounded in the image),
// the operands mlp_rows_bf16 multiplies -- the products and sums stay f32, so the prob
// rows equal the update's bf16 forward up to f32 summation order.
template <int O, int A, bool BF, class XL>
__device__ inline void forward16(const RWeights<O, A>& w, const XL& xl, int lane, float* z, int64_t* st = nullptr) {
  constexpr RDims R = RWeights<O, A>::R;
  const int g = lane >> 4;
  // the split W1 fragments of k-step s, [tile mo][part p]: k-step 0's issued before layer 0,
  // k-step 1's once k-step 0's MFMAs are issued -- each lands under other work instead of
  // an LDS round trip in front of every MFMA group (the persistent kernel's registers are
  // held by the fp64 dynamics, not here)
  bf16x8 wf[4][3];
  auto load_wf = [&](int s) {
#pragma unroll
    for (int mo = 0; mo < 4; ++mo)
#pragma unroll
      for (int p = 0; p < 3; ++p) wf[mo][p] = w.w1s[(p * 8 + mo * 2 + s) * 64 + lane];
  };
  load_wf(0);
  float xb[R.KS0p];
#pragma unroll
  for (int ks = 0; ks < R.KS0p; ++ks) xb[ks] = ks < R.KS0 ? (BF ? bf16r(xl(4 * ks + g)) : xl(4 * ks + g)) : 0.f;
  f32x4 h1[4], h2[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    h1[m] = as_f32x4(w.b0[m]);
    h2[m] = as_f32x4(w.b1[m]);
  }
  // layer 0: four independent 16-unit accumulators
#pragma unroll
  for (int ks = 0; ks < R.KS0; ++ks)
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) h1[mo] = MFMA16(f4get(w.a0[mo][ks >> 2], ks & 3), xb[ks], h1[mo]);
  if (st != nullptr) st[9] = (int64_t)__builtin_amdgcn_s_memrealtime();
  // layer 1 on split operands (fp32-accurate: h1 and W1 split exactly into three bf16
  // parts, six part products on v_mfma_f32_16x16x32_bf16, f32 accumulation): k-step s
  // covers tiles 2s, 2s+1 -- the lane's own registers, unit rb_unit(s, g, e) for element e
  // -- against the W1 fragments the rollout image holds split (section bs1)
  tanh4r<BF>(h1[0]);
  tanh4r<BF>(h1[1]);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 hp[3];
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      bf16x2 a, c, e, a2, c2, e2;
      split2(f32x2{h1[2 * s][r], h1[2 * s][r + 1]}, a, c, e);
      split2(f32x2{h1[2 * s + 1][r], h1[2 * s + 1][r + 1]}, a2, c2, e2);
      hp[0][r] = a[0]; hp[0][r + 1] = a[1]; hp[0][4 + r] = a2[0]; hp[0][4 + r + 1] = a2[1];
      hp[1][r] = c[0]; hp[1][r + 1] = c[1]; hp[1][4 + r] = c2[0]; hp[1][4 + r + 1] = c2[1];
      hp[2][r] = e[0]; hp[2][r + 1] = e[1]; hp[2][4 + r] = e2[0]; hp[2][4 + r + 1] = e2[1];
    }
    bf16x8 wc[4][3];
#pragma unroll
    for (int mo = 0; mo < 4; ++mo)
#pragma unroll
      for (int p = 0; p < 3; ++p) wc[mo][p] = wf[mo][p];
    if (s == 0) load_wf(1);
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) {
      const bf16x8 w0 = wc[mo][0], w1 = wc[mo][1], w2 = wc[mo][2];
      h2[mo] = MFMAB16(w2, hp[0], h2[mo]);  // smallest products first
      h2[mo] = MFMAB16(w0, hp[2], h2[mo]);
      h2[mo] = MFMAB16(w1, hp[1], h2[mo]);
      h2[mo] = MFMAB16(w1, hp[0], h2[mo]);
      h2[mo] = MFMAB16(w0, hp[1], h2[mo]);
      h2[mo] = MFMAB16(w0, hp[0], h2[mo]);
    }
    if (s == 0) {  // the second k-step's activations, under the first one's MFMAs
      tanh4r<BF>(h1[2]);
      tanh4r<BF>(h1[3]);
    }
  }
  if (st != nullptr) st[10] = (int64_t)__builtin_amdgcn_s_memrealtime();
  // tanh + head of output tile mo (head on VALU: 16 units per lane, then the column's 4 rows)
  float acc[A];
#pragma unroll
  for (int o = 0; o < A; ++o) acc[o] = 0.f;
#pragma unroll
  for (int mo = 0; mo < 4; ++mo) {
    tanh4r<BF>(h2[mo]);
#pragma unroll
    for (int o = 0; o < A; ++o) {
      const float4 hv = w.hv[o][mo];
      acc[o] += hv.x * h2[mo][0] + hv.y * h2[mo][1] + hv.z * h2[mo][2] + hv.w * h2[mo][3];
    }
  }
#pragma unroll
  for (int o = 0; o < A; ++o) z[o] = quad_sum(acc[o]) + w.hb[o];
}

// bf16 compute mode on v_mfma_f32_16x16x32_bf16: one k-step covers the inputs, two
// the 64 hidden units (8 MFMAs for layer 1 instead of 64 f32 16x16x4), same rounding
// points as forward16<BF = true> and mlp_rows_bf16.
template <int O, int A, bool BF, class XL>
__device__ inline void forward16(const RWeightsB<O, A>& w, const XL& xl, int lane, float* z, int64_t* st = nullptr) {
  const int g = lane >> 4;
  bf16x8 xb;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) xb[jj] = (__bf16)xl(8 * g + jj);
  f32x4 h1[4], h2[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    h1[m] = as_f32x4(w.b0[m]);
    h2[m] = as_f32x4(w.b1[m]);
  }
#pragma unroll
  for (int mo = 0; mo < 4; ++mo) h1[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w.a0[mo], xb, h1[mo], 0, 0, 0);
  if (st != nullptr) st[9] = (int64_t)__builtin_amdgcn_s_memrealtime();
  // B fragment of k-step p: tanh(h1) of tiles 2p (elements 0..3) and 2p+1 (4..7)
  bf16x8 hb[2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const f32x2 ta = tanh_fast2(f32x2{h1[2 * p][r], h1[2 * p][r + 1]});
      const f32x2 tb = tanh_fast2(f32x2{h1[2 * p + 1][r], h1[2 * p + 1][r + 1]});
      hb[p][r] = (__bf16)ta.x;
      hb[p][r + 1] = (__bf16)ta.y;
      hb[p][4 + r] = (__bf16)tb.x;
      hb[p][4 + r + 1] = (__bf16)tb.y;
    }
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) h2[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w.a1[mo][p], hb[p], h2[mo], 0, 0, 0);
  if (st != nullptr) st[10] = (int64_t)__builtin_amdgcn_s_memrealtime();
  float acc[A];
#pragma unroll
  for (int o = 0; o < A; ++o) acc[o] = 0.f;
#pragma unroll
  for (int mo = 0; mo < 4; ++mo) {
    tanh4r<true>(h2[mo]);
#pragma unroll
    for (int o = 0; o < A; ++o) {
      const float4 hv = w.hv[o][mo];
      acc[o] += hv.x * h2[mo][0] + hv.y * h2[mo][1] + hv.z * h2[mo][2] + hv.w * h2[mo][3];
    }
  }
#pragma unroll
  for (int o = 0; o < A; ++o) z[o] = quad_sum(acc[o]) + w.hb[o];
}

// per-block two-pass (mean, M2) partial of vals[ENVS_PER_BLOCK][D] (doubles in LDS):
// thread (k = tid/16, j = tid%16) covers envs j, j+16, ...; 16-lane butterflies.
// column k's (mean, M2) over the block's nvalid envs: lane j adds envs j, j + 16, j + 32,
// j + 48 in that order, then the 16-lane butterflies.  The four values are read from LDS
// together and kept for the M2 pass (one LDS round trip instead of eight dependent ones);
// a term past nvalid is skipped, as the loop over i < nvalid did
__device__ inline void block_moments(const double* vals, int nvalid, int D, int k, int j, double& mean, double& m2) {
  constexpr int Q = ENVS_PER_BLOCK / 16;
  const int kk = k < D ? k : D - 1;
  double v[Q];
  bool in[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = j + 16 * q;
    in[q] = k < D && i < nvalid;
    v[q] = vals[(i < nvalid ? i : 0) * D + kk];
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (in[q]) s += v[q];
  mean = nvalid > 0 ? div_count(sum16(s), (double)nvalid) : 0.0;
  double m = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (in[q]) {
      const double dv = v[q] - mean;
      m += dv * dv;
    }
  m2 = sum16(m);
}

// The 16 thread groups take columns K0 .. K0 + 15.  An env with more than COLS columns
// (HalfCheetah: 17 obs + the reward) makes a second pass with K0 = COLS, whose first groups
// take columns 16 .. D - 1 (the counts r[0], r[1] are column 0's, so the first pass's).
// K0 is a template argument: as a function argument, even one that is 0 everywhere, it
// changed the address arithmetic of every existing kernel.
constexpr int COLS = RB / 16;
constexpr int col_slots(int D) { return D > MAXD ? D : MAXD; }
template <int K0 = 0>
__device__ inline void publish_partial(const RollArgs& a, const double* vals, int nvalid, int D, bool with_rew,
                                       double* rec_out) {
  const int k = K0 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  double mean, m2;
  block_moments(vals, nvalid, D, k, j, mean, m2);
  if (k < D && j == 0) {
    double* r = rec_out + (int64_t)blockIdx.x * a.RS;
    r[2 + k] = mean;
    r[2 + D + k] = m2;
    if (k == 0) {
      r[0] = (double)nvalid;
      r[1] = with_rew ? (double)nvalid : 0.0;
    }
  }
}

// combine the per-block records of one column k into a batch (n, mean, M2):
// mean = sum n_b mean_b / n ; M2 = sum (M2_b + n_b (mean_b - mean)^2).
// Called by all 16 lanes of thread group k; every lane returns the same values.
// Lane j holds records j + 16q of a round (RB_MAX per lane, 128 blocks = 8192 envs).
constexpr int RB_MAX = 8;
template <int R>
struct RecRoundT {
  double rn[R], rm[R], rs[R];
  __device__ void load(const double* rec, int nb, int RS, int D, int O, int k, int j, int b0) {
    const bool isr = (k == O);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int b = b0 + j + 16 * q;
      const double* r = rec + (int64_t)(b < nb ? b : 0) * RS;
      rn[q] = b < nb ? r[isr ? 1 : 0] : 0.0;
      rm[q] = b < nb ? r[2 + k] : 0.0;
      rs[q] = b < nb ? r[2 + D + k] : 0.0;
    }
  }
  __device__ void accumulate(double& n, double& sm, double& raw) const {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      n += rn[q];
      sm += rn[q] * rm[q];
      raw += rs[q] + rn[q] * rm[q] * rm[q];
    }
  }
  // one-round batch (nb <= 16 * R): exact two-pass form from registers
  __device__ void batch(double& bn, double& bm, double& bs) const {
    double n = 0.0, sm = 0.0, raw = 0.0;
    accumulate(n, sm, raw);
    n = sum16(n);
    sm = sum16(sm);
    const double mean = n > 0.0 ? div_count(sm, n) : 0.0;
    double m2 = 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (rn[q] > 0.0) {
        const double dm = rm[q] - mean;
        m2 += rs[q] + rn[q] * dm * dm;
      }
    bn = n;
    bm = mean;
    bs = sum16(m2);
  }
};

using RecRound = RecRoundT<RB_MAX>;
// persistent rollout: 16 * RB_SMALL blocks (<= 4096 envs) gather in half the registers
constexpr int RB_SMALL = 4;

__device__ inline void batch_of_records(const double* rec, int nb, int RS, int D, int O, int k, int j, double& bn,
                                        double& bm, double& bs) {
  RecRound rr;
  if (nb <= 16 * RB_MAX) {
    rr.load(rec, nb, RS, D, O, k, j, 0);
    rr.batch(bn, bm, bs);
    return;
  }
  // many rounds: sum (M2_b + n_b mean_b^2) - n mean^2
  double n = 0.0, sm = 0.0, raw = 0.0;
  for (int b0 = 0; b0 < nb; b0 += 16 * RB_MAX) {
    rr.load(rec, nb, RS, D, O, k, j, b0);
    rr.accumulate(n, sm, raw);
  }
  n = sum16(n);
  sm = sum16(sm);
  const double mean = n > 0.0 ? div_count(sm, n) : 0.0;
  bn = n;
  bm = mean;
  bs = sum16(raw) - n * mean * mean;
}

// the filtered observation columns 4i + g of one env row (core.py:191-192: clip((o - mean)
// / (std + 1e-8), -5, 5)), as f32.  Every column's statistics are read from LDS before any
// arithmetic and the stores are left to the caller, so the (O + 3) / 4 divisions are
// independent chains rather than one LDS round trip + division per branchy store block
// (the same operations per value)
template <int ENV>
__device__ inline void filtered_obs(const double* s, int g, bool filter, const double* fmean, const double* fden,
                                    float* vf) {
  constexpr int O = EnvC<ENV>::OBS, NI = (O + 3) / 4;
  double o[O];
  EnvC<ENV>::obs(s, o);
  double v[NI], mu[NI], den[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    v[i] = o[4 * i];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (4 * i + q < O && g == q) v[i] = o[4 * i + q < O ? 4 * i + q : O - 1];
  }
  if (filter) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int kc = 4 * i + g, kk = kc < O ? kc : O - 1;
      mu[i] = fmean[kk];
      den[i] = fden[kk];
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      double x = v[i] - mu[i];
      x = x / den[i];
      v[i] = x < -5.0 ? -5.0 : (x > 5.0 ? 5.0 : x);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) vf[i] = (float)v[i];
}

// a whole iteration's sampling-noise rows (load_noise, rollout_device.h)
template <int ENV>
__global__ void noise_fill_kernel(RollArgs a, double* __restrict__ out) {
  using EC = EnvC<ENV>;
  constexpr int A = EC::ACT, P = EC::DISCRETE ? 1 : (A + 1) / 2;
  // grid (ceil(E * P / 256), min(T, 65535)): steps t = blockIdx.y + k * gridDim.y, no runtime
  // 64-bit division
  const int E = a.d.n_envs;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * P) return;
  const int c = i % P, e = i / P;
  for (int t = blockIdx.y; t < a.d.horizon; t += gridDim.y) {
    const int64_t row = (int64_t)t * E + e;
    const uint32_t gid = (uint32_t)(a.d.env_offset + e);
    const uint64_t w = (uint64_t)(*a.b.iteration) * (uint64_t)a.d.horizon + (uint64_t)t;
    double u0, u1;
    philox_uniform2(a.d.seed, 0, gid, w, (uint32_t)c, u0, u1);
    if constexpr (EC::DISCRETE) {
      out[row] = u0;
    } else {
      const double rad = sqrt(-2.0 * log(1.0 - u0));
      double sn, cn;
      sincos(2.0 * 3.141592653589793 * u1, &sn, &cn);
      out[row * A + 2 * c] = rad * cn;
      if (2 * c + 1 < A) out[row * A + 2 * c + 1] = rad * sn;
    }
  }
}

// EV (here and in the two kernels below): the evaluation instantiation (MRL_ROLLOUT_EVAL,
// rollout_device.h) -- the envs' reset alone, no partial of obs_0
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

#ifndef MRL_ROLLOUT_EVAL_UNIT
// rollout image: rimage_value (mlp_layout.h) of every element
// part p (0, 1, 2) of an f32 value's exact three-way bf16 split (mlp_split.hip)
__device__ inline float rb_part(float v, int p) {
  const __bf16 a = (__bf16)v;
  if (p == 0) return (float)a;
  const float r = v - (float)a;
  const __bf16 c = (__bf16)r;
  if (p == 1) return (float)c;
  return r - (float)c;
}

__global__ void rollout_pack_kernel(RDims r, MlpDims d, const float* __restrict__ th, float* __restrict__ out,
                                    int bf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < r.f32_size) {
    const float v = rimage_value(r, d, th, i);
    out[i] = (bf && i < r.b0) ? bf16r(v) : v;  // bf16 mode: the MFMA weights W0, W1
  } else if (i >= r.bs1 && i < r.size) {
    // split W1 fragments (fp32 mode): part p of the ba1 fragment elements, two per word
    const int rel = i - r.bs1, part = rel / (4 * 2 * 64 * 4), rr = rel % (4 * 2 * 64 * 4);
    const int frag = rr >> 2, q = rr & 3;
    const __bf16 lo = (__bf16)rb_part(rimage_bf16_elem(d, th, true, frag, 2 * q), part);
    const __bf16 hi = (__bf16)rb_part(rimage_bf16_elem(d, th, true, frag, 2 * q + 1), part);
    out[i] = __uint_as_float((uint32_t)__builtin_bit_cast(uint16_t, lo) |
                             ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16));
  } else if (i < r.size) {
    // bf16 fragments: two bf16 per word
    const bool l1 = i >= r.ba1;
    const int rel = i - (l1 ? r.ba1 : r.ba0), frag = rel >> 2, q = rel & 3;
    const __bf16 lo = (__bf16)rimage_bf16_elem(d, th, l1, frag, 2 * q);
    const __bf16 hi = (__bf16)rimage_bf16_elem(d, th, l1, frag, 2 * q + 1);
    out[i] = __uint_as_float((uint32_t)__builtin_bit_cast(uint16_t, lo) |
                             ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16));
  }
}
#endif  // MRL_ROLLOUT_EVAL_UNIT

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
    if (jj == 0 && blockIdx.x == 0) {
      if (k == 0) fs_out[0] = fn;
      if (isr) fs_out[1] = fn;
      fs_out[2 + k] = fM;
      fs_out[2 + D + k] = fS;
    }
    if (!isr && jj == 0) {
      const double var = fn > 1.0 ? fS / (fn - 1.0) : fM * fM;  // running_stat.py:27
      fmean[k] = fM;
      fden[k] = sqrt(var) + 1e-8;
    }
  }
  if constexpr (D > COLS && !EV) {  // the columns past the 16 thread groups: a second pass by the first groups
    const int k2 = k + COLS;
    if (k2 < D) {
      const bool isr2 = (k2 == O);
      double fn2 = fs_in[isr2 ? 1 : 0], fM2 = fs_in[2 + k2], fS2 = fs_in[2 + D + k2];
      double bn, bm, bs;
      batch_of_records(rec_in, a.nb, a.RS, D, O, k2, jj, bn, bm, bs);
      chan_merge(fn2, fM2, fS2, bn, bm, bs);
      if (jj == 0 && blockIdx.x == 0) {
        if (isr2) fs_out[1] = fn2;
        fs_out[2 + k2] = fM2;
        fs_out[2 + D + k2] = fS2;
      }
      if (!isr2 && jj == 0) {
        const double var = fn2 > 1.0 ? fS2 / (fn2 - 1.0) : fM2 * fM2;
        fmean[k2] = fM2;
        fden[k2] = sqrt(var) + 1e-8;
      }
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
  struct XL {
    const float* p;
    bool valid;
    __device__ inline float operator()(int c) const { return (valid && c < O) ? p[c] : 0.f; }
  } xl{&xt[wave][j][0], valid};
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

// ------------------------------------------------------------------ persistent rollout
// The whole horizon in ONE launch (mrl_rollout_run): the nb blocks of the step kernel
// stay resident (one block per CU of the launch stream's CU set) and loop over t.  Weights, env state, episode
// counters and the running stat live in registers for all T steps; the only cross-block
// dependency of a step -- the Welford partials of the E raw observations (and rewards)
// that every block merges into its copy of the running stat -- is handed off in memory
// as data-tagged granules: each (block, column) partial is ONE 16-B granule {fp64 mean,
// fp64 M2} written by a single write-through (sc1) store, the step tag riding in M2's
// sign bit (M2 >= 0); a consumer polls the granules themselves with sc1 loads until
// every tag carries the step it waits for, so one memory round trip both signals and
// delivers (MI355X_MICROARCH.md, hand-offs: untorn 16-B sc1 granules).  Counts are not
// sent: every block knows each block's number of envs.  Two parities as between step
// launches: block b can only overwrite the parity-p granule of gather step s at step
// s+2 after every block's step-s+1 granules arrived, i.e. after every block has read
// step s; so a slot only ever holds step s or s-2 (or the launch's memset zeros), and
// one tag bit that alternates between consecutive writes of a slot -- tag(s) =
// ((s >> 1) & 1) ^ 1, never the memset's 0 for s = 0, 1 -- tells them apart.
// Bit-identical to the step kernels.
constexpr int SYNC_ABORT = 32;             // u32 word: a block gave up waiting (own 128-B line)
constexpr int64_t SYNC_HEAD_BYTES = 256;   // then the granules: [2 parities][D][nb] x 16 B
constexpr uint32_t SPIN_LIMIT = 1u << 22;  // polls (~seconds): a non-resident grid exits

typedef uint32_t gran_t __attribute__((ext_vector_type(4)));  // one 16-B granule

__device__ inline uint32_t step_tag(int s) { return (((uint32_t)s >> 1) & 1u) ^ 1u; }

struct Granules {
  __amdgpu_buffer_rsrc_t rsrc;
  int nb, D;
  __device__ Granules(uint32_t* sync, int nb_, int D_) : nb(nb_), D(D_) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(sync) + SYNC_HEAD_BYTES, 0,
                                             2 * D_ * nb_ * 16, 0x00020000);
  }
  __device__ uint32_t off(int parity, int k, int b) const { return (uint32_t)(((parity * D + k) * nb + b) * 16); }
  __device__ void put(int step, int k, int b, double mean, double m2) const {
    const uint64_t mb = (uint64_t)__double_as_longlong(mean);
    const uint64_t sb = ((uint64_t)__double_as_longlong(m2) & ~(1ull << 63)) | ((uint64_t)step_tag(step) << 63);
    gran_t g = {(uint32_t)mb, (uint32_t)(mb >> 32), (uint32_t)sb, (uint32_t)(sb >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(g, rsrc, off(step & 1, k, b), 0, 16);  // aux 16 = sc1
  }
  __device__ gran_t get(int step, int k, int b) const {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, off(step & 1, k, b), 0, 16);
  }
};
__device__ inline double g_mean(gran_t g) { return __longlong_as_double((long long)(((uint64_t)g.y << 32) | g.x)); }
__device__ inline double g_m2(gran_t g) {
  return __longlong_as_double((long long)((((uint64_t)(g.w & 0x7fffffffu)) << 32) | g.z));
}
__device__ inline bool g_tag_is(gran_t g, int step) { return (g.w >> 31) == step_tag(step); }

// the block's (mean, M2) partial of vals[nvalid][D] (publish_partial's arithmetic) as
// the granules of gather step `step`; lane 0 of column group k writes column k's
// (K0: publish_partial's column pass)
template <int K0 = 0>
__device__ inline void publish_granules(const Granules& gr, const double* vals, int nvalid, int step) {
  const int k = K0 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  double mean, m2;
  block_moments(vals, nvalid, gr.D, k, j, mean, m2);
  if (k < gr.D && j == 0) gr.put(step, k, blockIdx.x, mean, m2);
}

// column k's records of blocks b0 + jj + 16q as RecRound registers, polled until every
// granule carries gather step `step`'s tag; n_b is known (envs of block b; 0 for the
// reward column of the reset partial).  false: the grid gave up (some block never
// published).
template <int R, class Under>
__device__ inline bool gather_granules(const Granules& gr, RecRoundT<R>& rr, int step, int k, int jj, int b0, int E,
                                       bool rew_counted, uint32_t* sync, Under&& under) {
  const bool isr = (k == gr.D - 1);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int b = b0 + jj + 16 * q;
    rr.rn[q] = (b < gr.nb && (!isr || rew_counted)) ? (double)min(ENVS_PER_BLOCK, E - b * ENVS_PER_BLOCK) : 0.0;
  }
  uint32_t it = 0;
  while (true) {
    gran_t gq[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int b = b0 + jj + 16 * q;
      gq[q] = gr.get(step, k, b < gr.nb ? b : 0);
    }
    if (it == 0) under();  // independent work while the first poll's loads are in flight
    bool ready = true;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const bool in = b0 + jj + 16 * q < gr.nb;
      ready = ready && (!in || g_tag_is(gq[q], step));
      rr.rm[q] = in ? g_mean(gq[q]) : 0.0;
      rr.rs[q] = in ? g_m2(gq[q]) : 0.0;
    }
    if (ready) return true;
    __builtin_amdgcn_s_sleep(1);
    if ((++it & 255) == 0 &&
        (it > SPIN_LIMIT || __hip_atomic_load(sync + SYNC_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      __hip_atomic_store(sync + SYNC_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
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
    struct XL {
      const float* p;
      bool valid;
      __device__ inline float operator()(int c) const { return (valid && c < O) ? p[c] : 0.f; }
    } xl{&xt[wave][j][0], valid};
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

#ifdef MRL_ROLLOUT_EVAL_UNIT
// The evaluation unit (rollout_eval.hip compiles this file with MRL_ROLLOUT_EVAL_UNIT): the EV
// instantiations of the three kernels above behind the launchers the entry points below call.
// They are a unit of their own because instantiated here, beside the training kernels, they
// changed a training kernel's listing (Swimmer's step kernel, a loop branch in its other
// sense: the envs' step functions gain callers in the module); this unit's device code holds
// the EV kernels alone, and this file's the kernels it held before.
void launch_rollout_reset_eval(const RollArgs& a, hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((rollout_reset_kernel<env(), true>), dim3(a.nb), dim3(RB), 0, s, a);
  });
}
void launch_rollout_step_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage, int t,
                              hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_step_kernel<env(), BF(), true>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage, t);
    });
  });
}
// independent blocks: no workspace, no residency check, no stamps
void launch_rollout_persistent_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage,
                                    hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_persistent_kernel<env(), BF(), false, true>), dim3(a.nb), dim3(RB), 0, s, a, logstd,
                         rimage, nullptr);
    });
  });
}

}  // namespace mrl
#else
__global__ void rollout_finish_kernel(RollArgs a, int O) {
  const int D = O + 1, T = a.d.horizon;
  const double* fs_in = a.b.filter_state + (T & 1) * a.FS;
  double* fs_out = a.b.filter_state;
  const double* rec_in = a.b.records + (int64_t)(T & 1) * a.nb * a.RS;
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  // the last step's rewards still go through rewfilt (core.py:199); obs_T is never pushed
  double n = 0.0, M = 0.0, S = 0.0;
  if (g == 0) {
    n = fs_in[1];
    M = fs_in[2 + O];
    S = fs_in[2 + D + O];
    double bn, bm, bs;
    batch_of_records(rec_in, a.nb, a.RS, D, O, O, j, bn, bm, bs);
    chan_merge(n, M, S, bn, bm, bs);
  }
  // copy the obs stat when fs_in is the other buffer (T odd)
  double cp[(MAXD_L + RB - 1) / RB * 2 + 1];
  int nc = 0;
  if ((T & 1) != 0)
    for (int k = threadIdx.x; k < O; k += RB) {
      cp[nc++] = fs_in[2 + k];
      cp[nc++] = fs_in[2 + D + k];
    }
  const double n_obs = fs_in[0];
  __syncthreads();  // fs_in may alias fs_out (T even)
  if ((T & 1) != 0) {
    nc = 0;
    for (int k = threadIdx.x; k < O; k += RB) {
      fs_out[2 + k] = cp[nc++];
      fs_out[2 + D + k] = cp[nc++];
    }
    if (threadIdx.x == 0) fs_out[0] = n_obs;
  }
  if (g == 0 && j == 0) {
    fs_out[1] = n;
    fs_out[2 + O] = M;
    fs_out[2 + D + O] = S;
  }
  if (threadIdx.x == 0) *a.b.iteration += 1;
}

}  // namespace mrl

using namespace mrl;

extern "C" {

// Humanoid: the state (SoA [NS][E]) and then each env's kinematics cache (AoS [E][KCACHE],
// humanoid.h save_kcache) -- the forward kinematics of the stored state
int64_t mrl_env_state_doubles(int32_t env_id) {
  return env_info(env_id).ns + (env_id == MRL_ENV_HUMANOID ? HM_KCACHE : 0);
}
int64_t mrl_filter_doubles(int32_t env_id) { return filt_doubles(env_info(env_id).obs); }
int64_t mrl_record_doubles(int32_t env_id) { return filt_doubles(env_info(env_id).obs); }
int64_t mrl_rollout_blocks(int32_t n_envs) { return env_blocks(n_envs); }
int64_t mrl_rollout_noise_doubles(const mrl_rollout_desc* d) {
  if (!d || d->n_envs <= 0 || d->horizon <= 0) return -1;
  if (roll_eval(d)) return 0;  // the head's mode: no noise is drawn
  const EnvInfo ei = env_info(d->env_id);
  return (int64_t)d->horizon * d->n_envs * (ei.discrete ? 1 : ei.act);
}

int mrl_rollout_noise(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, double* out, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (!out) return fail(E_ARG, "null noise rows");
  if (roll_eval(d)) return fail(E_ARG, "mrl_rollout_noise: MRL_ROLLOUT_EVAL draws no noise");
  RollArgs a = make_args(d, b);
  const EnvInfo ei = env_info(d->env_id);
  const int64_t per_step = (int64_t)d->n_envs * (ei.discrete ? 1 : (ei.act + 1) / 2);
  MRL_DISPATCH_ENV(d->env_id, noise_fill_kernel, dim3((unsigned)((per_step + 255) / 256), (unsigned)(d->horizon < 65535 ? d->horizon : 65535)),
                   dim3(256), 0, (hipStream_t)stream, a, out);
  return hip_check(hipGetLastError(), "mrl_rollout_noise");
}

int mrl_rollout_reset(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (d->env_id == MRL_ENV_HUMANOID) return fail(E_UNSUPPORTED, "Humanoid runs on the layered rollout (mrl_rollout_reset_rows)");
  RollArgs a = make_args(d, b);
  if (roll_eval(d)) launch_rollout_reset_eval(a, (hipStream_t)stream);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, rollout_reset_kernel, dim3(a.nb), dim3(RB), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "mrl_rollout_reset");
}

int64_t mrl_rollout_image_floats(const mrl_mlp_desc* pol) {
  if (!pol || pol->n_in <= 0 || pol->n_in > MAX_IN) return -1;
  return rollout_dims(pol->n_in).size;
}

int mrl_rollout_pack(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, float* rimage,
                     void* stream) {
  if (!d || !pol || !theta || !rimage) return fail(E_ARG, "null pointer");
  if (d->env_id == MRL_ENV_HUMANOID) return fail(E_UNSUPPORTED, "Humanoid runs on the layered rollout");
  int rc = check_fused_policy(d, pol);
  if (rc) return rc;
  const RDims r = rollout_dims(pol->n_in);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  hipLaunchKernelGGL(rollout_pack_kernel, dim3((r.size + 255) / 256), dim3(256), 0, (hipStream_t)stream, r, md, theta,
                     rimage, (int)(roll_compute(d) == MRL_COMPUTE_BF16));
  return hip_check(hipGetLastError(), "mrl_rollout_pack");
}

int64_t mrl_rollout_sync_bytes(const mrl_rollout_desc* d) {
  if (!d || d->n_envs <= 0) return -1;
  return SYNC_HEAD_BYTES + 2 * (int64_t)(env_info(d->env_id).obs + 1) * env_blocks(d->n_envs) * 16;
}

// Zeroes the hand-off workspace before a persistent launch (plain 16-B vector stores;
// the kernel boundary publishes them).  A kernel, not hipMemsetAsync: replayed from a
// captured hipGraph after other work had been launched eagerly, the memset node of
// ROCm 7.2 wrote a repeated 16-B pattern -- {int64 n, double 1/n}, bytes of a later
// eager launch's arguments -- instead of zeros.
__global__ __launch_bounds__(256) void sync_clear_kernel(uint4* __restrict__ p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The nb blocks fit one per CU of the launch stream (its CU mask) at this kernel's
// register use: the persistent launch may run (its blocks wait on each other, so the
// whole grid must be resident at once).  launch_cus > 0: the CUs of the stream a
// captured graph will replay on (the capture stream's mask says nothing about it);
// < 0: debug, no check.
static bool persistent_fits(int nb, hipStream_t s, int launch_cus) {
  if (launch_cus < 0) return true;
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return false;
  int cus = ncu;
  if (s != nullptr) {
    uint32_t mask[16] = {};
    const int words = (ncu + 31) / 32;
    if (words <= 16 && hipExtStreamGetCUMask(s, (uint32_t)words, mask) == hipSuccess) {
      cus = 0;
      for (int w = 0; w < words; ++w) cus += __builtin_popcount(mask[w]);
    }
  }
  if (launch_cus > 0) cus = min(launch_cus, ncu);
  return nb <= cus;
}

int mrl_rollout_run(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, const float* rimage,
                    const mrl_rollout_bufs* b, uint32_t* sync, int32_t persistent, void* stream) {
  int rc = check_fused_run(d, pol, theta, rimage, b);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  RollArgs a = make_args(d, b);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  const float* logstd = pol->head == MRL_HEAD_GAUSS ? theta + md.tls : nullptr;
  const bool bf = roll_compute(d) == MRL_COMPUTE_BF16, st = b->stamps != nullptr;
  if (roll_eval(d) && persistent) {
    launch_rollout_persistent_eval(a, bf, logstd, rimage, s);
    return hip_check(hipGetLastError(), "mrl_rollout_run");
  }
  if (!persistent || !sync || !persistent_fits(a.nb, s, d->launch_cus)) {
    rc = mrl_rollout_reset(d, b, stream);
    for (int32_t t = 0; t < d->horizon && rc == OK; ++t) rc = mrl_rollout_step(d, pol, theta, rimage, b, t, stream);
    return rc;
  }
  {
    const int64_t n16 = mrl_rollout_sync_bytes(d) / 16;  // SYNC_HEAD_BYTES + 16-B granules
    const int nblk = (int)std::min<int64_t>((n16 + 255) / 256, 256);
    hipLaunchKernelGGL(sync_clear_kernel, dim3(nblk), dim3(256), 0, s, reinterpret_cast<uint4*>(sync), n16);
  }
  // A plain launch: persistent_fits() guarantees one block per CU of the stream's CU
  // set, so every block becomes resident (kernels of other streams on those CUs finish
  // on their own), and the step hand-off polls are bounded (SPIN_LIMIT).  A cooperative
  // launch made HIP keep a runtime-owned queue that its teardown destroyed after an
  // attached rocprofv3 had finalised: the profiled process crashed at exit.
  dispatch_thread_env(d->env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      dispatch_bool(st, [&](auto ST) {
        hipLaunchKernelGGL((rollout_persistent_kernel<env(), BF(), ST()>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage,
                           sync);
      });
    });
  });
  return hip_check(hipGetLastError(), "mrl_rollout_run");
}

int mrl_rollout_step(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, const float* rimage,
                     const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_fused_run(d, pol, theta, rimage, b);
  if (rc) return rc;
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  const float* logstd = pol->head == MRL_HEAD_GAUSS ? theta + md.tls : nullptr;
  const bool bf = roll_compute(d) == MRL_COMPUTE_BF16;
  hipStream_t s = (hipStream_t)stream;
  if (roll_eval(d)) {
    launch_rollout_step_eval(a, bf, logstd, rimage, t, s);
    return hip_check(hipGetLastError(), "mrl_rollout_step");
  }
  dispatch_thread_env(d->env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_step_kernel<env(), BF()>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage, t);
    });
  });
  return hip_check(hipGetLastError(), "mrl_rollout_step");
}

int mrl_rollout_finish(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (roll_eval(d)) return OK;  // no reward partial to fold, and the noise's step base stays
  RollArgs a = make_args(d, b);
  hipLaunchKernelGGL(rollout_finish_kernel, dim3(1), dim3(RB), 0, (hipStream_t)stream, a, env_info(d->env_id).obs);
  return hip_check(hipGetLastError(), "mrl_rollout_finish");
}

}  // extern "C"
#endif  // MRL_ROLLOUT_EVAL_UNIT
