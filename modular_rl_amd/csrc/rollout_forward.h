// The fused rollout's policy forward: a wave's 16 envs through the 64-64 MLP on MFMA, the
// weights in registers (RWeights: fp32 compute, RWeightsB: bf16 compute) -- used by the step
// and the persistent kernel (rollout_kernels.h).
//
// One wave = 16 envs on v_mfma_f32_16x16x4_f32 (mlp_layout.h, rollout image): the
// step kernel is a latency chain at one wave per SIMD, and 16-row tiles halve both
// the MFMA chain and the tanh work of a 32-row tile.  The weight fragments of the
// wave go straight from global memory (L2-resident rollout image) into registers,
// loaded at kernel entry so their latency hides under the filter merge.
#pragma once
#include "rollout_device.h"

namespace mrl {

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

// forward16's input loader XL: column c of the lane's env row (filtered obs, f32 in LDS); zeros
// past the O columns and for a lane without an env
template <int O>
struct XRow {
  const float* p;
  bool valid;
  __device__ inline float operator()(int c) const { return (valid && c < O) ? p[c] : 0.f; }
};

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

}  // namespace mrl
