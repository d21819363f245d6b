// Device helpers of the bf16 throughput mode shared by its two kernel families (the rows
// kernel and the VJP of mlp_bf16.hip): the bf16 activation cache and the
// forward / JVP of one 32-row tile on v_mfma_f32_32x32x16_bf16 (layouts and rounding
// points: mlp_bf16.hip header).
#pragma once
#include "bf16_frag.h"

namespace mrl {

// ---- primal activation cache, bf16: per 32-row tile [layer 2][s 4][lane 64] x 16 B
// (8 KB per tile): every wave load / store instruction moves 1 KB contiguous.
constexpr int BCACHE_TILE_WORDS = 2 * 4 * 64 * 4;
__device__ inline void bcache_store(float* tile, int layer, int lane, const bf16x8* fr) {
#pragma unroll
  for (int s = 0; s < 4; ++s) reinterpret_cast<bf16x8*>(tile)[(layer * 4 + s) * 64 + lane] = fr[s];
}
__device__ inline void bcache_load(const float* tile, int layer, int lane, bf16x8* fr) {
#pragma unroll
  for (int s = 0; s < 4; ++s) fr[s] = reinterpret_cast<const bf16x8*>(tile)[(layer * 4 + s) * 64 + lane];
}

// forward: h1 / h2 fragments (bf16) and, with the f32 head, z
template <class XL>
__device__ inline void forward_b(const float* img, const MlpDims& d, const BDims& b, const XL& xl, int lane,
                                 bf16x8* h1b, bf16x8* h2b, float* z) {
  const int h = lane >> 5;
  bf16x8 xb[MAX_KS0B];
#pragma unroll
  for (int s0 = 0; s0 < MAX_KS0B; ++s0) xb[s0] = s0 < b.KS0B ? x_frag(xl, s0, h) : bf16x8{};
  f32x16 a1[2];
  a1[0] = load_bias16(img, b.fb0, 0, h);
  a1[1] = load_bias16(img, b.fb0, 1, h);
  layer0_b(img, b, xb, lane, a1);
  tanh16(a1[0]);
  tanh16(a1[1]);
#pragma unroll
  for (int s = 0; s < 4; ++s) h1b[s] = pack8(a1[s >> 1], s & 1);
#pragma unroll
  for (int o = 0; o < MAX_OUT; ++o) z[o] = 0.f;
#pragma unroll
  for (int mo = 0; mo < 2; ++mo) {
    f32x16 a = load_bias16(img, b.fb1, mo, h);
    chain_b(img, b, mo, h1b, lane, a);
    __builtin_amdgcn_sched_barrier(0);
    tanh16(a);
    h2b[2 * mo] = pack8(a, 0);
    h2b[2 * mo + 1] = pack8(a, 1);
    const f32x16 ar = unpack16(h2b, mo);
    head_partial_mt(img, d, ar, mo, h, z);  // d = head_dims(...)
    // scheduling fences keep the head's weight reads and the next tile's fragment
    // prefetch from all being hoisted (the static-shape builds otherwise spill)
    __builtin_amdgcn_sched_barrier(0);
  }
  head_finish(img, d, z);
}

// JVP to the head from cached bf16 h1 / h2 fragments (need_z: also the primal head)
template <class XL>
__device__ inline void jvp_b(const float* img, const float* imt, const MlpDims& d, const BDims& b, const XL& xl,
                             int lane, const bf16x8* h1b, const bf16x8* h2b, float* z, float* dz, bool need_z) {
  const int h = lane >> 5;
  bf16x8 xb[MAX_KS0B];
#pragma unroll
  for (int s0 = 0; s0 < MAX_KS0B; ++s0) xb[s0] = s0 < b.KS0B ? x_frag(xl, s0, h) : bf16x8{};
  f32x16 dh[2];
  dh[0] = load_bias16(imt, b.fb0, 0, h);
  dh[1] = load_bias16(imt, b.fb0, 1, h);
  layer0_b(imt, b, xb, lane, dh);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const f32x16 h1 = unpack16(h1b, m);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[m][r] *= dtanh(h1[r]);
  }
  bf16x8 dhb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) dhb[s] = pack8(dh[s >> 1], s & 1);
  float dzt[MAX_OUT];
#pragma unroll
  for (int o = 0; o < MAX_OUT; ++o) {
    if (need_z) z[o] = 0.f;
    dz[o] = 0.f;
    dzt[o] = 0.f;
  }
#pragma unroll
  for (int mo = 0; mo < 2; ++mo) {
    f32x16 da = load_bias16(imt, b.fb1, mo, h);
    chain_b(img, b, mo, dhb, lane, da);
    chain_b(imt, b, mo, h1b, lane, da);
    const f32x16 a = unpack16(h2b, mo);
#pragma unroll
    for (int r = 0; r < 16; ++r) da[r] *= dtanh(a[r]);
    if (need_z) head_partial_mt(img, d, a, mo, h, z);
    head_partial_mt(img, d, da, mo, h, dz);
    head_partial_mt(imt, d, a, mo, h, dzt);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (need_z) head_finish(img, d, z);
#pragma unroll
  for (int o = 0; o < MAX_OUT; ++o) dz[o] += dzt[o];
  head_finish(imt, d, dz);
}

}  // namespace mrl
