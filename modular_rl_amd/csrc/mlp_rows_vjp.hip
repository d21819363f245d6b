// The 32-row kernels of the fused 64-wide MLP path on v_mfma_f32_32x32x2_f32 (exact fp32;
// what they replace: mlp_kernels.hip header):
//
//   mlp_rows_kernel<EPI>  forward (+ JVP) of a 32-row tile per wave with a per-row
//                         epilogue: prob rows, TRPO losses, surrogate gradient rows,
//                         VF loss rows, or the KL-metric rows of the Fisher product.
//   mlp_vjp_kernel        forward recompute (or the activation cache) + backprop of
//                         head-gradient rows and the weight-gradient sums
//                         sum_rows act^T * grad  (MFMA with the row index as K, operands
//                         transposed through LDS).
//
// The two families share one unit on purpose: the uncached VJP recomputes the forward with
// the rows kernel's device helpers, and hipcc's inlining of those helpers -- and with it
// the VJP's schedule and register allocation -- depends on their other callers in the unit.
#include <math.h>

#include "mlp_host.h"

namespace mrl {

template <int EPI_K, int SH>
// 3 waves/SIMD: layer 2 is evaluated one M-tile at a time so the chain fits 168
// registers (the cached Fisher-product pass took 176 at a bound of 2, i.e. 2 waves)
__global__ __launch_bounds__(ROWS_BLOCK, 3) void mlp_rows_kernel(RowsArgs a, const float* __restrict__ img,
                                                               const float* __restrict__ imgt,
                                                               const int32_t* __restrict__ skip) {
  rows_shape<SH>(a);
  constexpr bool CACHED = EPI_K == EPI_FVP_CACHED;
  constexpr int EPI = CACHED ? MRL_EPI_FVP : EPI_K;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (skip != nullptr && *skip != 0) return;
  const MlpDims& d = a.d;
  const int fs = d.fwd_size;
  for (int i = threadIdx.x; i < fs / 4; i += ROWS_BLOCK)
    reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(img)[i];
  if (EPI == MRL_EPI_FVP)
    for (int i = threadIdx.x; i < fs / 4; i += ROWS_BLOCK)
      reinterpret_cast<float4*>(lds + fs)[i] = reinterpret_cast<const float4*>(imgt)[i];
  __syncthreads();
  const float* ldt = lds + fs;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int A = a.A;
  float ls[MAX_OUT], sd[MAX_OUT], dls[MAX_OUT];
#pragma unroll
  for (int j = 0; j < MAX_OUT; ++j) {
    ls[j] = (a.logstd != nullptr && j < A) ? a.logstd[j] : 0.f;
    sd[j] = expf(ls[j]);
    dls[j] = (a.dlogstd != nullptr && j < A) ? a.dlogstd[j] : 0.f;
  }
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  // PPOSGD (one block, n <= MRL_PPO_BLOCK_ROWS): every wave takes its tile exactly once, past
  // the end with all rows invalid, so the whole block meets in pposgd_row's reduction
  const int64_t ntiles = EPI == MRL_EPI_PPOSGD ? MRL_PPO_BLOCK_ROWS / 32 : (a.n + 31) / 32;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 32 + (lane & 31);
    const bool valid = row < a.n;
    XGlobal xl{a.x, a.ept, a.ts_limit, a.n_obs, row, valid};
    float z[MAX_OUT], dz[MAX_OUT];
    float* ctile = a.cache != nullptr ? a.cache + tile * CACHE_TILE_FLOATS : nullptr;
    if (CACHED) jvp_head_cached(lds, ldt, d, xl, lane, ctile, z, dz, a.head != MRL_HEAD_GAUSS);
    else if (EPI == MRL_EPI_FVP) forward_jvp_head_lowreg(lds, ldt, d, xl, lane, z, dz);
    else forward_head_lowreg(lds, d, xl, lane, z, a.cache_mode == MRL_CACHE_WRITE ? ctile : nullptr);
    if constexpr (EPI == MRL_EPI_PPOSGD) {
      pposgd_row<MAX_OUT>(a, row, valid && h == 0, z, dz, ls, sd, dls, acc0, acc1, acc2);
      continue;
    } else {
      if constexpr (EPI == MRL_EPI_PROB)
        if (a.feat != nullptr && valid) write_feature_row(a, row, h, xl);
      if (!valid || h != 0) continue;
      row_epilogue<EPI, MAX_OUT>(a, row, z, dz, ls, sd, dls, acc0, acc1, acc2);
    }
  }
  if (a.partial != nullptr) {
    acc0 = wave_sum(acc0);
    acc1 = wave_sum(acc1);
    acc2 = wave_sum(acc2);
    if (lane == 0) {
      double* p = a.partial + ((int64_t)blockIdx.x * 4 + wave) * 4;
      p[0] = acc0;
      p[1] = acc1;
      p[2] = acc2;
      p[3] = 0.0;
    }
  }
}

void launch_rows(int epi, int sh, const RowsArgs& a, const float* image, const float* image_t, int64_t blocks,
                 const int32_t* skip, hipStream_t s) {
  const size_t shm = (size_t)a.d.fwd_size * 4 * (epi == MRL_EPI_FVP ? 2 : 1);
  const dim3 grid(epi == MRL_EPI_PPOSGD ? 1 : blocks), blk(ROWS_BLOCK);
  with_rows_epilogue(epi, a.cache_mode, [&](auto ek) {
    constexpr int EK = decltype(ek)::value;
    with_rows_shape<EK>(sh, [&](auto shape) {
      hipLaunchKernelGGL((mlp_rows_kernel<EK, decltype(shape)::value>), grid, blk, shm, s, a, image, image_t, skip);
    });
  });
}

// ------------------------------------------------------------------ VJP
constexpr int SCR_FLOATS = 2 * 64 * IMG_PAD;  // per-wave transpose scratch

// write a transposed tile (two 32x32 C tiles of 64 units) as img[unit][h'][s'],
// row j = 2 s' + h', per-unit stride IMG_PAD (conflict-free b32 writes, b128 reads)
__device__ inline void write_img(float* img, const f32x16* t, int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int base = (j & 1) * 16 + (j >> 1);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) img[(32 * mt + cperm(r, h)) * IMG_PAD + base] = t[mt][r];
}

// every global operand one tile needs, loaded ahead of use; CACHED: the primal
// activations come from the cache instead of the layer-0 inputs
// gW2 and gW0 run on v_mfma_f32_16x16x4_f32 (their narrow side -- A <= 8 head
// outputs, O <= 16 inputs per tile -- pads to 16 instead of 32).  Their K is the 32
// rows of the tile, read from the transposed LDS images at position p = 8*kk + q
// (kk = lane >> 4, k-step q), i.e. row r(p) = 16*(kk&1) + 2q + (kk>>1).
__device__ inline int vjp_row16(int kk, int q) { return 16 * (kk & 1) + 2 * q + (kk >> 1); }

template <bool CACHED, bool WIDE>
struct VjpIn {
  float x0[CACHED ? 1 : 16];  // layer-0 B operands x[row][2s+h]
  f32x16 act[CACHED ? 2 : 1]; // cached h2[0], h2[1] (h1 is loaded by the tile itself)
  float xg[WIDE ? 16 : 8];    // gW0 A operands x[row0 + r(8kk+q)][16mt + (lane&15)] at [8mt + q]
  float g[4];                 // head-gradient rows ghead[row][r+4h]
  float gs[MAX_OUT];          // summed head columns (DiagGauss logstd), lane half 0 only
};

// Branch-free loads: row indices are clamped to the batch and columns to the row
// width, so every load is unconditional straight-line code; what must read as zero
// (head-gradient entries of rows past n, of outputs past A, the logstd sums off lane
// half 0) is masked when the tile USES the values (a select at load time would force
// a wait right after the loads are issued).  The clamped gW0 operands of rows past
// n multiply head-gradient rows that are exactly zero; those of columns past the
// input width land in gW0 rows that are never stored.
// gW0 A operands of one tile (used last: issued after the operands of the first phases)
template <bool WIDE>
__device__ inline void vjp_load_xg(const VjpArgs& a, int64_t tile, int lane, float* xg) {
  const int i16 = lane & 15, kk = lane >> 4;
  constexpr int MT0 = WIDE ? 2 : 1;
  const int64_t row0 = tile * 32, last = a.n - 1;
  if (a.ept == nullptr) {
#pragma unroll
    for (int mt = 0; mt < MT0; ++mt) {
      const int c = 16 * mt + i16, cc = c < a.n_obs ? c : a.n_obs - 1;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int64_t xr = row0 + vjp_row16(kk, q);
        xg[8 * mt + q] = a.x[(xr < last ? xr : last) * a.n_obs + cc];
      }
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < MT0; ++mt) {
      const int c = 16 * mt + i16;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int64_t xr = row0 + vjp_row16(kk, q);
        XGlobal xq{a.x, a.ept, a.ts_limit, a.n_obs, xr, xr < a.n};
        xg[8 * mt + q] = (c < a.d.O) ? xq(c) : 0.f;
      }
    }
  }
}

template <bool CACHED, bool WIDE>
__device__ inline void vjp_load(const VjpArgs& a, int64_t tile, int lane, VjpIn<CACHED, WIDE>& in) {
  const int h = lane >> 5, j = lane & 31;
  const int64_t row0 = tile * 32, row = row0 + j, last = a.n - 1;
  if constexpr (CACHED) {
    const float* ct = a.cache + tile * CACHE_TILE_FLOATS;
#pragma unroll
    for (int q = 0; q < 2; ++q) cache_load(ct, lane, 2 + q, in.act[q]);
  } else {
    XGlobal xl{a.x, a.ept, a.ts_limit, a.n_obs, row, row < a.n};
#pragma unroll
    for (int s = 0; s < 16; ++s) in.x0[s] = (s < a.d.KS0p) ? xl(2 * s + h) : 0.f;
  }
  const float* gr = a.ghead + (row < last ? row : last) * a.gh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = r + 4 * h;
    in.g[r] = gr[o < a.gh ? o : a.gh - 1];
  }
#pragma unroll
  for (int q = 0; q < MAX_OUT; ++q) {
    const int c = a.d.A + q;
    in.gs[q] = gr[c < a.gh ? c : a.gh - 1];
  }
}

// Bias gradients come from per-lane register partials (no per-tile LDS row sums).  One
// wave per SIMD, on the run-time shape: a two-wave schedule (256 registers, 9 spilled) and
// the static-shape instantiations measured slower.
template <bool CACHED, bool WIDE>
__global__ __launch_bounds__(256, 1) void mlp_vjp_kernel(VjpArgs a, const float* __restrict__ img,
                                                       const int32_t* __restrict__ skip) {
  constexpr int MT0 = WIDE ? 2 : 1;  // 16-input tiles of gW0
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (skip != nullptr && *skip != 0) return;
  const MlpDims& d = a.d;
  for (int i = threadIdx.x; i < d.total_size / 4; i += 256)
    reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(img)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
  float* scrA = lds + d.total_size + wave * SCR_FLOATS;
  float* scrB = scrA + 64 * IMG_PAD;
  const int A = d.A;

  f32x16 gW1[2][2];
  f32x4 gW2[4], gW0[MT0][4];  // 16x16 C tiles: gW2 [unit tile], gW0 [input tile][unit tile]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) gW1[m][n] = zero16();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    gW2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < MT0; ++m) gW0[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int i16 = lane & 15, kk = lane >> 4;
  // bias gradients as per-lane partials over the wave's tiles (row j of each C tile),
  // summed over the 32 rows once at the end instead of an LDS row sum per tile
  f32x16 pb0[2], pb1[2];
  float pG[4] = {0.f, 0.f, 0.f, 0.f};
  pb0[0] = pb0[1] = pb1[0] = pb1[1] = zero16();
  float gls[MAX_OUT];
#pragma unroll
  for (int q = 0; q < MAX_OUT; ++q) gls[q] = 0.f;

  const int64_t ntiles = (a.n + 31) / 32;
  const int64_t stride = (int64_t)gridDim.x * 4;
  // Every global operand of a tile is issued at the tile's start (h2 and the head rows
  // first, h1 and the gW0 operands, used later, after them).  A register prefetch of
  // the next tile (double buffering) measured slower: its 84 registers went to AGPRs
  // and were copied back every tile (1.11 ms vs 1.00 ms per launch at 4.19 M rows).
  VjpIn<CACHED, WIDE> cur;
  int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  for (; tile < ntiles; tile += stride) {
    vjp_load(a, tile, lane, cur);
    const int64_t row0 = tile * 32;
    Fwd f;
    const float* ct = CACHED ? a.cache + tile * CACHE_TILE_FLOATS : nullptr;
    if constexpr (CACHED) {
      // h1 is first used after the gh1 chain: its loads are issued after the ones the
      // first phases wait for
      cache_load(ct, lane, 0, f.h1[0]);
      cache_load(ct, lane, 1, f.h1[1]);
      f.h2[0] = cur.act[0];
      f.h2[1] = cur.act[1];
    } else {
      forward_tile_pre(lds, d, cur.x0, lane, f);
    }
    vjp_load_xg<WIDE>(a, tile, lane, cur.xg);  // used last

    // head gradient rows in C layout: register r of half h = out r + 4h (masked here,
    // not at load time: see vjp_load)
    const bool valid = row0 + j < a.n;
    float G[4];  // head-gradient rows: register r of half h = output r + 4h
#pragma unroll
    for (int r = 0; r < 4; ++r) G[r] = (valid && r + 4 * h < A) ? cur.g[r] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) pG[r] += G[r];
#pragma unroll
    for (int q = 0; q < MAX_OUT; ++q) gls[q] += (valid && h == 0 && q < a.n_sum) ? cur.gs[q] : 0.f;
    // Phase order keeps the MFMA pipe fed: every LDS transpose is issued while an
    // independent MFMA chain runs (the wave_lds barriers split scheduling regions, so
    // the source order is the schedule).  Accumulation orders are unchanged.
    // (a) transposes that need nothing computed: h2 image, G rows
    write_img(scrA, f.h2, lane);
    {
      const int base = (j & 1) * 16 + (j >> 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) scrB[(r + 4 * h) * IMG_PAD + base] = G[r];
    }
    // (b) gh2 = W2 . G   (K = outs, 4 k-steps) while the transposes land
    f32x16 g2[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      g2[mi] = zero16();
      const float4 w = frag4(lds, d.ba2, 4, mi, 0, lane);
      g2[mi] = MFMA32(w.x, G[0], g2[mi]);
      g2[mi] = MFMA32(w.y, G[1], g2[mi]);
      g2[mi] = MFMA32(w.z, G[2], g2[mi]);
      g2[mi] = MFMA32(w.w, G[3], g2[mi]);
    }
    WAVE_LDS_ORDER();
    // (c) gW2 += H2^T G  (row index as K through LDS; 16x16x4, head outputs as N)
    // k-steps 0-3 then 4-7, each half's operands read just before it (the same MFMA
    // order as one pass; half the live operand registers)
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
      const float4 bq = ld4(scrB + i16 * IMG_PAD + 8 * kk + 4 * hq);
      float4 aq[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) aq[mt] = ld4(scrA + (16 * mt + i16) * IMG_PAD + 8 * kk + 4 * hq);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) gW2[mt] = MFMA16(f4get(aq[mt], q), f4get(bq, q), gW2[mt]);
    }
    // (d) ga2 = gh2 * (1 - h2^2)
#pragma unroll
    for (int m = 0; m < 2; ++m) mul_dtanh16(g2[m], f.h2[m]);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) pb1[m][r] += g2[m][r];
    // (e) gh1 = W1 . ga2: registers + the weight image only, so its 64 MFMAs cover the
    //     h1 / ga2 transposes issued next
    f32x16 g1[2];
    g1[0] = zero16();
    g1[1] = zero16();
    chain<2>(lds, d.ba1, g2, lane, g1);
    WAVE_LDS_ORDER();
    write_img(scrA, f.h1, lane);
    write_img(scrB, g2, lane);
    WAVE_LDS_ORDER();
    // (f) gW1 += H1^T GA2, and ga1 = gh1 * (1 - h1^2) on the VALU under it
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const float4 a0 = ld4(scrA + j * IMG_PAD + h * 16 + 4 * s4);
      const float4 a1 = ld4(scrA + (32 + j) * IMG_PAD + h * 16 + 4 * s4);
      const float4 b0 = ld4(scrB + j * IMG_PAD + h * 16 + 4 * s4);
      const float4 b1 = ld4(scrB + (32 + j) * IMG_PAD + h * 16 + 4 * s4);
      gW1[0][0] = MFMA32(a0.x, b0.x, gW1[0][0]);
      gW1[0][1] = MFMA32(a0.x, b1.x, gW1[0][1]);
      gW1[1][0] = MFMA32(a1.x, b0.x, gW1[1][0]);
      gW1[1][1] = MFMA32(a1.x, b1.x, gW1[1][1]);
      gW1[0][0] = MFMA32(a0.y, b0.y, gW1[0][0]);
      gW1[0][1] = MFMA32(a0.y, b1.y, gW1[0][1]);
      gW1[1][0] = MFMA32(a1.y, b0.y, gW1[1][0]);
      gW1[1][1] = MFMA32(a1.y, b1.y, gW1[1][1]);
      gW1[0][0] = MFMA32(a0.z, b0.z, gW1[0][0]);
      gW1[0][1] = MFMA32(a0.z, b1.z, gW1[0][1]);
      gW1[1][0] = MFMA32(a1.z, b0.z, gW1[1][0]);
      gW1[1][1] = MFMA32(a1.z, b1.z, gW1[1][1]);
      gW1[0][0] = MFMA32(a0.w, b0.w, gW1[0][0]);
      gW1[0][1] = MFMA32(a0.w, b1.w, gW1[0][1]);
      gW1[1][0] = MFMA32(a1.w, b0.w, gW1[1][0]);
      gW1[1][1] = MFMA32(a1.w, b1.w, gW1[1][1]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) mul_dtanh16(g1[m], f.h1[m]);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) pb0[m][r] += g1[m][r];
    WAVE_LDS_ORDER();
    write_img(scrB, g1, lane);
    WAVE_LDS_ORDER();
    // (g) gW0 += X^T GA1 : A[i = input][k = row] straight from global x (16x16x4)
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
      float4 bq[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) bq[nt] = ld4(scrB + (16 * nt + i16) * IMG_PAD + 8 * kk + 4 * hq);
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
        for (int mt = 0; mt < MT0; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            gW0[mt][nt] = MFMA16(cur.xg[8 * mt + 4 * hq + q4], f4get(bq[nt], q4), gW0[mt][nt]);
    }
    WAVE_LDS_ORDER();
  }

  // per-wave partial gradient in flat theta layout
  float* out = a.slab + ((int64_t)blockIdx.x * 4 + wave) * d.P;
#pragma unroll
  for (int mt = 0; mt < MT0; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * mt + 4 * kk + r;
        if (i < d.O) out[d.tW0 + i * HID + 16 * nt + i16] = gW0[mt][nt][r];
      }
  // sum each partial over the 32 rows (lanes j of a half, butterfly), then lane j = 0
  // of half h holds units 32 m + cperm(r, h)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pb0[m][r] = half_sum(pb0[m][r]);
      pb1[m][r] = half_sum(pb1[m][r]);
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) pG[r] = half_sum(pG[r]);
  if (j == 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        out[d.tb0 + 32 * m + cperm(r, h)] = pb0[m][r];
        out[d.tb1 + 32 * m + cperm(r, h)] = pb1[m][r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r + 4 * h < A) out[d.tb2 + r + 4 * h] = pG[r];
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int mj = 0; mj < 2; ++mj)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[d.tW1 + (32 * mi + cperm(r, h)) * HID + 32 * mj + j] = gW1[mi][mj][r];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i16 < A) out[d.tW2 + (16 * mt + 4 * kk + r) * A + i16] = gW2[mt][r];
  for (int q = 0; q < a.n_sum; ++q) {
    const float s = wave_sumf(gls[q]);
    if (lane == 0) out[d.tls + q] = s;
  }
}

void launch_vjp(const VjpArgs& a, const float* image, int64_t blocks, const int32_t* skip, hipStream_t s) {
  const size_t shm = ((size_t)a.d.total_size + 4 * (size_t)SCR_FLOATS) * 4;
  const bool wide = a.d.O > 16;
  const dim3 grid(blocks), blk(256);
  with_bool(a.cache != nullptr, [&](auto cached) {
    with_bool(wide, [&](auto w) {
      hipLaunchKernelGGL((mlp_vjp_kernel<decltype(cached)::value, decltype(w)::value>), grid, blk, shm, s, a, image, skip);
    });
  });
}

}  // namespace mrl
