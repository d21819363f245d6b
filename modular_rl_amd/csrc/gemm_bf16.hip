// bf16-operand GEMMs of the layered MLP path's throughput mode (MRL_COMPUTE_BF16 with
// a bf16 tape): the operands live in HBM as bf16 (half the bytes of gemm.hip's
// fp32-staged tiles), accumulation stays f32 on v_mfma_f32_32x32x16_bf16.
//
//  mrl_gemm_bf16      C[M,N] = A[M,K] . B[K,N]  (+ A2 . B2)  + bias, epilogue store |
//                     tanh | * (1 - H^2); A row-major (K contiguous), B given as its
//                     transpose Bt[N,K] (K contiguous: the packed weight images), so
//                     both tiles stage global -> LDS as whole 16-B rows segments and
//                     every MFMA operand is one ds_read_b128.  Output f32 or bf16.
//                     Layer forward (tanh), JVP (dual product, * (1 - H^2)), VJP
//                     input grad (Bt = W itself, * (1 - H^2)).
//  mrl_gemm_bf16_tn   weight gradients C[M,N] = sum_r A[r,M] B[r,N] over the rows r
//                     (K = rows, split-K into f32 slabs); A and B are row-major
//                     activations / gradients, staged row-major and read as MFMA
//                     operands with the gfx950 transposing LDS read ds_read_b64_tr_b16.
//                     The bias gradient rides as a ones-column of A.
//
// This unit: the tiled NN kernel every other NN kernel is held bit-identical to, the
// small-M kernel, mrl_gemm_bf16 with its dispatch, and the cast / pack kernels.  The
// 256 x 256 NN kernel is gemm_bf16_big.hip, the streaming one gemm_bf16_stream.hip, the
// TN kernels and mrl_gemm_bf16_tn gemm_bf16_tn.hip; gemm_bf16_device.h holds what the
// kernels share, gemm_bf16_host.h what the launchers share.
//
// Tiled kernel: block 128 x BN (BN = 128: 2x2 waves of 64x64; BN = 32: 4 waves of 32x32,
// for the heads), global -> registers -> LDS double-buffered (the next K step's loads are
// in flight under this step's MFMAs), blocks dealt to the XCDs in contiguous tile runs.
#include <math.h>

#include "gemm_bf16_device.h"
#include "gemm_bf16_host.h"

namespace mrl {

// ------------------------------------------------------------------ NN / NT (Bt) GEMM
// QBK: K per LDS stage; row pitch QBK + 8 bf16 (144 B for 64, 80 B for 32): the 16
// rows a ds_read_b128 16-lane group touches start on distinct 4-bank groups
template <int BN, bool OUTBF, int QBK>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmB16Args g) {
  constexpr int QLD = QBK + 8;
  constexpr int MI = BN == 128 ? 2 : 1, NI = MI;
  constexpr int NA = QBM * (QBK / 8) / 256, NB = (BN * (QBK / 8) + 255) / 256;  // 16-B chunks per thread
  constexpr int STAGE = (QBM + BN) * QLD;                               // bf16 per LDS stage
  __shared__ __attribute__((aligned(16))) bfr_t smem[2 * STAGE];
  if (g.skip != nullptr && *g.skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
  const int wm = BN == 128 ? wave >> 1 : wave, wn = BN == 128 ? wave & 1 : 0;
  int64_t tm = blockIdx.y, tn = blockIdx.x;
  {
    const int64_t nx = gridDim.x, tiles = nx * gridDim.y;
    const int64_t L = blockIdx.x + nx * (int64_t)blockIdx.y;
    if (tiles % 8 == 0) {
      const int64_t T = (L % 8) * (tiles / 8) + L / 8;
      tm = T / nx;
      tn = T % nx;
    }
  }
  const int64_t m0 = tm * QBM, n0 = tn * BN;
  const int64_t ntk = (g.K + QBK - 1) / QBK;
  const int64_t nt = (g.A2 != nullptr ? 2 : 1) * ntk;
  // thread t stages chunk c (k = 8c) of rows r (+ RS i)
  constexpr int CPR = QBK / 8, RS = 256 / CPR;  // chunks per row, rows per pass
  const int sc = threadIdx.x % CPR, sr = threadIdx.x / CPR;
  u32x4v ra[NA], rb[NB];
  auto load = [&](int64_t t) {
    const bool p2 = t >= ntk;
    const int64_t k0 = (t - (p2 ? ntk : 0)) * QBK + 8 * sc;
    const bfr_t* A = p2 ? g.A2 : g.A;
    const bfr_t* B = p2 ? g.Bt2 : g.Bt;
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = load_chunk(A, m0 + sr + RS * i, g.M, g.lda, k0, g.K);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      rb[i] = sr + RS * i < BN ? load_chunk(B, n0 + sr + RS * i, g.N, g.ldb, k0, g.K) : u32x4v{0u, 0u, 0u, 0u};
  };
  auto store = [&](bfr_t* st) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4v*>(st + (sr + RS * i) * QLD + 8 * sc) = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (sr + RS * i < BN) *reinterpret_cast<u32x4v*>(st + (QBM + sr + RS * i) * QLD + 8 * sc) = rb[i];
  };
  f32x16 acc[MI][NI];
#pragma unroll
  for (int a = 0; a < MI; ++a)
#pragma unroll
    for (int b = 0; b < NI; ++b) acc[a][b] = zero16();
  if (nt > 0) {
    load(0);
    store(smem);
  }
  for (int64_t t = 0; t < nt; ++t) {
    __syncthreads();
    const bfr_t* As = smem + (t & 1) * STAGE;
    const bfr_t* Bs = As + QBM * QLD;
    if (t + 1 < nt) load(t + 1);
#pragma unroll
    for (int ks = 0; ks < QBK / 16; ++ks) {
      bf16x8 av[MI], bv[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        av[mi] = *reinterpret_cast<const bf16x8*>(As + (wm * 32 * MI + 32 * mi + j) * QLD + 16 * ks + 8 * h);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        bv[ni] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 32 * NI + 32 * ni + j) * QLD + 16 * ks + 8 * h);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = MFMA32B(bv[ni], av[mi], acc[mi][ni]);  // C^T tiles
    }
    if (t + 1 < nt) store(smem + ((t + 1) & 1) * STAGE);
  }
  // epilogue: the accumulators hold C^T tiles, so lane (j, h) holds ROW j of each 32x32
  // C tile, at columns cperm(r, h): four runs of 4 consecutive columns (8q + 4h + 0..3),
  // each one 8-B (bf16) / 16-B (f32) store, bias and H loads likewise vectorised
  const bool vec = (g.ldc & 3) == 0 && (g.epi != MRL_GEMM_DTANH || (g.ldh & 3) == 0);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int64_t row = m0 + wm * 32 * MI + mi * 32 + j;
      if (row >= g.M) continue;
      const int64_t cbase = n0 + wn * 32 * NI + ni * 32;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t c0 = cbase + 8 * q + 4 * h;
        float v[4];
        if (vec && c0 + 4 <= g.N) {
          const float4 b = g.bias != nullptr ? *reinterpret_cast<const float4*>(g.bias + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
          v[0] = acc[mi][ni][4 * q + 0] + b.x;
          v[1] = acc[mi][ni][4 * q + 1] + b.y;
          v[2] = acc[mi][ni][4 * q + 2] + b.z;
          v[3] = acc[mi][ni][4 * q + 3] + b.w;
          if (g.epi == MRL_GEMM_TANH) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
              const f32x2 t = tanh_fast2(f32x2{v[e], v[e + 1]});
              v[e] = t.x;
              v[e + 1] = t.y;
            }
          } else if (g.epi == MRL_GEMM_DTANH) {
            const uint2 hb = *reinterpret_cast<const uint2*>(g.H + row * g.ldh + c0);
            v[0] *= dtanh(__uint_as_float(hb.x << 16));
            v[1] *= dtanh(__uint_as_float(hb.x & 0xffff0000u));
            v[2] *= dtanh(__uint_as_float(hb.y << 16));
            v[3] *= dtanh(__uint_as_float(hb.y & 0xffff0000u));
          }
          if (OUTBF) {
            const uint2 o = {(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                             (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
            *reinterpret_cast<uint2*>(reinterpret_cast<bfr_t*>(g.C) + row * g.ldc + c0) = o;
          } else {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(g.C) + row * g.ldc + c0) = make_float4(v[0], v[1], v[2], v[3]);
          }
          continue;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t col = c0 + e;
          if (col >= g.N) continue;
          float x = acc[mi][ni][4 * q + e] + (g.bias != nullptr ? g.bias[col] : 0.f);
          if (g.epi == MRL_GEMM_TANH) x = tanh_fast(x);
          else if (g.epi == MRL_GEMM_DTANH) x *= dtanh(bf2f(g.H[row * g.ldh + col]));
          if (OUTBF) reinterpret_cast<bfr_t*>(g.C)[row * g.ldc + col] = f2bf(x);
          else reinterpret_cast<float*>(g.C)[row * g.ldc + col] = x;
        }
      }
    }
}

// ------------------------------------------------------------------ small-M NN GEMM
// The Humanoid rollout's per-step hidden layers (M = E = 1024 rows, K <= 512, N = 512)
// are latency-bound: the 128 x 128 tiled kernel gives 32 blocks a serial 8-stage K loop.
// Here a block takes a 64 x 64 tile (four waves of 32 x 32, one accumulator each) and
// stages its whole A / Bt panels (K <= 512) by LDS-DMA at entry, as four K quarters
// (128 k each) in separate LDS objects: quarter q's MFMAs start as soon as its DMA has
// landed (counted vmcnt + barrier) while the later quarters are still in flight.  Image
// [row][16 chunks] per quarter (256-B rows), chunk c of row r at c ^ (r & 15): the 16
// rows of a ds_read_b128 lane group cover the 64 banks once.  Same k order per output
// as gemm_bf16_kernel (k-steps of 16 ascending): bit-identical results.
constexpr int SBM = 64, SBN = 64, SQK = 128;  // tile, K per quarter
constexpr int SQ_ELEMS = SBM * SQK;            // bf16 per quarter image (16 KB)

template <bool OUTBF>
__global__ __launch_bounds__(256) void gemm_bf16_small_kernel(GemmB16Args g) {
  __shared__ __attribute__((aligned(16))) bfr_t a0[SQ_ELEMS], a1[SQ_ELEMS], a2[SQ_ELEMS], a3[SQ_ELEMS];
  __shared__ __attribute__((aligned(16))) bfr_t b0[SQ_ELEMS], b1[SQ_ELEMS], b2[SQ_ELEMS], b3[SQ_ELEMS];
  if (g.skip != nullptr && *g.skip != 0) return;
  const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.y * SBM, n0 = (int64_t)blockIdx.x * SBN;
  const int nq = (int)((g.K + SQK - 1) / SQK);  // quarters (host: K <= 512); k past K reads zeros
  // DMA: wave w, instruction i covers rows 16 w + 4 i + (lane >> 4), position lane & 15
  const int pos = lane & 15;
  auto dma = [&](bfr_t* qa, bfr_t* qb, int q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 16 * wave + 4 * i + (lane >> 4);
      const int c = pos ^ (r & 15);
      const int64_t k = (int64_t)q * SQK + 8 * c;
      const int64_t ra = min(m0 + r, g.M - 1), rb = min(n0 + r, g.N - 1);
      const void* sa = k < g.K ? (const void*)(g.A + ra * g.lda + k) : (const void*)kZero16;
      const void* sb = k < g.K ? (const void*)(g.Bt + rb * g.ldb + k) : (const void*)kZero16;
      glds16b(sa, qa + (16 * wave + 4 * i) * 128);
      glds16b(sb, qb + (16 * wave + 4 * i) * 128);
    }
  };
  dma(a0, b0, 0);
  if (nq > 1) dma(a1, b1, 1);
  if (nq > 2) dma(a2, b2, 2);
  if (nq > 3) dma(a3, b3, 3);
  f32x16 acc = zero16();
  const int ra = 32 * wm + j, rb = 32 * wn + j;
  // quarter q: this wave's DMA of it has landed (8 instructions per later quarter still
  // in flight), then every wave's (the barrier); 8 k-steps, branch-free (zeros past K)
  auto quarter = [&](const bfr_t* As, const bfr_t* Bs, int later) {
    if (later >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (later == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the fragment reads as inline asm: the compiler's LDS-DMA alias tracking (a few
    // DMAs deep) would otherwise drain every quarter still in flight (vmcnt 0) before
    // them; their completion is this lambda's explicit lgkmcnt wait, which takes the
    // fragments as operands so no MFMA is scheduled above it
    u32x4v av[8], bv[8];
    const uint32_t la = (uint32_t)reinterpret_cast<uintptr_t>(As) + 2 * ra * 128;
    const uint32_t lb = (uint32_t)reinterpret_cast<uintptr_t>(Bs) + 2 * rb * 128;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int c = 2 * ks + h;
      asm volatile("ds_read_b128 %0, %1" : "=v"(av[ks]) : "v"(la + 16 * (c ^ (ra & 15))));
      asm volatile("ds_read_b128 %0, %1" : "=v"(bv[ks]) : "v"(lb + 16 * (c ^ (rb & 15))));
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]), "+v"(av[6]),
                   "+v"(av[7]), "+v"(bv[0]), "+v"(bv[1]), "+v"(bv[2]), "+v"(bv[3]), "+v"(bv[4]), "+v"(bv[5]),
                   "+v"(bv[6]), "+v"(bv[7]));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)  // C^T tile: lane (j, h) holds row j
      acc = MFMA32B(__builtin_bit_cast(bf16x8, bv[ks]), __builtin_bit_cast(bf16x8, av[ks]), acc);
  };
  quarter(a0, b0, nq - 1);
  if (nq > 1) quarter(a1, b1, nq - 2);
  if (nq > 2) quarter(a2, b2, nq - 3);
  if (nq > 3) quarter(a3, b3, 0);
  // epilogue: a copy of gemm_bf16_kernel's (one 32 x 32 tile per wave) without the DTANH
  // arm, which the host never sends here
  const int64_t row = m0 + 32 * wm + j;
  if (row >= g.M) return;
  const bool vec = (g.ldc & 3) == 0;
  const int64_t cbase = n0 + 32 * wn;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t c0 = cbase + 8 * q + 4 * h;
    float v[4];
    if (vec && c0 + 4 <= g.N) {
      const float4 b = g.bias != nullptr ? *reinterpret_cast<const float4*>(g.bias + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[0] = acc[4 * q + 0] + b.x;
      v[1] = acc[4 * q + 1] + b.y;
      v[2] = acc[4 * q + 2] + b.z;
      v[3] = acc[4 * q + 3] + b.w;
      if (g.epi == MRL_GEMM_TANH) {
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const f32x2 t = tanh_fast2(f32x2{v[e], v[e + 1]});
          v[e] = t.x;
          v[e + 1] = t.y;
        }
      }
      if (OUTBF) {
        const uint2 o = {(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                         (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
        *reinterpret_cast<uint2*>(reinterpret_cast<bfr_t*>(g.C) + row * g.ldc + c0) = o;
      } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(g.C) + row * g.ldc + c0) = make_float4(v[0], v[1], v[2], v[3]);
      }
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t col = c0 + e;
      if (col >= g.N) continue;
      float x = acc[4 * q + e] + (g.bias != nullptr ? g.bias[col] : 0.f);
      if (g.epi == MRL_GEMM_TANH) x = tanh_fast(x);
      if (OUTBF) reinterpret_cast<bfr_t*>(g.C)[row * g.ldc + col] = f2bf(x);
      else reinterpret_cast<float*>(g.C)[row * g.ldc + col] = x;
    }
  }
}

// ------------------------------------------------------------------ casts / packs
// y[r][c] = bf16(x[r][c]) for c < cols, 0 for cols <= c < ldy (zero K padding)
__global__ void cast_rows_bf16_kernel(const float* __restrict__ x, int64_t rows, int64_t cols, int64_t ldx,
                                      bfr_t* __restrict__ y, int64_t ldy) {
  const int64_t total = rows * ldy;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ldy, c = i % ldy;
    y[i] = c < cols ? f2bf(x[r * ldx + c]) : (bfr_t)0;
  }
}

// W [din][dout] (f32, row-major) -> bf16 image: transpose 0: [din][ld] (= W, zero
// columns dout..ld-1), transpose 1: [dout][ld] (= W^T, zero columns din..ld-1)
__global__ void pack_w_bf16_kernel(const float* __restrict__ w, int64_t din, int64_t dout, int transpose,
                                   bfr_t* __restrict__ out, int64_t ld) {
  const int64_t rows = transpose ? dout : din, cols = transpose ? din : dout;
  const int64_t total = rows * ld;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ld, c = i % ld;
    out[i] = c < cols ? f2bf(transpose ? w[c * dout + r] : w[r * dout + c]) : (bfr_t)0;
  }
}

// the tiled kernel with QBK-deep K stages: 128 x 32 tiles (`narrow`: nn_route sends
// N <= 32 there), else 128 x 128
template <int QBK>
static void launch_tiled(const GemmB16Args& g, bool narrow, bool bf, hipStream_t s) {
  const unsigned gm = (unsigned)((g.M + QBM - 1) / QBM);
  if (narrow) {
    const dim3 grid(1, gm);
    if (bf) hipLaunchKernelGGL((gemm_bf16_kernel<32, true, QBK>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16_kernel<32, false, QBK>), grid, dim3(256), 0, s, g);
  } else {
    const dim3 grid((unsigned)((g.N + 127) / 128), gm);
    if (bf) hipLaunchKernelGGL((gemm_bf16_kernel<128, true, QBK>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16_kernel<128, false, QBK>), grid, dim3(256), 0, s, g);
  }
}

#ifndef MRL_GEMM_BF16_BK
#define MRL_GEMM_BF16_BK 64
#endif

// The one decision of which NN kernel takes a product: mrl_gemm_bf16 launches what it
// returns and mrl_gemm_bf16_route reports it.
// lds_limit: the tiled kernel only (the big, streaming and small-M kernels hold 100-132 KB
// of LDS per block, the first two for the whole product), with 32-deep K stages when the
// 64-deep ones do not fit the limit; every NN kernel sums each output's k-steps of 16 in
// the same order, so the results do not change
static int nn_route(const GemmB16Args& g, bool dual, int64_t lds_limit, BigPlan* big, StreamPlan* st) {
  const bool narrow = g.N <= 32;
  const int t64 = narrow ? MRL_GEMM_ROUTE_TILED32_BK64 : MRL_GEMM_ROUTE_TILED128_BK64;
  const int t32 = narrow ? MRL_GEMM_ROUTE_TILED32_BK32 : MRL_GEMM_ROUTE_TILED128_BK32;
  if (lds_limit > 0)
    return (int64_t)sizeof(bfr_t) * 2 * (QBM + (narrow ? 32 : 128)) * (64 + 8) <= lds_limit ? t64 : t32;
  if (big_gemm_plan(g, dual, big)) return MRL_GEMM_ROUTE_BIG;  // tall products: 256 x 256
  // small M (the Humanoid rollout's per-step layers): whole-K panels, 64 x 64 tiles
  if (!dual && g.M <= env_or("MRL_GEMM_SMALL_MAX_M", MRL_GEMM_SMALL_MAX_M) && g.K <= 4 * SQK && g.N >= 64 &&
      g.epi != MRL_GEMM_DTANH)
    return MRL_GEMM_ROUTE_SMALL;
  if (stream_gemm_plan(g, dual, st)) return st->kp == 384 ? MRL_GEMM_ROUTE_STREAM384 : MRL_GEMM_ROUTE_STREAM512;
  return MRL_GEMM_BF16_BK == 64 ? t64 : t32;
}

static GemmB16Args nn_args(const mrl_gemm_bf16_desc* d, const int32_t* skip) {
  return {d->m, d->n, d->k, d->a, d->bt, d->a2, d->bt2, d->lda, d->ldb,
          d->c, d->ldc, d->bias, d->h, d->ldh, d->epilogue, skip};
}

}  // namespace mrl

using namespace mrl;

extern "C" {

int32_t mrl_gemm_bf16_route(const mrl_gemm_bf16_desc* d) {
  if (!d) return MRL_GEMM_ROUTE_INVALID;
  if (d->m <= 0 || d->n <= 0) return MRL_GEMM_ROUTE_NONE;
  BigPlan big;
  StreamPlan st;
  return nn_route(nn_args(d, nullptr), d->a2 != nullptr, d->lds_limit, &big, &st);
}

int mrl_gemm_bf16(const mrl_gemm_bf16_desc* d, const int32_t* skip, void* stream) {
  if (!d || !d->a || !d->bt || !d->c) return fail(E_ARG, "mrl_gemm_bf16: null pointer");
  if ((d->a2 == nullptr) != (d->bt2 == nullptr)) return fail(E_ARG, "mrl_gemm_bf16: a2/bt2 must be both set or both null");
  if (d->epilogue < MRL_GEMM_STORE || d->epilogue > MRL_GEMM_DTANH) return fail(E_ARG, "mrl_gemm_bf16: bad epilogue");
  if (d->epilogue == MRL_GEMM_DTANH && !d->h) return fail(E_ARG, "mrl_gemm_bf16: DTANH needs h");
  if ((d->lda & 7) || (d->ldb & 7) || d->lda < d->k || d->ldb < d->k)
    return fail(E_ARG, "mrl_gemm_bf16: lda / ldb must be multiples of 8 and >= k (zero padding columns)");
  const uintptr_t al = reinterpret_cast<uintptr_t>(d->a) | reinterpret_cast<uintptr_t>(d->bt) |
                       reinterpret_cast<uintptr_t>(d->a2) | reinterpret_cast<uintptr_t>(d->bt2);
  if (al & 15) return fail(E_ARG, "mrl_gemm_bf16: operands must be 16-byte aligned");
  if (d->m <= 0 || d->n <= 0) return OK;
  const GemmB16Args g = nn_args(d, skip);
  hipStream_t s = (hipStream_t)stream;
  const bool bf = d->c_bf16 != 0, dual = d->a2 != nullptr;
  BigPlan big;
  StreamPlan st;
  switch (nn_route(g, dual, d->lds_limit, &big, &st)) {
    case MRL_GEMM_ROUTE_BIG: big_gemm_launch(g, bf, dual, big, s); break;
    case MRL_GEMM_ROUTE_SMALL: {
      const dim3 grid((unsigned)((g.N + SBN - 1) / SBN), (unsigned)((g.M + SBM - 1) / SBM));
      if (bf) hipLaunchKernelGGL((gemm_bf16_small_kernel<true>), grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_bf16_small_kernel<false>), grid, dim3(256), 0, s, g);
      break;
    }
    case MRL_GEMM_ROUTE_STREAM384:
    case MRL_GEMM_ROUTE_STREAM512: stream_gemm_launch(g, bf, st, s); break;
    case MRL_GEMM_ROUTE_TILED128_BK64: launch_tiled<64>(g, false, bf, s); break;
    case MRL_GEMM_ROUTE_TILED32_BK64: launch_tiled<64>(g, true, bf, s); break;
    case MRL_GEMM_ROUTE_TILED128_BK32: launch_tiled<32>(g, false, bf, s); break;
    default: launch_tiled<32>(g, true, bf, s); break;
  }
  return hip_check(hipGetLastError(), "mrl_gemm_bf16");
}

int mrl_cast_rows_bf16(const float* x, int64_t rows, int64_t cols, int64_t ldx, uint16_t* y, int64_t ldy,
                       void* stream) {
  if (!x || !y) return fail(E_ARG, "mrl_cast_rows_bf16: null pointer");
  if (ldy < cols) return fail(E_ARG, "mrl_cast_rows_bf16: ldy < cols");
  if (rows <= 0 || ldy <= 0) return OK;
  int64_t gsz = (rows * ldy + 255) / 256;
  if (gsz > 8192) gsz = 8192;
  hipLaunchKernelGGL(cast_rows_bf16_kernel, dim3((unsigned)gsz), dim3(256), 0, (hipStream_t)stream, x, rows, cols, ldx,
                     y, ldy);
  return hip_check(hipGetLastError(), "mrl_cast_rows_bf16");
}

int mrl_pack_w_bf16(const float* w, int64_t din, int64_t dout, int32_t transpose, uint16_t* out, int64_t ld,
                    void* stream) {
  if (!w || !out) return fail(E_ARG, "mrl_pack_w_bf16: null pointer");
  if (ld < (transpose ? din : dout)) return fail(E_ARG, "mrl_pack_w_bf16: ld too small");
  const int64_t total = (transpose ? dout : din) * ld;
  if (total <= 0) return OK;
  int64_t gsz = (total + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  hipLaunchKernelGGL(pack_w_bf16_kernel, dim3((unsigned)gsz), dim3(256), 0, (hipStream_t)stream, w, din, dout, transpose,
                     out, ld);
  return hip_check(hipGetLastError(), "mrl_pack_w_bf16");
}

}  // extern "C"
