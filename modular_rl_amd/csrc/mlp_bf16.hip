// bf16 throughput mode of the fused 64-wide MLP kernels (MRL_COMPUTE_BF16): the same
// passes as the f32 kernels of mlp_rows_vjp.hip (forward + row epilogues, Fisher-product
// JVP, VJP) on v_mfma_f32_32x32x16_bf16 -- 16x the f32 MFMA rate -- with f32 accumulation.
// The tile forward / JVP and the activation cache are in mlp_bf16_device.h.  The rows and
// the VJP kernels share this unit on purpose: the uncached VJP recomputes the forward with
// the rows kernel's forward_b, and hipcc's inlining of it -- and with it the schedule and
// register allocation of mlp_vjp_bf16_kernel<false, 0> -- depends on its other callers in
// the unit (in a unit of its own that kernel's code changed), as in mlp_rows_vjp.hip.
//
// Rounding points (bf16 RNE): the weights W0, W1 (and the tangent's dW0, dW1), the
// layer inputs x, h1, h2 and the backpropagated head rows / layer-2 gradients that
// enter an MFMA.  Biases, tanh, tanh', the head layer (n_out <= 8, f32 VALU on the
// bf16-rounded h2) and every row epilogue stay f32.  fp32 (mlp_rows_vjp.hip) is the
// parity dtype; this mode is checked against the fp64 oracle at a bf16 bound
// (tests/test_gpu_bf16.py).
//
// Layouts.  A 32-row tile keeps activations transposed in the accumulators exactly as
// the f32 kernels do ("F layout", D[unit][row]: row on the lane, 16 units in the
// registers, unit = 32*mt + cperm(r, h)); the C/D layout of the bf16 MFMA is the f32
// one.  Registers 8s'..8s'+7 of a tile, converted to bf16, are the B fragment of a
// k-step whose k index j of lane half h is unit cperm(8s' + j, h): layers chain with
// no data movement, the weight fragments of the image are permuted to match.
// The weight gradients sum over rows (the lane index of an F tile), so the VJP turns
// F tiles into "T layout" tiles D[row][unit] (unit on the lane, rows in the
// registers) with an identity MFMA (X^T . I: exact, the values are bf16 already) and
// feeds T tiles as both operands of X^T . Y -- no LDS transposes at all.
//
// Replaces the same reference functions as mlp_kernels.hip (core.py:269-270,
// trpo.py:68-70, core.py:608, 670-671) in reduced precision.
#include <math.h>
#include <stdlib.h>

#include "mlp_bf16_device.h"
#include "mlp_host.h"

namespace mrl {

__global__ void mlp_pack_bf16_kernel(MlpDims d, BDims b, const float* __restrict__ th, float* __restrict__ image,
                                     int words, const int32_t* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  if (w < b.fa0) {
    // f32 section: the f32 image's element at the same segment-relative position
    int idx;
    if (w < b.fb1) idx = d.fb0 + (w - b.fb0);
    else if (w < b.hv) idx = d.fb1 + (w - b.fb1);
    else if (w < b.hb) idx = d.hv + (w - b.hv);
    else idx = d.hb + (w - b.hb);
    image[w] = image_value(d, th, idx);
    return;
  }
  int seg, rel;
  if (w < b.fa1) { seg = 0; rel = w - b.fa0; }
  else if (w < b.bw2) { seg = 1; rel = w - b.fa1; }
  else if (w < b.bt1) { seg = 2; rel = w - b.bw2; }
  else { seg = 3; rel = w - b.bt1; }
  const int frag = rel >> 2, q = rel & 3;
  const __bf16 lo = (__bf16)bimage_elem(d, b, th, seg, frag, 2 * q);
  const __bf16 hi = (__bf16)bimage_elem(d, b, th, seg, frag, 2 * q + 1);
  const uint32_t v = (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
  image[w] = __uint_as_float(v);
}

constexpr int ROWS_BLOCK_B = 256;
constexpr int ROWS_MAX_BLOCKS_B = 3072;

// waves per SIMD the row kernels are compiled for: 3 (168 VGPRs) for the cached FVP pass
// of the static shapes -- it waits on memory for half its wave time and a third wave
// hides some of it (CartPole 0.313 -> 0.265 ms, Hopper 0.353 -> 0.286 ms at 4.19 M
// rows; Hopper's spills 16 bytes a lane) -- 2 for the others (the loss / gradient passes
// measured level or slower at 3; the run-time shape and the uncached FVP pass spill).
// Measured and not kept: the PROB / LOSSES / SURRGRAD passes of the static
// shapes at 4 waves.
template <int EPI_K, int SH>
constexpr int rows_b_occ() {
  return ((SH & ~SH_TIME) != 0 && EPI_K == EPI_FVP_CACHED) ? 3 : 2;
}

template <int EPI_K, int SH>
__global__ __launch_bounds__(ROWS_BLOCK_B, (rows_b_occ<EPI_K, SH>())) void mlp_rows_bf16_kernel(RowsArgs a, BDims b,
                                                                       const float* __restrict__ img_g,
                                                                       const float* __restrict__ imt_g,
                                                                       const int32_t* __restrict__ skip) {
  rows_shape<SH>(a, b);
  constexpr bool CACHED = EPI_K == EPI_FVP_CACHED;
  constexpr int EPI = CACHED ? MRL_EPI_FVP : EPI_K;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (skip != nullptr && *skip != 0) return;
  const int fw = b.fwd_words;
  for (int i = threadIdx.x; i < fw / 4; i += ROWS_BLOCK_B)
    reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(img_g)[i];
  if (EPI == MRL_EPI_FVP)
    for (int i = threadIdx.x; i < fw / 4; i += ROWS_BLOCK_B)
      reinterpret_cast<float4*>(lds + fw)[i] = reinterpret_cast<const float4*>(imt_g)[i];
  __syncthreads();
  const float* img = lds;
  const float* imt = lds + fw;
  const MlpDims dd = head_dims(a.d, b);
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
    XGlobalNB xl{a.x, a.ept, a.ts_limit, a.n_obs, row, valid};
    float z[MAX_OUT], dz[MAX_OUT];
    float* ctile = a.cache != nullptr ? a.cache + tile * BCACHE_TILE_WORDS : nullptr;
    bf16x8 h1b[4], h2b[4];
    if constexpr (EPI == MRL_EPI_FVP) {
      if (CACHED) {
        bcache_load(ctile, 0, lane, h1b);
        bcache_load(ctile, 1, lane, h2b);
      } else {
        forward_b(img, dd, b, xl, lane, h1b, h2b, z);
      }
      jvp_b(img, imt, dd, b, xl, lane, h1b, h2b, z, dz, CACHED && a.head != MRL_HEAD_GAUSS);
    } else {
      forward_b(img, dd, b, xl, lane, h1b, h2b, z);
      if (a.cache_mode == MRL_CACHE_WRITE && ctile != nullptr) {
        bcache_store(ctile, 0, lane, h1b);
        bcache_store(ctile, 1, lane, h2b);
      }
#pragma unroll
      for (int o = 0; o < MAX_OUT; ++o) dz[o] = 0.f;
    }
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

// ------------------------------------------------------------------ VJP
struct VjpArgsB {
  MlpDims d;
  BDims b;
  int n_obs, gh, n_sum;
  const float* x;
  const int32_t* ept;
  double ts_limit;
  int64_t n;
  const float* ghead;
  float* slab;
  const float* cache;
};

// T tile of F tile mt from its fragments: D[row][unit] = sum over the two k-steps
__device__ inline f32x16 transpose_f(const bf16x8* fr, int mt, const bf16x8* ip) {
  f32x16 t = zero16();
  t = MFMA32B(fr[2 * mt], ip[0], t);
  t = MFMA32B(fr[2 * mt + 1], ip[1], t);
  return t;
}

typedef uint32_t vu4 __attribute__((ext_vector_type(4)));  // a 16-B register quad (asm operands)

// SH != 0: a static shape of mlp_layout.h (plain rows), every dimension a constant
template <int SH>
__device__ inline VjpArgsB vjp_shape_b(const VjpArgsB& in) {
  VjpArgsB a = in;
  if constexpr (SH != 0) {
    constexpr StaticShape S = STATIC_SHAPES[SH];
    a.d = static_dims(SH);
    a.b = bf16_dims(S.O, S.A);
    a.n_obs = S.O;
    a.n_sum = S.head == MRL_HEAD_GAUSS ? S.A : 0;
    a.gh = S.A + a.n_sum;
    a.ept = nullptr;
  }
  return a;
}

// Weight-gradient accumulators per wave (128 registers, in AGPRs: one wave per SIMD),
// written as one slab row per wave (reduced in fixed order by mrl_reduce_rows_f32).
template <bool CACHED, int SH>
__global__ __launch_bounds__(256, 1) void mlp_vjp_bf16_kernel(VjpArgsB a_in, const float* __restrict__ img_g,
                                                             const int32_t* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // the staged cache tiles of the next tile pair (PF), 16 KB per wave
  __shared__ __attribute__((aligned(16))) bf16x8 vjp_stage[(CACHED && SH != 0) ? 4 * 2 * 2 * 4 * 64 : 1];
  if (skip != nullptr && *skip != 0) return;
  const VjpArgsB a = vjp_shape_b<SH>(a_in);
  const MlpDims& d = a.d;
  const BDims& b = a.b;
  for (int i = threadIdx.x; i < b.total_words / 4; i += 256)
    reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(img_g)[i];
  __syncthreads();
  const float* img = lds;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j32 = lane & 31;
  const int A = d.A;
  const bf16x8 ip[2] = {ident_perm(0, lane), ident_perm(1, lane)};

  f32x16 gW2[2], gW1[2][2], gW0[2];  // T-tile products: [u2][o], [u1][u2], [in][u1]
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    gW2[m] = zero16();
    gW0[m] = zero16();
#pragma unroll
    for (int n = 0; n < 2; ++n) gW1[m][n] = zero16();
  }
  float gb0[2] = {0.f, 0.f}, gb1[2] = {0.f, 0.f};  // per lane = unit, this half's rows
  float gb2[MAX_OUT], gls[MAX_OUT];
#pragma unroll
  for (int o = 0; o < MAX_OUT; ++o) {
    gb2[o] = 0.f;
    gls[o] = 0.f;
  }

  // Two tiles per iteration, phase by phase: the MFMA -> VALU -> MFMA dependency chain of
  // one tile (gh2 -> tanh' -> transpose -> weight-gradient products) issues between the
  // steps of the other's, so one wave per SIMD still overlaps MFMA latency.  A second tile
  // past the batch is a clamped copy of the last one with every head row masked to zero:
  // all its contributions vanish.
  const int64_t ntiles = (a.n + 31) / 32;
  const int64_t stride = (int64_t)gridDim.x * 4;
  // PF (the cached static-shape kernels, one wave per SIMD): the cache tiles of the next
  // tile pair are staged by LDS-DMA into this wave's own 16 KB of vjp_stage while this
  // pair computes (no registers held across the loop, no barrier: a wave reads only what
  // it staged); read back by inline-asm ds_reads, which the compiler's LDS-DMA alias
  // tracking cannot turn into vmcnt(0) drains in front of the image reads.
  constexpr bool PF = CACHED && SH != 0;
  auto tile_of = [&](int64_t t0, int u) {
    const int64_t tu = t0 + u * stride;
    return tu < ntiles ? tu : ntiles - 1;
  };
  bf16x8* const stg = vjp_stage + wave * (2 * 2 * 4 * 64);  // [u][layer][s][lane]
  auto dma_pair = [&](int64_t t0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(a.cache + tile_of(t0, u) * BCACHE_TILE_WORDS);
#pragma unroll
      for (int f = 0; f < 8; ++f)  // f = layer * 4 + s
        __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + f * 64 + lane),
                                         (__attribute__((address_space(3))) void*)(stg + (u * 8 + f) * 64), 16, 0, 0);
    }
  };
  // the pair's input and head rows: every load unconditional from a clamped address
  // (static n_obs / A / n_sum), issued together one pair ahead, validity applied as 0 / 1
  // factors at use (a select on a loaded value becomes a branch and a vmcnt(0) drain)
  float xr[2][8 * MAX_KS0B], gr_[2][8], glr[2][MAX_OUT];
  auto load_rows = [&](int64_t t0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t row = tile_of(t0, u) * 32 + j32;
      const int64_t rc = row < a.n ? row : 0;
      const float* xp = a.x + rc * a.n_obs;
#pragma unroll
      for (int s0 = 0; s0 < MAX_KS0B; ++s0)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int k = 16 * s0 + 8 * h + jj;
          xr[u][8 * s0 + jj] = s0 < b.KS0B ? xp[k < a.n_obs ? k : a.n_obs - 1] : 0.f;
        }
      const float* gp = a.ghead + rc * a.gh;
#pragma unroll
      for (int o = 0; o < 8; ++o) gr_[u][o] = gp[o < A ? o : A - 1];
#pragma unroll
      for (int q = 0; q < MAX_OUT; ++q) glr[u][q] = q < a.n_sum ? gp[A + q] : 0.f;
    }
  };
  if constexpr (PF) {
    const int64_t t0 = (int64_t)blockIdx.x * 4 + wave;
    if (t0 < ntiles) {
      load_rows(t0);
      dma_pair(t0);
    }
  }
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += 2 * stride) {
    bf16x8 h1b[2][4], h2b[2][4], gB[2], xb[2][MAX_KS0B];
    bool live[2];
    if constexpr (PF) {
      // this pair's staged tiles: own DMA landed -> registers -> the next pair's DMA
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t base = (uint32_t)reinterpret_cast<uintptr_t>(stg) + 16 * lane;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) {
          vu4 v1, v2;
          asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v1) : "v"(base), "i"(((u * 8 + sI) * 64) * 16));
          asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v2) : "v"(base), "i"(((u * 8 + 4 + sI) * 64) * 16));
          h1b[u][sI] = __builtin_bit_cast(bf16x8, v1);
          h2b[u][sI] = __builtin_bit_cast(bf16x8, v2);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h1b[0][0]), "+v"(h1b[0][1]), "+v"(h1b[0][2]), "+v"(h1b[0][3]),
                   "+v"(h1b[1][0]), "+v"(h1b[1][1]), "+v"(h1b[1][2]), "+v"(h1b[1][3]), "+v"(h2b[0][0]),
                   "+v"(h2b[0][1]), "+v"(h2b[0][2]), "+v"(h2b[0][3]), "+v"(h2b[1][0]), "+v"(h2b[1][1]),
                   "+v"(h2b[1][2]), "+v"(h2b[1][3])::"memory");
    }
    if constexpr (PF) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t tu = tile + u * stride;
        live[u] = tu < ntiles;
        const int64_t row = (live[u] ? tu : ntiles - 1) * 32 + j32;
        float fv = (live[u] && row < a.n && h == 0) ? 1.f : 0.f, fx = row < a.n ? 1.f : 0.f;
        asm volatile("" : "+v"(fv), "+v"(fx));
#pragma unroll
        for (int o = 0; o < 8; ++o) {
          const float g = o < A ? gr_[u][o] * fv : 0.f;
          gb2[o] += g;
          gB[u][o] = (__bf16)g;
        }
#pragma unroll
        for (int q = 0; q < MAX_OUT; ++q) gls[q] += q < a.n_sum ? glr[u][q] * fv : 0.f;
#pragma unroll
        for (int s0 = 0; s0 < MAX_KS0B; ++s0)
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const int k = 16 * s0 + 8 * h + jj;
            xb[u][s0][jj] = (__bf16)((s0 < b.KS0B && k < a.n_obs) ? xr[u][8 * s0 + jj] * fx : 0.f);
          }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if constexpr (PF) break;
      const int64_t tu = tile + u * stride;
      live[u] = tu < ntiles;
      const int64_t tc = live[u] ? tu : ntiles - 1;
      const int64_t row = tc * 32 + j32;
      const bool valid = live[u] && row < a.n;
      XGlobalNB xl{a.x, a.ept, a.ts_limit, a.n_obs, row, row < a.n};
      if constexpr (CACHED) {
        bcache_load(a.cache + tc * BCACHE_TILE_WORDS, 1, lane, h2b[u]);
        bcache_load(a.cache + tc * BCACHE_TILE_WORDS, 0, lane, h1b[u]);
      } else {
        float zz[MAX_OUT];
        forward_b(img, head_dims(d, b), b, xl, lane, h1b[u], h2b[u], zz);
      }
#pragma unroll
      for (int s0 = 0; s0 < MAX_KS0B; ++s0) xb[u][s0] = s0 < b.KS0B ? x_frag(xl, s0, h) : bf16x8{};
      // head-gradient row (f32) and its bf16 operand: o = 8h + j (h = 1: zero, A <= 8)
      const float* gr = a.ghead + (row < a.n ? row : 0) * a.gh;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float g = (valid && h == 0 && o < A) ? gr[o] : 0.f;
        gb2[o] += g;
        gB[u][o] = (__bf16)g;
      }
#pragma unroll
      for (int q = 0; q < MAX_OUT; ++q) gls[q] += (valid && h == 0 && q < a.n_sum) ? gr[A + q] : 0.f;
    }
    if constexpr (PF) {  // the next pair's rows and cache tiles, under this pair's MFMAs
      if (tile + 2 * stride < ntiles) {
        load_rows(tile + 2 * stride);
        dma_pair(tile + 2 * stride);
      }
    }
    // gh2 = W2 . G (F layout), ga2 = gh2 (1 - h2^2)
    bf16x8 ga2b[2][4];
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) {
      f32x16 g2[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) g2[u] = MFMA32B(frag_at(img, b.bw2, mo, lane), gB[u], zero16());
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f32x16 h2 = unpack16(h2b[u], mo);
#pragma unroll
        for (int r = 0; r < 16; ++r) g2[u][r] *= dtanh(h2[r]);
        ga2b[u][2 * mo] = pack8(g2[u], 0);
        ga2b[u][2 * mo + 1] = pack8(g2[u], 1);
      }
    }
    // gW2 += H2^T G
    {
      f32x16 gT[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) gT[u] = MFMA32B(gB[u], ident_nat(0, lane), zero16());  // D[row][o]
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        f32x16 h2T[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) h2T[u] = transpose_f(h2b[u], m, ip);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          gW2[m] = MFMA32B(pack8(h2T[u], 0), pack8(gT[u], 0), gW2[m]);
          gW2[m] = MFMA32B(pack8(h2T[u], 1), pack8(gT[u], 1), gW2[m]);
        }
      }
    }
    // ga2 and the inputs in T layout
    bf16x8 ga2T[2][2][2], xT[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      f32x16 t[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) t[u] = transpose_f(ga2b[u], m, ip);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) gb1[m] += t[u][r];
        ga2T[u][m][0] = pack8(t[u], 0);
        ga2T[u][m][1] = pack8(t[u], 1);
      }
    }
    {
      f32x16 t[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        t[u] = zero16();
#pragma unroll
        for (int s0 = 0; s0 < MAX_KS0B; ++s0)
          if (s0 < b.KS0B) t[u] = MFMA32B(xb[u][s0], ident_nat(16 * s0, lane), t[u]);  // D[row][in]
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        xT[u][0] = pack8(t[u], 0);
        xT[u][1] = pack8(t[u], 1);
      }
    }
    // per u1 tile: gh1 (T layout) = ga2^T . W1^T, ga1 = gh1 (1 - h1^2), then
    // gW1 += H1^T GA2 and gW0 += X^T GA1
#pragma unroll
    for (int no = 0; no < 2; ++no) {
      f32x16 ga1[2], h1T[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) ga1[u] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) ga1[u] = MFMA32B(ga2b[u][s], frag_at(img, b.bt1, no * 4 + s, lane), ga1[u]);
#pragma unroll
      for (int u = 0; u < 2; ++u) h1T[u] = transpose_f(h1b[u], no, ip);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ga1[u][r] *= dtanh(h1T[u][r]);
          gb0[no] += ga1[u][r];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const bf16x8 h1p = pack8(h1T[u], sp);
          gW1[no][0] = MFMA32B(h1p, ga2T[u][0][sp], gW1[no][0]);
          gW1[no][1] = MFMA32B(h1p, ga2T[u][1][sp], gW1[no][1]);
          gW0[no] = MFMA32B(xT[u][sp], pack8(ga1[u], sp), gW0[no]);
        }
    }
    (void)live;
  }

  // per-wave partial gradient in flat theta layout; accumulator tiles are D[i][j] with
  // j = lane & 31 and i = cperm(r, h)
  float* out = a.slab + ((int64_t)blockIdx.x * 4 + wave) * d.P;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = cperm(r, h);
      if (i < d.O) out[d.tW0 + i * HID + 32 * m + j32] = gW0[m][r];
      if (j32 < A) out[d.tW2 + (32 * m + i) * A + j32] = gW2[m][r];
#pragma unroll
      for (int n = 0; n < 2; ++n) out[d.tW1 + (32 * m + i) * HID + 32 * n + j32] = gW1[m][n][r];
    }
  // bias sums: this half's rows, then the other half's (lanes l, l ^ 32 hold one unit)
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float s0 = xor32_add(gb0[m]);
    const float s1 = xor32_add(gb1[m]);
    if (h == 0) {
      out[d.tb0 + 32 * m + j32] = s0;
      out[d.tb1 + 32 * m + j32] = s1;
    }
  }
#pragma unroll
  for (int o = 0; o < MAX_OUT; ++o) {
    const float sum = wave_sumf(gb2[o]);
    if (lane == 0 && o < A) out[d.tb2 + o] = sum;
  }
  for (int q = 0; q < a.n_sum; ++q) {
    const float sum = wave_sumf(gls[q]);
    if (lane == 0) out[d.tls + q] = sum;
  }
}

static void launch_vjp_bf16(const mrl_mlp_desc* d, const float* image, const float* x, const int32_t* ep_t, double ts_limit,
                     const float* ghead, int64_t n, float* slab, const float* act_cache, int64_t blocks,
                     const int32_t* skip, hipStream_t s) {
  VjpArgsB a = vjp_args<VjpArgsB>(d, x, ep_t, ts_limit, ghead, n, slab, act_cache);
  a.b = bf16_dims(d->n_in, d->n_out);
  const size_t shm = (size_t)a.b.total_words * 4;
  const dim3 grid(blocks), blk(256);
  // the benchmark policies and value nets as static shapes (plain rows only: the VF
  // fit reads its materialised [obs, t / limit] rows; a time feature built from ep_t
  // takes the generic kernel, which spills at the VF's shape)
  with_bool(act_cache != nullptr, [&](auto cached) {
    with_static_shape<SH_POLICY | SH_VALUE>(static_shape_of(d, ep_t != nullptr), [&](auto shape) {
      hipLaunchKernelGGL((mlp_vjp_bf16_kernel<decltype(cached)::value, decltype(shape)::value>), grid, blk, shm, s, a,
                         image, skip);
    });
  });
}

}  // namespace mrl

using namespace mrl;

// Grid caps, swept with tools/fvp_probe.py at 4.19 M rows (MRL_ROWS_BF16_BLOCKS
// overrides both): the Fisher-product JVP (154 VGPRs: 3 blocks per CU) is fastest at
// exactly one resident round (768: 0.347 ms; 1024: 0.47, 1536: 0.356, 2048: 0.395);
// the forward passes (≤ 128 VGPRs) at three rounds and more (3072: surrgrad 0.526,
// prob 0.299 ms; 2048: 0.538 / 0.303).
constexpr int ROWS_FVP_BLOCKS_B = 768;
// caps per 256 CUs, scaled by the desc's `cus` (mlp_host.h)
static int64_t rows_blocks_b(int64_t n, bool fvp = false, int64_t cus = 256) {
  static const int64_t env_cap = [] {
    const char* e = getenv("MRL_ROWS_BF16_BLOCKS");
    return (int64_t)(e ? atoi(e) : 0);
  }();
  return grid_blocks(n, env_cap > 0 ? env_cap : scaled_cap(fvp ? ROWS_FVP_BLOCKS_B : ROWS_MAX_BLOCKS_B, cus));
}
constexpr int VJP_MAX_BLOCKS_B = 256;  // one block (4 waves) per CU at one wave per SIMD
static int64_t vjp_blocks_b(int64_t n, int64_t cus = 256) { return grid_blocks(n, scaled_cap(VJP_MAX_BLOCKS_B, cus)); }

extern "C" {

int64_t mrl_mlp_image_words_bf16(const mrl_mlp_desc* d) {
  if (check_desc(d) != OK) return -1;
  return bf16_dims(d->n_in, d->n_out).total_words;
}
int64_t mrl_act_cache_words_bf16(int64_t n) { return ceil_div(n, 32) * BCACHE_TILE_WORDS; }
int64_t mrl_partial_rows_bf16(int64_t n) { return rows_blocks_b(n) * 4; }
int64_t mrl_slab_rows_bf16(int64_t n) { return vjp_blocks_b(n) * 4; }
int64_t mrl_mlp_partial_rows_bf16(const mrl_mlp_desc* d, int64_t n) {
  if (check_desc(d) != OK) return -1;
  return rows_blocks_b(n, false, desc_cus(d)) * 4;
}
int64_t mrl_mlp_slab_rows_bf16(const mrl_mlp_desc* d, int64_t n) {
  if (check_desc(d) != OK) return -1;
  return vjp_blocks_b(n, desc_cus(d)) * 4;
}

int mrl_mlp_pack_bf16(const mrl_mlp_desc* d, const float* theta, float* image, int32_t fwd_only,
                      const int32_t* skip, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!theta || !image) return fail(E_ARG, "null pointer");
  const MlpDims m = mlp_dims(d->n_in, d->n_out, d->head == MRL_HEAD_GAUSS);
  const BDims b = bf16_dims(d->n_in, d->n_out);
  const int words = fwd_only ? b.fwd_words : b.total_words;
  hipLaunchKernelGGL(mlp_pack_bf16_kernel, dim3((words + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, b, theta,
                     image, words, skip);
  return hip_check(hipGetLastError(), "mrl_mlp_pack_bf16");
}

int mrl_mlp_rows_bf16(const mrl_mlp_desc* d, int32_t epi, const float* theta, const float* image,
                      const float* tangent, const float* image_t, const mrl_rows_io* io, const int32_t* skip,
                      void* stream) {
  RowsArgs a;
  int rc = rows_args(d, epi, theta, image, tangent, image_t, io, a);
  if (rc) return rc > 0 ? OK : rc;
  const BDims b = bf16_dims(d->n_in, d->n_out);
  const size_t shm = (size_t)b.fwd_words * 4 * (epi == MRL_EPI_FVP ? 2 : 1);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(epi == MRL_EPI_PPOSGD ? 1 : rows_blocks_b(io->n, epi == MRL_EPI_FVP, io->partial != nullptr ? desc_cus(d) : 256)),
      blk(ROWS_BLOCK_B);
  const int sh = static_shape_of(d, io->ep_t != nullptr, epi == MRL_EPI_PROB);
  with_rows_epilogue(epi, a.cache_mode, [&](auto ek) {
    constexpr int EK = decltype(ek)::value;
    with_rows_shape<EK>(sh, [&](auto shape) {
      hipLaunchKernelGGL((mlp_rows_bf16_kernel<EK, decltype(shape)::value>), grid, blk, shm, s, a, b, image, image_t, skip);
    });
  });
  return hip_check(hipGetLastError(), "mrl_mlp_rows_bf16");
}

int mrl_mlp_vjp_bf16(const mrl_mlp_desc* d, const float* image, const float* x, const int32_t* ep_t, double ts_limit,
                     const float* ghead, int64_t n, float* slab, const float* act_cache, const int32_t* skip,
                     void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!image || !x || !ghead || !slab) return fail(E_ARG, "null pointer");
  if ((rc = check_time_feature(d, ep_t)) != OK) return rc;
  if (n <= 0) return OK;
  launch_vjp_bf16(d, image, x, ep_t, ts_limit, ghead, n, slab, act_cache, vjp_blocks_b(n, desc_cus(d)), skip,
                  (hipStream_t)stream);
  return hip_check(hipGetLastError(), "mrl_mlp_vjp_bf16");
}

}  // extern "C"
