// The device-resident conjugate-gradient solve of the TRPO update (trpo.py:104-122, `cg`
// of misc_utils.py) and the step scaling that follows it: one workgroup for n <= 65,536
// (plain and register-resident kernels, the latter also packing the next Fisher product's
// split tangent image), 256 blocks above.  All sums are fp64 in fixed orders, so every path
// is reproducible run to run.
#include <math.h>

#include "../../include/mrl_hip.h"
#include "block_reduce.h"
#include "mrl_common.h"
#include "fvp_split_role.h"

namespace mrl {

// ------------------------------------------------------------------ CG (one workgroup)
constexpr int CG_T = 1024;

// The sum of the block's CG_T values as the pairwise tree red[i] += red[i + o],
// o = CG_T/2 .. 1, adds them (the tree every CG kernel's results are defined by), in
// two barriers instead of eleven: wave 0 lane i gathers its 16 values v[i + 64 k] and
// adds them in the tree's cross-wave order (o = 512 .. 64: k with k + 8, k + 4, k + 2,
// k + 1), then o = 32 .. 1 as lane shuffles.  red: CG_T + 1 doubles (the result slot
// red[CG_T] is only written after the first barrier, so back-to-back sums need no third).
// (The shuffles take the default width, the wave: with an explicit 64 as the only width in
// the unit the compiler specialises the shuffle and emits another, equivalent, lane test.)
__device__ inline double block_sum(double v, double* red) {
  static_assert(CG_T == 1024, "the cross-wave tree below is CG_T = 16 x 64");
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x < 64) {
    const double* q = red + threadIdx.x;
    // b[k] = (v[k] + v[k + 8]) + (v[k + 4] + v[k + 12]) (in units of 64), one k at a time
    auto quad = [&](int k) { return (q[64 * k] + q[64 * (k + 8)]) + (q[64 * (k + 4)] + q[64 * (k + 12)]); };
    // (the fences keep the gathers one quad at a time: four doubles in flight, not
    // sixteen, beside the CG kernels' register-resident vectors)
    const double b0 = quad(0);
    asm volatile("" ::: "memory");
    const double c0 = b0 + quad(2);
    asm volatile("" ::: "memory");
    const double b1 = quad(1);
    asm volatile("" ::: "memory");
    double t = c0 + (b1 + quad(3));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    if (threadIdx.x == 0) red[CG_T] = t;
  }
  __syncthreads();
  return red[CG_T];
}

// The solver's scalars, written by one thread.  state = (r.r, p.z of the last update,
// updates done), flag[0] = converged (every later update returns at once).
__device__ inline void cg_state_init(double rdotr, double* state, int32_t* flag) {
  state[0] = rdotr;
  state[1] = 0.0;
  state[2] = 0.0;
  flag[0] = 0;
  flag[1] = 0;
}
__device__ inline void cg_state_update(double newr, double pz, double tol, double* state, int32_t* flag) {
  state[0] = newr;
  state[1] = pz;
  state[2] += 1.0;
  if (newr < tol) flag[0] = 1;
}

__global__ __launch_bounds__(CG_T) void cg_init_kernel(const double* __restrict__ b, int64_t n, double* x, double* r,
                                                       double* p, float* p32, double* ax, double* state,
                                                       int32_t* flag) {
  __shared__ double red[CG_T + 1];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    const double bi = b[i];
    x[i] = 0.0;
    if (ax) ax[i] = 0.0;
    r[i] = bi;
    p[i] = bi;
    p32[i] = (float)bi;
    s += bi * bi;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) cg_state_init(s, state, flag);
}

__global__ __launch_bounds__(CG_T) void cg_update_kernel(const float* __restrict__ fvp, double damping, double tol,
                                                         int64_t n, double* x, double* r, double* p, float* p32,
                                                         double* ax, double* state, int32_t* flag) {
  __shared__ double red[CG_T + 1];
  if (flag[0] != 0) return;
  const double rdotr = state[0];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    const double z = (double)fvp[i] + damping * p[i];
    s += p[i] * z;
  }
  const double pz = block_sum(s, red);
  const double v = rdotr / pz;
  s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    const double pi = p[i];
    const double z = (double)fvp[i] + damping * pi;
    x[i] += v * pi;
    if (ax) ax[i] += v * z;  // A x = sum_k v_k A p_k: the step scaling needs no extra Fisher product
    const double ri = r[i] - v * z;
    r[i] = ri;
    s += ri * ri;
  }
  const double newr = block_sum(s, red);
  const double mu = newr / rdotr;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    const double pi = r[i] + mu * p[i];
    p[i] = pi;
    p32[i] = (float)pi;
  }
  if (threadIdx.x == 0) cg_state_update(newr, pz, tol, state, flag);
}

// The same update with each thread's K-element slice of p / r / x / A x held in
// registers: every operand is loaded once, up front, instead of once per pass
// (three dependent global passes of the plain kernel).  Per-thread accumulation
// order and the block_sum tree are the plain kernel's, so the results are identical.
// PACK: the next Fisher product's tangent image too -- the split image of p32
// (split_image_item, as mlp_pack_split_kernel writes it), one launch instead of two
struct CgPack {
  MlpDims d;
  BDims b;
  float* image;
};

template <int K, bool PACK>
__device__ inline void cg_update_reg_body(const float* fvp, double damping, double tol, int64_t n, double* x,
                                          double* r, double* p, float* p32, double* ax, double* state, int32_t* flag,
                                          const CgPack& pk, double* red) {
  const double rdotr = state[0];
  // z = fvp + damping p is recomputed where it is used (the same value) from the f32 fvp
  // kept in registers: 8 VGPRs fewer than a double z, no spills at CG_T threads
  double pr[K], rr[K], xr[K], ar[K];
  float fr[K];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t i = threadIdx.x + (int64_t)k * CG_T;
    pr[k] = rr[k] = xr[k] = ar[k] = 0.0;
    fr[k] = 0.f;
    if (i < n) {
      const double pi = p[i];
      fr[k] = fvp[i];
      const double z = (double)fr[k] + damping * pi;
      pr[k] = pi;
      rr[k] = r[i];
      xr[k] = x[i];
      if (ax) ar[k] = ax[i];
      s += pi * z;
    }
  }
  const double pz = block_sum(s, red);
  const double v = rdotr / pz;
  s = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t i = threadIdx.x + (int64_t)k * CG_T;
    if (i < n) {
      const double z = (double)fr[k] + damping * pr[k];
      x[i] = xr[k] + v * pr[k];
      if (ax) ax[i] = ar[k] + v * z;
      const double ri = rr[k] - v * z;
      r[i] = ri;
      rr[k] = ri;
      s += ri * ri;
    }
  }
  const double newr = block_sum(s, red);
  const double mu = newr / rdotr;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t i = threadIdx.x + (int64_t)k * CG_T;
    if (i < n) {
      const double pi = rr[k] + mu * pr[k];
      p[i] = pi;
      p32[i] = (float)pi;
    }
  }
  if (threadIdx.x == 0) cg_state_update(newr, pz, tol, state, flag);
  if constexpr (PACK) {
    // the new p32 staged in LDS (8192 floats), read there by the image gathers
    __shared__ float sp[8 * CG_T];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[threadIdx.x + k * CG_T] = (float)(rr[k] + mu * pr[k]);
    __syncthreads();
    const int items = split_image_items(pk.b);
    for (int u = threadIdx.x; u < items; u += CG_T) split_image_item(pk.d, pk.b, sp, pk.image, u);
  }
}

template <int K, bool PACK = false>
__global__ __launch_bounds__(CG_T) void cg_update_reg_kernel(const float* __restrict__ fvp, double damping, double tol,
                                                             int64_t n, double* x, double* r, double* p, float* p32,
                                                             double* ax, double* state, int32_t* flag,
                                                             CgPack pk = CgPack{}) {
  __shared__ double red[CG_T + 1];
  if (flag[0] != 0) return;
  cg_update_reg_body<K, PACK>(fvp, damping, tol, n, x, r, p, p32, ax, state, flag, pk, red);
}


__global__ __launch_bounds__(CG_T) void trpo_step_kernel(const float* __restrict__ fvp, const double* __restrict__ x,
                                                         const float* __restrict__ g, double damping, double max_kl,
                                                         int64_t n, double* fullstep, double* out) {
  __shared__ double red[CG_T + 1];
  double s = 0.0, sg = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    s += x[i] * ((double)fvp[i] + damping * x[i]);
    sg += (double)g[i] * x[i];
  }
  const double xFx = block_sum(s, red);
  const double gx = block_sum(sg, red);
  const double shs = 0.5 * xFx;
  const double lm = sqrt(shs / max_kl);
  for (int64_t i = threadIdx.x; i < n; i += CG_T) fullstep[i] = x[i] / lm;
  if (threadIdx.x == 0) {
    out[0] = shs;
    out[1] = lm;
    out[2] = -gx;
    out[3] = -gx / lm;
  }
}

// same scaling from A x accumulated by the CG updates (A linear: A sum v_k p_k = sum v_k z_k)
__global__ __launch_bounds__(CG_T) void trpo_step_ax_kernel(const double* __restrict__ ax, const double* __restrict__ x,
                                                            const float* __restrict__ g, double max_kl, int64_t n,
                                                            double* fullstep, double* out) {
  __shared__ double red[CG_T + 1];
  double s = 0.0, sg = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_T) {
    s += x[i] * ax[i];
    sg += (double)g[i] * x[i];
  }
  const double xAx = block_sum(s, red);
  const double gx = block_sum(sg, red);
  const double shs = 0.5 * xAx;
  const double lm = sqrt(shs / max_kl);
  for (int64_t i = threadIdx.x; i < n; i += CG_T) fullstep[i] = x[i] / lm;
  if (threadIdx.x == 0) {
    out[0] = shs;
    out[1] = lm;
    out[2] = -gx;
    out[3] = -gx / lm;
  }
}

// ---- multi-block CG / step scaling for large n (wide nets: Humanoid P = 727,074).
// The single-block kernels above stream n fp64 elements through one CU (1.6 ms per
// CG update at P = 727 k); here each of CGB blocks owns one contiguous chunk, block
// partial sums go to a scratch area of `state` / `out` (mrl_cg_state_doubles), and
// every block reduces the CGB partials in the same fixed order, so all blocks derive
// bit-identical scalars.  The scalars and the flag are written by a 1-thread kernel
// after the last pass, so no block ever reads a value this update is writing.
constexpr int CGB = 256;                    // blocks of the multi-block passes
constexpr int CGB_T = 256;                  // threads per block
constexpr int64_t CG_SMALL_N = 65536;       // n at or below: the single-block kernels
constexpr int CG_SCALARS = 8;               // state[0..7]; partials from state[8]

__device__ inline void cg_chunk(int64_t n, int64_t& lo, int64_t& hi) {
  const int64_t chunk = ((n + CGB - 1) / CGB + CGB_T - 1) / CGB_T * CGB_T;
  lo = (int64_t)blockIdx.x * chunk;
  hi = min(n, lo + chunk);
}
__device__ inline double blk_sum(double v, double* red) {
  lds_tree_sum<CGB_T>(v, red);
  const double r = red[0];
  __syncthreads();
  return r;
}
// sum of the CGB partials part[0..CGB) in a fixed order (identical in every block)
__device__ inline double part_sum(const double* part, double* red) {
  return blk_sum(threadIdx.x < CGB ? part[threadIdx.x] : 0.0, red);
}

__global__ __launch_bounds__(CGB_T) void cgm_init_kernel(const double* __restrict__ b, int64_t n, double* x, double* r,
                                                          double* p, float* p32, double* ax, double* part) {
  __shared__ double red[CGB_T];
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) {
    const double bi = b[i];
    x[i] = 0.0;
    if (ax) ax[i] = 0.0;
    r[i] = bi;
    p[i] = bi;
    p32[i] = (float)bi;
    s += bi * bi;
  }
  s = blk_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(CGB_T) void cgm_init_final_kernel(double* state, int32_t* flag) {
  __shared__ double red[CGB_T];
  const double s = part_sum(state + CG_SCALARS, red);
  if (threadIdx.x == 0) cg_state_init(s, state, flag);
}
// pass 1: p.z partials
__global__ __launch_bounds__(CGB_T) void cgm_pz_kernel(const float* __restrict__ fvp, double damping, int64_t n,
                                                        const double* __restrict__ p, double* state,
                                                        const int32_t* flag) {
  __shared__ double red[CGB_T];
  if (flag[0] != 0) return;
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) s += p[i] * ((double)fvp[i] + damping * p[i]);
  s = blk_sum(s, red);
  if (threadIdx.x == 0) state[CG_SCALARS + blockIdx.x] = s;
}
// pass 2: v = rdotr / p.z; x += v p; ax += v z; r -= v z; r.r partials
__global__ __launch_bounds__(CGB_T) void cgm_xr_kernel(const float* __restrict__ fvp, double damping, int64_t n,
                                                        double* x, double* r, const double* __restrict__ p,
                                                        double* ax, double* state, const int32_t* flag) {
  __shared__ double red[CGB_T];
  if (flag[0] != 0) return;
  const double v = state[0] / part_sum(state + CG_SCALARS, red);
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) {
    const double pi = p[i];
    const double z = (double)fvp[i] + damping * pi;
    x[i] += v * pi;
    if (ax) ax[i] += v * z;
    const double ri = r[i] - v * z;
    r[i] = ri;
    s += ri * ri;
  }
  s = blk_sum(s, red);
  if (threadIdx.x == 0) state[CG_SCALARS + CGB + blockIdx.x] = s;
}
// pass 3: mu = r.r / rdotr; p = r + mu p
__global__ __launch_bounds__(CGB_T) void cgm_p_kernel(int64_t n, const double* __restrict__ r, double* p, float* p32,
                                                       const double* state, const int32_t* flag) {
  __shared__ double red[CGB_T];
  if (flag[0] != 0) return;
  const double mu = part_sum(state + CG_SCALARS + CGB, red) / state[0];
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) {
    const double pi = r[i] + mu * p[i];
    p[i] = pi;
    p32[i] = (float)pi;
  }
}
__global__ __launch_bounds__(CGB_T) void cgm_final_kernel(double tol, double* state, int32_t* flag) {
  __shared__ double red[CGB_T];
  if (flag[0] != 0) return;
  const double pz = part_sum(state + CG_SCALARS, red);
  const double newr = part_sum(state + CG_SCALARS + CGB, red);
  if (threadIdx.x == 0) cg_state_update(newr, pz, tol, state, flag);
}
// step scaling: x.ax and g.x partials, then every block derives shs / lm and writes its
// chunk of fullstep = x / lm (block 0 the scalars)
__global__ __launch_bounds__(CGB_T) void cgm_step_part_kernel(const double* __restrict__ ax,
                                                               const double* __restrict__ x, const float* __restrict__ g,
                                                               int64_t n, double* out) {
  __shared__ double red[CGB_T];
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  double s = 0.0, sg = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) {
    s += x[i] * ax[i];
    sg += (double)g[i] * x[i];
  }
  s = blk_sum(s, red);
  sg = blk_sum(sg, red);
  if (threadIdx.x == 0) {
    out[CG_SCALARS + blockIdx.x] = s;
    out[CG_SCALARS + CGB + blockIdx.x] = sg;
  }
}
__global__ __launch_bounds__(CGB_T) void cgm_step_kernel(const double* __restrict__ x, double max_kl, int64_t n,
                                                          double* fullstep, double* out) {
  __shared__ double red[CGB_T];
  const double xAx = part_sum(out + CG_SCALARS, red);
  const double gx = part_sum(out + CG_SCALARS + CGB, red);
  const double shs = 0.5 * xAx;
  const double lm = sqrt(shs / max_kl);
  int64_t lo, hi;
  cg_chunk(n, lo, hi);
  for (int64_t i = lo + threadIdx.x; i < hi; i += CGB_T) fullstep[i] = x[i] / lm;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = shs;
    out[1] = lm;
    out[2] = -gx;
    out[3] = -gx / lm;
  }
}

}  // namespace mrl

using namespace mrl;

extern "C" {

int64_t mrl_cg_state_doubles(int64_t n) { return n > CG_SMALL_N ? CG_SCALARS + 2 * CGB : 4; }

int mrl_cg_init(const double* b, int64_t n, double* x, double* r, double* p, float* p32, double* ax, double* state,
                int32_t* flag, void* stream) {
  if (!b || !x || !r || !p || !p32 || !state || !flag) return fail(E_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n > CG_SMALL_N) {
    hipLaunchKernelGGL(cgm_init_kernel, dim3(CGB), dim3(CGB_T), 0, s, b, n, x, r, p, p32, ax, state + CG_SCALARS);
    hipLaunchKernelGGL(cgm_init_final_kernel, dim3(1), dim3(CGB_T), 0, s, state, flag);
  } else {
    hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(CG_T), 0, s, b, n, x, r, p, p32, ax, state, flag);
  }
  return hip_check(hipGetLastError(), "mrl_cg_init");
}

int mrl_cg_update(const float* fvp, double damping, double residual_tol, int64_t n, double* x, double* r, double* p,
                  float* p32, double* ax, double* state, int32_t* flag, void* stream) {
  if (!fvp || !x || !r || !p || !p32 || !state || !flag) return fail(E_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n > CG_SMALL_N) {
    hipLaunchKernelGGL(cgm_pz_kernel, dim3(CGB), dim3(CGB_T), 0, s, fvp, damping, n, p, state, flag);
    hipLaunchKernelGGL(cgm_xr_kernel, dim3(CGB), dim3(CGB_T), 0, s, fvp, damping, n, x, r, p, ax, state, flag);
    hipLaunchKernelGGL(cgm_p_kernel, dim3(CGB), dim3(CGB_T), 0, s, n, r, p, p32, state, flag);
    hipLaunchKernelGGL(cgm_final_kernel, dim3(1), dim3(CGB_T), 0, s, residual_tol, state, flag);
  } else if (n <= 8 * CG_T) {  // the slices stay in registers
    hipLaunchKernelGGL(cg_update_reg_kernel<8>, dim3(1), dim3(CG_T), 0, s, fvp, damping, residual_tol, n, x, r, p,
                       p32, ax, state, flag);
  } else {
    hipLaunchKernelGGL(cg_update_kernel, dim3(1), dim3(CG_T), 0, s, fvp, damping, residual_tol, n, x, r, p, p32, ax,
                       state, flag);
  }
  return hip_check(hipGetLastError(), "mrl_cg_update");
}

int mrl_cg_update_pack(const float* fvp, double damping, double residual_tol, int64_t n, double* x, double* r,
                       double* p, float* p32, double* ax, double* state, int32_t* flag, const mrl_mlp_desc* d,
                       float* image_t, void* stream) {
  if (!fvp || !x || !r || !p || !p32 || !state || !flag || !d || !image_t) return fail(E_ARG, "null pointer");
  if (!(n <= CG_SMALL_N && n <= 8 * CG_T))
    return fail(E_UNSUPPORTED, "mrl_cg_update_pack: the single-block register CG update only (n <= 8192)");
  const int64_t words = mrl_mlp_image_words_split(d);
  if (words < 0) return fail(E_UNSUPPORTED, "mrl_cg_update_pack: no split image for this net");
  if (mrl_mlp_num_params(d) != n) return fail(E_ARG, "mrl_cg_update_pack: n is not the net's parameter count");
  CgPack pk;
  pk.d = mlp_dims(d->n_in, d->n_out, d->head == MRL_HEAD_GAUSS);
  pk.b = bf16_dims(d->n_in, d->n_out);
  pk.image = image_t;
  hipLaunchKernelGGL((cg_update_reg_kernel<8, true>), dim3(1), dim3(CG_T), 0, (hipStream_t)stream, fvp, damping,
                     residual_tol, n, x, r, p, p32, ax, state, flag, pk);
  return hip_check(hipGetLastError(), "mrl_cg_update_pack");
}

int mrl_trpo_step(const float* fvp, const double* x, const float* g, double damping, double max_kl, int64_t n,
                  double* fullstep, double* out, void* stream) {
  if (!fvp || !x || !g || !fullstep || !out) return fail(E_ARG, "null pointer");
  hipLaunchKernelGGL(trpo_step_kernel, dim3(1), dim3(CG_T), 0, (hipStream_t)stream, fvp, x, g, damping, max_kl, n,
                     fullstep, out);
  return hip_check(hipGetLastError(), "mrl_trpo_step");
}

int mrl_trpo_step_ax(const double* ax, const double* x, const float* g, double max_kl, int64_t n, double* fullstep,
                     double* out, void* stream) {
  if (!ax || !x || !g || !fullstep || !out) return fail(E_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n > CG_SMALL_N) {
    hipLaunchKernelGGL(cgm_step_part_kernel, dim3(CGB), dim3(CGB_T), 0, s, ax, x, g, n, out);
    hipLaunchKernelGGL(cgm_step_kernel, dim3(CGB), dim3(CGB_T), 0, s, x, max_kl, n, fullstep, out);
  } else {
    hipLaunchKernelGGL(trpo_step_ax_kernel, dim3(1), dim3(CG_T), 0, s, ax, x, g, max_kl, n, fullstep, out);
  }
  return hip_check(hipGetLastError(), "mrl_trpo_step_ax");
}

}  // extern "C"
