// The flat-vector layer: column sums of a slab (the fixed-order reductions of per-wave
// partial rows and split-K slabs) and the elementwise kernels of the update -- axpy-cast,
// line-search candidates, Adam, row gather, cast-scale.
#include <math.h>

#include "../../include/mrl_hip.h"
#include "block_reduce.h"
#include "mrl_common.h"
#include "vector_host.h"

namespace mrl {

// ------------------------------------------------------------------ slab reductions
// RG row groups of 64 columns per block (blockDim = 64 * RG); group g sums rows
// g, g + RG, ... with 8 independent accumulators (8 loads in flight per lane), then
// the RG group sums are added in a fixed pairwise order
template <class T, class O, int RG = 4>
__global__ void reduce_rows_kernel(const T* __restrict__ slab, int64_t rows, int64_t cols, O* __restrict__ out,
                                   const int32_t* __restrict__ skip) {
  __shared__ double part[RG][64];
  if (skip != nullptr && *skip != 0) return;
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + c;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (col < cols) {
    int64_t r = g;
    for (; r + 7 * RG < rows; r += 8 * RG) {
#pragma unroll
      for (int q = 0; q < 8; ++q) s[q] += (double)slab[(r + RG * q) * cols + col];
    }
    for (; r < rows; r += RG) s[0] += (double)slab[r * cols + col];
  }
  part[g][c] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if constexpr (RG == 4) {
    if (g == 0 && col < cols) out[col] = (O)(((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]);
  } else {
#pragma unroll
    for (int w = RG / 2; w >= 1; w >>= 1) {
      if (g < w) part[g][c] += part[g + w][c];
      __syncthreads();
    }
    if (g == 0 && col < cols) out[col] = (O)part[0][c];
  }
}

// few columns (per-wave loss partials): one block per column, 256 threads over rows
template <class T, class O>
__global__ void reduce_rows_narrow_kernel(const T* __restrict__ slab, int64_t rows, int64_t cols, O* __restrict__ out,
                                          const int32_t* __restrict__ skip) {
  __shared__ double red[256];
  if (skip != nullptr && *skip != 0) return;
  const int64_t col = blockIdx.x;
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < rows; r += 256) s += (double)slab[r * cols + col];
  lds_tree_sum<256>(s, red);
  if (threadIdx.x == 0) out[col] = (O)red[0];
}

// ------------------------------------------------------------------ elementwise
__global__ void axpy_cast_kernel(const float* __restrict__ a, const double* __restrict__ b, double frac, int64_t n,
                                 float* __restrict__ o) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    o[i] = (float)((double)a[i] + frac * b[i]);
}

// K line-search candidates (trpo.py:149-150): row k = (float)(theta_old + 0.5^(k0+k) fullstep)
// -- axpy_cast_kernel's arithmetic per row (linesearch's stepfrac is an exact power of two)
__global__ void ls_candidates_kernel(const float* __restrict__ a, const double* __restrict__ b, int k0, int K,
                                     int64_t n, float* __restrict__ o) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double ai = (double)a[i], bi = b[i];
    for (int k = 0; k < K; ++k) o[(int64_t)k * n + i] = (float)(ai + ldexp(1.0, -(k0 + k)) * bi);
  }
}

// Adam step in floatX (ppo.py:231-258): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// theta -= a_t m / (sqrt(v) + eps), a_t = lr sqrt(1-b2^t)/(1-b1^t) from the host
__global__ void adam_kernel(float* __restrict__ th, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, float a_t, float b1, float b2, float eps, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    th[i] = th[i] - a_t * mi / (sqrtf(vi) + eps);
  }
}

// dst row i = src row idx[i] (rows of `words` 32-bit words): minibatch gathers
__global__ void gather_rows_kernel(const uint32_t* __restrict__ src, const int64_t* __restrict__ idx, int64_t n,
                                   int64_t words, uint32_t* __restrict__ dst) {
  const int64_t total = n * words;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / words, c = i - r * words;
    dst[i] = src[idx[r] * words + c];
  }
}

__global__ void cast_scale_kernel(const float* __restrict__ a, double s, int64_t n, double* __restrict__ o) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    o[i] = s * (double)a[i];
}

}  // namespace mrl

using namespace mrl;

extern "C" {

int mrl_reduce_rows_f32(const float* slab, int64_t rows, int64_t cols, float* out, const int32_t* skip, void* stream) {
  if (!slab || !out) return fail(E_ARG, "null pointer");
  if (cols <= 0) return OK;
  // tall slabs (the fused VJP's per-wave rows: 1,024 x 5,126 for Hopper, only 81
  // column blocks wide): 16 row groups (1,024 threads) so the row split fills the chip;
  // short wide ones (the layered GEMMs' split-K slabs, 64 rows) keep 4 groups
  if (rows >= 256)
    hipLaunchKernelGGL((reduce_rows_kernel<float, float, 16>), dim3((cols + 63) / 64), dim3(1024), 0,
                       (hipStream_t)stream, slab, rows, cols, out, skip);
  else
    hipLaunchKernelGGL((reduce_rows_kernel<float, float, 4>), dim3((cols + 63) / 64), dim3(256), 0,
                       (hipStream_t)stream, slab, rows, cols, out, skip);
  return hip_check(hipGetLastError(), "mrl_reduce_rows_f32");
}
int mrl_reduce_rows_f64(const double* slab, int64_t rows, int64_t cols, double* out, const int32_t* skip,
                        void* stream) {
  if (!slab || !out) return fail(E_ARG, "null pointer");
  if (cols <= 0) return OK;
  if (cols <= 16)
    hipLaunchKernelGGL((reduce_rows_narrow_kernel<double, double>), dim3(cols), dim3(256), 0, (hipStream_t)stream,
                       slab, rows, cols, out, skip);
  else
    hipLaunchKernelGGL((reduce_rows_kernel<double, double>), dim3((cols + 63) / 64), dim3(256), 0,
                       (hipStream_t)stream, slab, rows, cols, out, skip);
  return hip_check(hipGetLastError(), "mrl_reduce_rows_f64");
}

int mrl_axpy_cast(const float* theta_old, const double* fullstep, double frac, int64_t n, float* theta_out,
                  void* stream) {
  if (!theta_old || !fullstep || !theta_out) return fail(E_ARG, "null pointer");
  hipLaunchKernelGGL(axpy_cast_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, theta_old, fullstep, frac,
                     n, theta_out);
  return hip_check(hipGetLastError(), "mrl_axpy_cast");
}

int mrl_linesearch_candidates(const float* theta_old, const double* fullstep, int32_t k0, int32_t K, int64_t n,
                              float* out, void* stream) {
  if (!theta_old || !fullstep || !out) return fail(E_ARG, "null pointer");
  if (K <= 0 || k0 < 0 || k0 + K > 64) return fail(E_ARG, "mrl_linesearch_candidates: need 0 < K, 0 <= k0, k0 + K <= 64");
  hipLaunchKernelGGL(ls_candidates_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, theta_old, fullstep,
                     (int)k0, (int)K, n, out);
  return hip_check(hipGetLastError(), "mrl_linesearch_candidates");
}

int mrl_adam_step(float* theta, const float* g, float* m, float* v, double a_t, double beta1, double beta2,
                  double eps, int64_t n, void* stream) {
  if (!theta || !g || !m || !v) return fail(E_ARG, "null pointer");
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, theta, g, m, v, (float)a_t,
                     (float)beta1, (float)beta2, (float)eps, n);
  return hip_check(hipGetLastError(), "mrl_adam_step");
}

int mrl_gather_rows(const void* src, const int64_t* idx, int64_t n, int64_t row_bytes, void* dst, void* stream) {
  if (!src || !idx || !dst) return fail(E_ARG, "null pointer");
  if (row_bytes <= 0 || row_bytes % 4 != 0) return fail(E_ARG, "row_bytes must be a positive multiple of 4");
  if (n <= 0) return OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(n * (row_bytes / 4))), dim3(256), 0, (hipStream_t)stream,
                     (const uint32_t*)src, idx, n, row_bytes / 4, (uint32_t*)dst);
  return hip_check(hipGetLastError(), "mrl_gather_rows");
}

int mrl_cast_scale_f32_f64(const float* in, double scale, int64_t n, double* out, void* stream) {
  if (!in || !out) return fail(E_ARG, "null pointer");
  hipLaunchKernelGGL(cast_scale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, scale, n, out);
  return hip_check(hipGetLastError(), "mrl_cast_scale_f32_f64");
}

}  // extern "C"
