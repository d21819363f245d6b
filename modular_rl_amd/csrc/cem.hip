// Cross-entropy method, the two steps around the population rollout (cem.py:32-50):
//   mrl_cem_sample  ths = th_mean + sample_std * randn(batch_size, P)          cem.py:42
//   mrl_cem_refit   elite_inds = ys.argsort()[-n_elite:]; mean / var of them  cem.py:46-49
// The population stays on the device between them (mrl_pop_rollout, pop_rollout.hip, reads it in
// place; that unit includes the env headers, which set the fp contraction of what follows them,
// so these kernels stay in a unit without them).
#include <math.h>

#include "../../include/mrl_hip.h"
#include "mrl_common.h"

namespace mrl {

constexpr int CEM_TB = 256;

// one thread per (candidate i, pair c): normals 2c, 2c+1 of row i = Box-Muller of Philox
// (seed, domain 2, gid i, word generation, call c), as noise_fill_kernel draws them
__global__ __launch_bounds__(CEM_TB) void cem_sample_kernel(const double* __restrict__ mean,
                                                            const double* __restrict__ sd, int64_t P, int64_t N,
                                                            uint64_t seed, uint64_t generation,
                                                            float* __restrict__ thetas, int64_t ld) {
  const int64_t c = (int64_t)blockIdx.x * CEM_TB + threadIdx.x;
  if (2 * c >= P) return;
  const int64_t p0 = 2 * c, p1 = 2 * c + 1;
  const double m0 = mean[p0], s0 = sd[p0];
  const double m1 = p1 < P ? mean[p1] : 0.0, s1 = p1 < P ? sd[p1] : 0.0;
  for (int64_t i = blockIdx.y; i < N; i += gridDim.y) {
    double u0, u1;
    philox_uniform2(seed, 2, (uint32_t)i, generation, (uint32_t)c, u0, u1);
    const double rad = sqrt(-2.0 * log(1.0 - u0));
    double sn, cn;
    sincos(2.0 * 3.141592653589793 * u1, &sn, &cn);
    float* row = thetas + i * ld;
    // product and sum rounded separately (numpy's th_mean + sample_std * z)
    row[p0] = (float)__dadd_rn(m0, __dmul_rn(s0, rad * cn));
    if (p1 < P) row[p1] = (float)__dadd_rn(m1, __dmul_rn(s1, rad * sn));
  }
}

// j before i in the total order (y, index) with a NaN below every number
__device__ inline bool cem_before(double yj, int64_t j, double yi, int64_t i) {
  const bool nj = yj != yj, ni = yi != yi;
  if (nj != ni) return nj;
  if (!nj && yj != yi) return yj < yi;
  return j < i;
}

// rank[i] = candidates before i (an O(N^2) count: no sort, no atomics, one writer per slot);
// the n_elite highest ranks are the elites, listed in rank order
__global__ __launch_bounds__(CEM_TB) void cem_rank_kernel(const double* __restrict__ ys, int64_t N, int32_t n_elite,
                                                          int32_t* __restrict__ rank, int32_t* __restrict__ elite) {
  const int64_t i = (int64_t)blockIdx.x * CEM_TB + threadIdx.x;
  if (i >= N) return;
  const double yi = ys[i];
  int64_t r = 0;
  for (int64_t j = 0; j < N; ++j) r += cem_before(ys[j], j, yi, i) ? 1 : 0;
  rank[i] = (int32_t)r;
  const int64_t k = r - (N - n_elite);
  if (k >= 0) elite[k] = (int32_t)i;
}

// one thread per parameter: mean over the elites in list order, then the centred second pass
__global__ __launch_bounds__(CEM_TB) void cem_moments_kernel(const float* __restrict__ thetas, int64_t ld, int64_t P,
                                                             const int32_t* __restrict__ elite, int32_t n_elite,
                                                             double* __restrict__ mean_out,
                                                             double* __restrict__ var_out) {
  const int64_t p = (int64_t)blockIdx.x * CEM_TB + threadIdx.x;
  if (p >= P) return;
  double sum = 0.0;
  for (int k = 0; k < n_elite; ++k) sum += (double)thetas[(int64_t)elite[k] * ld + p];
  const double m = sum / (double)n_elite;
  double sq = 0.0;
  for (int k = 0; k < n_elite; ++k) {
    const double dlt = (double)thetas[(int64_t)elite[k] * ld + p] - m;
    sq += dlt * dlt;
  }
  mean_out[p] = m;
  var_out[p] = sq / (double)n_elite;
}

}  // namespace mrl

using namespace mrl;

static constexpr int64_t CEM_MAX_N = 0x7fffffff;  // candidate ids are Philox gids / int32 indices

extern "C" {

int mrl_cem_sample(const double* mean, const double* sample_std, int64_t P, int64_t N, uint64_t seed,
                   uint64_t generation, float* thetas, int64_t ld_theta, void* stream) {
  if (!mean) return fail(E_ARG, "mrl_cem_sample: null mean");
  if (!sample_std) return fail(E_ARG, "mrl_cem_sample: null sample_std");
  if (!thetas) return fail(E_ARG, "mrl_cem_sample: null thetas");
  if (P <= 0 || P > CEM_MAX_N) return fail(E_ARG, "mrl_cem_sample: P out of range");
  if (N <= 0 || N > CEM_MAX_N) return fail(E_ARG, "mrl_cem_sample: N out of range");
  if (ld_theta < P) return fail(E_ARG, "mrl_cem_sample: ld_theta < P");
  const int64_t pairs = (P + 1) / 2;
  const dim3 grid((unsigned)((pairs + CEM_TB - 1) / CEM_TB), (unsigned)(N < 65535 ? N : 65535));
  hipLaunchKernelGGL(cem_sample_kernel, grid, dim3(CEM_TB), 0, (hipStream_t)stream, mean, sample_std, P, N, seed,
                     generation, thetas, ld_theta);
  return hip_check(hipGetLastError(), "mrl_cem_sample");
}

// the rank of every candidate (int32 [N])
size_t mrl_cem_refit_workspace_bytes(int64_t N, int64_t P) {
  if (N <= 0 || N > CEM_MAX_N || P <= 0) return 0;
  return (size_t)N * sizeof(int32_t);
}

int mrl_cem_refit(const float* thetas, int64_t ld_theta, int64_t N, int64_t P, const double* ys, int32_t n_elite,
                  double* mean_out, double* var_out, int32_t* elite_idx, void* workspace, void* stream) {
  if (!thetas) return fail(E_ARG, "mrl_cem_refit: null thetas");
  if (!ys) return fail(E_ARG, "mrl_cem_refit: null ys");
  if (!mean_out || !var_out) return fail(E_ARG, "mrl_cem_refit: null mean_out / var_out");
  if (!elite_idx) return fail(E_ARG, "mrl_cem_refit: null elite_idx");
  if (!workspace) return fail(E_ARG, "mrl_cem_refit: null workspace (mrl_cem_refit_workspace_bytes)");
  if (P <= 0 || P > CEM_MAX_N) return fail(E_ARG, "mrl_cem_refit: P out of range");
  if (N <= 0 || N > CEM_MAX_N) return fail(E_ARG, "mrl_cem_refit: N out of range");
  if (ld_theta < P) return fail(E_ARG, "mrl_cem_refit: ld_theta < P");
  if (n_elite < 1 || n_elite > N) return fail(E_ARG, "mrl_cem_refit: n_elite must be in 1 .. N");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cem_rank_kernel, dim3((unsigned)((N + CEM_TB - 1) / CEM_TB)), dim3(CEM_TB), 0, s, ys, N, n_elite,
                     reinterpret_cast<int32_t*>(workspace), elite_idx);
  hipLaunchKernelGGL(cem_moments_kernel, dim3((unsigned)((P + CEM_TB - 1) / CEM_TB)), dim3(CEM_TB), 0, s, thetas,
                     ld_theta, P, elite_idx, n_elite, mean_out, var_out);
  return hip_check(hipGetLastError(), "mrl_cem_refit");
}

}  // extern "C"
