// The pairwise LDS tree of the fp64 vector layer (gae.hip, cg.hip, vector_ops.hip).  A sum's
// value depends on the order of its additions, and results here are compared bit for bit
// (exact-fit against general GAE kernel, single- against multi-block CG, run against run),
// so the order red[i] += red[i + o], o = N/2 .. 1, is written once.  cg.hip's block_sum is
// the same order at N = 1024 evaluated in two barriers; it stays beside the CG kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace mrl {

// The N threads' values summed as the pairwise tree red[i] += red[i + o], o = N/2 .. 1.
// red: N doubles of LDS; the sum is red[0], valid for every thread on return.
template <int N>
__device__ inline void lds_tree_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

// two values through the same tree, one barrier per level: the sums are red0[0], red1[0]
template <int N>
__device__ inline void lds_tree_sum2(double v0, double v1, double* red0, double* red1) {
  red0[threadIdx.x] = v0;
  red1[threadIdx.x] = v1;
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red0[threadIdx.x] += red0[threadIdx.x + o];
      red1[threadIdx.x] += red1[threadIdx.x + o];
    }
    __syncthreads();
  }
}

}  // namespace mrl
