// Host-side launch helpers shared by gae.hip, episode_stats.hip and vector_ops.hip: the
// capped grid of the elementwise kernels, and the chunk length of the blocked time-major
// kernels with its dispatch onto a kernel template.
#pragma once
#include <stdint.h>

#include <type_traits>

namespace mrl {

inline int64_t grid_for(int64_t n, int64_t bs = 256, int64_t cap = 2048) {
  int64_t g = (n + bs - 1) / bs;
  if (g < 1) g = 1;
  return g > cap ? cap : g;
}

// chunk length of a kernel whose block covers nc chunks of L steps per segment: the smallest
// power of two that covers T in one segment, at most lmax
inline int chunk_len(int64_t T, int nc, int lmax) {
  int L = 1;
  while (L < lmax && (int64_t)nc * L < T) L <<= 1;
  return L;
}

// a chunk length (1, 2, 4, 8, 16, else 32) as a template argument: f(integral_constant<int, L>)
template <class F>
inline void dispatch_chunk_len(int L, F&& f) {
  switch (L) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}

}  // namespace mrl
