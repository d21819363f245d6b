// Device helpers shared by the 16-row cached VJP (mlp_vjp16.hip) and the one-pass Fisher /
// gradient kernel built on it (mlp_fisher.hip).
#pragma once
#include "mlp_host.h"

namespace mrl {

// a 0 / 1 factor the optimiser cannot see through: v * opaque(m) stays a multiply, so the
// load of v is not sunk into a branch on m (hipcc drains every outstanding load at such a
// branch's join, the prefetch with it)
__device__ inline float opaque(float m) {
  asm volatile("" : "+v"(m));
  return m;
}
// 16 B per lane global -> LDS (global_load_lds_dwordx4): lane L's bytes land at l + 16 L
// (l wave-uniform); no VGPR destination
__device__ inline void glds16(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
constexpr int VJP16_W_FLOATS = 2 * 32 * 64 + 2 * 4 * 64;  // BA1 + BA2 of the image
constexpr int VJP16_H1_FLOATS = 16 * 64;                  // h1 of one 16-row tile
// cache offset (floats) of element (32-row tile's row j, unit w of 32-unit slot `slot`)
__device__ inline int cache_off(int slot, int j, int w) {
  return ((slot * 4 + (w >> 3)) * 64 + 32 * ((w >> 2) & 1) + j) * 4 + (w & 3);
}

}  // namespace mrl
