// The population rollouts' episode protocol, once, for pop_rollout.hip (64-64 net, a lane per
// candidate, theta streamed from memory), pop_rollout_small.hip (small nets, a lane per
// candidate, theta in LDS) and pop_rollout_humanoid.hip (Humanoid-v2, a wave per candidate).
// Here are
//   the argument blocks -- five common fields, the net's shape;
//   the column helpers -- the frozen filter of an observation column, filter / clip / cast, the
//   Welford update.  The wave kernel calls them.  The two lane kernels state the same
//   expressions in their own text: they run at 256 / 255 VGPRs, and every fold of their episode
//   into a shared function changed their listings, so a change to the protocol is
//   made here and at the two sites that name this header.
// The host side (argument checks, shape, launch limits) is pop_rollout_host.h.
#pragma once
#include <stddef.h>

#include "rollout_device.h"

namespace mrl {

constexpr int POP_W = 64;          // candidates per block of the lane kernels (one wave)
constexpr int POP_MAX_HID = 3;     // hidden layers of a net given by hid_sizes
constexpr int POP_MAX_WIDTH = 64;  // units per hidden layer

// The five fields every population kernel's argument block starts with.  A list, not a base
// struct: a base's tail padding (limit is an int before 8-byte alignment) would move the shape
// that follows it, and the kernarg layout is part of each kernel's descriptor.
#define MRL_POP_ARGS_COMMON                                                                      \
  const float* thetas;                                                                           \
  int64_t ld;                                                                                    \
  const double* fstate;                                                                          \
  mrl_pop_io io;                                                                                 \
  int limit; /* steps an episode may take: min(timestep_limit or MAX_STEPS, MAX_STEPS) */

struct PopShape {
  int n_hid;
  int dims[POP_MAX_HID + 2];  // obs, hid_sizes..., act
};
struct PopSmallShape {
  PopShape sh;
  int PU;    // floats of theta the forward reads (all but logstd)
  int maxw;  // widest layer, input and head included
};

struct PopArgs {
  MRL_POP_ARGS_COMMON
};
struct PopSmallArgs {
  MRL_POP_ARGS_COMMON
  PopSmallShape net;
};
struct HmPopArgs {
  MRL_POP_ARGS_COMMON
  PopShape sh;
};
static_assert(sizeof(PopArgs) == 96 && offsetof(PopArgs, io) == 24 && offsetof(PopArgs, limit) == 88, "kernarg layout");
static_assert(sizeof(PopSmallArgs) == 128 && offsetof(PopSmallArgs, limit) == 88 && offsetof(PopSmallArgs, net) == 92 &&
                  offsetof(PopSmallShape, sh) == 0 && offsetof(PopSmallShape, PU) == 24 &&
                  offsetof(PopSmallShape, maxw) == 28,
              "kernarg layout");
static_assert(sizeof(HmPopArgs) == 120 && offsetof(HmPopArgs, limit) == 88 && offsetof(HmPopArgs, sh) == 92 &&
                  offsetof(PopShape, dims) == 4,
              "kernarg layout");

// ------------------------------------------------------------------ column helpers
// column k of the frozen filter: mrl_obfilter_update_apply(update = 0); below two observations
// (or no state) mean 0 / denominator 1, which leaves the observation bit for bit
__device__ __forceinline__ void pop_frozen_filter(const double* fstate, int D, int k, double& mean, double& den) {
  mean = 0.0;
  den = 1.0;
  if (fstate != nullptr) frozen_filter_column(fstate, D, k, mean, den);
}

// the policy's input: the filtered observation, clipped at +-5, as f32
__device__ __forceinline__ float pop_filtered(double o, double mean, double den) {
  double v = o - mean;
  v = v / den;
  return (float)(v < -5.0 ? -5.0 : (v > 5.0 ? 5.0 : v));
}

// observation o as the wn-th of its column's Welford partial (mean, M2)
__device__ __forceinline__ void welford_add(double o, double wn, double& mean, double& m2) {
  const double dlt = o - mean;
  mean += dlt / wn;
  m2 += dlt * (o - mean);
}

}  // namespace mrl
