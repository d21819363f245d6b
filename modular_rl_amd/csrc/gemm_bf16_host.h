// Host side shared by the units of the bf16-operand GEMM layer: the dispatch thresholds
// with their environment overrides, the CU count the persistent kernels size their grids
// by, and the launchers mrl_gemm_bf16 (gemm_bf16.hip) calls in the other units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace mrl {

#ifndef MRL_GEMM_STREAM_MIN_M  // rows from which the streaming kernel takes the NN GEMM (0: never)
#define MRL_GEMM_STREAM_MIN_M 32768
#endif
#ifndef MRL_GEMM_SMALL_MAX_M  // rows up to which the whole-K 64 x 64 kernel takes the NN GEMM (0: never)
#define MRL_GEMM_SMALL_MAX_M 8192
#endif
#ifndef MRL_GEMM_BIG_MIN_M  // rows from which the 256 x 256 LDS-DMA kernel takes the NN GEMM (0: never)
#define MRL_GEMM_BIG_MIN_M 65536
#endif

// the environment's value of `name`, or the compiled default; read at every call (the
// tests flip these between calls)
inline int64_t env_or(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}

// CUs of the current device if the persistent kernels can deal their blocks to the 8
// XCDs evenly (at least 8, a multiple of 8), else 0
inline int cu_count() {
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return ncu >= 8 && ncu % 8 == 0 ? ncu : 0;
}

struct GemmB16Args;

// Each persistent kernel's decision is one `plan` function, which both mrl_gemm_bf16 and
// mrl_gemm_bf16_route go through (gemm_bf16.hip's nn_route); the `launch` functions only
// launch what a plan accepted.
struct BigPlan {
  int64_t ntm;  // row tiles
  int ntn;      // column tiles
  int per_xcd;  // blocks per XCD
};
struct StreamPlan {
  int nslice, groups_per_xcd;
  int kp;   // K plan: 384 or 512
  int ncu;  // blocks launched (those past 8 groups_per_xcd nslice return at once)
};

// The 256 x 256 kernel for a tall NN product (a positive multiple of four 32-deep K stages,
// N >= 128, one 512-thread block per CU): whether it takes the product, and its plan.
// gemm_bf16_big.hip
bool big_gemm_plan(const GemmB16Args& g, bool dual, BigPlan* pl);
void big_gemm_launch(const GemmB16Args& g, bool outbf, bool dual, const BigPlan& pl, hipStream_t s);
// The streaming kernel for a tall single NN product (K of 257..512 with rows that cover all
// but the plan's last k-step, N >= 64, one block per CU): whether it takes the product (else
// the tiled kernel runs), and its plan.  gemm_bf16_stream.hip
bool stream_gemm_plan(const GemmB16Args& g, bool dual, StreamPlan* pl);
void stream_gemm_launch(const GemmB16Args& g, bool outbf, const StreamPlan& pl, hipStream_t s);

}  // namespace mrl
