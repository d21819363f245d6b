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

// The 256 x 256 kernel for a tall NN product (a multiple of four 32-deep K stages, N >= 128,
// one 512-thread block per CU): launched here and true, or false.  gemm_bf16_big.hip
bool big_gemm_launch(const GemmB16Args& g, bool outbf, bool dual, hipStream_t s);
// The streaming kernel for a tall NN product (K of 257..512, N >= 64, one block per CU):
// launched here and true, or false (the tiled kernel runs).  gemm_bf16_stream.hip
bool stream_gemm_launch(const GemmB16Args& g, bool outbf, bool dual, hipStream_t s);

}  // namespace mrl
