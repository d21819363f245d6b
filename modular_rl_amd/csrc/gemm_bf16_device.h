// Device side shared by the units of the bf16-operand GEMM layer (gemm_bf16.hip,
// gemm_bf16_big.hip, gemm_bf16_stream.hip, gemm_bf16_tn.hip): the raw bf16 types and
// conversions, the kernels' argument blocks and the 16-B operand loads (registers and
// LDS-DMA) with their zero block.
//
// The epilogue of a 32 x 32 C^T accumulator tile is NOT here: the tiled, streaming and
// small-M kernels each carry its text (gemm_bf16_kernel's is the model; the other two are
// marked as copies).  As a shared function template it compiled to the same instructions
// in another block order and register assignment, and these kernels' listings are the
// record their measured timings refer to; change all three together.
#pragma once
#include "../../include/mrl_hip.h"
#include "mlp_device.h"

namespace mrl {

typedef uint16_t bfr_t;  // raw bf16 bits in memory
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));

__device__ inline float bf2f(bfr_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ inline bfr_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }  // RNE

constexpr int QBM = 128;  // rows of a block tile of the tiled NN and TN kernels

struct GemmB16Args {
  int64_t M, N, K;
  const bfr_t* A;
  const bfr_t* Bt;
  const bfr_t* A2;
  const bfr_t* Bt2;
  int64_t lda, ldb;
  void* C;
  int64_t ldc;
  const float* bias;
  const bfr_t* H;
  int64_t ldh;
  int epi;
  const int32_t* skip;
};

struct GemmTnArgs {
  int64_t M, N, K;  // C[M][N] over K rows
  const bfr_t* A;   // [K][lda]: columns 0..m_real-1 (column m_real = 1 if ones)
  const bfr_t* B;   // [K][ldb]
  int64_t lda, ldb;
  int64_t m_real;
  int64_t k_chunk;  // rows per split
  float* slab;
  int64_t slab_stride, ldc;
  const int32_t* skip;
};

// one 16-B chunk (8 bf16 along k) of row r, k offset kc of a row-major [rows][ld]
// operand; chunks at or past K read as zero (K's padding columns are zero in memory)
__device__ inline u32x4v load_chunk(const bfr_t* __restrict__ p, int64_t r, int64_t rows, int64_t ld, int64_t kc,
                                    int64_t K) {
  if (r < rows && kc < K) return *reinterpret_cast<const u32x4v*>(p + r * ld + kc);
  return u32x4v{0u, 0u, 0u, 0u};
}

// LDS-DMA of 16 B per lane (global_load_lds_dwordx4: lane-linear destination); the
// source of a chunk past an operand's edge is the zero block (one copy per unit)
static __device__ const uint32_t kZero16[4] = {0u, 0u, 0u, 0u};

__device__ inline void glds16b(const void* g, bfr_t* l) {
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

}  // namespace mrl
