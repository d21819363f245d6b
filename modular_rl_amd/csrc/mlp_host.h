// Host-side glue shared by the units of the fused 64-wide MLP path -- mlp_kernels.hip (the
// C ABI and the small kernels), the big kernels' units (mlp_rows_vjp.hip, mlp_vjp16.hip,
// mlp_fisher.hip), mlp_bf16.hip and mlp_split.hip: descriptor checks, the
// static-shape lookup, grid sizing, the VJP kernels' argument block and the launchers the
// ABI unit calls.  The error state (g_err behind fail / hip_check / mrl_last_error,
// mrl_common.h) is one thread-local of the library, defined in mlp_kernels.hip.
#pragma once
#include "../../include/mrl_hip.h"
#include "bf16_frag.h"
#include "mlp_device.h"
#include "rows_epilogue.h"

namespace mrl {

constexpr int ROWS_BLOCK = 256;
// The cached FVP rows kernel fits 3 blocks per CU (168 VGPRs, 2 x 23 KB images):
// 1536 = two full rounds of 768 resident blocks (1024 left a one-third second round;
// FVP rows 0.92 -> 0.90 ms at 4.19 M rows, the other rows kernels unchanged or faster)
#ifndef MRL_ROWS_MAX_BLOCKS
#define MRL_ROWS_MAX_BLOCKS 1536
#endif
constexpr int ROWS_MAX_BLOCKS = MRL_ROWS_MAX_BLOCKS;
constexpr int VJP_MAX_BLOCKS = 256;
constexpr int VJP16_WAVES = 8;  // waves per block of mlp_vjp16_kernel
// mlp_fisher_hyb_kernel: three waves per SIMD -- four producer waves and the VJP of their
// tiles on eight (four accumulate gW1 / gW2 / b1 / b2 / logstd, four gW0 / b0); a VJP pair
// fills one slab row, so the kernel keeps four slab rows and four partial rows per block
constexpr int HYB_WAVES = 12;
constexpr int HYB_VJP_WAVES = 8;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int check_desc(const mrl_mlp_desc* d) {
  if (d == nullptr) return fail(E_ARG, "null mlp desc");
  if (d->n_hidden != HID || d->n_layers != 2)
    return fail(E_UNSUPPORTED, "only hid_sizes=[64,64] is implemented on the HIP path (got " +
                                   std::to_string(d->n_layers) + "x" + std::to_string(d->n_hidden) + ")");
  if (d->n_in < 1 || d->n_in > MAX_IN) return fail(E_UNSUPPORTED, "n_in must be in [1, 32]");
  if (d->n_out < 1 || d->n_out > MAX_OUT) return fail(E_UNSUPPORTED, "n_out must be in [1, 8]");
  if (d->head < 0 || d->head > 2) return fail(E_ARG, "bad head kind");
  if (d->head == MRL_HEAD_LINEAR && d->n_out != 1) return fail(E_ARG, "linear head needs n_out=1");
  if (d->cus < 0 || d->cus > 1024) return fail(E_ARG, "cus must be in [0, 1024]");
  return OK;
}

inline MlpDims dims_of(const mrl_mlp_desc* d) { return mlp_dims(d->n_in, d->n_out, d->head == MRL_HEAD_GAUSS); }

// the static shape (mlp_layout.h) a launch matches, or 0: plain rows only (a time
// feature column built from ep_t takes the generic kernels, except the value nets'
// prediction pass: time_ok, SH_TIME variants)
inline int static_shape_of(const mrl_mlp_desc* d, bool has_ept, bool time_ok = false) {
  if (has_ept && !time_ok) return 0;
  for (int i = 1; i < N_STATIC_SHAPES; ++i)
    if (STATIC_SHAPES[i].O == d->n_in && STATIC_SHAPES[i].A == d->n_out && STATIC_SHAPES[i].head == d->head) {
      if (!has_ept) return i;
      return STATIC_SHAPES[i].head == MRL_HEAD_LINEAR ? (i | SH_TIME) : 0;
    }
  return 0;
}

// Grids of one block (four waves, a 32-row tile per wave and step) per 128 rows, capped
// for passes sized for `cus` CUs (the caps are per 256): the VJP runs one block per CU, so
// on a fit stream of 192 CUs a 256-block grid would take two rounds
inline int64_t desc_cus(const mrl_mlp_desc* d) { return d != nullptr && d->cus > 0 ? d->cus : 256; }
inline int64_t scaled_cap(int64_t cap, int64_t cus) { return cap * cus / 256 > 0 ? cap * cus / 256 : 1; }
inline int64_t grid_blocks(int64_t n, int64_t cap) {
  const int64_t b = ceil_div(ceil_div(n, 32), 4);
  return b < 1 ? 1 : b > cap ? cap : b;
}

// ------------------------------------------------------------------ VJP arguments
struct VjpArgs {
  MlpDims d;
  int n_obs, gh, n_sum;
  const float* x;
  const int32_t* ept;
  double ts_limit;
  int64_t n;
  const float* ghead;
  float* slab;
  const float* cache;  // primal activation cache (CACHED kernel)
};

// ------------------------------------------------------------------ launchers
// mlp_rows_kernel<epi, sh> (mlp_rows_vjp.hip) for mrl_mlp_rows
void launch_rows(int epi, int sh, const RowsArgs& a, const float* image, const float* image_t, int64_t blocks,
                 const int32_t* skip, hipStream_t s);
// mlp_rows_split_kernel<epi, sh> (mlp_split.hip) for mrl_mlp_rows_split
int launch_rows_split(int epi, int sh, const RowsArgs& a, const BDims& b, const float* image_s, int64_t blocks,
                      const int32_t* skip, void* stream);
// mlp_vjp_kernel (mlp_rows_vjp.hip) and mlp_vjp16_kernel (mlp_vjp16.hip) for mrl_mlp_vjp
void launch_vjp(const VjpArgs& a, const float* image, int64_t blocks, const int32_t* skip, hipStream_t s);
void launch_vjp16(const VjpArgs& a, const float* image, int64_t blocks, const int32_t* skip, hipStream_t s);

}  // namespace mrl
