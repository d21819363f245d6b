// Host-side glue shared by the units of the fused 64-wide MLP path -- mlp_kernels.hip (the
// C ABI and the small kernels), the big kernels' units (mlp_rows_vjp.hip, mlp_vjp16.hip,
// mlp_fisher.hip), mlp_bf16.hip and mlp_split.hip: descriptor checks, the rows passes'
// argument block and checks, the static-shape lookup and launch ladder, grid sizing, the
// VJP kernels' argument block and the launchers the ABI unit calls.  The error state (g_err behind fail / hip_check / mrl_last_error,
// mrl_common.h) is one thread-local of the library, defined in mlp_kernels.hip.
#pragma once
#include <type_traits>

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

// a time feature built from ep_t sits beside n_in - 1 observation columns, and the clamped
// column loads of the kernels (load_x, XGlobalNB) read column n_obs - 1: a net of the time
// feature alone (n_in == 1) has none
inline int check_time_feature(const mrl_mlp_desc* d, const int32_t* ep_t) {
  if (ep_t != nullptr && d->n_in < 2)
    return fail(E_ARG, "a time-feature net (ep_t) needs n_in >= 2: n_obs = n_in - 1 observation columns (got n_obs = 0)");
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

// The launch ladder: f(std::integral_constant<int, SH>) with the run-time shape `sh` as a
// compile-time constant when the set ALLOWED (bits sh_bit) has it, else with FALLBACK (0:
// the run-time-shape kernel).  Only the shapes of ALLOWED and FALLBACK are instantiated.
constexpr unsigned sh_bit(int sh) { return 1u << sh; }
constexpr unsigned SH_POLICY = sh_bit(1) | sh_bit(2), SH_VALUE = sh_bit(3) | sh_bit(4);
constexpr unsigned SH_VALUE_TIME = sh_bit(3 | SH_TIME) | sh_bit(4 | SH_TIME);
template <unsigned ALLOWED, int FALLBACK = 0, int SH = 1, class F>
inline void with_static_shape(int sh, F&& f) {
  if constexpr (SH > (4 | SH_TIME)) {
    f(std::integral_constant<int, FALLBACK>{});
  } else {
    if constexpr ((ALLOWED & sh_bit(SH)) != 0)
      if (sh == SH) return f(std::integral_constant<int, SH>{});
    with_static_shape<ALLOWED, FALLBACK, SH + 1>(sh, f);
  }
}
// f(std::true_type) or f(std::false_type): a run-time flag as a template argument
template <class F>
inline void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
// the static shapes a rows epilogue is compiled for: the prediction for every shape (and
// the value nets' time-feature variants), the VF loss for the value shapes, the policy
// epilogues for the policy shapes
constexpr unsigned rows_shapes(int epi_k) {
  return epi_k == MRL_EPI_PROB ? SH_POLICY | SH_VALUE | SH_VALUE_TIME : epi_k == MRL_EPI_VFLOSS ? SH_VALUE : SH_POLICY;
}
// The ladder of mlp_rows_kernel and mlp_rows_bf16_kernel.  Their units compile every
// epilogue for all four plain shapes (the library's set of kernels, kept as it is); a
// shape outside the epilogue's rows_shapes is never launched: it takes the run-time shape.
template <int EPI_K, class F>
inline void with_rows_shape(int sh, F&& f) {
  constexpr unsigned COMPILED = SH_POLICY | SH_VALUE | (EPI_K == MRL_EPI_PROB ? SH_VALUE_TIME : 0u);
  with_static_shape<COMPILED>((rows_shapes(EPI_K) >> sh) & 1u ? sh : 0, f);
}
// f(std::integral_constant<int, EPI_K>) for a rows epilogue rows_args accepted (the
// Fisher product on the activation cache: EPI_FVP_CACHED)
template <class F>
inline void with_rows_epilogue(int epi, int cache_mode, F&& f) {
  switch (epi) {
    case MRL_EPI_PROB: return f(std::integral_constant<int, MRL_EPI_PROB>{});
    case MRL_EPI_LOSSES: return f(std::integral_constant<int, MRL_EPI_LOSSES>{});
    case MRL_EPI_SURRGRAD: return f(std::integral_constant<int, MRL_EPI_SURRGRAD>{});
    case MRL_EPI_VFLOSS: return f(std::integral_constant<int, MRL_EPI_VFLOSS>{});
    case MRL_EPI_FVP:
      if (cache_mode == MRL_CACHE_READ) return f(std::integral_constant<int, EPI_FVP_CACHED>{});
      return f(std::integral_constant<int, MRL_EPI_FVP>{});
    case MRL_EPI_PPOGRAD: return f(std::integral_constant<int, MRL_EPI_PPOGRAD>{});
    case MRL_EPI_PPOSGD: return f(std::integral_constant<int, MRL_EPI_PPOSGD>{});
    case MRL_EPI_PPOCLIP: return f(std::integral_constant<int, MRL_EPI_PPOCLIP>{});
  }
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

// ------------------------------------------------------------------ rows arguments
// the fields every rows pass sets; plain policy rows (no ep_t) unless the caller adds it
inline RowsArgs rows_args_plain(const mrl_mlp_desc* d, const float* theta, const mrl_rows_io* io, int cache_mode) {
  RowsArgs a{};
  a.d = dims_of(d);
  a.head = d->head;
  a.n_obs = d->n_in;
  a.gh = d->head == MRL_HEAD_GAUSS ? 2 * d->n_out : d->n_out;
  a.A = d->n_out;
  a.x = io->x;
  a.n = io->n;
  a.inv_ng = io->inv_n_global;
  a.logstd = (d->head == MRL_HEAD_GAUSS && theta) ? theta + a.d.tls : nullptr;
  a.cache = io->act_cache;
  a.cache_mode = cache_mode;
  return a;
}

// the RowsArgs of one row pass and the argument checks of its epilogue (mrl_mlp_rows,
// mrl_mlp_rows_split, mrl_mlp_rows_bf16); 1 = nothing to do (n <= 0)
inline int rows_args(const mrl_mlp_desc* d, int32_t epi, const float* theta, const float* image, const float* tangent,
                     const float* image_t, const mrl_rows_io* io, RowsArgs& a) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!io || !image || !io->x) return fail(E_ARG, "null pointer");
  if ((rc = check_time_feature(d, io->ep_t)) != OK) return rc;
  if (io->n <= 0) return 1;
  a = rows_args_plain(d, theta, io, io->act_cache != nullptr ? io->cache_mode : 0);
  a.n_obs = d->n_in - (io->ep_t ? 1 : 0);
  a.ept = io->ep_t;
  a.ts_limit = io->timestep_limit;
  a.act = io->act;
  a.adv = io->adv;
  a.oldprob = io->oldprob;
  a.target = io->target;
  a.out = io->out;
  a.ghead = io->ghead;
  a.partial = io->partial;
  a.dlogstd = (d->head == MRL_HEAD_GAUSS && tangent) ? tangent + a.d.tls : nullptr;
  a.kl_coeff = (float)io->kl_coeff;
  a.kl_cutoff = (float)io->kl_cutoff;
  a.cutoff_coeff = (float)io->cutoff_coeff;
  a.reverse_kl = epi == MRL_EPI_PPOCLIP ? 0 : io->reverse_kl;
  a.feat = io->feat_out;
  if (a.feat != nullptr && (epi != MRL_EPI_PROB || io->ep_t == nullptr))
    return fail(E_ARG, "feat_out is for MRL_EPI_PROB with ep_t (the value prediction)");
  if (a.cache_mode == MRL_CACHE_READ && epi != MRL_EPI_FVP) return fail(E_ARG, "MRL_CACHE_READ is for MRL_EPI_FVP");
  if (a.cache_mode == MRL_CACHE_WRITE && (epi == MRL_EPI_FVP || epi == MRL_EPI_PPOSGD))
    return fail(E_ARG, "MRL_CACHE_WRITE is for the plain forward epilogues");
  switch (epi) {
    case MRL_EPI_PROB:
      if (!io->out) return fail(E_ARG, "EPI_PROB needs out");
      if (d->head == MRL_HEAD_GAUSS && !theta) return fail(E_ARG, "DiagGauss needs theta (logstd)");
      break;
    case MRL_EPI_LOSSES:
    case MRL_EPI_SURRGRAD:
    case MRL_EPI_PPOGRAD:
    case MRL_EPI_PPOSGD:
    case MRL_EPI_PPOCLIP:
      if (d->head == MRL_HEAD_LINEAR) return fail(E_ARG, "policy epilogue on a value net");
      if (!io->act || !io->adv || !io->oldprob || !io->partial) return fail(E_ARG, "losses need act/adv/oldprob/partial");
      if (epi != MRL_EPI_LOSSES && !io->ghead) return fail(E_ARG, "gradient epilogues need ghead");
      if (d->head == MRL_HEAD_GAUSS && !theta) return fail(E_ARG, "DiagGauss needs theta (logstd)");
      if (epi == MRL_EPI_PPOSGD && io->n > MRL_PPO_BLOCK_ROWS) return fail(E_ARG, "PPOSGD minibatch exceeds one block");
      if (epi == MRL_EPI_PPOCLIP && !clip_range_ok(io->kl_cutoff)) return fail(E_ARG, "PPOCLIP needs a clip range in (0, 1)");
      break;
    case MRL_EPI_VFLOSS:
      if (d->head != MRL_HEAD_LINEAR || !io->target || !io->ghead || !io->partial)
        return fail(E_ARG, "VFLOSS needs a linear head, target, ghead, partial");
      break;
    case MRL_EPI_FVP:
      if (!tangent || !image_t || !io->ghead) return fail(E_ARG, "FVP needs tangent, image_t, ghead");
      if (d->head == MRL_HEAD_GAUSS && !theta) return fail(E_ARG, "DiagGauss needs theta (logstd)");
      break;
    default:
      return fail(E_ARG, "unknown epilogue");
  }
  return OK;
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

// VjpArgs, or the bf16 kernel's VjpArgsB (mlp_bf16.hip: the same fields and the bf16
// image's dimensions, which its launcher adds)
template <class Args = VjpArgs>
inline Args vjp_args(const mrl_mlp_desc* d, const float* x, const int32_t* ep_t, double ts_limit, const float* ghead,
                     int64_t n, float* slab, const float* act_cache) {
  Args a{};
  a.d = dims_of(d);
  a.n_obs = d->n_in - (ep_t ? 1 : 0);
  a.n_sum = d->head == MRL_HEAD_GAUSS ? d->n_out : 0;
  a.gh = d->n_out + a.n_sum;
  a.x = x;
  a.ept = ep_t;
  a.ts_limit = ts_limit;
  a.n = n;
  a.ghead = ghead;
  a.slab = slab;
  a.cache = act_cache;
  return a;
}

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
