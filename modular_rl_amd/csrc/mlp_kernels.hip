// The C ABI of the fused 64-wide MLP path on v_mfma_f32_32x32x2_f32 (exact fp32), its
// small kernels (image pack, probtype rows) and the line-search scorer (the slab
// reductions it and every gradient pass end with are vector_ops.hip's).
// The big kernels live in their own units:
//
//   mlp_rows_vjp.hip  mlp_rows_kernel<EPI>  forward (+ JVP) of a 32-row tile per wave with
//                     a per-row epilogue: prob rows, TRPO losses, surrogate gradient rows,
//                     VF loss rows, or the KL-metric rows of the Fisher product.
//                     mlp_vjp_kernel        forward recompute + backprop of head-gradient
//                     rows and the weight-gradient sums  sum_rows act^T * grad  (MFMA
//                     with the row index as K, operands transposed through LDS).
//   mlp_vjp16.hip     mlp_vjp16_kernel      the transpose-free VJP on the activation cache.
//   mlp_fisher.hip    mlp_fisher_hyb_kernel the one-pass Fisher product / policy gradient
//                     (with its entry points).
// The bf16 mode (mlp_bf16.hip) and the split-operand mode (mlp_split.hip) have their own
// entry points; the argument checks and launch ladders all of them share are mlp_host.h's.
//
// Replaces the Theano-compiled functions of the reference: _act_prob
// (core.py:269-270), compute_policy_gradient / compute_losses /
// compute_fisher_vector_product (trpo.py:68-70), NnRegression.predict and
// LbfgsOptimizer.f_lossgrad (core.py:608, 670-671).  The Fisher product uses the
// exact Gauss-Newton form of Theano's double backprop:
// JVP -> per-row KL metric -> VJP.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "mlp_host.h"

namespace mrl {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
int fail(int code, const std::string& s) {
  g_err = s;
  return code;
}
int hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return E_HIP;
  }
  return OK;
}

// ------------------------------------------------------------------ pack
__global__ void mlp_pack_kernel(MlpDims d, const float* __restrict__ th, float* __restrict__ image, int count,
                                const int32_t* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) image[i] = image_value(d, th, i);
}

// per-row probtype values on probability rows (mrl_probtype_rows): the helpers the
// row epilogues use, one thread per row
__global__ void probtype_rows_kernel(int head, int A, int64_t n, const float* __restrict__ prob,
                                     const float* __restrict__ prob2, const void* __restrict__ x,
                                     float* __restrict__ loglik, float* __restrict__ kl, float* __restrict__ ent) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    if (head == MRL_HEAD_SOFTMAX) {
      const float* p = prob + r * A;
      if (loglik) loglik[r] = logf(p[reinterpret_cast<const int32_t*>(x)[r]]);
      if (kl) {
        const float* q = prob2 + r * A;
        float k = 0.f;
        for (int j = 0; j < A; ++j) k += cat_kl_term(p[j], q[j]);
        kl[r] = k;
      }
      if (ent) {
        float h = 0.f;
        for (int j = 0; j < A; ++j) h += cat_ent_term(p[j]);
        ent[r] = h;
      }
    } else {
      const float* p = prob + r * 2 * A;
      float sumlog = 0.f;
      for (int j = 0; j < A; ++j) sumlog += logf(p[A + j]);
      if (loglik) {
        const float* xv = reinterpret_cast<const float*>(x) + r * A;
        float q = 0.f;
        for (int j = 0; j < A; ++j) {
          const float u = (xv[j] - p[j]) / p[A + j];
          q += u * u;
        }
        loglik[r] = gauss_loglik(q, sumlog, A);
      }
      if (kl) {
        const float* p2 = prob2 + r * 2 * A;
        float k = 0.f;
        for (int j = 0; j < A; ++j) k += gauss_kl_term(p[j], p[A + j], p2[j], p2[A + j]);
        kl[r] = k - 0.5f * A;
      }
      if (ent) ent[r] = gauss_entropy(sumlog, A);
    }
  }
}

}  // namespace mrl

using namespace mrl;

extern "C" {

const char* mrl_last_error(void) { return mrl::g_err.c_str(); }
int32_t mrl_version(void) { return 1; }

int64_t mrl_mlp_num_params(const mrl_mlp_desc* d) {
  if (check_desc(d) != OK) return -1;
  return dims_of(d).P;
}
int64_t mrl_mlp_image_floats(const mrl_mlp_desc* d) {
  if (check_desc(d) != OK) return -1;
  return dims_of(d).total_size;
}
int64_t mrl_partial_rows(int64_t n) { return grid_blocks(n, ROWS_MAX_BLOCKS) * 4; }
int64_t mrl_act_cache_floats(int64_t n) { return ceil_div(n, 32) * CACHE_TILE_FLOATS; }
int64_t mrl_slab_rows(int64_t n) { return grid_blocks(n, VJP_MAX_BLOCKS) * 4; }
int64_t mrl_mlp_partial_rows(const mrl_mlp_desc* d, int64_t n) {
  if (check_desc(d) != OK) return -1;
  return grid_blocks(n, scaled_cap(ROWS_MAX_BLOCKS, desc_cus(d))) * 4;
}
int64_t mrl_mlp_slab_rows(const mrl_mlp_desc* d, int64_t n) {
  if (check_desc(d) != OK) return -1;
  return grid_blocks(n, scaled_cap(VJP_MAX_BLOCKS, desc_cus(d))) * 4;
}

int mrl_mlp_pack(const mrl_mlp_desc* d, const float* theta, float* image, int32_t fwd_only, const int32_t* skip,
                 void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!theta || !image) return fail(E_ARG, "null pointer");
  MlpDims m = dims_of(d);
  int count = fwd_only ? m.fwd_size : m.total_size;
  hipLaunchKernelGGL(mlp_pack_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, theta, image,
                     count, skip);
  return hip_check(hipGetLastError(), "mrl_mlp_pack");
}

int mrl_mlp_rows(const mrl_mlp_desc* d, int32_t epi, const float* theta, const float* image, const float* tangent,
                 const float* image_t, const mrl_rows_io* io, const int32_t* skip, void* stream) {
  RowsArgs a;
  int rc = rows_args(d, epi, theta, image, tangent, image_t, io, a);
  if (rc) return rc > 0 ? OK : rc;
  // cus sizes the passes whose sums follow the grid (per-wave partials); the others
  // (forward / PROB / FVP rows) keep the device-wide grid wherever they run
  const int64_t blocks = grid_blocks(io->n, scaled_cap(ROWS_MAX_BLOCKS, io->partial != nullptr ? desc_cus(d) : 256));
  launch_rows(epi, static_shape_of(d, io->ep_t != nullptr, epi == MRL_EPI_PROB), a, image, image_t, blocks, skip,
              (hipStream_t)stream);
  return hip_check(hipGetLastError(), "mrl_mlp_rows");
}

int mrl_mlp_rows_split(const mrl_mlp_desc* d, int32_t epi, const float* theta, const float* image_s,
                       const mrl_rows_io* io, const int32_t* skip, void* stream) {
  if (epi != MRL_EPI_PROB && epi != MRL_EPI_LOSSES && epi != MRL_EPI_SURRGRAD && epi != MRL_EPI_VFLOSS)
    return fail(E_UNSUPPORTED, "mrl_mlp_rows_split: PROB, LOSSES, SURRGRAD or VFLOSS");
  if (d != nullptr && (d->n_in > MAX_IN || d->n_out > MAX_OUT || d->n_hidden != HID || d->n_layers != 2))
    return fail(E_UNSUPPORTED, "mrl_mlp_rows_split: the 64-wide fused shape only");
  RowsArgs a;
  int rc = rows_args(d, epi, theta, image_s, nullptr, nullptr, io, a);
  if (rc) return rc > 0 ? OK : rc;
  // the grid (and so the partial rows) of mrl_mlp_rows: mrl_mlp_partial_rows holds for both
  const int64_t blocks = grid_blocks(io->n, scaled_cap(ROWS_MAX_BLOCKS, io->partial != nullptr ? desc_cus(d) : 256));
  const int sh = static_shape_of(d, io->ep_t != nullptr, epi == MRL_EPI_PROB);
  return launch_rows_split(epi, sh, a, bf16_dims(d->n_in, d->n_out), image_s, blocks, skip, stream);
}

int mrl_mlp_vjp(const mrl_mlp_desc* d, const float* image, const float* x, const int32_t* ep_t, double ts_limit,
                const float* ghead, int64_t n, float* slab, const float* act_cache, const int32_t* skip,
                void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!image || !x || !ghead || !slab) return fail(E_ARG, "null pointer");
  if ((rc = check_time_feature(d, ep_t)) != OK) return rc;
  if (n <= 0) return OK;
  const VjpArgs a = vjp_args(d, x, ep_t, ts_limit, ghead, n, slab, act_cache);
  const int64_t blocks = grid_blocks(n, scaled_cap(VJP_MAX_BLOCKS, desc_cus(d)));
  // with a cache, the transpose-free 16-row kernel; it takes the bias gradient b0 through a
  // ones column of gW0's padding, so not at O % 16 == 0.  The 32-row kernel runs on the
  // run-time shape (the static shapes are used by the rows kernels only)
  if (act_cache != nullptr && a.d.O % 16 != 0) launch_vjp16(a, image, blocks, skip, (hipStream_t)stream);
  else launch_vjp(a, image, blocks, skip, (hipStream_t)stream);
  return hip_check(hipGetLastError(), "mrl_mlp_vjp");
}

int mrl_probtype_rows(int32_t head, int32_t k, int64_t n, const float* prob, const float* prob2, const void* x,
                      float* loglik, float* kl, float* ent, void* stream) {
  if (head != MRL_HEAD_SOFTMAX && head != MRL_HEAD_GAUSS) return fail(E_ARG, "mrl_probtype_rows: bad head kind");
  if (k < 1) return fail(E_ARG, "mrl_probtype_rows: k < 1");
  if (!prob || (loglik && !x) || (kl && !prob2)) return fail(E_ARG, "null pointer");
  if (n <= 0) return OK;
  hipLaunchKernelGGL(probtype_rows_kernel, dim3(std::min<int64_t>(ceil_div(n, 256), 2048)), dim3(256), 0, (hipStream_t)stream, (int)head, (int)k, n,
                     prob, prob2, x, loglik, kl, ent);
  return hip_check(hipGetLastError(), "mrl_probtype_rows");
}

// K line-search candidates of the fused policy scored in one call, read back once by the
// caller (trpo.py:143-159): candidates -> per candidate its forward image + a LOSSES pass
// into its own partial rows -> out[k] = the candidate's (surr, kl, ent, n) sums.
int mrl_linesearch_eval(const mrl_mlp_desc* pol, int32_t compute, const float* theta_old, const double* fullstep,
                        int32_t k0, int32_t K, const mrl_rows_io* io, float* cand, float* images, int64_t image_stride,
                        double* partials, int64_t partial_stride, double* out, void* stream) {
  int rc = check_desc(pol);
  if (rc) return rc;
  if (!io || !cand || !images || !partials || !out) return fail(E_ARG, "mrl_linesearch_eval: null pointer");
  if ((rc = check_time_feature(pol, io->ep_t)) != OK) return rc;
  if (compute != MRL_COMPUTE_F32 && compute != MRL_COMPUTE_BF16 && compute != MRL_COMPUTE_SPLIT)
    return fail(E_ARG, "bad compute");
  const bool bf = compute == MRL_COMPUTE_BF16, sp = compute == MRL_COMPUTE_SPLIT;
  const int64_t P = mrl_mlp_num_params(pol);
  const int64_t img = bf ? mrl_mlp_image_words_bf16(pol) : sp ? mrl_mlp_image_words_split(pol) : mrl_mlp_image_floats(pol);
  // the LOSSES pass sizes its grid (and so its partial rows) by the desc's CU count
  const int64_t prow = bf ? mrl_mlp_partial_rows_bf16(pol, io->n) : mrl_mlp_partial_rows(pol, io->n);
  if (image_stride < img || partial_stride < prow * 4) return fail(E_ARG, "mrl_linesearch_eval: strides too small");
  rc = mrl_linesearch_candidates(theta_old, fullstep, k0, K, P, cand, stream);
  for (int32_t k = 0; k < K && rc == OK; ++k) {
    const float* th = cand + (int64_t)k * P;
    float* im = images + (int64_t)k * image_stride;
    mrl_rows_io iok = *io;
    iok.partial = partials + (int64_t)k * partial_stride;
    iok.cache_mode = MRL_CACHE_NONE;
    iok.act_cache = nullptr;
    rc = bf ? mrl_mlp_pack_bf16(pol, th, im, 1, nullptr, stream)
            : sp ? mrl_mlp_pack_split(pol, th, im, nullptr, stream) : mrl_mlp_pack(pol, th, im, 1, nullptr, stream);
    if (rc == OK)
      rc = bf ? mrl_mlp_rows_bf16(pol, MRL_EPI_LOSSES, th, im, nullptr, nullptr, &iok, nullptr, stream)
            : sp ? mrl_mlp_rows_split(pol, MRL_EPI_LOSSES, th, im, &iok, nullptr, stream)
                 : mrl_mlp_rows(pol, MRL_EPI_LOSSES, th, im, nullptr, nullptr, &iok, nullptr, stream);
    if (rc == OK) rc = mrl_reduce_rows_f64(iok.partial, prow, 4, out + 4 * (int64_t)k, nullptr, stream);
  }
  return rc;
}

}  // extern "C"

