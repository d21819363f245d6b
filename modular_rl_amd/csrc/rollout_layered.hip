// Layered-policy rollout: the training kernels and the C entry points.
//
// For policies the fused step kernel does not cover (wide nets, Humanoid's 376-d obs),
// step t is three launches: lrollout_obs (filter merge + normalised obs rows) ->
// the policy's GEMM forward over the E rows (LayeredMlpNet) -> lrollout_act (sample,
// env step, raw next obs + reward as SoA rows [O+1][E] fp64, block partials).
// The kernel templates are rollout_layered_kernels.h's; this unit instantiates them for
// training, owns the partials kernel and the stand-alone stepper's Humanoid kernels, and
// holds the entry points.  The evaluation instantiations are rollout_layered_eval.hip's.
// Shares the env functions, the column partial and the record merge with the other rollout
// units (rollout_device.h).
#include "rollout_host.h"
#include "rollout_layered_kernels.h"

namespace mrl {

// per-(env block, column chunk) two-pass partial of the SoA rows raw[k][e0 .. e0+nvalid):
// column k = 32*blockIdx.y + (tid & 31); 8 thread groups stride the envs.
__global__ __launch_bounds__(RB) void lrollout_partials_kernel(RollArgs a, int D, int rec_parity, int with_rew) {
  __shared__ double red[8][LCOLS];
  const int E = a.d.n_envs;
  const int e0 = blockIdx.x * ENVS_PER_BLOCK;
  const int nvalid = min(ENVS_PER_BLOCK, E - e0);
  const int c = threadIdx.x & (LCOLS - 1), g = threadIdx.x >> 5;
  const int k = blockIdx.y * LCOLS + c;
  double* r = a.b.records + (int64_t)rec_parity * a.nb * a.RS + (int64_t)blockIdx.x * a.RS;
  const double* col = a.b.raw_obs + (int64_t)(k < D ? k : 0) * E + e0;
  double mean, t2;
  col_partial([&](int row) { return col[row]; }, nvalid, k < D, red, c, g, mean, t2);
  if (g == 0 && k < D) {
    r[2 + k] = mean;
    r[2 + D + k] = t2;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    r[0] = (double)nvalid;
    r[1] = with_rew ? (double)nvalid : 0.0;
  }
}

// ------------------------------------------------------------------ Humanoid, stand-alone stepper
// The stand-alone env stepper's (env_api.hip) Humanoid kernels: hm_reset_kernel / hm_act_kernel
// with the caller's rows and ctrl.  They are compiled in this unit, beside hm_act_kernel, and
// env_api.hip launches them through launch_hm_env_reset / launch_hm_env_step (rollout_host.h).
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_env_reset_kernel(RollArgs a, mrl_env_io io) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  const int E = a.d.n_envs;
  hm_load_tables<WPB>(S, lane);
  if (e >= E || (io.mask != nullptr && io.mask[e] == 0)) return;  // after the tables' barrier
  const uint32_t w = (uint32_t)a.b.env_int[E + e];
  hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
  hm::forward(W, S, lane);
  double* orow = io.obs + (int64_t)e * HM_OBS;
  hm::observation(W, S, lane, [&](int k, double v) { orow[k] = v; });
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, a.b.env_state + (int64_t)HM_NS * E + (int64_t)e * HM_KCACHE, lane);
  if (lane == 0) {
    a.b.env_int[E + e] = (int32_t)(w + 1);
    a.b.env_int[e] = 0;
  }
}

// hm_act_kernel with the caller's ctrl in place of the sampled one
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_env_step_kernel(RollArgs a, mrl_env_io io, int auto_reset) {
  __shared__ hm::Shared S;
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  constexpr int A = HM_ACT;
  const int E = a.d.n_envs;
  const bool live = e < E;
  const int ec = live ? e : E - 1;  // a block's waves past E load a valid env, store nothing
  double* const kc = a.b.env_state + (int64_t)HM_NS * E + (int64_t)ec * HM_KCACHE;
  hm_load_tables<WPB>(S, lane);
  if (!live) return;  // after the tables' barrier
  if (lane < HM_NS) W.s[lane] = a.b.env_state[(int64_t)lane * E + e];
  hm::load_kcache(W, kc, lane);
  WAVE_SYNC();
  if (lane < A) W.s[HM_NQ + HM_NV + lane] = (double)reinterpret_cast<const float*>(io.act)[(int64_t)e * A + lane];
  WAVE_SYNC();
  // one forward and one observation site, as in hm_act_kernel: passes 0..FRAME_SKIP-1 are
  // the substeps, pass FRAME_SKIP observes the new state (into final_obs when the env is
  // reset in this call), pass FRAME_SKIP + 1 the reset one
  double x_before = 0.0, rew = 0.0;
  for (int pass = 0;; ++pass) {
    if (pass > 0) hm::forward(W, S, lane);  // pass 0: the kinematics cache
    if (pass < hm::FRAME_SKIP) {
      if (pass == 0) x_before = W.com[0];
      hm::accelerations(W, S, lane);
      hm::integrate(W, lane);
      continue;
    }
    double* orow = io.obs + (int64_t)e * HM_OBS;
    double* orow2 = nullptr;
    bool again = false;
    if (pass == hm::FRAME_SKIP) {
      bool done, term, last;
      hm::reward_done(W, lane, x_before, rew, done);
      const int ept = a.b.env_int[e];
      env_step_flags<MRL_ENV_HUMANOID>(a, ept, done, term, last);
      if (lane == 0) {
        io.ep_t[e] = ept;
        io.rew[e] = rew;
        io.flags[e] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
      }
      again = last && auto_reset;
      if (!again && lane == 0) a.b.env_int[e] = ept + 1;
      double* frow = io.final_obs != nullptr ? io.final_obs + (int64_t)e * HM_OBS : nullptr;
      if (again) orow = frow;  // the obs row waits for the reset state
      else if (last) orow2 = frow;
    }
    if (orow != nullptr)
      hm::observation(W, S, lane, [&](int k, double v) {
        orow[k] = v;
        if (orow2 != nullptr) orow2[k] = v;
      });
    if (!again) break;
    const uint32_t w = (uint32_t)a.b.env_int[E + e];
    hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
    if (lane == 0) {
      a.b.env_int[E + e] = (int32_t)(w + 1);
      a.b.env_int[e] = 0;
    }
  }
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * E + e] = W.s[lane];
  hm::save_kcache(W, kc, lane);  // W holds forward() of the state just stored
}

void launch_hm_env_reset(const RollArgs& a, const mrl_env_io& io, hipStream_t s) {
  MRL_LAUNCH_HM(hm_env_reset_kernel, hm_lds_state, a.d.n_envs, s, a, io);
}
void launch_hm_env_step(const RollArgs& a, const mrl_env_io& io, int auto_reset, hipStream_t s) {
  MRL_LAUNCH_HM(hm_env_step_kernel, hm_lds_bytes, a.d.n_envs, s, a, io, auto_reset);
}

}  // namespace mrl

using namespace mrl;

extern "C" {

static int check_rows(const mrl_rollout_desc* d, const mrl_rollout_bufs* b) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (!b->raw_obs) return fail(E_ARG, "the layered rollout needs raw_obs [(obs_dim+1) * n_envs] doubles");
  if (env_info(d->env_id).obs + 1 > MAXD_L) return fail(E_UNSUPPORTED, "obs dim too large");
  return OK;
}

int mrl_rollout_reset_rows(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  RollArgs a = make_args(d, b);
  const int D = env_info(d->env_id).obs + 1;
  // one wave per block: the per-env step is latency-bound, so spread the waves over CUs
  const dim3 genv((d->n_envs + 63) / 64), gpart(a.nb, (D + LCOLS - 1) / LCOLS);
  hipStream_t s = (hipStream_t)stream;
  if (d->env_id == MRL_ENV_HUMANOID) MRL_LAUNCH_HM(hm_reset_kernel, hm_lds_state, d->n_envs, s, a);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, lrollout_reset_kernel, genv, dim3(64), 0, s, a);
  // evaluation: the reset kernels as they are (raw_obs feeds the obs kernel), no partial of obs_0
  if (!roll_eval(d)) hipLaunchKernelGGL(lrollout_partials_kernel, gpart, dim3(RB), 0, s, a, D, 0, 0);
  return hip_check(hipGetLastError(), "mrl_rollout_reset_rows");
}

int mrl_rollout_obs(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  if (!b->obs) return fail(E_ARG, "null obs");
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const dim3 grid(a.nb, (env_info(d->env_id).obs + 1 + LCOLS - 1) / LCOLS);
  if (roll_eval(d)) launch_lrollout_obs_eval(a, t, (hipStream_t)stream);
  else MRL_DISPATCH_ENV(d->env_id, lrollout_obs_kernel, grid, dim3(RB), 0, (hipStream_t)stream, a, t);
  return hip_check(hipGetLastError(), "mrl_rollout_obs");
}

static int rollout_act(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* z, const HeadRows& hr,
                       const float* logstd, const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_rows(d, b);
  if (rc) return rc;
  if (!b->act || !b->prob || !b->rew || !b->flags || !b->ep_t || (!z && !hr.hid && !hr.hid16))
    return fail(E_ARG, "null trajectory buffer");
  if ((hr.hid || hr.hid16) && d->env_id != MRL_ENV_HUMANOID)
    return fail(E_UNSUPPORTED, "the fused head is the Humanoid step's");
  rc = check_noise(d, b);
  if (rc) return rc;
  EnvInfo ei = env_info(d->env_id);
  const bool gauss = head == MRL_HEAD_GAUSS;
  if (n_out != ei.act || gauss == (bool)ei.discrete || (!gauss && head != MRL_HEAD_SOFTMAX))
    return fail(E_ARG, "policy head does not match the env");
  if (gauss && !logstd) return fail(E_ARG, "DiagGauss needs logstd");
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const int D = ei.obs + 1;
  const dim3 genv((d->n_envs + 63) / 64), gpart(a.nb, (D + LCOLS - 1) / LCOLS);
  hipStream_t s = (hipStream_t)stream;
  if (roll_eval(d)) {
    launch_lrollout_act_eval(a, z, hr, logstd, t, s);
    return hip_check(hipGetLastError(), "mrl_rollout_act");
  }
  if (d->env_id == MRL_ENV_HUMANOID) MRL_LAUNCH_HM(hm_act_kernel, hm_lds_bytes, d->n_envs, s, a, z, hr, logstd, t);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, lrollout_act_kernel, genv, dim3(64), 0, s, a, z, logstd, t);
  hipLaunchKernelGGL(lrollout_partials_kernel, gpart, dim3(RB), 0, s, a, D, (t + 1) & 1, 1);
  return hip_check(hipGetLastError(), "mrl_rollout_act");
}

int mrl_rollout_act(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* z, const float* logstd,
                    const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!z) return fail(E_ARG, "null z rows");
  return rollout_act(d, head, n_out, z, HeadRows{nullptr, nullptr, nullptr, 0, 0, nullptr}, logstd, b, t, stream);
}

int mrl_rollout_act_head(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const float* hidden,
                         int32_t n_hidden, const float* w_head, const float* b_head, const float* logstd,
                         const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!d || !hidden || !w_head || !b_head || n_hidden <= 0) return fail(E_ARG, "mrl_rollout_act_head: bad arguments");
  if (d->env_id != MRL_ENV_HUMANOID || n_out != HM_ACT)
    return fail(E_UNSUPPORTED, "mrl_rollout_act_head: the fused head is the Humanoid step's (17 outputs)");
  return rollout_act(d, head, n_out, nullptr,
                     HeadRows{hidden, w_head, b_head, n_hidden, (int)(roll_compute(d) == MRL_COMPUTE_BF16), nullptr}, logstd,
                     b, t, stream);
}

int mrl_rollout_act_head_bf16(const mrl_rollout_desc* d, int32_t head, int32_t n_out, const uint16_t* hidden16,
                              int32_t n_hidden, const float* w_head, const float* b_head, const float* logstd,
                              const mrl_rollout_bufs* b, int32_t t, void* stream) {
  if (!d || !hidden16 || !w_head || !b_head || n_hidden <= 0)
    return fail(E_ARG, "mrl_rollout_act_head_bf16: bad arguments");
  if (d->env_id != MRL_ENV_HUMANOID || n_out != HM_ACT)
    return fail(E_UNSUPPORTED, "mrl_rollout_act_head_bf16: the fused head is the Humanoid step's (17 outputs)");
  if (roll_compute(d) != MRL_COMPUTE_BF16) return fail(E_ARG, "mrl_rollout_act_head_bf16: bf16 hidden rows need MRL_COMPUTE_BF16");
  return rollout_act(d, head, n_out, nullptr, HeadRows{nullptr, w_head, b_head, n_hidden, 1, hidden16}, logstd, b, t,
                     stream);
}

}  // extern "C"
