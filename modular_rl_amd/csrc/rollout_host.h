// Host-side glue shared by the rollout units -- rollout.hip and rollout_layered.hip with their
// evaluation units rollout_eval.hip and rollout_layered_eval.hip, env_api.hip and the
// population rollouts pop_rollout*.hip (whose own checks and shapes are pop_rollout_host.h's,
// over pop_rollout_device.h): the descriptor checks, the launch arguments,
// the dispatch of an env id (over rollout_device.h's MRL_ENV_LIST) or a flag onto a kernel
// template, and the launch of the Humanoid wave-per-env kernels.  The error state (fail /
// hip_check, mrl_common.h) is mlp_kernels.hip's.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "rollout_device.h"

namespace mrl {

// desc.compute: the policy net's dtype, and the evaluation flag beside it (MRL_ROLLOUT_EVAL)
inline int roll_compute(const mrl_rollout_desc* d) { return d->compute & ~MRL_ROLLOUT_EVAL; }
inline bool roll_eval(const mrl_rollout_desc* d) { return (d->compute & MRL_ROLLOUT_EVAL) != 0; }

inline int check_roll(const mrl_rollout_desc* d, const mrl_rollout_bufs* b) {
  if (!d || !b) return fail(E_ARG, "null desc/bufs");
  if (!env_known(d->env_id)) return fail(E_UNSUPPORTED, "unknown env_id");
  if (d->n_envs <= 0 || d->horizon <= 0 || d->timestep_limit <= 0) return fail(E_ARG, "bad sizes");
  if (roll_compute(d) != MRL_COMPUTE_F32 && roll_compute(d) != MRL_COMPUTE_BF16) return fail(E_ARG, "bad compute");
  if (!b->env_state || !b->env_int || !b->filter_state || !b->records || !b->iteration) return fail(E_ARG, "null state");
  return OK;
}

// the sampling-noise rows of a step: required in training, refused in evaluation, which draws none
inline int check_noise(const mrl_rollout_desc* d, const mrl_rollout_bufs* b) {
  if (roll_eval(d)) {
    if (b->noise) return fail(E_ARG, "bufs.noise: MRL_ROLLOUT_EVAL takes the head's mode and reads no noise rows");
    return OK;
  }
  if (!b->noise) return fail(E_ARG, "bufs.noise: sampling-noise rows (mrl_rollout_noise or injected) required");
  return OK;
}

// blocks of ENVS_PER_BLOCK envs (or filter rows) covering n
inline int64_t env_blocks(int64_t n) { return (n + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK; }

inline RollArgs make_args(const mrl_rollout_desc* d, const mrl_rollout_bufs* b) {
  RollArgs a;
  a.d = *d;
  a.b = *b;
  a.nb = (int)env_blocks(d->n_envs);
  a.FS = filt_doubles(env_info(d->env_id).obs);
  a.RS = a.FS;
  return a;
}

inline int check_fused_policy(const mrl_rollout_desc* d, const mrl_mlp_desc* pol) {
  EnvInfo ei = env_info(d->env_id);
  const bool gauss = pol->head == MRL_HEAD_GAUSS;
  if (pol->n_in != ei.obs || pol->n_out != ei.act || gauss == (bool)ei.discrete || pol->n_hidden != HID ||
      pol->n_layers != 2)
    return fail(E_ARG, "policy shape does not match the env");
  return OK;
}

// the arguments mrl_rollout_run and mrl_rollout_step share
inline int check_fused_run(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, const float* rimage,
                           const mrl_rollout_bufs* b) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (!pol || !theta || !rimage) return fail(E_ARG, "null policy");
  if (d->env_id == MRL_ENV_HUMANOID) return fail(E_UNSUPPORTED, "Humanoid runs on the layered rollout");
  if (!b->obs || !b->act || !b->prob || !b->rew || !b->flags || !b->ep_t) return fail(E_ARG, "null trajectory buffer");
  rc = check_noise(d, b);
  if (rc) return rc;
  return check_fused_policy(d, pol);
}

// ------------------------------------------------------------------ dispatch
// A kernel template <int ENV> launched for a run-time env id, f(integral_constant<int, ENV>)
// over MRL_ENV_LIST: every env (an id that is not in the list goes to Humanoid) ...
template <class F>
inline void dispatch_env(int id, F&& f) {
#define MRL_ENV_CASE(ID, E) \
  if (id == ID) return f(std::integral_constant<int, ID>{});
  MRL_ENV_LIST(MRL_ENV_CASE, MRL_ENV_CASE)
#undef MRL_ENV_CASE
  f(std::integral_constant<int, MRL_ENV_HUMANOID>{});
}
#define MRL_DISPATCH_ENV(id, KERNEL, ...) \
  dispatch_env((id), [&](auto env) { hipLaunchKernelGGL(KERNEL<env()>, __VA_ARGS__); })

// ... or those that are stepped by a thread per env (all but Humanoid: the callers have
// turned it away or launch its wave-per-env kernel; any other id goes to Hopper)
template <class F>
inline void dispatch_thread_env(int id, F&& f) {
#define MRL_ENV_CASE(ID, E) \
  if (id == ID) return f(std::integral_constant<int, ID>{});
  MRL_ENV_LIST(MRL_ENV_CASE, MRL_ENV_NONE)
#undef MRL_ENV_CASE
  f(std::integral_constant<int, MRL_ENV_HOPPER>{});
}
#define MRL_DISPATCH_THREAD_ENV(id, KERNEL, ...) \
  dispatch_thread_env((id), [&](auto env) { hipLaunchKernelGGL(KERNEL<env()>, __VA_ARGS__); })

// a run-time flag as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
inline void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// one block's LDS on gfx950 (a CU's whole 160 KB)
constexpr size_t LDS_PER_BLOCK = 160 * 1024;

// ------------------------------------------------------------------ Humanoid launch
// Dynamic LDS padding for the wave-per-env Humanoid step: while the envs fit one wave
// per SIMD, at most 4 blocks (waves) may share a CU, so the dispatcher cannot stack two
// latency chains on one SIMD and leave another idle.
inline size_t hm_lds_pad(int n_envs) {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      ncu = n;
    else
      ncu = -1;
  }
  if (ncu <= 0 || n_envs > 4 * ncu) return 0;
  constexpr size_t used = sizeof(hm::Wave) + sizeof(hm::Shared), want = LDS_PER_BLOCK / 5 + 1024;
  return used < want ? want - used : 0;
}
// MRL_HM_WPB (per launch): four envs per block (hm_block, the default) or 1
inline int hm_wpb() {
  // r04i (C5 bf16, 1024 envs): the rollout alone 225 -> 212 ms per iteration, beside the
  // co-scheduled fit 269 -> 260 ms (one table copy per four envs, 94 KB of LDS per CU)
  const char* e = getenv("MRL_HM_WPB");
  return (e && atoi(e) == 1) ? 1 : 4;
}
// dynamic LDS of a launch (the static tables / state come on top): the WPB = 4 states, and
// for the step kernels the one-wave block's padding
inline size_t hm_lds_state(int wpb, int) { return wpb == 1 ? 0 : (size_t)wpb * sizeof(hm::Wave); }
inline size_t hm_lds_bytes(int wpb, int n_envs) { return wpb == 1 ? hm_lds_pad(n_envs) : hm_lds_state(wpb, n_envs); }

// a kernel template <int WPB> over n_envs envs, a wave each: hm_wpb() envs per block, LDS
// (hm_lds_state for the reset kernels, hm_lds_bytes for the step kernels) bytes of dynamic LDS
#define MRL_LAUNCH_HM(KERNEL, LDS, n_envs, stream, ...)                                  \
  do {                                                                                   \
    const int wpb_ = hm_wpb();                                                           \
    const dim3 gb_(((n_envs) + wpb_ - 1) / wpb_), bb_(64 * wpb_);                         \
    const size_t lds_ = LDS(wpb_, (n_envs));                                             \
    if (wpb_ == 4) hipLaunchKernelGGL(KERNEL<4>, gb_, bb_, lds_, (stream), __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL<1>, gb_, bb_, lds_, (stream), __VA_ARGS__);           \
  } while (0)

// hm_env_reset_kernel / hm_env_step_kernel (rollout_layered.hip) for mrl_env_reset / mrl_env_step
void launch_hm_env_reset(const RollArgs& a, const mrl_env_io& io, hipStream_t s);
void launch_hm_env_step(const RollArgs& a, const mrl_env_io& io, int auto_reset, hipStream_t s);

// The evaluation instantiations (MRL_ROLLOUT_EVAL) of the kernel templates of rollout_kernels.h
// and rollout_layered_kernels.h, defined in rollout_eval.hip and rollout_layered_eval.hip for the
// entry points of rollout.hip and rollout_layered.hip, which have checked the arguments.
void launch_rollout_reset_eval(const RollArgs& a, hipStream_t s);
void launch_rollout_step_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage, int t,
                              hipStream_t s);
void launch_rollout_persistent_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage,
                                    hipStream_t s);
struct HeadRows;
void launch_lrollout_obs_eval(const RollArgs& a, int t, hipStream_t s);
void launch_lrollout_act_eval(const RollArgs& a, const float* z, const HeadRows& hr, const float* logstd, int t,
                              hipStream_t s);

}  // namespace mrl
