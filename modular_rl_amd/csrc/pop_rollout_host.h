// Host side of the population rollouts (pop_rollout*.hip), once: the argument checks the three
// entry points share and their order, the net's shape from (env, hid_sizes), the step limit and
// the common launch arguments.  The device side is pop_rollout_device.h.
#pragma once
#include <string>

#include "pop_rollout_device.h"
#include "rollout_host.h"

namespace mrl {

// The entry points' argument checks, in their order: the first one that fails, or null.  `own`
// is the entry point's own check (what it names, or null), between null bufs and null thetas:
// the policy desc of mrl_pop_rollout, pop_check_hid of the other two.
inline const char* pop_check_args(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const char* own,
                                  const float* thetas, const mrl_pop_io* io) {
  if (!d) return "null desc";
  if (!b) return "null bufs";
  if (own) return own;
  if (!thetas) return "null thetas";
  if (!io) return "null io";
  if (!env_known(d->env_id)) return "desc.env_id: unknown env";
  if (d->n_envs <= 0) return "desc.n_envs <= 0";
  if (!b->env_state) return "null bufs.env_state";
  if (!b->env_int) return "null bufs.env_int";
  if (!io->ret || !io->len || !io->flags || !io->stat) return "null io.ret / len / flags / stat";
  if (io->trace_steps < 0) return "io.trace_steps < 0";
  const bool any = io->trace_obs || io->trace_act || io->trace_rew || io->trace_steps > 0;
  const bool all = io->trace_obs && io->trace_act && io->trace_rew && io->trace_steps > 0;
  if (any && !all) return "the trace is only partly set (trace_steps, trace_obs, trace_act, trace_rew)";
  return nullptr;
}

inline const char* pop_check_hid(const int32_t* hid_sizes, int32_t n_hid) {
  if (n_hid < 0) return "n_hid < 0";
  if (n_hid > 0 && !hid_sizes) return "null hid_sizes";
  return nullptr;
}

// floats of theta the forward of the tanh MLP obs -> hid_sizes -> act reads (flat Keras order:
// every layer's kernel and bias); a Gauss head's logstd follows them
inline int64_t pop_forward_floats(const EnvInfo& ei, const int32_t* hid_sizes, int32_t n_hid) {
  int64_t P = 0, din = ei.obs;
  for (int l = 0; l < n_hid; ++l) {
    P += din * hid_sizes[l] + hid_sizes[l];
    din = hid_sizes[l];
  }
  return P + din * ei.act + ei.act;
}
inline int64_t pop_num_params(const EnvInfo& ei, int64_t forward_floats) {
  return forward_floats + (ei.discrete ? 0 : ei.act);
}

// The net's shape from the caller's arguments, for the lane kernels (wave = false: the
// thread-per-env envs) or the wave kernel (wave = true: Humanoid).  E_ARG: an unknown env,
// n_hid < 0, null hid_sizes with n_hid > 0; E_UNSUPPORTED: an env of the other kind, more than
// three hidden layers, a width outside [1, 64] -- where a _fits predicate answers 0.  `what`
// names the failed check.
inline int pop_net_shape(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid, bool wave, PopSmallShape& net,
                         const char*& what) {
  if (!env_known(env_id)) return what = "desc.env_id: unknown env", E_ARG;
  if ((what = pop_check_hid(hid_sizes, n_hid))) return E_ARG;
  if (wave != (env_id == MRL_ENV_HUMANOID))
    return what = wave ? "the wave-per-env envs only (Humanoid)" : "Humanoid is not supported (the thread-per-env envs only)",
           E_UNSUPPORTED;
  if (n_hid > POP_MAX_HID) return what = "more than 3 hidden layers", E_UNSUPPORTED;
  for (int l = 0; l < n_hid; ++l)
    if (hid_sizes[l] < 1 || hid_sizes[l] > POP_MAX_WIDTH) return what = "a hidden width outside [1, 64]", E_UNSUPPORTED;
  const EnvInfo ei = env_info(env_id);
  PopShape& sh = net.sh;
  sh.n_hid = n_hid;
  sh.dims[0] = ei.obs;
  for (int l = 0; l < n_hid; ++l) sh.dims[1 + l] = hid_sizes[l];
  sh.dims[n_hid + 1] = ei.act;
  for (int l = n_hid + 2; l < POP_MAX_HID + 2; ++l) sh.dims[l] = 0;
  net.PU = (int)pop_forward_floats(ei, hid_sizes, n_hid);
  net.maxw = 0;
  for (int l = 0; l <= n_hid + 1; ++l) net.maxw = sh.dims[l] > net.maxw ? sh.dims[l] : net.maxw;
  return OK;
}

// steps an episode may take: min(timestep_limit or MAX_STEPS, MAX_STEPS)
inline int pop_limit(const mrl_rollout_desc* d, const EnvInfo& ei) {
  return d->timestep_limit > 0 && d->timestep_limit < ei.max_steps ? d->timestep_limit : ei.max_steps;
}

// the five common fields of a kernel's argument block
template <class Args>
inline void pop_fill(Args& p, const mrl_rollout_desc* d, const float* thetas, int64_t ld_theta, const double* filter_state,
                     const mrl_pop_io* io) {
  p.thetas = thetas;
  p.ld = ld_theta;
  p.fstate = filter_state;
  p.io = *io;
  p.limit = pop_limit(d, env_info(d->env_id));
}

}  // namespace mrl
