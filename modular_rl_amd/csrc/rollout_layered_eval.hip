// The evaluation instantiations (MRL_ROLLOUT_EVAL, include/mrl_hip.h) of the layered rollout's
// obs and act kernels and of Humanoid's wave-per-env step, as a unit of their own: the kernel
// templates of rollout_layered_kernels.h with EV = true, behind launch_lrollout_*_eval
// (rollout_host.h) for rollout_layered.hip's entry points.  No partials launch follows an
// evaluation step: there is nothing to merge.
#include "rollout_host.h"
#include "rollout_layered_kernels.h"

namespace mrl {

void launch_lrollout_obs_eval(const RollArgs& a, int t, hipStream_t s) {
  const dim3 grid(a.nb, (env_info(a.d.env_id).obs + 1 + LCOLS - 1) / LCOLS);
  dispatch_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((lrollout_obs_kernel<env(), true>), grid, dim3(RB), 0, s, a, t);
  });
}
void launch_lrollout_act_eval(const RollArgs& a, const float* z, const HeadRows& hr, const float* logstd, int t,
                              hipStream_t s) {
  const int E = a.d.n_envs;
  if (a.d.env_id == MRL_ENV_HUMANOID) {
    const int wpb = hm_wpb();
    const dim3 grid((E + wpb - 1) / wpb), block(64 * wpb);
    const size_t lds = hm_lds_bytes(wpb, E);
    if (wpb == 4) hipLaunchKernelGGL((hm_act_kernel<4, true>), grid, block, lds, s, a, z, hr, logstd, t);
    else hipLaunchKernelGGL((hm_act_kernel<1, true>), grid, block, lds, s, a, z, hr, logstd, t);
    return;
  }
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((lrollout_act_kernel<env(), true>), dim3((E + 63) / 64), dim3(64), 0, s, a, z, logstd, t);
  });
}

}  // namespace mrl
