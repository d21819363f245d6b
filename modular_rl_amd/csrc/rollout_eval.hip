// The evaluation instantiations (MRL_ROLLOUT_EVAL, include/mrl_hip.h) of the fused rollout's
// reset, step and persistent kernels, as a unit of their own: the kernel templates of
// rollout_kernels.h with EV = true, behind launch_rollout_*_eval (rollout_host.h) for
// rollout.hip's entry points.  Why they are not instantiated in rollout.hip itself is told at
// the top of rollout_kernels.h.
#include "rollout_host.h"
#include "rollout_kernels.h"

namespace mrl {

void launch_rollout_reset_eval(const RollArgs& a, hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    hipLaunchKernelGGL((rollout_reset_kernel<env(), true>), dim3(a.nb), dim3(RB), 0, s, a);
  });
}
void launch_rollout_step_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage, int t,
                              hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_step_kernel<env(), BF(), true>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage, t);
    });
  });
}
// independent blocks: no workspace, no residency check, no stamps
void launch_rollout_persistent_eval(const RollArgs& a, bool bf, const float* logstd, const float* rimage,
                                    hipStream_t s) {
  dispatch_thread_env(a.d.env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_persistent_kernel<env(), BF(), false, true>), dim3(a.nb), dim3(RB), 0, s, a, logstd,
                         rimage, nullptr);
    });
  });
}

}  // namespace mrl
