// The evaluation instantiations (MRL_ROLLOUT_EVAL, include/mrl_hip.h) of the fused rollout's
// reset, step and persistent kernels, as a unit of their own: rollout.hip's kernel templates
// with EV = true, behind launch_rollout_*_eval (rollout_host.h).  Why they are not instantiated
// in rollout.hip itself is told there, at the launchers.
#define MRL_ROLLOUT_EVAL_UNIT 1
#include "rollout.hip"
