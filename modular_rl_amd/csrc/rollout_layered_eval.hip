// The evaluation instantiations (MRL_ROLLOUT_EVAL, include/mrl_hip.h) of the layered rollout's
// obs and act kernels and of Humanoid's wave-per-env step, as a unit of their own:
// rollout_layered.hip's kernel templates with EV = true, behind launch_lrollout_*_eval
// (rollout_host.h).
#define MRL_ROLLOUT_EVAL_UNIT 1
#include "rollout_layered.hip"
