"""One generation's Humanoid population rollout (WavePopulationRollout, 200 candidates, limit 1000)
against as many live env steps through VecEnv.step: stream events, median of 7 after 2 warm-up
calls.  Usage: python tools/measure_hm_pop.py [OUT.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modular_rl_amd import _lib  # noqa: E402
from modular_rl_amd.envs import VecEnv, WavePopulationRollout  # noqa: E402
from modular_rl_amd.nets import glorot_init  # noqa: E402

N, LIMIT, REPS, WARM = 200, 1000, 7, 2


def timed(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(m) for m in ms]


def pop_case(hid, thetas, shared):
    pop = WavePopulationRollout("Humanoid-v2", N, seed=3, timestep_limit=LIMIT, hid_sizes=hid)
    th = torch.as_tensor(thetas).cuda()

    def run():
        pop.episodes_started.zero_()  # the same episodes every repetition
        (pop.evaluate if shared else pop)(th)

    med, all_ms = timed(run)
    L = pop.len.cpu().numpy()
    return dict(hid=list(hid), shared=shared, ms=med, all_ms=all_ms, live_steps=int(L.sum()), max_len=int(L.max()),
                mean_len=float(L.mean()), us_per_live_step=1e3 * med / int(L.sum()),
                us_per_step_of_longest=1e3 * med / int(L.max()))


out = {"n": N, "limit": LIMIT, "reps": REPS, "warmup": WARM, "device": torch.cuda.get_device_name(0)}
rng = np.random.default_rng(0)
# generation 0 of the battery line: glorot mean, initial_std 1
base = glorot_init(rng, 376, 17, _lib.HEAD_GAUSS, [10, 5])
th = (base[None, :] + rng.standard_normal((N, base.size))).astype(np.float32)
out["battery_gen0"] = pop_case((10, 5), th, False)
# theta = 0: the action is 0 whatever the shape, so every shape runs the SAME episodes and the
# differences between them are the forward's cost alone
out["zero_policy"] = []
for hid in ((), (10, 5), (64, 64)):
    P = 17 + sum(a * b + b for a, b in zip([376, *hid], [*hid, 17]))
    out["zero_policy"].append(pop_case(hid, np.zeros(P, dtype=np.float32), True))

# the launch-per-step path: VecEnv.step with a fixed action, as many live steps
env = VecEnv("Humanoid-v2", N, seed=3)
env.reset()
act = torch.zeros(N, 17, dtype=torch.float32, device="cuda")
for live in sorted({out["battery_gen0"]["live_steps"], out["zero_policy"][1]["live_steps"]}):
    K = max(1, -(-live // N))

    def run():
        for _ in range(K):
            env.step(act)

    med, all_ms = timed(run)
    out.setdefault("vecenv", []).append(dict(launches=K, live_steps=K * N, ms=med, all_ms=all_ms,
                                             us_per_live_step=1e3 * med / (K * N), us_per_launch=1e3 * med / K))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
