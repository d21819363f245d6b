"""Wall time of one PpoClipUpdater.update and one PpoSgdUpdater.update on the same Hopper
batch (256 envs x 256 steps, 1 epoch), with modular_rl_amd.timing.

    python tools/ppo_update_time.py [--reps 3]
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, '.')
from modular_rl_amd import agentzoo, timing  # noqa: E402
from modular_rl_amd.core import compute_advantage_batch  # noqa: E402
from modular_rl_amd.envs import make  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    env = make("Hopper-v2")
    cfg = dict(n_envs=256, horizon=256, timestep_limit=1000, epochs=1, seed=1, use_graph=0)
    out = {}
    for name in ("PpoClipAgent", "PpoSgdAgent"):
        agent = getattr(agentzoo, name)(env.observation_space, env.action_space, cfg)
        batch = agent.make_collector(env).collect()
        compute_advantage_batch(agent.baseline, batch, 0.995, 0.97)
        theta = agent.policy.get_flat()
        np.random.seed(0)
        agent.updater.update(batch)          # warm-up: workspaces, kernel load
        timing.enable(True)
        for _ in range(args.reps):
            agent.policy.set_from_flat(theta)
            timing.tick()
            timing.start(name)
            agent.updater.update(batch)
            timing.stop(name)
        count, mean_ms, _ = timing.summary()[name]
        timing.enable(False)
        out[name] = dict(rows=int(batch.n), reps=int(count), update_ms=float(mean_ms))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
