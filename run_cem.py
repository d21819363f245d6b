#!/usr/bin/env python
"""Run the cross-entropy method (`run_cem.py` of the reference) on the MI355X path.

    python run_cem.py --env CartPole-v0 --agent modular_rl_amd.agentzoo.DeterministicAgent \
        --batch_size 64 --n_iter 3

Same two-phase argparse as the reference (`run_cem.py:14-29`): GENERAL_OPTIONS + --env/--agent
first, then the agent class's ``options`` and ``CEM_OPTIONS``; ``timestep_limit`` defaults to
the env's max_episode_steps (`run_cem.py:35-36`); the callback prints the per-iteration table
(`run_cem.py:41-49`).  ``--snapshot_every`` writes agent snapshots as array files
(modular_rl_amd/checkpoint.py) and ``--load_snapshot`` starts from one (parameters and filter
state; generations count from 0).  The reference's gym monitor, video and h5 log are not kept.
"""
import argparse
import os
import sys

import numpy as np

from modular_rl_amd.cem import CEM_OPTIONS, run_cem_algorithm
from modular_rl_amd.checkpoint import load_snapshot, save_snapshot
from modular_rl_amd.core import get_agent_cls
from modular_rl_amd.envs import make
from modular_rl_amd.misc_utils import GENERAL_OPTIONS, update_argument_parser


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    update_argument_parser(parser, GENERAL_OPTIONS)
    parser.add_argument("--env", default="CartPole-v0")
    parser.add_argument("--agent", default="modular_rl_amd.agentzoo.DeterministicAgent")
    args, _ = parser.parse_known_args([a for a in argv if a not in ("-h", "--help")])
    env = make(args.env)
    env_spec = env.spec
    agent_ctor = get_agent_cls(args.agent)
    update_argument_parser(parser, agent_ctor.options)
    update_argument_parser(parser, CEM_OPTIONS)
    args = parser.parse_args(argv)
    if args.timestep_limit == 0:
        args.timestep_limit = env_spec.max_episode_steps
    cfg = args.__dict__
    np.random.seed(args.seed)
    agent = agent_ctor(env.observation_space, env.action_space, cfg)
    counter = [0]
    if args.load_snapshot:  # parameters and filter state; the generations count from 0 again
        load_snapshot(args.load_snapshot, agent)

    def callback(stats):
        print("*********** Iteration %i ****************" % counter[0])
        for k, v in stats.items():
            if np.asarray(v).size == 1:
                print("%-10s %s" % (k, v))
        sys.stdout.flush()
        counter[0] += 1
        if args.snapshot_every and (counter[0] % args.snapshot_every == 0 or counter[0] == args.n_iter):
            base = os.path.splitext(args.outfile)[0]
            save_snapshot("%s.snap%04i.npz" % (base, counter[0]), agent, counter[0], env_spec.id)

    run_cem_algorithm(env, agent, callback=callback, usercfg=cfg)
    env.close()


if __name__ == "__main__":
    main()
