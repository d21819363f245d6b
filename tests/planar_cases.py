"""Shapes, seeds and float64 reference runs shared by the Reacher-v2 / Swimmer-v2 tests (test
helper, not collected): the CPU tests check on the twin that the chosen seeds keep every goal
candidate drawn clear of the disc's edge, the GPU tests then hold the device to the twin's
goals on those seeds."""
import functools

import numpy as np

from oracle import rollout_np as RO
from oracle import trpo_np as T
from tests import cem_np
from tests.chain_cases import MARGIN, PERSISTENT_CASES, POP_LIMIT, POP_N, ROLLOUT_CASES, STEP_CASES  # noqa: F401
from tests.chain_cases import rollout_seeds, step_seed  # noqa: F401
from tests.planar_chains_np import KINDS, PlanarEnvs

ENV_IDS = ("Reacher-v2", "Swimmer-v2")
# env -> (obs, act, discrete, TimeLimit)
SHAPES = {"Reacher-v2": (11, 2, False, 50), "Swimmer-v2": (8, 2, False, 1000)}
KIND_IDS = {"Reacher-v2": 12, "Swimmer-v2": 11}
NS = {"Reacher-v2": 6, "Swimmer-v2": 10}
ACT_HIGH = {"Reacher-v2": 1.0, "Swimmer-v2": 1.0}

REACHER_OWN_LIMIT_CASE = (7, 60, None)  # the env's own TimeLimit (50) ends every row inside the run
ALL_STEP_CASES = tuple((env_id, *case) for env_id in ENV_IDS for case in STEP_CASES) + (
    ("Reacher-v2", *REACHER_OWN_LIMIT_CASE),)
LAYERED_CASE =("Swimmer-v2", [32], 70, 12, 5)  # env, hid_sizes, E, T, limit (cuts inside T)
POP_SEEDS = {"Reacher-v2": 23, "Swimmer-v2": 24}
SMALL_HID = (10, 5)


def step_actions(env_id, E, Tn):
    """3-sigma normal actions [Tn, E, 2] float32: the control clamp is hit."""
    return (3.0 * np.random.default_rng(E).standard_normal((Tn, E, SHAPES[env_id][1]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_steps(env_id, E, Tn, limit):
    """The VecEnv comparison's loop on the twin: per step (rew, ep_t, flags, final obs of the
    ended rows, obs, state, episodes started), after the reset's (obs, state); and the twin's
    least distance of a goal candidate to the disc's edge.  limit None: the env's TimeLimit."""
    envs = PlanarEnvs(env_id, E, step_seed(E))
    actions = step_actions(env_id, E, Tn)
    envs.reset(np.arange(E))
    first = (envs.obs(), envs.state.copy())
    cut = envs.max_steps if limit is None else limit
    steps = []
    for t in range(Tn):
        rew, dn = envs.step(actions[t])
        ept = envs.ep_t.copy()
        term = dn | (ept + 1 >= envs.max_steps)
        last = term | (ept + 1 >= cut)
        envs.ep_t = ept + 1
        idx = np.nonzero(last)[0]
        fin = envs.obs()[idx]
        if len(idx):
            envs.reset(idx)
        steps.append(dict(rew=rew, ep_t=ept, term=term, last=last, idx=idx, final_obs=fin, obs=envs.obs(),
                          state=envs.state.copy(), ep_count=envs.ep_count.copy()))
    return first, steps, envs.min_margin


def policy_theta(env_id, hid, seed):
    """(spec, theta) of the test policies: Glorot + 0.1 normal, rounded to float32 values."""
    O, A, _, _ = SHAPES[env_id]
    rng = np.random.default_rng(seed)
    spec = T.Spec(O, list(hid), A, "gauss")
    th = T.mlp_init(rng, spec.shapes, True) + 0.1 * rng.standard_normal(spec.P)
    th[-A:] = -0.5 + 0.1 * rng.standard_normal(A)
    return spec, th.astype(np.float32).astype(np.float64)


def rollout_noise(env_id, E, Tn, it):
    return np.random.default_rng(it).standard_normal((Tn, E, SHAPES[env_id][1]))


@functools.lru_cache(maxsize=None)
def _reference_rollout(env_id, hid, E, Tn, limit, inject, iterations):
    pseed, seed = rollout_seeds(E)
    spec, th = policy_theta(env_id, hid, pseed)
    envs = PlanarEnvs(KINDS[env_id], E, seed)
    fs = RO.FilterState(envs.O + 1)
    out = []
    for it in range(iterations):
        noise = rollout_noise(env_id, E, Tn, it) if inject else None
        want, fs = RO.collect(envs, fs, spec, th, Tn, limit, it, filt=True, noise=noise)
        out.append((want, fs.copy(), noise, envs.min_margin))
    return spec, th, out


def reference_rollout(env_id, hid, E, Tn, limit, inject, iterations=2):
    """oracle.rollout_np.collect on the twin: a list of (trajectory dict, filter state after,
    noise or None, least goal-edge distance so far) per iteration."""
    return _reference_rollout(env_id, tuple(hid), E, Tn, limit, inject, iterations)


def population(env_id, n, seed, hid=(64, 64), spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P] (test_gpu_cem's populations)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    O, A, _, _ = SHAPES[env_id]
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, O, A, _lib.HEAD_GAUSS, [int(h) for h in hid])
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_population(env_id):
    """The population rollout on the twin (no filter state: observations clipped only, the
    Gauss mean as the action).  Returns (live (step, env) rows, episodes the env itself
    ended, least goal-edge distance)."""
    O, A, _, _ = SHAPES[env_id]
    seed = POP_SEEDS[env_id]
    th = population(env_id, POP_N, seed).astype(np.float64)
    envs = PlanarEnvs(KINDS[env_id], POP_N, seed)
    envs.reset(np.arange(POP_N))
    rows = ended = 0
    for t in range(POP_LIMIT):
        z = cem_np.forward_64_64(th, cem_np.filter_obs(envs.obs()), A)
        rows += POP_N
        _, done = envs.step(z.astype(np.float32))
        ended += int(done.sum())
    return rows, ended, envs.min_margin
