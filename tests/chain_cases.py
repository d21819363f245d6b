"""Shapes, seeds and float64 reference runs shared by the cart-and-pole env tests (test
helper, not collected): the CPU tests check on the twin that the chosen seeds keep every
compared state clear of the termination thresholds, the GPU tests then hold the device to
exact flags on those seeds."""
import functools

import numpy as np

from oracle import rollout_np as RO
from oracle import trpo_np as T
from tests import cem_np
from tests.classic_cases import ROLLOUT_CASES  # noqa: F401  (the rollout comparison's sizes)
from tests.mujoco_chains_np import KINDS, ChainEnvs, margin

ENV_IDS = ("InvertedPendulum-v2", "InvertedDoublePendulum-v2")
# env -> (obs, act, discrete, TimeLimit)
SHAPES = {"InvertedPendulum-v2": (4, 1, False, 1000), "InvertedDoublePendulum-v2": (11, 1, False, 1000)}
KIND_IDS = {"InvertedPendulum-v2": 8, "InvertedDoublePendulum-v2": 9}
NS = {"InvertedPendulum-v2": 4, "InvertedDoublePendulum-v2": 6}
ACT_HIGH = {"InvertedPendulum-v2": 3.0, "InvertedDoublePendulum-v2": 1.0}

# (E, Tn, limit) of the VecEnv comparison: one partial block; three blocks, the last partial
STEP_CASES = ((7, 30, 12), (150, 24, 9))
LAYERED_CASE = ("InvertedDoublePendulum-v2", [32], 70, 12, 5)  # env, hid_sizes, E, T, limit (cuts inside T)
# persistent launch against step launches: two blocks (the last partial), one partial block
PERSISTENT_CASES = ((100, 40, 15), (40, 24, 7))

POP_N, POP_LIMIT = 96, 25
POP_SEEDS = {"InvertedPendulum-v2": 21, "InvertedDoublePendulum-v2": 22}

MARGIN = 1e-6  # least distance to a termination threshold the GPU comparisons rely on


def step_seed(E):
    return 4242 + E


def step_actions(env_id, E, Tn):
    """3-sigma normal actions [Tn, E, 1] float32: the control clamp is hit."""
    return (3.0 * np.random.default_rng(E).standard_normal((Tn, E, SHAPES[env_id][1]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_steps(env_id, E, Tn, limit):
    """The VecEnv comparison's loop on the twin: per step (rew, ep_t, flags, final obs of the
    ended rows, obs, state, episodes started), after the reset's (obs, state); and the twin's
    least distance to the termination threshold."""
    envs = ChainEnvs(env_id, E, step_seed(E))
    actions = step_actions(env_id, E, Tn)
    envs.reset(np.arange(E))
    first = (envs.obs(), envs.state.copy())
    steps = []
    for t in range(Tn):
        rew, dn = envs.step(actions[t])
        ept = envs.ep_t.copy()
        term = dn | (ept + 1 >= envs.max_steps)
        last = term | (ept + 1 >= limit)
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


def rollout_seeds(E):
    """(policy seed, collector seed) of a rollout case."""
    return E, 1234 + E


def rollout_noise(env_id, E, Tn, it):
    return np.random.default_rng(it).standard_normal((Tn, E, SHAPES[env_id][1]))


@functools.lru_cache(maxsize=None)
def _reference_rollout(env_id, hid, E, Tn, limit, inject, iterations):
    pseed, seed = rollout_seeds(E)
    spec, th = policy_theta(env_id, hid, pseed)
    envs = ChainEnvs(KINDS[env_id], E, seed)
    fs = RO.FilterState(envs.O + 1)
    out = []
    for it in range(iterations):
        noise = rollout_noise(env_id, E, Tn, it) if inject else None
        want, fs = RO.collect(envs, fs, spec, th, Tn, limit, it, filt=True, noise=noise)
        out.append((want, fs.copy(), noise, envs.min_margin))
    return spec, th, out


def reference_rollout(env_id, hid, E, Tn, limit, inject, iterations=2):
    """oracle.rollout_np.collect on the twin: a list of (trajectory dict, filter state after,
    noise or None, least threshold distance so far) per iteration."""
    return _reference_rollout(env_id, tuple(hid), E, Tn, limit, inject, iterations)


def population(env_id, n, seed, spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P] (test_gpu_cem's populations)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    O, A, _, _ = SHAPES[env_id]
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, O, A, _lib.HEAD_GAUSS)
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_population(env_id):
    """The population rollout on the twin (no filter state: observations clipped only, the
    Gauss mean as the action).  Returns (live (step, env) rows, episodes the env itself
    ended, least threshold distance)."""
    O, A, _, _ = SHAPES[env_id]
    seed = POP_SEEDS[env_id]
    th = population(env_id, POP_N, seed).astype(np.float64)
    envs = ChainEnvs(KINDS[env_id], POP_N, seed)
    envs.reset(np.arange(POP_N))
    alive = np.ones(POP_N, dtype=bool)
    rows = ended = 0
    least = np.inf
    for t in range(POP_LIMIT):
        if not alive.any():
            break
        z = cem_np.forward_64_64(th, cem_np.filter_obs(envs.obs()), A)
        rows += int(alive.sum())
        _, done = envs.step(z.astype(np.float32))
        least = min(least, float(margin(envs.kind, envs.state)[alive].min()))
        ended += int((alive & done).sum())
        alive &= ~done
    return rows, ended, least
