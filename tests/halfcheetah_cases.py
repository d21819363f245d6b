"""Shapes, seeds and float64 reference runs shared by the HalfCheetah-v2 tests (test helper, not
collected).  The env never ends an episode by itself, so, unlike the other envs' cases, no seed
has to keep clear of a termination threshold.  Its contact and stop forces are continuous in
position only (their dampers switch on at the threshold: tests/halfcheetah_np.py, TreeEnvs)."""
import functools

import numpy as np

from oracle import rollout_np as RO
from oracle import trpo_np as T
from tests.chain_cases import PERSISTENT_CASES, POP_LIMIT, POP_N, ROLLOUT_CASES, STEP_CASES  # noqa: F401
from tests.chain_cases import rollout_seeds, step_seed  # noqa: F401
from tests.halfcheetah_np import HALFCHEETAH, TreeEnvs

ENV_ID = "HalfCheetah-v2"
OBS, ACT, NS, LIMIT = 17, 6, 18, 1000
LAYERED_CASE = ([32], 70, 12, 5)  # hid_sizes, E, T, limit (cuts inside T)
POP_SEED = 25
SMALL_HID = (10, 5)


def step_actions(E, Tn):
    """3-sigma normal actions [Tn, E, 6] float32: the control clamp is hit."""
    return (3.0 * np.random.default_rng(E).standard_normal((Tn, E, ACT))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_steps(E, Tn, limit):
    """The VecEnv comparison's loop on the twin: per step (rew, ep_t, flags, final obs of the
    ended rows, obs, state, episodes started), after the reset's (obs, state)."""
    envs = TreeEnvs(ENV_ID, E, step_seed(E))
    actions = step_actions(E, Tn)
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
    return first, steps


def policy_theta(hid, seed):
    """(spec, theta) of the test policies: Glorot + 0.1 normal, rounded to float32 values."""
    rng = np.random.default_rng(seed)
    spec = T.Spec(OBS, list(hid), ACT, "gauss")
    th = T.mlp_init(rng, spec.shapes, True) + 0.1 * rng.standard_normal(spec.P)
    th[-ACT:] = -0.5 + 0.1 * rng.standard_normal(ACT)
    return spec, th.astype(np.float32).astype(np.float64)


def rollout_noise(E, Tn, it):
    return np.random.default_rng(it).standard_normal((Tn, E, ACT))


@functools.lru_cache(maxsize=None)
def _reference_rollout(hid, E, Tn, limit, inject, iterations):
    pseed, seed = rollout_seeds(E)
    spec, th = policy_theta(hid, pseed)
    envs = TreeEnvs(HALFCHEETAH, E, seed)
    fs = RO.FilterState(envs.O + 1)
    out = []
    for it in range(iterations):
        noise = rollout_noise(E, Tn, it) if inject else None
        want, fs = RO.collect(envs, fs, spec, th, Tn, limit, it, filt=True, noise=noise)
        out.append((want, fs.copy(), noise))
    return spec, th, out


def reference_rollout(hid, E, Tn, limit, inject, iterations=2):
    """oracle.rollout_np.collect on the twin: a list of (trajectory dict, filter state after,
    noise or None) per iteration."""
    return _reference_rollout(tuple(hid), E, Tn, limit, inject, iterations)


def population(n, seed, hid=(64, 64), spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P] (test_gpu_cem's populations)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, OBS, ACT, _lib.HEAD_GAUSS, [int(h) for h in hid])
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)
