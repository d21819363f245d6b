"""Shapes, seeds and float64 reference runs shared by the classic-control env tests (test
helper, not collected): the CPU tests check on the twin that the chosen seeds keep clear of
float-rounding ties, the GPU tests then hold the device to exact actions on those seeds."""
import numpy as np

from oracle import philox
from oracle import rollout_np as RO
from oracle import trpo_np as T
from tests import cem_np
from tests.classic_envs_np import KINDS, ClassicEnvs

ENV_IDS = ("Pendulum-v0", "MountainCar-v0", "Acrobot-v1")
# env -> (obs, act, discrete, TimeLimit)
SHAPES = {"Pendulum-v0": (3, 1, False, 200), "MountainCar-v0": (2, 3, True, 200), "Acrobot-v1": (6, 3, True, 500)}

# (E, T, limit, inject) of the rollout-against-collect comparison: one partial block with
# injected noise, three blocks (the last partial) cut at 9, and one env alone
ROLLOUT_CASES = ((7, 30, 12, True), (130, 16, 9, False), (1, 40, 200, False))
LAYERED_CASE = ("Acrobot-v1", [32], 70, 12, 5)  # env, hid_sizes, E, T, limit (cuts inside T)

POP_N, POP_LIMIT = 96, 25
POP_SEEDS = {"Pendulum-v0": 11, "MountainCar-v0": 12, "Acrobot-v1": 13}


def policy_theta(env_id, hid, seed):
    """(spec, theta) of the test policies: Glorot + 0.1 normal, rounded to float32 values."""
    O, A, disc, _ = SHAPES[env_id]
    head = "softmax" if disc else "gauss"
    rng = np.random.default_rng(seed)
    spec = T.Spec(O, list(hid), A, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.1 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-A:] = -0.5 + 0.1 * rng.standard_normal(A)
    return spec, th.astype(np.float32).astype(np.float64)


def rollout_seeds(E):
    """(policy seed, collector seed) of a rollout case."""
    return E, 1234 + E


def rollout_noise(env_id, E, Tn, it):
    rng = np.random.default_rng(it)
    return rng.random((Tn, E)) if SHAPES[env_id][2] else rng.standard_normal((Tn, E, SHAPES[env_id][1]))


def reference_rollout(env_id, hid, E, Tn, limit, inject, iterations=2):
    """oracle.rollout_np.collect on the twin: a list of (trajectory dict, filter state after,
    noise or None, margin) per iteration; margin [Tn, E] = min_q |cs_q - u| of the Categorical
    draw (None for Pendulum)."""
    pseed, seed = rollout_seeds(E)
    spec, th = policy_theta(env_id, hid, pseed)
    envs = ClassicEnvs(KINDS[env_id], E, seed)
    fs = RO.FilterState(envs.O + 1)
    out = []
    for it in range(iterations):
        noise = rollout_noise(env_id, E, Tn, it) if inject else None
        want, fs = RO.collect(envs, fs, spec, th, Tn, limit, it, filt=True, noise=noise)
        margin = None
        if envs.discrete:
            cs = np.cumsum(want["prob"], axis=2, dtype=np.float32).astype(np.float64)
            if noise is not None:
                u = noise
            else:
                u = np.stack([philox.uniform2(seed, 0, envs.gid, np.uint64(it * Tn + t), 0)[0] for t in range(Tn)])
            margin = np.abs(cs - u[:, :, None]).min(axis=2)
        out.append((want, fs.copy(), noise, margin))
    return spec, th, out


def population(env_id, n, seed, spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P] (test_gpu_cem's populations)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    O, A, disc, _ = SHAPES[env_id]
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, O, A, _lib.HEAD_SOFTMAX if disc else _lib.HEAD_GAUSS)
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)


def reference_population(env_id):
    """The population rollout on the twin (no filter state: observations clipped only, float64
    arg-max / Gauss mean).  Returns (rows, clear): live (step, env) rows, and those whose top
    two logits are more than 1e-4 apart (all of them for Pendulum)."""
    O, A, disc, _ = SHAPES[env_id]
    seed = POP_SEEDS[env_id]
    th = population(env_id, POP_N, seed).astype(np.float64)
    envs = ClassicEnvs(KINDS[env_id], POP_N, seed)
    envs.reset(np.arange(POP_N))
    alive = np.ones(POP_N, dtype=bool)
    rows = clear = 0
    for t in range(POP_LIMIT):
        if not alive.any():
            break
        z = cem_np.forward_64_64(th, cem_np.filter_obs(envs.obs()), A)
        rows += int(alive.sum())
        if disc:
            srt = np.sort(z, axis=1)
            clear += int(((srt[:, -1] - srt[:, -2]) > 1e-4)[alive].sum())
            act = np.argmax(z, axis=1)
        else:
            clear += int(alive.sum())
            act = z.astype(np.float32)
        _, done = envs.step(act)
        alive &= ~done
    return rows, clear
