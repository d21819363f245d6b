"""float64 numpy twin of the wave-per-candidate population rollout on Humanoid-v2 (test helper,
not collected): the policy forward at Humanoid's dims -- ``cem_np.forward`` takes
``[376, ..., 17]`` as it is --, the f32 error bound of the device forward, the test populations
and the CPU episode twin the replay test's seed was chosen on."""
import numpy as np

from tests import cem_np

ENV_ID = "Humanoid-v2"
OBS, ACT, _ = cem_np.ENVS[ENV_ID]
U = 2.0 ** -24  # unit roundoff of float32

forward = cem_np.forward


def dims_of(hid):
    return cem_np.dims_of(ENV_ID, hid)


def num_params(hid):
    return cem_np.num_params(dims_of(hid), True)


def population(hid, n, seed, spread=0.1):
    """theta_i = glorot + spread * normal, float32 [n, P]."""
    return cem_np.population(ENV_ID, hid, n, seed, spread)


def forward_with_bound(thetas, x, dims, c):
    """The float64 head rows z [N, 17] and, per entry, a bound on what an f32 forward of any
    summation order may differ from them by.

    Layer by layer, with e the bound on the layer's inputs (the f32 rounding of the filtered
    observation at the start: u |x|): the computed pre-activation of output j differs from the
    exact one of the exact inputs by at most
        sum_k e_k |W_kj|  +  c (din + 2) u (sum_k |x_k W_kj| + |b_j|)
    -- the inputs' error carried through the weights, plus the accumulation bound of din
    products, din - 1 sums and the bias in f32 (any order; Higham, gamma_n ~ n u).  tanh is
    1-Lipschitz, so a hidden unit inherits its pre-activation's bound, plus tanhf's own error,
    taken as 4 u (two f32 ulps just below 1)."""
    x = np.asarray(x, dtype=np.float64)
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim == 1:
        thetas = np.broadcast_to(thetas, (x.shape[0], thetas.size))
    z = np.zeros((x.shape[0], dims[-1]))
    tol = np.zeros_like(z)
    for i in range(x.shape[0]):
        parts = cem_np.split_theta(thetas[i], dims)
        h, e = x[i], U * np.abs(x[i])
        for l, (W, b) in enumerate(parts):
            pre = h @ W + b
            e = e @ np.abs(W) + c * (W.shape[0] + 2) * U * (np.abs(h) @ np.abs(W) + np.abs(b))
            if l < len(parts) - 1:
                h, e = np.tanh(pre), e + 4 * U
            else:
                z[i], tol[i] = pre, e
    return z, tol


def twin_episodes(thetas, seed, limit, hid=(10, 5)):
    """Candidate i's episode on the CPU oracle envs (oracle/rollout_np.Envs) under the float64
    forward on the clipped, f32-rounded raw observation: (len [N], terminated [N])."""
    from oracle import rollout_np as RO
    th = np.asarray(thetas, dtype=np.float64)
    n = th.shape[0]
    envs = RO.Envs(RO.HUMANOID, n, seed)
    envs.reset(np.arange(n))
    length = np.zeros(n, dtype=np.int64)
    term = np.zeros(n, dtype=bool)
    alive = np.ones(n, dtype=bool)
    for t in range(limit):
        z = forward(th, cem_np.filter_obs(envs.obs(), None), dims_of(hid))
        _, done = envs.step(z.astype(np.float32).astype(np.float64))
        ended = alive & (np.asarray(done, dtype=bool) | (t + 1 >= limit))
        length[ended] = t + 1
        term[ended] = np.asarray(done, dtype=bool)[ended]
        alive &= ~ended
        if not alive.any():
            break
    return length, term
