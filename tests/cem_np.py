"""float64 numpy twin of the cross-entropy path (test helper, not collected):
the ``cem`` update (elite order, mean, variance, std schedule), the deterministic policy
forward of a tanh MLP of any depth on filtered observations (the 64-64 net is dims
``[n_in, 64, 64, n_out]``), the env table, the test populations and the per-candidate Welford
partial."""
import numpy as np


def n_elite_of(batch_size, elite_frac):
    return int(np.round(batch_size * elite_frac))


def sample_std_of(th_std, extra_std, iteration, std_decay_time):
    return np.sqrt(th_std + np.square(extra_std) * max(1.0 - iteration / float(std_decay_time), 0))


def elite_order(ys, n_elite):
    """Indices of the n_elite largest ys under the total order (y, index), NaN lowest,
    ascending."""
    ys = np.asarray(ys, dtype=np.float64)
    key = sorted(range(len(ys)), key=lambda i: ((0, 0.0, i) if np.isnan(ys[i]) else (1, ys[i], i)))
    return np.array(key[len(ys) - n_elite:], dtype=np.int64)


def refit(ths, ys, n_elite):
    ths = np.asarray(ths, dtype=np.float64)
    idx = elite_order(ys, n_elite)
    el = ths[idx]
    return el.mean(axis=0), el.var(axis=0), idx


def cem_replay(pops, yss, th_mean, batch_size, elite_frac, initial_std, extra_std, std_decay_time):
    """The generator's outputs when generation g draws ``pops[g]`` and scores ``yss[g]``."""
    n_elite = n_elite_of(batch_size, elite_frac)
    th_std = np.ones(np.asarray(th_mean).size) * initial_std
    out = []
    for it, (ths, ys) in enumerate(zip(pops, yss)):
        std = sample_std_of(th_std, extra_std, it, std_decay_time)
        th_mean, th_std, _ = refit(ths, ys, n_elite)
        out.append({"ys": np.asarray(ys), "th": th_mean, "ymean": np.mean(ys), "std": std})
    return out


# env -> (obs, act, head is gauss)
ENVS = {
    "CartPole-v0": (4, 2, False), "Hopper-v2": (11, 3, True), "Pendulum-v0": (3, 1, True),
    "MountainCar-v0": (2, 3, False), "Acrobot-v1": (6, 3, False), "InvertedPendulum-v2": (4, 1, True),
    "InvertedDoublePendulum-v2": (11, 1, True), "Humanoid-v2": (376, 17, True),
}


def dims_of(env_id, hid):
    O, A, _ = ENVS[env_id]
    return [O, *[int(h) for h in hid], A]


def num_params(dims, gauss):
    """Keras count: every layer's kernel and bias, plus logstd for a Gauss head."""
    return sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1)) + (dims[-1] if gauss else 0)


def split_theta(theta, dims):
    """Keras order: W0 [dims[0], dims[1]], b0, W1, b1, ... (, logstd): the (W, b) pairs."""
    th = np.asarray(theta, dtype=np.float64)
    o, parts = 0, []
    for r, c in zip(dims[:-1], dims[1:]):
        W = th[o:o + r * c].reshape(r, c)
        o += r * c
        b = th[o:o + c]
        o += c
        parts.append((W, b))
    return parts


def filter_obs(obs, filter_state=None, clip=5.0):
    """ZFilter with a frozen state (n_obs, n_rew, M[D], S[D]); None or n < 2: clip only.
    Rounded to float32 as the policy's input is."""
    o = np.asarray(obs, dtype=np.float64)
    O = o.shape[-1]
    if filter_state is not None and filter_state[0] >= 2:
        fs = np.asarray(filter_state, dtype=np.float64)
        n, M, S = fs[0], fs[2:2 + O], fs[2 + O + 1:2 + O + 1 + O]
        o = (o - M) / (np.sqrt(S / (n - 1)) + 1e-8)
    return np.clip(o, -clip, clip).astype(np.float32).astype(np.float64)


def forward(thetas, x, dims):
    """Head rows z [N, dims[-1]] of candidate i's net on its row x[i] (thetas [N, P] or [P]);
    tanh on every hidden layer, none on the head; no hidden layer: x @ W + b."""
    x = np.asarray(x, dtype=np.float64)
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim == 1:
        thetas = np.broadcast_to(thetas, (x.shape[0], thetas.size))
    z = np.zeros((x.shape[0], dims[-1]))
    for i in range(x.shape[0]):
        parts = split_theta(thetas[i], dims)
        h = x[i]
        for W, b in parts[:-1]:
            h = np.tanh(h @ W + b)
        W, b = parts[-1]
        z[i] = h @ W + b
    return z


def forward_64_64(thetas, x, n_out):
    """forward at the env's 64-64 net, [n_in, 64, 64, n_out]."""
    return forward(thetas, x, [np.shape(x)[1], 64, 64, n_out])


def population(env_id, hid, n, seed, spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P]."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    O, A, gauss = ENVS[env_id]
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, O, A, _lib.HEAD_GAUSS if gauss else _lib.HEAD_SOFTMAX, [int(h) for h in hid])
    assert base.size == num_params(dims_of(env_id, hid), gauss)
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)


def welford_partial(rows):
    """count, mean, M2 of the rows [n, O] (two-pass)."""
    r = np.asarray(rows, dtype=np.float64)
    m = r.mean(axis=0)
    return np.concatenate([[float(r.shape[0])], m, np.square(r - m).sum(axis=0)])
