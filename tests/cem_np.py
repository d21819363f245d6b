"""float64 numpy twin of the cross-entropy path (test helper, not collected):
the ``cem`` update (elite order, mean, variance, std schedule), the deterministic policy
forward on filtered observations, and the per-candidate Welford partial."""
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


def split_theta(theta, n_in, n_out):
    """Keras order: W0 [n_in, 64], b0, W1 [64, 64], b1, W2 [64, n_out], b2 (, logstd)."""
    th = np.asarray(theta, dtype=np.float64)
    o, parts = 0, []
    for (r, c) in ((n_in, 64), (64, 64), (64, n_out)):
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


def forward(thetas, x, n_out):
    """Head rows z [N, n_out] of candidate i's net on its row x[i] (thetas [N, P] or [P])."""
    x = np.asarray(x, dtype=np.float64)
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim == 1:
        thetas = np.broadcast_to(thetas, (x.shape[0], thetas.size))
    z = np.zeros((x.shape[0], n_out))
    for i in range(x.shape[0]):
        (W0, b0), (W1, b1), (W2, b2) = split_theta(thetas[i], x.shape[1], n_out)
        z[i] = np.tanh(np.tanh(x[i] @ W0 + b0) @ W1 + b1) @ W2 + b2
    return z


def welford_partial(rows):
    """count, mean, M2 of the rows [n, O] (two-pass)."""
    r = np.asarray(rows, dtype=np.float64)
    m = r.mean(axis=0)
    return np.concatenate([[float(r.shape[0])], m, np.square(r - m).sum(axis=0)])
