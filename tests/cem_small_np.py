"""float64 numpy twin of the small-net population rollout (test helper, not collected): the
deterministic policy forward of a tanh MLP of any depth, and the zero-padding of a two-layer
net to the 64-64 shape of ``mrl_pop_rollout``."""
import numpy as np

# env -> (obs, act, head is gauss)
ENVS = {
    "CartPole-v0": (4, 2, False), "Hopper-v2": (11, 3, True), "Pendulum-v0": (3, 1, True),
    "MountainCar-v0": (2, 3, False), "Acrobot-v1": (6, 3, False), "InvertedPendulum-v2": (4, 1, True),
    "InvertedDoublePendulum-v2": (11, 1, True),
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


def pad_to_64_64(theta, n_in, hid, n_out, gauss):
    """The flat 64-64 theta computing what the n_in-hid[0]-hid[1]-n_out theta computes: the
    extra hidden units have zero weights and biases; a Gauss head's logstd is carried over."""
    assert len(hid) == 2
    h0, h1 = int(hid[0]), int(hid[1])
    th = np.asarray(theta)
    (W0, b0), (W1, b1), (W2, b2) = split_theta(th, [n_in, h0, h1, n_out])
    P0, p1, P2 = np.zeros((n_in, 64)), np.zeros((64, 64)), np.zeros((64, n_out))
    c0, c1 = np.zeros(64), np.zeros(64)
    P0[:, :h0], c0[:h0] = W0, b0
    p1[:h0, :h1], c1[:h1] = W1, b1
    P2[:h1, :] = W2
    parts = [P0.ravel(), c0, p1.ravel(), c1, P2.ravel(), np.asarray(b2, dtype=np.float64)]
    if gauss:
        parts.append(np.asarray(th[-n_out:], dtype=np.float64))
    out = np.concatenate(parts).astype(th.dtype)
    assert out.size == num_params([n_in, 64, 64, n_out], gauss)
    return out


def population(env_id, hid, n, seed, spread=0.5):
    """theta_i = glorot + spread * normal, float32 [n, P] (the 64-64 tests' recipe)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import glorot_init
    O, A, gauss = ENVS[env_id]
    rng = np.random.default_rng(seed)
    base = glorot_init(rng, O, A, _lib.HEAD_GAUSS if gauss else _lib.HEAD_SOFTMAX, [int(h) for h in hid])
    assert base.size == num_params(dims_of(env_id, hid), gauss)
    return (base[None, :] + spread * rng.standard_normal((n, base.size))).astype(np.float32)
