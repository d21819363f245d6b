"""The small-net population rollout's twin (test helper, not collected): the general float64
forward, parameter count, env table and populations are ``cem_np``'s, re-exported here; this
file adds the zero-padding of a two-layer net to the 64-64 shape of ``mrl_pop_rollout``."""
import numpy as np

from tests.cem_np import ENVS, dims_of, forward, num_params, population, split_theta  # noqa: F401


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
