"""float64 restatement of the rollout's evaluation mode (MRL_ROLLOUT_EVAL) -- test helper, not
collected.  oracle.rollout_np.collect's loop with the two things the mode changes: the action
is the head's mode (ProbType.maxprob: the Gauss mean, the arg-max logit with the lowest index on
a tie) and the observation filter is frozen -- applied from ``fs`` as mrl_pop_rollout applies a
state, never updated.  Everything else is collect's own: oracle.rollout_np.Envs or a twin's
``*Envs``, oracle.trpo_np's forward on the stored float32 observations, the episode bookkeeping,
the reset stream, and the trajectory dict's shape."""
import numpy as np

from oracle import trpo_np as T


def frozen_filter(fs, o):
    """clip((o - M) / (sqrt(S / (n - 1)) + 1e-8), +-5); with fewer than two observations in the
    state the observation is clipped only (agentzoo.FrozenZFilter, mrl_pop_rollout)."""
    O = o.shape[-1]
    if fs.n >= 2:
        o = (o - fs.M[:O]) / (np.sqrt(fs.S[:O] / (fs.n - 1)) + 1e-8)
    return np.clip(o, -5.0, 5.0)


def mode_action(spec, z):
    """The head's mode: z itself (the Gauss mean) or np.argmax of the logits (lowest index on a tie)."""
    return np.argmax(z, axis=1) if spec.head == "softmax" else z.astype(np.float32)


def collect_eval(envs, fs, spec, theta, Tn, timestep_limit, filt=True):
    """One evaluation iteration: reset all envs, Tn lock-step steps; ``fs`` (an
    oracle.rollout_np.FilterState) is read and left as it is.  Returns collect's trajectory dict."""
    E, O, A = envs.E, envs.O, envs.A
    envs.reset(np.arange(E))
    out = dict(obs=np.zeros((Tn, E, O), np.float32), rew=np.zeros((Tn, E), np.float32),
               flags=np.zeros((Tn, E), np.uint8), ep_t=np.zeros((Tn, E), np.int32),
               act=np.zeros((Tn, E), np.int32) if spec.head == "softmax" else np.zeros((Tn, E, A), np.float32),
               prob=np.zeros((Tn, E, A if spec.head == "softmax" else 2 * A), np.float32))
    for t in range(Tn):
        o = envs.obs()
        x32 = (frozen_filter(fs, o) if filt else o).astype(np.float32)
        out["obs"][t] = x32
        z, _ = T.mlp_forward(spec, theta, x32.astype(np.float64))
        if spec.head == "softmax":
            out["prob"][t] = T.softmax(z).astype(np.float32)
        else:
            _, _, logstd = spec.split(theta)
            sd = np.exp(logstd.astype(np.float32))
            out["prob"][t] = np.concatenate([z.astype(np.float32), np.repeat(sd[None, :], E, axis=0)], axis=1)
        act = mode_action(spec, z)
        out["act"][t] = act
        rew, done = envs.step(act)
        ept = envs.ep_t.copy()
        out["ep_t"][t] = ept
        term = done | (ept + 1 >= envs.max_steps)
        last = term | (ept + 1 >= timestep_limit) | (t == Tn - 1)
        out["rew"][t] = rew.astype(np.float32)
        out["flags"][t] = last.astype(np.uint8) | (term.astype(np.uint8) << 1)
        envs.ep_t = ept + 1
        if t < Tn - 1 and last.any():
            envs.reset(np.nonzero(last)[0])
    return out
