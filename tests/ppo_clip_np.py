"""The clipped-surrogate PPO epilogue (MRL_EPI_PPOCLIP, csrc/rows_epilogue.h) and its updater
(ppo.PpoClipUpdater) restated on the CPU -- test infrastructure shared by
tests/test_ppo_clip_host.py and tests/test_gpu_ppo_clip.py.

``clip_rows``      float64 oracle of one row pass from the head pre-activations z: the ratio
                   r = exp(logp_new(a) - logp_old(a)), the per-row terms (min(r A, clamp(r, 1 - eps,
                   1 + eps) A), KL(old, new), entropy), the head-gradient rows (the surrogate's,
                   -inv_ng r A d logp / d head, zero for a clipped row) and the row's regime.
``clip_rows_f32``  the same in numpy float32 in row_epilogue's operation order (the restatement
                   whose distance from the oracle is the floor the kernels are held to 4x of).
``clip_update``    float64 twin of PpoClipUpdater.update for given epoch permutations, float32
                   Adam state (as oracle/ppo_np.sgd_update is PpoSgdUpdater's).
``rows_case``      the fixed inputs of the per-entry GPU tests.

The clip bounds are 1 -+ eps formed in float32 from the float32 eps, as the kernel forms them:
the oracle takes those two numbers as given, so "on the bound" means the same row for both.
"""
import functools

import numpy as np

from oracle import ppo_np as PO
from oracle import trpo_np as T

F = np.float32
LOG2PI = float(np.log(2.0 * np.pi))
LOG2PI_F, LOG2PIE_F = F(1.8378770664093453), F(2.8378770664093453)
UNCLIPPED, CLIPPED_HIGH, CLIPPED_LOW, OUTSIDE_KEPT = 0, 1, 2, 3
REGIME_NAMES = ("unclipped", "clipped high", "clipped low", "outside, kept")


def clip_bounds(eps):
    """(1 - eps, 1 + eps) as the kernel forms them: float32 arithmetic on the float32 eps."""
    e = F(eps)
    return float(F(1.0) - e), float(F(1.0) + e)


def regimes(ratio, adv, eps):
    """Per row: UNCLIPPED (r inside [1 - eps, 1 + eps]), CLIPPED_HIGH (A > 0, r > 1 + eps),
    CLIPPED_LOW (A < 0, r < 1 - eps), OUTSIDE_KEPT (r outside the range, the advantage of the
    sign -- or 0 -- for which min keeps r A).  Strict inequalities: a row on a bound is UNCLIPPED."""
    lo, hi = clip_bounds(eps)
    reg = np.full(ratio.shape, OUTSIDE_KEPT, dtype=np.int64)
    reg[(ratio >= lo) & (ratio <= hi)] = UNCLIPPED
    reg[(adv > 0) & (ratio > hi)] = CLIPPED_HIGH
    reg[(adv < 0) & (ratio < lo)] = CLIPPED_LOW
    return reg


def bound_distance(ratio, eps):
    """|r - (1 -+ eps)|: the row's distance from the nearer clip bound."""
    lo, hi = clip_bounds(eps)
    return np.minimum(np.abs(ratio - lo), np.abs(ratio - hi))


def clip_rows(head, z, logstd, act, adv, oldprob, eps, inv_ng):
    """float64 oracle of one MRL_EPI_PPOCLIP pass over head pre-activations z [n, A].
    head: 'softmax' (act int [n], oldprob [n, A]) or 'gauss' (logstd [A], act [n, A], oldprob
    [n, 2A]).  Returns ratio [n], terms [n, 3], ghead [n, gh], regime [n], clipped [n]."""
    z = np.asarray(z, dtype=np.float64)
    adv = np.asarray(adv, dtype=np.float64)
    op = np.asarray(oldprob, dtype=np.float64)
    n, A = z.shape
    lo, hi = clip_bounds(eps)
    if head == "softmax":
        a = np.asarray(act).astype(np.int64)
        p = T.softmax(z)
        idx = np.arange(n)
        ratio = np.exp(np.log(p[idx, a]) - np.log(op[idx, a]))
        kl = (op * np.log(op / p)).sum(axis=1)
        ent = -(p * np.log(p)).sum(axis=1)
        onehot = np.zeros_like(p)
        onehot[idx, a] = 1.0
        dlogp = onehot - p                                   # d logp(a) / d z
    else:
        a = np.asarray(act, dtype=np.float64)
        ls = np.asarray(logstd, dtype=np.float64)
        sd = np.exp(ls)
        m0, s0 = op[:, :A], op[:, A:]
        u, u0 = (a - z) / sd, (a - m0) / s0
        logp = -0.5 * (u * u).sum(axis=1) - 0.5 * LOG2PI * A - ls.sum()
        oldlogp = -0.5 * (u0 * u0).sum(axis=1) - 0.5 * LOG2PI * A - np.log(s0).sum(axis=1)
        ratio = np.exp(logp - oldlogp)
        kl = (np.log(sd / s0) + (s0 * s0 + (m0 - z) ** 2) / (2.0 * sd * sd)).sum(axis=1) - 0.5 * A
        ent = np.full(n, ls.sum() + 0.5 * (LOG2PI + 1.0) * A)
        dlogp = np.concatenate([u / sd, u * u - 1.0], axis=1)  # d logp(a) / d (mean, logstd)
    reg = regimes(ratio, adv, eps)
    clipped = (reg == CLIPPED_HIGH) | (reg == CLIPPED_LOW)
    surr = np.minimum(ratio * adv, np.clip(ratio, lo, hi) * adv)
    w = np.where(clipped, 0.0, -inv_ng * ratio * adv)
    return dict(ratio=ratio, terms=np.stack([surr, kl, ent], axis=1), ghead=w[:, None] * dlogp, regime=reg,
                clipped=clipped)


def clip_rows_f32(head, z, logstd, act, adv, oldprob, eps, inv_ng):
    """row_epilogue<MRL_EPI_PPOCLIP> in numpy float32, in the kernel's operation order (sums
    over the columns in order; the float64 accumulators stay float64).  Same keys as clip_rows,
    values as float64."""
    z, adv, op = (np.ascontiguousarray(v, dtype=np.float32) for v in (z, adv, oldprob))
    n, A = z.shape
    zero = np.zeros(n, dtype=np.float32)
    e = F(eps)
    lo, hi = F(1.0) - e, F(1.0) + e
    if head == "softmax":
        a = np.asarray(act).astype(np.int64)
        idx = np.arange(n)
        m = z[:, 0].copy()
        for j in range(1, A):
            m = np.maximum(m, z[:, j])
        ex = np.exp(z - m[:, None])
        s = zero.copy()
        for j in range(A):
            s = s + ex[:, j]
        p = ex / s[:, None]
        kl, ent = zero.copy(), zero.copy()
        for j in range(A):
            kl = kl + op[:, j] * np.log(op[:, j] / p[:, j])
            ent = ent + (-(p[:, j] * np.log(p[:, j])))
        ratio = np.exp(np.log(p[idx, a]) - np.log(op[idx, a]))
    else:
        ac = np.ascontiguousarray(act, dtype=np.float32)
        ls = np.ascontiguousarray(logstd, dtype=np.float32)
        sd = np.exp(ls)
        m0, s0 = op[:, :A], op[:, A:]
        q, q0, sls0, kl, sls = zero.copy(), zero.copy(), zero.copy(), zero.copy(), F(0.0)
        u = (ac - z) / sd
        for j in range(A):
            u0 = (ac[:, j] - m0[:, j]) / s0[:, j]
            q = q + u[:, j] * u[:, j]
            q0 = q0 + u0 * u0
            sls = sls + ls[j]
            sls0 = sls0 + np.log(s0[:, j])
            dm = m0[:, j] - z[:, j]
            sj = np.repeat(sd[j], n)
            kl = kl + (np.log(sj / s0[:, j]) + (s0[:, j] * s0[:, j] + dm * dm) / (F(2.0) * sj * sj))
        kl = kl - F(0.5 * A)
        half = F(0.5) * LOG2PI_F * F(A)
        ratio = np.exp((F(-0.5) * q - half - sls) - (F(-0.5) * q0 - half - sls0))
        ent = np.repeat(sls + F(0.5) * LOG2PIE_F * F(A), n)
    clipped = ((adv > 0) & (ratio > hi)) | ((adv < 0) & (ratio < lo))
    surr = np.minimum(ratio * adv, np.minimum(np.maximum(ratio, lo), hi) * adv)
    w = np.where(clipped, F(0.0), F(-inv_ng) * ratio * adv).astype(np.float32)
    if head == "softmax":
        g = np.empty((n, A), dtype=np.float32)
        for j in range(A):
            g[:, j] = w * ((a == j).astype(np.float32) - p[:, j])
    else:
        g = np.concatenate([w[:, None] * u / sd, w[:, None] * (u * u - F(1.0))], axis=1)
    assert g.dtype == np.float32 and surr.dtype == np.float32 and ratio.dtype == np.float32
    f64 = np.float64
    return dict(ratio=ratio.astype(f64), terms=np.stack([surr.astype(f64), kl.astype(f64), ent.astype(f64)], axis=1),
                ghead=g.astype(f64), clipped=clipped)


# ------------------------------------------------------------------ through the net
def _logstd(spec, th):
    return th[-spec.n_out:] if spec.head == "gauss" else None


def policy_rows(spec, th, ob, act, adv, oldprob, eps, inv_ng, z=None):
    """clip_rows of the policy net at theta (z: other head pre-activations of the same rows)."""
    if z is None:
        z = T.mlp_forward(spec, th, ob)[0]
    return clip_rows(spec.head, z, _logstd(spec, th), act, adv, oldprob, eps, inv_ng)


def clip_loss_grad(spec, th, ob, act, adv, oldprob, eps):
    """(-mean min(r A, clamp(r) A), its gradient in theta, the rows) by analytic backprop of
    the oracle's head-gradient rows."""
    n = ob.shape[0]
    z, acts = T.mlp_forward(spec, th, ob)
    r = policy_rows(spec, th, ob, act, adv, oldprob, eps, 1.0 / n, z=z)
    A = spec.n_out
    grads = T.mlp_vjp(spec, th, acts, r["ghead"][:, :A])
    if spec.head == "gauss":
        grads = grads + [r["ghead"][:, A:].sum(axis=0)]
    return -r["terms"][:, 0].mean(), T.flatten(grads), r


def clip_update(spec, theta, ob, act, adv, oldprob, perms, clip_param=0.2, stepsize=3e-4, minibatch_size=4096,
                target_kl=0.0, adam_state=None):
    """PpoClipUpdater.update for the given epoch permutations: float64 rows and gradients,
    float32 theta and Adam state (b1 0.9, b2 0.999, eps 1e-8, the float32 step size of
    oracle/ppo_np.sgd_update).  Returns (theta_new, info, adam_state, margin): margin is the
    smallest distance of any minibatch row's ratio from a clip bound over the whole update."""
    th = theta.astype(np.float32)
    m, v, t = adam_state if adam_state is not None else (np.zeros_like(th), np.zeros_like(th), 0)
    N = ob.shape[0]
    before = PO.losses(spec, th.astype(np.float64), ob, act, adv, oldprob)
    b1, b2, aeps = F(0.9), F(0.999), F(1e-8)
    margin, epochs_run = np.inf, 0
    for perm in perms:
        kls = []
        for i in range(0, N, minibatch_size):
            idx = perm[i:i + minibatch_size]
            _, g, r = clip_loss_grad(spec, th.astype(np.float64), ob[idx], act[idx], adv[idx], oldprob[idx], clip_param)
            kls.append(r["terms"][:, 1].mean())
            margin = min(margin, bound_distance(r["ratio"], clip_param).min())
            g = g.astype(np.float32)
            t += 1
            a_t = F(stepsize) * np.sqrt(F(1) - b2 ** F(t)) / (F(1) - b1 ** F(t))
            m = b1 * m + (F(1) - b1) * g
            v = b2 * v + (F(1) - b2) * g * g
            th = th - a_t * m / (np.sqrt(v) + aeps)
        epochs_run += 1
        if target_kl > 0 and np.mean(kls) > 1.5 * target_kl:
            break
    after = PO.losses(spec, th.astype(np.float64), ob, act, adv, oldprob)
    info = PO._info(before, after)
    info["epochs_run"] = epochs_run
    return th.astype(np.float64), info, (m, v, t), margin


# ------------------------------------------------------------------ the fixed inputs of the row tests
EPS = 0.2
N_IN = 5
ROW_COUNTS = [1, 31, 32, 33, 64, 65, 257]
BIG_N = 1536 * 256 + 257   # tests/test_gpu_head_rows.py: the grid-stride loop's second trip
HEAD_WIDTHS = [("softmax", 2), ("softmax", 3), ("softmax", 8), ("gauss", 1), ("gauss", 3), ("gauss", 8)]
BIG_WIDTH = {"softmax": 2, "gauss": 3}
POOL = 257                 # every row count is a prefix of its (head, A) pool of 257 rows
MIN_SHARE, MAX_BAND_SHARE = 0.05, 0.01


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


MAX_LOG_RATIO = 0.7   # the inputs' ratios stay within [exp(-0.7), exp(0.7)] ~ [0.50, 2.01]


def _old_rows(spec, th, dth, s, ob, pnew, noise, gap=0.0):
    """Old prob rows of theta + s * dtheta and actions sampled from them; a row whose ratio
    leaves exp(-+MAX_LOG_RATIO) has its old row moved halfway to the new one until it does not
    (the absolute rounding error of r, which sets the band around the clip bounds, grows with
    r: a heavy tail of ratios would widen the band for every row).  gap > 0: likewise a row
    whose ratio is within gap of a clip bound, so that none is left there."""
    A = spec.n_out
    oldprob = _r32(T.policy_prob(spec, th + s * dth, ob))
    act = T.sample(spec, oldprob, noise)
    if spec.head == "gauss":
        act = _r32(act)
    for _ in range(40):
        lr = T.loglik(spec, act, pnew) - T.loglik(spec, act, oldprob)
        bad = (np.abs(lr) > MAX_LOG_RATIO) | (bound_distance(np.exp(lr), EPS) < gap)
        if not bad.any():
            break
        if spec.head == "gauss":
            mid = np.concatenate([0.5 * (oldprob[bad, :A] + pnew[bad, :A]), np.sqrt(oldprob[bad, A:] * pnew[bad, A:])], axis=1)
        else:
            mid = 0.5 * (oldprob[bad] + pnew[bad])
            mid = mid / mid.sum(axis=1, keepdims=True)
        oldprob[bad] = _r32(mid)
    assert not bad.any()
    return oldprob, act


BF16_GAP = 0.05       # the bf16 entry's inputs keep this far from 1 -+ eps (tests/test_gpu_ppo_clip.py)


@functools.lru_cache(maxsize=None)
def rows_case(head, A, n, gap=0.0):
    """Inputs of one per-entry case, every array float64 holding float32 values: a policy net
    N_IN -> 64 -> 64 -> A at theta, n observation rows, actions sampled from the old policy,
    standard-normal advantages, and old prob rows of theta + s * dtheta (_old_rows).  s is raised in steps
    of 1.25x until, for the float64 oracle at theta, each clipped / kept-outside regime holds
    at least 8 % of the pool's rows (tests/test_ppo_clip_host.py asserts the issue's 5 % for
    all four regimes and the 1 % band share on what comes out).  A case of n <= POOL rows is
    the first n rows of its pool's case.  gap: no float64 ratio within gap of a clip bound
    (the bf16 entry's inputs, BF16_GAP: bf16 rounding moves r by far more than float32 does, and
    with ratios spread evenly a band sized for it would hold a tenth of the rows)."""
    if n < POOL:
        big = rows_case(head, A, POOL, gap)
        c = dict(big)
        for k in ("ob", "act", "adv", "oldprob"):
            c[k] = big[k][:n]
        c["n"] = n
        return c
    rng = np.random.default_rng([41, 1 if head == "softmax" else 2, A, n % 1000003])
    spec = T.Spec(N_IN, [64, 64], A, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-A:] = -0.3 + 0.1 * rng.standard_normal(A)
    th = _r32(th)
    ob = _r32(rng.standard_normal((n, N_IN)))
    adv = _r32(rng.standard_normal(n))
    dth = rng.standard_normal(spec.P)
    noise = rng.standard_normal((n, A)) if head == "gauss" else rng.random(n)
    pnew = _r32(T.policy_prob(spec, th, ob))
    k = min(n, 4096)                                  # s is chosen on the first 4096 rows
    s = 0.002
    for _ in range(60):
        oldprob, act = _old_rows(spec, th, dth, s, ob[:k], pnew[:k], noise[:k], gap)
        r = policy_rows(spec, th, ob[:k], act, adv[:k], oldprob, EPS, 1.0 / k)
        if (np.bincount(r["regime"], minlength=4) / k)[1:].min() >= 0.08:
            break
        s *= 1.25
    if k < n:
        oldprob, act = _old_rows(spec, th, dth, s, ob, pnew, noise, gap)
    return dict(head=head, A=A, n=n, spec=spec, theta=th, ob=ob, act=act, adv=adv, oldprob=oldprob, scale=s)


def case_list():
    """(head, A, n) of every per-entry case."""
    out = [(h, A, n) for h, A in HEAD_WIDTHS for n in ROW_COUNTS]
    return out + [(h, A, BIG_N) for h, A in BIG_WIDTH.items()]
