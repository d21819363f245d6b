"""The per-row head epilogues (csrc/rows_epilogue.h) row by row and column by column.

``mrl_head_rows`` (the layered path's ``head_rows_kernel``, csrc/gemm.hip) is driven
directly with head pre-activations ``z`` (and tangents ``dz``) the test supplies, and
``mrl_probtype_rows`` with probability rows; every output entry is compared with a
float64 numpy reference written here from the reference's formulas (core.py:349-359
Categorical, core.py:412-430 DiagGauss, trpo.py:42-64, ppo.py:46-52 and 150-156,
core.py:611-617), never in sums over the batch: the losses are checked per wave of 64
rows (the finest grain ``partial`` has), the prob and head-gradient rows per entry.

Bounds.  ``z`` is given exactly, so the error is the fp32 evaluation of the formulas
(with cancellation in the KL of near-equal distributions) and the device expf / logf.
``f32_rows`` restates ``row_epilogue``'s operation order in numpy float32; its largest
distance from the float64 reference over every case of this file, in units of a
per-entry scale (the largest term the entry is formed from, times max(1, |exponent|)
where a rounded sum is exponentiated), is the FLOOR of that output, and the kernel is
allowed 4x the floor (ulp-level differences between the device's and numpy's expf /
logf, and the device's fused multiply-adds).  An entry whose scale is 0 (a copied
value, a wave without rows, an advantage of exactly 0) must be exact.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import trpo_np as T

pytestmark = pytest.mark.gpu

HEADS = {"linear": 0, "softmax": 1, "gauss": 2}
PROB, LOSSES, SURRGRAD, VFLOSS, FVP, PPOGRAD, PPOSGD = 0, 1, 2, 3, 4, 5, 6
SENT = 777.25  # sentinel the output buffers are filled with
F = np.float32
F32_TINY = float(np.finfo(np.float32).tiny)
LOG2PI = float(np.log(2.0 * np.pi))
LOG2PI_F, LOG2PIE_F = F(1.8378770664093453), F(2.8378770664093453)

NS = [1, 255, 256, 257]             # one block, the block edge, two blocks
AS = [1, 2, 8, 9, 17, 32]           # 8: the last of MA = 8, 9: the first of MA = 32
BIG_N = 1536 * 256 + 257            # the grid-stride loop's second trip (1536 blocks of 256 rows)
SGD_NS = [1, 63, 64, 65, 128]
PROBTYPE_BIG_N = 2048 * 256 + 1     # mrl_probtype_rows' stride loop

# name -> (epilogue, reverse_kl, kl_coeff)
POLICY_EPIS = {"prob": (PROB, 0, 0.0), "losses": (LOSSES, 0, 0.0), "surrgrad": (SURRGRAD, 0, 0.0),
               "ppograd": (PPOGRAD, 0, 37.5), "ppograd_rev": (PPOGRAD, 1, 37.5), "fvp": (FVP, 0, 0.0)}
LINEAR_EPIS = {"prob": (PROB, 0, 0.0), "vfloss": (VFLOSS, 0, 0.0), "fvp": (FVP, 0, 0.0)}
SGD_KL_COEFF, SGD_CUTOFF_COEFF = 1.5, 1000.0

# FLOOR[key]: the float32 restatement's largest distance from the float64 reference, in
# scale units, measured on the CPU over every case below (measure_floors(); numpy 2.2,
# rounded up to two digits).  The kernel's bound is 4x the floor (TOL).
FLOOR = {
    # mrl_head_rows, key = head.epilogue.output (surr / kl / ent: the partial columns per wave)
    "softmax.prob.out": 2.5e-7, "softmax.fvp.ghead": 4.1e-7,
    "softmax.losses.surr": 8.1e-8, "softmax.losses.kl": 2.5e-7, "softmax.losses.ent": 1.7e-6,
    "softmax.surrgrad.surr": 8.1e-8, "softmax.surrgrad.kl": 2.5e-7, "softmax.surrgrad.ent": 1.7e-6,
    "softmax.surrgrad.ghead": 4.0e-7,
    "softmax.ppograd.surr": 8.1e-8, "softmax.ppograd.kl": 2.5e-7, "softmax.ppograd.ent": 1.7e-6,
    "softmax.ppograd.ghead": 2.7e-7,
    "softmax.ppograd_rev.surr": 8.1e-8, "softmax.ppograd_rev.kl": 3.1e-7, "softmax.ppograd_rev.ent": 1.7e-6,
    "softmax.ppograd_rev.ghead": 1.8e-6,
    "softmax.sgd_below.surr": 1.0e-7, "softmax.sgd_below.kl": 2.3e-7, "softmax.sgd_below.ent": 7.3e-7,
    "softmax.sgd_below.ghead": 3.4e-7,
    "softmax.sgd_above.surr": 7.0e-8, "softmax.sgd_above.kl": 1.8e-7, "softmax.sgd_above.ent": 9.0e-7,
    "softmax.sgd_above.ghead": 1.3e-7,
    "gauss.prob.out": 1.7e-7, "gauss.fvp.ghead": 4.6e-7,
    "gauss.losses.surr": 2.9e-7, "gauss.losses.kl": 2.4e-7, "gauss.losses.ent": 1.7e-7,
    "gauss.surrgrad.surr": 2.9e-7, "gauss.surrgrad.kl": 2.4e-7, "gauss.surrgrad.ent": 1.7e-7,
    "gauss.surrgrad.ghead": 6.6e-7,
    "gauss.ppograd.surr": 2.9e-7, "gauss.ppograd.kl": 2.4e-7, "gauss.ppograd.ent": 1.7e-7,
    "gauss.ppograd.ghead": 5.3e-7,
    "gauss.ppograd_rev.surr": 2.9e-7, "gauss.ppograd_rev.kl": 1.4e-7, "gauss.ppograd_rev.ent": 1.7e-7,
    "gauss.ppograd_rev.ghead": 4.5e-7,
    "gauss.sgd_below.surr": 2.5e-7, "gauss.sgd_below.kl": 1.5e-7, "gauss.sgd_below.ent": 1.1e-7,
    "gauss.sgd_below.ghead": 5.1e-7,
    "gauss.sgd_above.surr": 1.7e-7, "gauss.sgd_above.kl": 2.1e-7, "gauss.sgd_above.ent": 1.2e-7,
    "gauss.sgd_above.ghead": 3.2e-7,
    # the linear head copies z (exact); VFLOSS: surr = the squared-error column, kl / ent columns 0
    "linear.prob.out": 0.0, "linear.fvp.ghead": 7.4e-8,
    "linear.vfloss.surr": 2.5e-8, "linear.vfloss.kl": 0.0, "linear.vfloss.ent": 0.0, "linear.vfloss.ghead": 1.2e-7,
    # mrl_probtype_rows
    "probtype.softmax.loglik": 2.5e-7, "probtype.softmax.kl": 1.3e-6, "probtype.softmax.ent": 4.5e-6,
    "probtype.gauss.loglik": 4.0e-7, "probtype.gauss.kl": 5.7e-7, "probtype.gauss.ent": 6.0e-8,
}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}


# ------------------------------------------------------------------ inputs (CPU, screened)
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def make_inputs(head, A, n, near=False):
    """fp32 inputs of one case.  softmax: logits spread up to +-30 (no probability
    underflows in f32), oldprob rows with probabilities down to 1e-6, near-equal and far
    old / new rows mixed; gauss: logstd in [-3, 1], old / new means up to 3 std apart,
    actions up to 4 std out, screened so that |logp - oldlogp| <= 20 (the ratio stays
    finite in f32); advantages of both signs and exact 0.  near: every old row close to
    the new one (a small minibatch KL)."""
    rng = np.random.default_rng([HEADS[head], A, n % 1000003, int(near)])
    d = {"head": head, "A": A, "n": n}
    adv = rng.standard_normal(n)
    adv[::5] = 0.0
    d["adv"] = _f32(adv)
    d["dz"] = _f32(rng.standard_normal((n, A)))
    if head == "linear":
        d["z"] = _f32(5.0 * rng.standard_normal((n, 1)))
        t = 5.0 * rng.standard_normal(n)
        t[::7] = d["z"][::7, 0]  # exact zeros of the error
        d["target"] = _f32(t)
        return d
    if head == "softmax":
        spread = rng.choice([0.5, 3.0, 10.0, 30.0], size=(n, 1))
        d["z"] = _f32(rng.uniform(-1.0, 1.0, (n, A)) * spread)
        z = d["z"].astype(np.float64)
        kind = np.zeros((n, 1), dtype=np.int64) if near else rng.integers(0, 3, size=(n, 1))
        e = rng.standard_normal((n, A))
        zo = np.where(kind == 0, z + 0.05 * e, np.where(kind == 1, z + e, 0.3 * z + e))
        po = np.maximum(T.softmax(zo), 1e-6)
        d["oldprob"] = _f32(po / po.sum(axis=1, keepdims=True))
        d["act"] = rng.integers(0, A, n).astype(np.int32)
        assert T.softmax(z).astype(np.float32).min() > 1e-30 and d["oldprob"].min() > 0.9e-6
        return d
    sp = SimpleNamespace(head="gauss", n_out=A)
    d["logstd"] = _f32(rng.uniform(-3.0, 1.0, A))
    d["dlogstd"] = _f32(rng.standard_normal(A))
    d["z"] = _f32(2.0 * rng.standard_normal((n, A)))
    z, sd = d["z"].astype(np.float64), np.exp(d["logstd"].astype(np.float64))
    g = 0.02 if near else 1.0
    far = rng.random((n, A)) < min(1.0, 2.0 / A)
    gap = np.where(far, rng.uniform(-3.0, 3.0, (n, A)), rng.uniform(-0.1, 0.1, (n, A))) * g
    srel = rng.uniform(-0.3, 0.3, (n, A)) * g
    out = np.where(rng.random((n, A)) < min(1.0, 2.0 / A), rng.uniform(-4.0, 4.0, (n, A)),
                   rng.uniform(-1.0, 1.0, (n, A)))
    prob = np.concatenate([z, np.repeat(sd[None, :], n, axis=0)], axis=1)
    for _ in range(60):
        s0 = sd * np.exp(srel)
        m0 = z + gap * sd
        d["oldprob"] = _f32(np.concatenate([m0, s0], axis=1))
        d["act"] = _f32(m0 + out * s0)
        a, op = d["act"].astype(np.float64), d["oldprob"].astype(np.float64)
        bad = np.abs(T.loglik(sp, a, prob) - T.loglik(sp, a, op)) > 20.0
        if not bad.any():
            break
        gap[bad] *= 0.5
        srel[bad] *= 0.5
        out[bad] *= 0.5
    assert not bad.any()
    return d


# ------------------------------------------------------------------ float64 reference
def _rowmax(a):
    return np.max(np.abs(a), axis=1)


def ref_rows(d, epi, inv_ng=1.0, kl_coeff=0.0, reverse=0, kl_cutoff=0.0, cutoff_coeff=0.0):
    """float64 values of one epilogue over the rows of d, each with its scale:
    out / ghead -> (value [n, w], scale [n, w]); terms / tscale [n, 3]: the row's
    (ratio * adv, kl, entropy) (VFLOSS: (err^2, 0, 0)) that ``partial`` sums per wave.
    PPOSGD: kl_coeff is the updater's coefficient; the slope the minibatch KL sets is
    returned as r["slope"] (ppo.py:46-47, 153)."""
    head, A, n = d["head"], d["A"], d["n"]
    sp = SimpleNamespace(head=head, n_out=A)
    z = d["z"].astype(np.float64)
    dz = d["dz"].astype(np.float64)
    r = {}
    if head == "linear":
        if epi == PROB:
            r["out"] = (z, np.zeros_like(z))  # copied
        elif epi == VFLOSS:
            err = z[:, 0] - d["target"].astype(np.float64)
            zero = np.zeros(n)
            r["terms"] = np.stack([err * err, zero, zero], axis=1)
            r["tscale"] = r["terms"].copy()
            g = (2.0 * inv_ng * err)[:, None]
            r["ghead"] = (g, np.abs(g))
        else:
            g = dz * inv_ng
            r["ghead"] = (g, np.abs(g))
        return r
    idx = np.arange(n)
    losses = epi in (LOSSES, SURRGRAD, PPOGRAD, PPOSGD)
    if losses:
        adv = d["adv"].astype(np.float64)
        op = d["oldprob"].astype(np.float64)
        act = d["act"].astype(np.float64 if head == "gauss" else np.int64)
    if head == "softmax":
        p = T.softmax(z)
        lp = np.log(p)
        Lp = np.maximum(1.0, np.abs(lp))  # |log p| ~ |z - max|: the exponent's rounding shows in p
        if epi == PROB:
            r["out"] = (p, p * Lp)
            return r
        if epi == FVP:
            pd = (p * dz).sum(axis=1, keepdims=True)
            r["ghead"] = (p * (dz - pd) * inv_ng,
                          p * Lp * np.maximum(np.abs(dz), (p * np.abs(dz)).sum(axis=1, keepdims=True)) * abs(inv_ng))
            return r
        prob = p
        lop = np.log(op)
        logp, oldlogp = T.loglik(sp, act, p), T.loglik(sp, act, op)
        E = np.maximum(1.0, np.maximum(np.abs(logp), np.abs(oldlogp)))
        both = np.maximum(Lp, np.abs(lop))
        klscale = _rowmax((p if reverse else op) * both)
        entscale = _rowmax(p * Lp)
    else:
        sd = np.exp(d["logstd"].astype(np.float64))
        sdr = np.repeat(sd[None, :], n, axis=0)
        prob = np.concatenate([z, sdr], axis=1)
        if epi == PROB:
            r["out"] = (prob, np.concatenate([np.zeros_like(z), sdr], axis=1))  # means are copied
            return r
        if epi == FVP:
            g = np.concatenate([dz / (sd * sd) * inv_ng,
                                np.repeat((2.0 * d["dlogstd"].astype(np.float64) * inv_ng)[None, :], n, axis=0)], axis=1)
            r["ghead"] = (g, np.abs(g))
            return r
        m0, s0 = op[:, :A], op[:, A:]
        u, u0 = (act - z) / sd, (act - m0) / s0
        logp, oldlogp = T.loglik(sp, act, prob), T.loglik(sp, act, op)
        ls = np.log(sd)
        E = np.maximum.reduce([np.ones(n), 0.5 * (u * u).sum(axis=1), 0.5 * (u0 * u0).sum(axis=1),
                               np.full(n, 0.5 * LOG2PI * A), np.full(n, np.abs(ls.sum())),
                               np.abs(np.log(s0).sum(axis=1))])
        a0, b0, a1, b1 = (z, sdr, m0, s0) if reverse else (m0, s0, z, sdr)  # kl[a, b]
        quad = (b0 * b0 + (a0 - a1) ** 2) / (2.0 * b1 * b1)
        klscale = np.maximum.reduce([_rowmax(np.log(b1 / b0)), _rowmax(quad), np.full(n, 0.5 * A)])
        entscale = np.full(n, max(np.abs(ls).max(), 0.5 * (LOG2PI + 1.0) * A))
    ratio = np.exp(logp - oldlogp)
    kl = T.kl(sp, prob, op) if reverse else T.kl(sp, op, prob)
    r["terms"] = np.stack([ratio * adv, kl, T.entropy(sp, prob)], axis=1)
    r["tscale"] = np.stack([np.abs(ratio * adv) * E, klscale, entscale], axis=1)
    if epi == LOSSES:
        return r
    slope, extra = kl_coeff, 0.0
    if epi == PPOSGD:
        kl_mb = kl.sum() * inv_ng
        r["kl_mb"] = kl_mb
        if kl_mb > kl_cutoff:
            slope = kl_coeff + 2.0 * cutoff_coeff * (kl_mb - kl_cutoff)
            extra = 2.0 * cutoff_coeff * klscale.sum() * abs(inv_ng)  # the slope inherits the KL's error
        r["slope"] = slope
    w = (-inv_ng * ratio * adv)[:, None]
    wE = np.abs(w) * E[:, None]
    c = slope * inv_ng if epi in (PPOGRAD, PPOSGD) else 0.0
    cs = (abs(slope) + extra) * abs(inv_ng) if epi in (PPOGRAD, PPOSGD) else 0.0
    if head == "softmax":
        onehot = np.zeros_like(p)
        onehot[idx, act] = 1.0
        g = w * (onehot - p)
        sc = wE * np.maximum(onehot, p * Lp)
        if c != 0.0:
            if reverse:
                g = g + c * p * (lp - lop - kl[:, None])
                sc = sc + cs * p * np.maximum(both, klscale[:, None])
            else:
                g = g + c * (p * op.sum(axis=1, keepdims=True) - op)
                sc = sc + cs * np.maximum(p * Lp, op)
    else:
        gm, gs = w * u / sd, w * (u * u - 1.0)
        scm, scs = wE * np.abs(u) / sd, wE * np.maximum(u * u, 1.0)
        if c != 0.0:
            dm = z - m0
            if reverse:
                gm, gs = gm + c * dm / (s0 * s0), gs + c * (sd * sd / (s0 * s0) - 1.0)
                scm, scs = scm + cs * np.abs(dm) / (s0 * s0), scs + cs * np.maximum(sd * sd / (s0 * s0), 1.0)
            else:
                t = (s0 * s0 + dm * dm) / (sd * sd)
                gm, gs = gm + c * dm / (sd * sd), gs + c * (1.0 - t)
                scm, scs = scm + cs * np.abs(dm) / (sd * sd), scs + cs * np.maximum(t, 1.0)
        g, sc = np.concatenate([gm, gs], axis=1), np.concatenate([scm, scs], axis=1)
    r["ghead"] = (g, sc)
    return r


# ------------------------------------------------------------------ float32 restatement
def f32_rows(d, epi, inv_ng=1.0, kl_coeff=0.0, reverse=0, kl_cutoff=0.0, cutoff_coeff=0.0):
    """row_epilogue / fvp_metric_row / pposgd_row in numpy float32, in the kernel's
    operation order (sums run over the columns in order; the fp64 accumulators of the
    loss terms stay fp64).  Returns out, ghead [n, w] and terms [n, 3] as float64."""
    head, A, n = d["head"], d["A"], d["n"]
    z, dz = d["z"], d["dz"]
    s_ng = F(inv_ng)
    r = {}
    zero = np.zeros(n, dtype=np.float32)
    if head == "linear":
        if epi == PROB:
            r["out"] = z
        elif epi == VFLOSS:
            err = z[:, 0] - d["target"]
            e64 = err.astype(np.float64)
            r["terms"] = np.stack([e64 * e64, 0 * e64, 0 * e64], axis=1)
            r["ghead"] = (F(2.0 * inv_ng) * err)[:, None]
        else:
            r["ghead"] = dz * s_ng
        return {k: np.asarray(v, dtype=np.float64) for k, v in r.items()}
    idx = np.arange(n)
    grads = epi in (SURRGRAD, PPOGRAD, PPOSGD)
    if epi not in (PROB, FVP):
        adv, op = d["adv"], d["oldprob"]
    if head == "softmax":
        m = z[:, 0].copy()
        for j in range(1, A):
            m = np.maximum(m, z[:, j])
        e = np.exp(z - m[:, None])
        s = zero.copy()
        for j in range(A):
            s = s + e[:, j]
        p = e / s[:, None]
        if epi == PROB:
            r["out"] = p
        elif epi == FVP:
            pd = zero.copy()
            for j in range(A):
                pd = pd + p[:, j] * dz[:, j]
            r["ghead"] = p * (dz - pd[:, None]) * s_ng
        else:
            act = d["act"]
            kl, ent = zero.copy(), zero.copy()
            for j in range(A):
                t = p[:, j] * np.log(p[:, j] / op[:, j]) if reverse else op[:, j] * np.log(op[:, j] / p[:, j])
                kl = kl + t
                ent = ent + (-(p[:, j] * np.log(p[:, j])))
            ratio = np.exp(np.log(p[idx, act]) - np.log(op[idx, act]))
    else:
        ls = d["logstd"]
        sd = np.exp(ls)
        if epi == PROB:
            r["out"] = np.concatenate([z, np.repeat(sd[None, :], n, axis=0)], axis=1)
        elif epi == FVP:
            r["ghead"] = np.concatenate([dz / (sd * sd) * s_ng,
                                         np.repeat((F(2.0) * d["dlogstd"] * s_ng)[None, :], n, axis=0)], axis=1)
        else:
            ac, m0, s0 = d["act"], op[:, :A], op[:, A:]

            def gkl(a0, b0, a1, b1):
                dm = a0 - a1
                return np.log(b1 / b0) + (b0 * b0 + dm * dm) / (F(2.0) * b1 * b1)

            q, q0, sls0, kl, sls = zero.copy(), zero.copy(), zero.copy(), zero.copy(), F(0.0)
            u = (ac - z) / sd
            for j in range(A):
                u0 = (ac[:, j] - m0[:, j]) / s0[:, j]
                q = q + u[:, j] * u[:, j]
                q0 = q0 + u0 * u0
                sls = sls + ls[j]
                sls0 = sls0 + np.log(s0[:, j])
                sj = np.repeat(sd[j], n)
                kl = kl + (gkl(z[:, j], sj, m0[:, j], s0[:, j]) if reverse else gkl(m0[:, j], s0[:, j], z[:, j], sj))
            kl = kl - F(0.5 * A)
            half_l2pi_a = F(0.5) * LOG2PI_F * F(A)
            logp = F(-0.5) * q - half_l2pi_a - sls
            oldlogp = F(-0.5) * q0 - half_l2pi_a - sls0
            ratio = np.exp(logp - oldlogp)
            ent = np.repeat(sls + F(0.5) * LOG2PIE_F * F(A), n)
    if epi in (PROB, FVP):
        return {k: np.asarray(v, dtype=np.float64) for k, v in r.items()}
    r["terms"] = np.stack([(ratio * adv).astype(np.float64), kl.astype(np.float64), ent.astype(np.float64)], axis=1)
    if grads:
        kc = F(kl_coeff)
        if epi == PPOSGD:
            kl_mb = r["terms"][:, 1].sum() * inv_ng
            if kl_mb > float(F(kl_cutoff)):
                kc = F(kl_coeff) + F(2.0 * float(F(cutoff_coeff)) * (kl_mb - float(F(kl_cutoff))))
        ppo = epi in (PPOGRAD, PPOSGD)
        c = kc * s_ng
        w = F(-inv_ng) * ratio * adv
        if head == "softmax":
            g = np.empty((n, A), dtype=np.float32)
            for j in range(A):
                gj = w * ((act == j).astype(np.float32) - p[:, j])
                if ppo:
                    gj = gj + c * (p[:, j] * (np.log(p[:, j] / op[:, j]) - kl) if reverse else p[:, j] - op[:, j])
                g[:, j] = gj
        else:
            gm, gs = w[:, None] * u / sd, w[:, None] * (u * u - F(1.0))
            if ppo:
                dm = z - m0
                if reverse:
                    gm = gm + c * dm / (s0 * s0)
                    gs = gs + c * (sd * sd / (s0 * s0) - F(1.0))
                else:
                    gm = gm + c * dm / (sd * sd)
                    gs = gs + c * (F(1.0) - (s0 * s0 + dm * dm) / (sd * sd))
            g = np.concatenate([gm, gs], axis=1)
        assert g.dtype == np.float32
        r["ghead"] = g
    return {k: np.asarray(v, dtype=np.float64) for k, v in r.items()}


# ------------------------------------------------------------------ comparison in scale units
def _units(got, ref, scale):
    """max |got - ref| / scale; an entry of scale 0 must be exact (inf otherwise).  A
    distance below float32's smallest normal number counts as 0: a result down there has
    no relative precision left (and may be flushed to 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err = np.where(err <= F32_TINY, 0.0, err)
    pos = scale > 0
    if (err[~pos] != 0).any():
        return np.inf
    return float((err[pos] / scale[pos]).max()) if pos.any() else 0.0


def wave_of_row(n, prow):
    """partial row head_rows_kernel adds row r to: block (r / 256) mod grid, wave (r mod 256) / 64."""
    r = np.arange(n)
    return ((r // 256) % (prow // 4)) * 4 + (r % 256) // 64


def partial_rows_of(n):
    """mrl_partial_rows(n): 4 waves x min(ceil(n / 128), 1536) blocks."""
    return 4 * min(max((n + 127) // 128, 1), 1536)


def compare(key, ref, out=None, ghead=None, terms=None, partial=None, n=0):
    """{key.what: distance in scale units}.  terms: per-row loss terms (summed here per
    wave, as partial holds them); partial: the kernel's [prow, 4] rows."""
    u = {}
    if "out" in ref:
        u[key + ".out"] = _units(out, *ref["out"])
    if "ghead" in ref:
        u[key + ".ghead"] = _units(ghead, *ref["ghead"])
    if "terms" in ref:
        prow = partial_rows_of(n)
        wv = wave_of_row(n, prow)
        for c, what in enumerate(("surr", "kl", "ent")):
            want = np.bincount(wv, weights=ref["terms"][:, c], minlength=prow)
            scale = np.bincount(wv, weights=ref["tscale"][:, c], minlength=prow)
            got = partial[:, c] if partial is not None else np.bincount(wv, weights=terms[:, c], minlength=prow)
            u[f"{key}.{what}"] = _units(got, want, scale)
    return u


def sgd_cases(head, A):
    """(n, side, inputs, kl_cutoff): a cutoff the float64 minibatch KL clears by 2x on either
    side (a categorical of one outcome has KL 0: only the side below exists)."""
    for n in SGD_NS:
        for side in ("below", "above"):
            d = make_inputs(head, A, n, near=(side == "below"))
            kl_mb = ref_rows(d, LOSSES)["terms"][:, 1].sum() / n
            if side == "above" and kl_mb == 0.0:
                continue
            cutoff = float(F(2.5 * kl_mb if side == "below" else 0.4 * kl_mb)) if kl_mb > 0 else 0.02
            assert kl_mb <= 0.5 * cutoff if side == "below" else kl_mb >= 2.0 * cutoff
            yield n, side, d, cutoff


def _sgd_kw(n, cutoff):
    return dict(inv_ng=1.0 / n, kl_coeff=SGD_KL_COEFF, kl_cutoff=cutoff, cutoff_coeff=SGD_CUTOFF_COEFF)


def all_cases():
    """(key, inputs, epilogue, scalar arguments) of every mrl_head_rows comparison in this file."""
    for head in ("softmax", "gauss"):
        for A in AS:
            for n in NS:
                for name, (epi, rev, kc) in POLICY_EPIS.items():
                    yield f"{head}.{name}", make_inputs(head, A, n), epi, dict(inv_ng=1.0 / (n + 3), kl_coeff=kc, reverse=rev)
            for n, side, d, cutoff in sgd_cases(head, A):
                yield f"{head}.sgd_{side}", d, PPOSGD, _sgd_kw(n, cutoff)
        for name, (epi, rev, kc) in POLICY_EPIS.items():
            yield f"{head}.{name}", make_inputs(head, 2, BIG_N), epi, dict(inv_ng=1.0 / BIG_N, kl_coeff=kc, reverse=rev)
    for n in NS:
        for name, (epi, rev, kc) in LINEAR_EPIS.items():
            yield f"linear.{name}", make_inputs("linear", 1, n), epi, dict(inv_ng=1.0 / (n + 3))


def measure_floors():
    floors = {}
    for key, d, epi, kw in all_cases():
        f = f32_rows(d, epi, **kw)
        for k, v in compare(key, ref_rows(d, epi, **kw), f.get("out"), f.get("ghead"), f.get("terms"), n=d["n"]).items():
            floors[k] = max(floors.get(k, 0.0), v)
    for head in ("softmax", "gauss"):
        for k, n in probtype_cases():
            for what, v in probtype_units(head, k, n, probtype_f32(head, k, n)).items():
                floors[what] = max(floors.get(what, 0.0), v)
    return floors


def test_recorded_floors_are_the_float32_restatements_distance():
    """FLOOR is what measure_floors() gives (CPU only): no recorded floor is below the
    restatement's distance by more than the spread between numpy builds' expf / logf
    (1.5x), and every comparison of this file has one."""
    got = measure_floors()
    assert set(got) == set(FLOOR), set(got) ^ set(FLOOR)
    for k, v in got.items():
        assert np.isfinite(v) and v <= 1.5 * FLOOR[k], (k, v, FLOOR[k])


# ------------------------------------------------------------------ the kernel
def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run_head(d, epi, inv_ng=1.0, kl_coeff=0.0, reverse=0, kl_cutoff=0.0, cutoff_coeff=0.0, skip=0, slack=3,
             n_rows=None):
    """One mrl_head_rows launch into sentinel-filled buffers with `slack` rows to spare.
    Returns (out [n + slack, w], ghead [n + slack, gh], partial [prow + 2, 4], error)."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    head, A, n = d["head"], d["A"], d["n"]
    gh = 2 * A if head == "gauss" else A
    prow = int(_lib.load().mrl_partial_rows(n))
    assert prow == partial_rows_of(n)
    out = torch.full(((n + slack) * gh,), SENT, dtype=torch.float32, device="cuda")
    ghead = torch.full(((n + slack) * gh,), SENT, dtype=torch.float32, device="cuda")
    partial = torch.full(((prow + 2) * 4,), SENT, dtype=torch.float64, device="cuda")
    t = {k: _dev(d.get(k)) for k in ("z", "dz", "logstd", "dlogstd", "act", "adv", "oldprob", "target")}
    skipt = torch.tensor([skip], dtype=torch.int32, device="cuda")
    io = _lib.RowsIO(None, None, 1.0, n if n_rows is None else n_rows, float(inv_ng), ptr(t["act"]), ptr(t["adv"]),
                     ptr(t["oldprob"]), ptr(t["target"]), ptr(out), ptr(ghead), ptr(partial), float(kl_coeff),
                     float(kl_cutoff), float(cutoff_coeff), int(reverse), 0, None, None)
    error = None
    try:
        call("mrl_head_rows", HEADS[head], A, epi, ptr(t["z"]), ptr(t["dz"]), ptr(t["logstd"]), ptr(t["dlogstd"]),
             ctypes.byref(io), ptr(skipt), stream())
    except _lib.MrlError as e:
        error = e
    torch.cuda.synchronize()
    host = [b.cpu().numpy().astype(np.float64) for b in (out, ghead, partial)]
    return host[0].reshape(n + slack, gh), host[1].reshape(n + slack, gh), host[2].reshape(prow + 2, 4), error


def check_case(key, d, epi, kw):
    n = d["n"]
    out, ghead, partial, error = run_head(d, epi, **kw)
    assert error is None, error
    ref = ref_rows(d, epi, **kw)
    prow = partial_rows_of(n)
    ctx = (key, d["A"], n)
    # nothing past row n (rows are contiguous at the stride gh: nothing past column gh
    # either), nothing at all in a buffer the epilogue does not write
    assert (out[n if "out" in ref else 0:] == SENT).all(), ctx
    assert (ghead[n if "ghead" in ref else 0:] == SENT).all(), ctx
    assert (partial[prow:] == SENT).all(), ctx
    # every partial row is written: zeros from waves without rows and from the epilogues
    # without loss terms, column 3 always zero
    assert (partial[:prow, 3] == 0.0).all(), ctx
    if "terms" not in ref:
        assert (partial[:prow] == 0.0).all(), ctx
    units = compare(key, ref, out[:n], ghead[:n], partial=partial[:prow], n=n)
    for k, v in units.items():
        assert v <= TOL[k], (ctx, k, v, TOL[k])
    if "terms" in ref:  # the column sums are the float64 sums of the per-row reference
        for c in range(3):
            assert abs(partial[:prow, c].sum() - ref["terms"][:, c].sum()) <= TOL[f"{key}.{('surr', 'kl', 'ent')[c]}"] * \
                ref["tscale"][:, c].sum(), (ctx, c)
    return units


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("head", ["softmax", "gauss"])
def test_policy_head_rows_per_entry(head, A, n):
    d = make_inputs(head, A, n)
    for name, (epi, rev, kc) in POLICY_EPIS.items():
        check_case(f"{head}.{name}", d, epi, dict(inv_ng=1.0 / (n + 3), kl_coeff=kc, reverse=rev))


@pytest.mark.parametrize("n", NS)
def test_linear_head_rows_per_entry(n):
    d = make_inputs("linear", 1, n)
    for name, (epi, _, _) in LINEAR_EPIS.items():
        check_case(f"linear.{name}", d, epi, dict(inv_ng=1.0 / (n + 3)))


@pytest.mark.parametrize("head", ["softmax", "gauss"])
def test_head_rows_grid_stride_second_trip(head):
    """n = 1536 * 256 + 257: the smallest batch whose last rows are a block's second trip."""
    d = make_inputs(head, 2, BIG_N)
    for name, (epi, rev, kc) in POLICY_EPIS.items():
        check_case(f"{head}.{name}", d, epi, dict(inv_ng=1.0 / BIG_N, kl_coeff=kc, reverse=rev))


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("head", ["softmax", "gauss"])
def test_pposgd_head_rows_both_sides_of_the_cutoff(head, A):
    """One minibatch per launch at 1, 63, 64, 65 and 128 rows (waves without rows add 0 to
    the block's KL and write zero partial rows), the minibatch KL 2x above and 2x below
    the cutoff: slope kl_coeff + 2 cutoff_coeff (kl - cutoff) above it, kl_coeff below."""
    sides = set()
    for n, side, d, cutoff in sgd_cases(head, A):
        kw = _sgd_kw(n, cutoff)
        ref = ref_rows(d, PPOSGD, **kw)
        assert (ref["slope"] > SGD_KL_COEFF) == (side == "above")
        check_case(f"{head}.sgd_{side}", d, PPOSGD, kw)
        sides.add(side)
    assert "below" in sides and ("above" in sides or (head, A) == ("softmax", 1))


@pytest.mark.parametrize("head", ["softmax", "gauss"])
def test_pposgd_rejects_129_rows_without_writing(head):
    d = make_inputs(head, 3, 129)
    out, ghead, partial, error = run_head(d, PPOSGD, **_sgd_kw(129, 0.02))
    assert error is not None and "exceeds one block" in str(error)
    assert (out == SENT).all() and (ghead == SENT).all() and (partial == SENT).all()


@pytest.mark.parametrize("head", ["softmax", "gauss", "linear"])
def test_skip_flag_leaves_every_output_untouched(head):
    d = make_inputs(head, 1 if head == "linear" else 3, 100)
    epis = dict(LINEAR_EPIS if head == "linear" else POLICY_EPIS)
    if head != "linear":
        epis["sgd"] = (PPOSGD, 0, SGD_KL_COEFF)
    for name, (epi, rev, kc) in epis.items():
        out, ghead, partial, error = run_head(d, epi, inv_ng=0.01, kl_coeff=kc, reverse=rev, kl_cutoff=0.02,
                                              cutoff_coeff=SGD_CUTOFF_COEFF, skip=1)
        assert error is None, error
        assert (out == SENT).all() and (ghead == SENT).all() and (partial == SENT).all(), name


# ------------------------------------------------------------------ mrl_probtype_rows
def probtype_cases():
    for k in (1, 3, 8, 9, 32):
        for n in (1, 257):
            yield k, n
    yield 3, PROBTYPE_BIG_N


def _probtype_inputs(head, k, n):
    """prob rows (the float32 rounding of the new distribution), prob2 = the old rows, x = the actions."""
    d = make_inputs(head, k, n)
    if head == "softmax":
        prob = _f32(T.softmax(d["z"].astype(np.float64)))
    else:
        prob = np.concatenate([d["z"], np.repeat(np.exp(d["logstd"])[None, :], n, axis=0)], axis=1)
    return prob, d["oldprob"], d["act"]


def probtype_ref(head, k, n):
    """float64 (loglik, kl[prob, prob2], entropy) per row with their scales."""
    prob, prob2, x = (a.astype(np.float64) for a in _probtype_inputs(head, k, n))
    sp = SimpleNamespace(head=head, n_out=k)
    ll, kl, ent = T.loglik(sp, x, prob), T.kl(sp, prob, prob2), T.entropy(sp, prob)
    if head == "softmax":
        Lp = np.maximum(1.0, np.abs(np.log(prob)))
        return (ll, np.abs(ll)), (kl, _rowmax(prob * np.maximum(1.0, np.abs(np.log(prob / prob2))))), \
            (ent, _rowmax(prob * Lp))
    m, s, m2, s2 = prob[:, :k], prob[:, k:], prob2[:, :k], prob2[:, k:]
    u = (x - m) / s
    lls = np.maximum.reduce([0.5 * (u * u).sum(axis=1), np.full(n, 0.5 * LOG2PI * k), np.abs(np.log(s).sum(axis=1))])
    kls = np.maximum.reduce([_rowmax(np.log(s2 / s)), _rowmax((s * s + (m - m2) ** 2) / (2.0 * s2 * s2)),
                             np.full(n, 0.5 * k)])
    ents = np.maximum(_rowmax(np.log(s)), 0.5 * (LOG2PI + 1.0) * k)
    return (ll, lls), (kl, kls), (ent, ents)


def probtype_f32(head, k, n):
    """probtype_rows_kernel in numpy float32."""
    p, p2, x = _probtype_inputs(head, k, n)
    zero = np.zeros(n, dtype=np.float32)
    kl, ent = zero.copy(), zero.copy()
    if head == "softmax":
        ll = np.log(p[np.arange(n), x])
        for j in range(k):
            kl = kl + p[:, j] * np.log(p[:, j] / p2[:, j])
            ent = ent + (-(p[:, j] * np.log(p[:, j])))
        return ll, kl, ent
    sumlog, q = zero.copy(), zero.copy()
    for j in range(k):
        sumlog = sumlog + np.log(p[:, k + j])
        u = (x[:, j] - p[:, j]) / p[:, k + j]
        q = q + u * u
        dm = p[:, j] - p2[:, j]
        kl = kl + (np.log(p2[:, k + j] / p[:, k + j]) + (p[:, k + j] * p[:, k + j] + dm * dm) /
                   (F(2.0) * p2[:, k + j] * p2[:, k + j]))
    ll = F(-0.5) * q - F(0.5) * LOG2PI_F * F(k) - sumlog
    return ll, kl - F(0.5 * k), sumlog + F(0.5) * LOG2PIE_F * F(k)


def probtype_units(head, k, n, got):
    return {f"probtype.{head}.{what}": _units(g, *r)
            for what, g, r in zip(("loglik", "kl", "ent"), got, probtype_ref(head, k, n))}


@pytest.mark.parametrize("k,n", list(probtype_cases()))
@pytest.mark.parametrize("head", ["softmax", "gauss"])
def test_probtype_rows_per_row(head, k, n):
    from modular_rl_amd._lib import call, ptr, stream
    prob, prob2, x = (_dev(a) for a in _probtype_inputs(head, k, n))
    outs = [torch.full((n + 3,), SENT, dtype=torch.float32, device="cuda") for _ in range(3)]
    call("mrl_probtype_rows", HEADS[head], k, n, ptr(prob), ptr(prob2), ptr(x), ptr(outs[0]), ptr(outs[1]),
         ptr(outs[2]), stream())
    torch.cuda.synchronize()
    host = [o.cpu().numpy().astype(np.float64) for o in outs]
    assert all((h[n:] == SENT).all() for h in host)
    for key, v in probtype_units(head, k, n, [h[:n] for h in host]).items():
        assert v <= TOL[key], (key, k, n, v, TOL[key])
