"""The one-pass Fisher product and policy gradient (mlp_fisher_hyb_kernel) at three waves
per SIMD: four producer waves per block and the VJP of their tiles divided between two
waves each.  Row counts at every boundary of the launch geometry -- a single row, a tile,
one tile per producer wave, a last round in which some waves of a block have a tile and
others none, and more than two rounds (every mailbox slot reused, the gradient's two-round
lag included) -- on the whole device and on a one-CU stream (one block: many rounds at
small N).  Tolerances are those of test_gpu_split.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import trpo_np as T

SHAPES = [("gauss", 11, 3), ("softmax", 4, 2)]  # the static shapes: Hopper-v2, CartPole-v0
W = 4              # producer waves per block (a 32-row tile each per round)
DEVICE_BLOCKS = 256  # the grid's cap on the whole device; one block per CU of a subset


def _sizes(blocks):
    w, b = W, blocks
    return sorted({1, 31, 32, 33, 32 * w - 1, 32 * w, 32 * w + 1, 32 * w * b - 1, 32 * w * b + 1, 32 * w * b * 3 + 17})


# (cus, N): cus = 0 is the whole device, cus = 1 the smallest stream a desc accepts
GEOMETRY = [(0, n) for n in _sizes(DEVICE_BLOCKS)] + [(1, n) for n in _sizes(1)]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).cuda()  # a copy: the shared arrays are read-only


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _problem(head, nin, nout, N):
    """Inputs and the float64 oracle's results, computed once per (shape, N) and shared by
    the tests (read-only)."""
    rng = np.random.default_rng(nin * 19 + N)
    spec = T.Spec(nin, [64, 64], nout, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-nout:] = 0.3 * rng.standard_normal(nout)
    th = _f32(th)
    ob = _f32(rng.standard_normal((N, nin)))
    oldprob = _f32(T.policy_prob(spec, th + 0.01 * rng.standard_normal(spec.P), ob))
    act = T.sample(spec, oldprob, rng.standard_normal((N, nout)) if head == "gauss" else rng.random(N))
    if head == "gauss":
        act = _f32(act)
    adv = _f32(rng.standard_normal(N))
    v = (0.1 * rng.standard_normal(spec.P)).astype(np.float32)
    want = dict(fvp=T.fisher_vector_product(spec, th, v.astype(np.float64), ob),
                pg=T.policy_gradient(spec, th, ob, act, adv, oldprob),
                sums=T.surr_kl_ent(spec, th, ob, act, adv, oldprob))
    for a in (th, ob, oldprob, act, adv, v, *want.values()):
        a.setflags(write=False)
    return spec, th, ob, oldprob, act, adv, v, want


def _net(monkeypatch, head, nin, nout, th, cus):
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import MlpNet
    monkeypatch.setenv("MRL_FISHER", "split")
    monkeypatch.setenv("MRL_GRAD_ONEPASS", "1")
    net = MlpNet(nin, nout, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX)
    assert net.fisher_onepass and net.grad_onepass
    net.set_flat(th.copy())  # the shared problem's arrays are read-only
    if cus:
        net.size_for_cus(cus)
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("head,nin,nout", SHAPES)
@pytest.mark.parametrize("cus,N", GEOMETRY)
def test_fisher_product_at_geometry_boundaries(head, nin, nout, cus, N, monkeypatch):
    """mrl_mlp_fisher_hyb against the float64 oracle at 1e-4, against the two-kernel pair
    (split JVP rows, then the hybrid VJP) at 1e-5, and bit-identical over three runs."""
    from modular_rl_amd import _lib
    spec, th, ob, oldprob, act, adv, v, want = _problem(head, nin, nout, N)
    net = _net(monkeypatch, head, nin, nout, th, cus)
    x, vt = _dev(ob), _dev(v)
    a = _dev(act, torch.int32 if head == "softmax" else torch.float32)
    partial = torch.zeros(net.partial_rows(N) * 4, dtype=torch.float64, device="cuda")
    gh = torch.zeros(N * net.gh, dtype=torch.float32, device="cuda")
    net.rows(_lib.EPI_SURRGRAD, x, N, inv_n_global=1.0 / N, act=a, adv=_dev(adv), oldprob=_dev(oldprob), ghead=gh,
             partial=partial)  # records the activation cache
    imgs = net.new_tangent_image()
    net.pack_tangent(vt, imgs)
    assert net.fisher_onepass_applies(x, N, imgs)
    f1 = [torch.full((net.P,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    for f in f1:
        assert net.fisher_product(x, N, 1.0 / N, vt, imgs, f)
    torch.cuda.synchronize()
    for f in f1[1:]:
        assert torch.equal(f, f1[0])
    gh2 = torch.full_like(gh, float("nan"))
    net.rows(_lib.EPI_FVP, x, N, inv_n_global=1.0 / N, ghead=gh2, tangent=vt, image_t=imgs)
    f2 = torch.zeros(net.P, dtype=torch.float32, device="cuda")
    net.vjp_flat(x, N, gh2, f2)
    one, two = f1[0].cpu().numpy().astype(np.float64), f2.cpu().numpy().astype(np.float64)
    assert np.isfinite(one).all()
    print(f"fvp {head} cus={cus} N={N}: pair {_rel(one, two):.3e} oracle {_rel(one, want['fvp']):.3e}")
    assert _rel(one, two) < 1e-5
    assert _rel(one, want["fvp"]) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("head,nin,nout", SHAPES)
@pytest.mark.parametrize("cus,N", GEOMETRY)
def test_policy_gradient_at_geometry_boundaries(head, nin, nout, cus, N, monkeypatch):
    """mrl_mlp_grad_hyb against the float64 oracle at 1e-4, against the two-kernel pair
    (SURRGRAD rows of mrl_mlp_rows_split, then the hybrid VJP) at 1e-5, bit-identical over
    three runs; the activation cache it records bit for bit the pair's; the surr / KL /
    entropy sums to 1e-12."""
    from modular_rl_amd import _lib
    spec, th, ob, oldprob, act, adv, v, want = _problem(head, nin, nout, N)
    net = _net(monkeypatch, head, nin, nout, th, cus)
    x, advd, opd = _dev(ob), _dev(adv), _dev(oldprob)
    a = _dev(act, torch.int32 if head == "softmax" else torch.float32)
    ncache = ((N + 31) // 32) * 64 * 64
    # the two-kernel pair
    net._cache(N).fill_(float("nan"))
    partial = torch.zeros(net.partial_rows(N) * 4, dtype=torch.float64, device="cuda")
    gh = torch.full((N * net.gh,), float("nan"), device="cuda")
    net.rows(_lib.EPI_SURRGRAD, x, N, inv_n_global=1.0 / N, act=a, adv=advd, oldprob=opd, ghead=gh, partial=partial)
    s2 = torch.zeros(4, dtype=torch.float64, device="cuda")
    net.reduce_partial(partial, N, s2)
    c2 = net._cache(N)[:ncache].clone()
    g2 = torch.zeros(net.P, device="cuda")
    net.vjp_flat(x, N, gh, g2)
    # the one launch, three times
    runs = []
    for _ in range(3):
        net._cache(N).fill_(float("nan"))
        g1 = torch.full((net.P,), float("nan"), device="cuda")
        s1 = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
        assert net.policy_gradient(x, N, 1.0 / N, a, advd, opd, g1, s1)
        runs.append((g1, s1, net._cache(N)[:ncache].clone()))
    torch.cuda.synchronize()
    for g1, s1, c1 in runs[1:]:
        assert torch.equal(g1, runs[0][0]) and torch.equal(s1, runs[0][1]) and torch.equal(c1, runs[0][2])
    g1, s1, c1 = (t.cpu().numpy().astype(np.float64) for t in runs[0])
    assert np.array_equal(c1, c2.cpu().numpy().astype(np.float64), equal_nan=True)
    assert np.isfinite(g1).all()
    two = g2.cpu().numpy().astype(np.float64)
    print(f"pg {head} cus={cus} N={N}: pair {_rel(g1, two):.3e} oracle {_rel(g1, want['pg']):.3e}")
    assert _rel(g1, two) < 1e-5
    np.testing.assert_allclose(s1[:3], s2.cpu().numpy()[:3], rtol=1e-12, atol=1e-12 * np.abs(s1[:3]).max())
    assert s1[3] == 0.0
    assert _rel(g1, want["pg"]) < 1e-4


def test_host_sizing_matches_the_launch_geometry():
    """No GPU: mrl_mlp_fisher_hyb_fits accepts exactly the static shapes, its LDS total (the
    kernel's static arrays -- W2 fragments, one 4 KB h1 buffer per VJP wave of eight, the
    split W1^T, the mailbox slots of four producer waves -- plus the split images) is within
    160 KB for both instantiations, and mrl_mlp_slab_rows is four rows (one per VJP wave
    pair, and per producer wave) per block of the grid."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    kinds = {"gauss": _lib.HEAD_GAUSS, "softmax": _lib.HEAD_SOFTMAX}
    for head, nin, nout in SHAPES:
        d = _lib.MlpDesc(nin, nout, kinds[head], 64, 2)
        assert lib.mrl_mlp_fisher_hyb_fits(ctypes.byref(d)) == 1
        image = 4 * lib.mrl_mlp_image_words_split(ctypes.byref(d))
        mbox_slot = W * 32 * 16 * 4
        static = 2 * 4 * 64 * 4 + 8 * 16 * 64 * 4 + 2 * 4 * 3 * 64 * 16
        product, gradient = 2 * image + static + 2 * mbox_slot, image + static + 3 * mbox_slot
        assert max(product, gradient) <= 160 * 1024, (head, product, gradient)
        for cus in (0, 1, 48, 192, 256):
            dc = _lib.MlpDesc(nin, nout, kinds[head], 64, 2, cus)
            blocks_cap = DEVICE_BLOCKS if cus == 0 else cus
            for _, n in GEOMETRY + [(0, 4096 * 1024)]:
                blocks = min(-(-(-(-n // 32)) // W), blocks_cap)
                assert lib.mrl_mlp_slab_rows(ctypes.byref(dc), n) == 4 * blocks, (head, cus, n)
    # not a static shape, and a value net: the one-pass kernel does not apply
    assert lib.mrl_mlp_fisher_hyb_fits(ctypes.byref(_lib.MlpDesc(17, 6, _lib.HEAD_GAUSS, 64, 2))) == 0
    assert lib.mrl_mlp_fisher_hyb_fits(ctypes.byref(_lib.MlpDesc(11, 1, _lib.HEAD_LINEAR, 64, 2))) == 0
