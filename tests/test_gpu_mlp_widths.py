"""The fused 64-wide MLP kernels at every input / output width edge, entry by entry
(cases, float64 references, per-entry scales and TOL = 4 x FLOOR: tests/mlp_width_cases.py;
the CPU side: tests/test_mlp_widths_host.py).  Everything goes through ``MlpNet`` and the C
ABI under it; the kernel variants are chosen as the other tests choose them (MRL_FISHER /
MRL_ROWS_SPLIT / MRL_FISHER_ONEPASS / MRL_GRAD_ONEPASS before the net is constructed,
``net.use_cache``, ``image=net.image`` for the uncached exact-f32 VJP).

Guard bands.  Every input (x, ep_t, the head rows G, the tangent) is a view at a multiple of
256 bytes inside a larger allocation whose other bytes are NaN (ep_t: a huge step index), and
every output (out, feat_out, ghead, the result vector) a view between sentinel margins: after
each call the margins are bit-unchanged and the result is finite.  The kernels' masks are
multiplicative, so a stray read inside the allocation surfaces as a NaN.  The activation cache
is not guarded: the recording pass writes the rows past N of its last tile on purpose.

The cached VJP (``vjp_flat`` after a recording pass) is mlp_vjp16_kernel at O % 16 != 0 -- its
hybrid form (the two 64x64x16 products on split bf16 operands) at O < 16, the exact-f32 WIDE
form at O > 16 -- and the 32-row kernel reading the cache at O = 16 and 32."""
import numpy as np
import pytest
import torch

from tests import mlp_width_cases as C

pytestmark = pytest.mark.gpu

PAD = 64        # margin elements: 256 bytes of float32 / int32
SENT = 777.25   # sentinel of the output margins
HUGE_T = 1 << 30
POLICY_SHAPES = [s for s in C.SHAPES if s[0] != "linear"]


class Guarded:
    """A [shape] view 256 bytes into an allocation with PAD margin elements either side."""

    def __init__(self, shape, dtype=torch.float32, data=None, fill=float("nan")):
        n = int(np.prod(shape))
        self.full = torch.full((PAD + n + PAD,), fill, dtype=dtype, device="cuda")
        self.n = n
        self.v = self.full[PAD:PAD + n].view(*shape)
        assert self.v.data_ptr() % 256 == 0
        if data is not None:
            self.v.copy_(torch.from_numpy(np.array(data)).to(dtype).view(*shape))
        self.margins = self._margins().clone()

    def _margins(self):
        return torch.cat([self.full[:PAD], self.full[PAD + self.n:]]).view(torch.int32)

    def intact(self):
        return torch.equal(self._margins(), self.margins)

    def numpy(self):
        return self.v.cpu().numpy()


def _in(a, dtype=torch.float32):
    return Guarded(a.shape, dtype, data=a, fill=HUGE_T if dtype == torch.int32 else float("nan"))


def _out(*shape):
    g = Guarded(shape, fill=SENT)
    g.v.fill_(float("nan"))  # a result entry the kernel leaves unwritten is not finite
    return g


def _intact(*gs):
    assert all(g.intact() for g in gs), "a guard margin was written"


def _nets(monkeypatch, head, O, A):
    """(the exact-f32 net: MRL_FISHER=f32, so no split rows either; the default net: split
    forward rows, split Fisher rows, hybrid cached VJP)."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import MlpNet
    h = {"gauss": _lib.HEAD_GAUSS, "softmax": _lib.HEAD_SOFTMAX, "linear": _lib.HEAD_LINEAR}[head]
    monkeypatch.setenv("MRL_FISHER", "f32")
    f32 = MlpNet(O, A, h)
    for k, v in (("MRL_FISHER", "split"), ("MRL_ROWS_SPLIT", "1"), ("MRL_FISHER_ONEPASS", "1"), ("MRL_GRAD_ONEPASS", "1")):
        monkeypatch.setenv(k, v)
    split = MlpNet(O, A, h)
    assert not f32.fisher_split and not f32.rows_split and split.fisher_split and split.rows_split
    # no width of the list is a static shape: the one-launch forms must not apply
    assert not C.fisher_hyb_fits(O, A, head) and not split.fisher_onepass and not split.grad_onepass
    return {"f32": f32, "split": split}


def _rows_inputs(c):
    x = _in(c.obs)
    et = _in(c.ept, torch.int32) if c.ept is not None else None
    return x, et, dict(ep_t=None if et is None else et.v, timestep_limit=C.EPT_LIMIT if et is not None else 1.0)


def _record(net, c, x, kw):
    """A recording pass at the net's theta over the case's rows (SURRGRAD; VFLOSS for a value
    net): h1 / h2 into the activation cache the cached VJP and Fisher rows then read."""
    from modular_rl_amd import _lib
    N, A = c.N, c.A
    partial = torch.zeros(net.partial_rows(N) * 4, dtype=torch.float64, device="cuda")
    gh = torch.zeros(N * net.gh, dtype=torch.float32, device="cuda")
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    if c.head == "linear":
        net.rows(_lib.EPI_VFLOSS, x.v, N, inv_n_global=1.0 / N, target=z(N), ghead=gh, partial=partial, **kw)
    elif c.head == "softmax":
        net.rows(_lib.EPI_SURRGRAD, x.v, N, inv_n_global=1.0 / N, act=z(N, dt=torch.int32), adv=z(N) + 1,
                 oldprob=z(N, A) + 1.0 / A, ghead=gh, partial=partial)
    else:
        net.rows(_lib.EPI_SURRGRAD, x.v, N, inv_n_global=1.0 / N, act=z(N, A), adv=z(N) + 1,
                 oldprob=torch.cat([z(N, A), z(N, A) + 1], dim=1).contiguous(), ghead=gh, partial=partial)
    assert net._cache_key is not None
    torch.cuda.synchronize()


def _check(c, ref, name, got, what):
    bad = C.within(c, name, got, ref)
    assert bad == [], (what, (c.head, c.O, c.A, c.N), bad)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape", list(C.SHAPES), ids=C.shape_id)
def test_forward_rows_per_entry(shape, monkeypatch):
    """EPI_PROB on the exact-f32 rows kernel and on mrl_mlp_rows_split: z (the gauss mean
    columns, the value) and the softmax probabilities per entry, the gauss std columns as
    exp(logstd), the value nets' feature rows [obs, f32(ep_t / limit)] exactly."""
    head, O, A, ept = shape
    nets = _nets(monkeypatch, head, O, A)
    for N in C.SHAPES[shape]:
        c, ref = C.make_case(head, O, A, N, ept), C.reference(head, O, A, N, ept)
        x, et, kw = _rows_inputs(c)
        for name, net in nets.items():
            net.set_flat(np.array(c.th))
            out = _out(N) if head == "linear" else _out(N, c.gh)
            feat = _out(N, O) if ept else None
            net.forward(x.v, N, out=out.v, feat_out=None if feat is None else feat.v, **kw)
            torch.cuda.synchronize()
            _intact(x, out, *([et, feat] if ept else []))
            got = out.numpy().astype(np.float64).reshape(N, -1)
            assert np.isfinite(got).all(), (name, N)
            if head == "softmax":
                _check(c, ref, "prob", got, name)
            else:
                _check(c, ref, "z", got[:, :A], name)
            if head == "gauss":
                std = np.exp(c.th[-A:].astype(np.float64))
                np.testing.assert_allclose(got[:, A:], np.repeat(std[None, :], N, axis=0), rtol=C.STD_RTOL, atol=0)
            if ept:
                assert np.array_equal(feat.numpy(), c.X.astype(np.float32)), (name, N)


# ------------------------------------------------------------------ VJP of supplied head rows
@pytest.mark.parametrize("shape", list(C.SHAPES), ids=C.shape_id)
def test_vjp_of_supplied_head_rows_per_entry(shape, monkeypatch):
    """mrl_mlp_vjp of head rows the test supplies (dense, and non-zero only in the last row's
    last columns): the uncached 32-row kernel, then the cached kernel of the width after an
    exact-f32 recording pass and after a split one.  Every entry of every parameter block at
    TOL; the log-std slots are the column sums of G[:, A:]; for the value nets the gradient
    row of the time-feature column and the b0 gradient (the ones column beside it) are
    checked on their own."""
    head, O, A, ept = shape
    nets = _nets(monkeypatch, head, O, A)
    kernel = C.vjp_kernel(O, cached=True)
    assert kernel == ("vjp32" if O in (16, 32) else "vjp16_wide" if O > 16 else "vjp16")
    sl = C.block_slices(O, A, head)
    for N in C.SHAPES[shape]:
        c, ref = C.make_case(head, O, A, N, ept), C.reference(head, O, A, N, ept)
        x, et, kw = _rows_inputs(c)
        G = {k: _in(g) for k, g in c.G.items()}

        def run(net, gname, what, **extra):
            out = _out(c.P)
            net.vjp_flat(x.v, N, G[gname].v.view(-1), out.v, **kw, **extra)
            torch.cuda.synchronize()
            _intact(x, G[gname], out, *([et] if ept else []))
            got = out.numpy().astype(np.float64)
            what = (what, gname, kernel)
            _check(c, ref, "vjp." + gname, got, what)
            if ept:
                want, scale = ref["vjp." + gname]
                t_row = slice(sl["W0"].start + (O - 1) * 64, sl["W0"].stop)
                for part, key in ((t_row, "vjp.W0"), (sl["b0"], "vjp.b0")):
                    assert C.distance(got[part], want[part], scale[part]) <= C.TOL[key], (what, N, key)

        for net in nets.values():
            net.set_flat(np.array(c.th))
        for gname in G:
            run(nets["f32"], gname, "uncached", image=nets["f32"].image)
        for name, net in nets.items():
            _record(net, c, x, kw)
            key = net._cache_key
            for gname in G:
                run(net, gname, "cached after the %s rows" % name)
            assert net._cache_key == key == net._key(x.v, N, kw["ep_t"], kw["timestep_limit"])


# ------------------------------------------------------------------ Fisher product
@pytest.mark.parametrize("shape", POLICY_SHAPES, ids=C.shape_id)
def test_fisher_product_per_entry(shape, monkeypatch):
    """The exact-f32 pair (rows(EPI_FVP) + vjp_flat) uncached and on the activation cache, and
    the split pair (mrl_mlp_fvp_split + the cached VJP), per entry against
    T.fisher_vector_product.  No width here is a static shape, so MlpNet.fisher_product
    (mrl_mlp_fisher_hyb) must decline."""
    from modular_rl_amd import _lib
    head, O, A, ept = shape
    nets = _nets(monkeypatch, head, O, A)
    for N in C.SHAPES[shape]:
        c, ref = C.make_case(head, O, A, N, ept), C.reference(head, O, A, N, ept)
        x, _, kw = _rows_inputs(c)
        v = _in(c.v)

        def product(net, image_t, what):
            gh, fv = _out(N * c.gh), _out(c.P)
            net.rows(_lib.EPI_FVP, x.v, N, inv_n_global=1.0 / N, ghead=gh.v, tangent=v.v, image_t=image_t)
            torch.cuda.synchronize()
            assert np.isfinite(gh.numpy()).all(), what
            net.vjp_flat(x.v, N, gh.v, fv.v)
            torch.cuda.synchronize()
            _intact(x, v, gh, fv)
            _check(c, ref, "fvp", fv.numpy().astype(np.float64), what)

        f32, split = nets["f32"], nets["split"]
        f32.set_flat(np.array(c.th))
        imgt = torch.zeros_like(f32.image)
        f32.pack(theta=v.v, image=imgt, fwd_only=True)
        f32.use_cache = False
        product(f32, imgt, "exact f32, uncached")
        f32.use_cache = True
        _record(f32, c, x, kw)
        product(f32, imgt, "exact f32, cached")
        split.set_flat(np.array(c.th))
        _record(split, c, x, kw)
        imgs = split.new_tangent_image()
        split.pack_tangent(v.v, imgs)
        fv = _out(c.P)
        assert split.fisher_product(x.v, N, 1.0 / N, v.v, imgs, fv.v) is False
        assert split._cache_key == split._key(x.v, N, None, 1.0)  # so rows() below takes mrl_mlp_fvp_split
        product(split, imgs, "split")


# ------------------------------------------------------------------ bf16, the corner widths
@pytest.mark.parametrize("shape", C.BF16_SHAPES, ids=C.shape_id)
def test_bf16_corner_widths(shape):
    """The bf16 kernels at the corner widths and N = 3001, under the two bounds of
    tests/test_gpu_bf16.py (its emulation of the same rounding points, and the oracle), which
    rest on averaging over rows; inputs and outputs between guard bands as above."""
    from modular_rl_amd import _lib
    from modular_rl_amd.nets import MlpNet
    from oracle import trpo_np as T
    from tests.test_gpu_bf16 import BF16_EMU_RTOL, BF16_ORACLE_RTOL, _rel, emu_forward, emu_vjp
    head, O, A = shape
    N = C.BF16_N
    c = C.make_case(head, O, A, N, False)
    th = c.th.astype(np.float64)
    net = MlpNet(O, A, _lib.HEAD_GAUSS if head == "gauss" else _lib.HEAD_SOFTMAX, dtype="bf16")
    net.set_flat(np.array(c.th))
    x, _, kw = _rows_inputs(c)
    out = _out(N, c.gh)
    net.forward(x.v, N, out=out.v)
    torch.cuda.synchronize()
    _intact(x, out)
    got = out.numpy().astype(np.float64)
    z, acts = emu_forward(c.spec, th, c.X)
    np.testing.assert_allclose(got, T.head_prob(c.spec, th, z), rtol=BF16_EMU_RTOL, atol=1e-3)
    assert _rel(got, T.policy_prob(c.spec, th, c.X)) < BF16_ORACLE_RTOL
    G = c.G["dense"].astype(np.float64)
    emu = emu_vjp(c.spec, th, acts, G[:, :A], G[:, A:].sum(0) if head == "gauss" else None)
    want, _ = C.vjp_reference(c, G)
    Gd = _in(c.G["dense"])
    for cached in (False, True):
        net.use_cache = cached
        if cached:
            _record(net, c, x, kw)
        fv = _out(c.P)
        net.vjp_flat(x.v, N, Gd.v.view(-1), fv.v)
        torch.cuda.synchronize()
        _intact(x, Gd, fv)
        g = fv.numpy().astype(np.float64)
        assert np.isfinite(g).all()
        assert _rel(g, emu) < BF16_EMU_RTOL, (cached, _rel(g, emu))
        assert _rel(g, want) < BF16_ORACLE_RTOL, (cached, _rel(g, want))
