"""GPU parity of the device-resident CG and step scaling (mrl_cg_init / mrl_cg_update /
mrl_trpo_step_ax / mrl_trpo_step) on a synthetic SPD operator, for the single-block
register path (n <= 8,192), the single-block streaming path (n <= 65,536) and the 256-block
path of wide nets (n > 65,536, e.g. Humanoid P = 727,074), against a numpy restatement of
`trpo.py:165-200` / `trpo.py:119-124` with the same float32 Fisher-product hand-off
(z = (double) fvp32 + damping * p).  Sizes sit on both sides of every switch: 1,024 (one
element per thread), 8,192 | 8,193, 65,536 | 65,537 (512-element chunks, blocks 129 .. 255
empty), 131,072 | 131,073 (the chunk grows to 768)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _oracle(A, b, damping, iters, tol, max_kl, g):
    """The device algorithm in numpy: fvp arrives as float32 of A @ float32(p)."""
    x = np.zeros_like(b)
    ax = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rdotr = r.dot(r)
    its = 0
    for _ in range(iters):
        fvp = A(p.astype(np.float32).astype(np.float64)).astype(np.float32)
        z = fvp.astype(np.float64) + damping * p
        v = rdotr / p.dot(z)
        x += v * p
        ax += v * z
        r -= v * z
        newr = r.dot(r)
        p = r + (newr / rdotr) * p
        rdotr = newr
        its += 1
        if rdotr < tol:
            break
    shs = 0.5 * x.dot(ax)
    lm = np.sqrt(shs / max_kl)
    return x, its, shs, lm, -g.astype(np.float64).dot(x)


SIZES = [5_000, 200_003, 1, 1023, 1024, 1025, 8192, 8193, 65536, 65537, 131072, 131073]
ONE_PER_PATH = [1025, 8193, 65537]


class _Cg:
    """The device CG's buffers for one n, each with a guard tail that must stay unwritten."""
    GUARD = 64

    def __init__(self, lib, n, with_ax=True):
        self.n = n
        f64 = dict(dtype=torch.float64, device="cuda")
        g = self.GUARD
        self.x, self.r, self.p, self.ax, self.fullstep = (torch.full((n + g,), -77.0, **f64) for _ in range(5))
        self.p32 = torch.full((n + g,), -77.0, dtype=torch.float32, device="cuda")
        self.ns = int(lib.mrl_cg_state_doubles(n))
        assert self.ns >= 4 and (n <= 65536 or self.ns > 4)
        self.state = torch.full((self.ns + g,), -77.0, **f64)
        self.state[:self.ns] = 0.0
        self.out = torch.full((self.ns + g,), -77.0, **f64)
        self.out[:self.ns] = 0.0
        self.flag = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.with_ax = with_ax

    def axp(self):
        from modular_rl_amd._lib import ptr
        return ptr(self.ax) if self.with_ax else None

    def init(self, bt):
        from modular_rl_amd._lib import call, ptr, stream
        call("mrl_cg_init", ptr(bt), self.n, ptr(self.x), ptr(self.r), ptr(self.p), ptr(self.p32), self.axp(),
             ptr(self.state), ptr(self.flag), stream())

    def update(self, fvp, damping, tol):
        from modular_rl_amd._lib import call, ptr, stream
        call("mrl_cg_update", ptr(fvp), ctypes.c_double(damping), ctypes.c_double(tol), self.n, ptr(self.x),
             ptr(self.r), ptr(self.p), ptr(self.p32), self.axp(), ptr(self.state), ptr(self.flag), stream())

    def snapshot(self):
        """Every buffer the CG owns, guards included, as raw bits."""
        torch.cuda.synchronize()
        names = ("x", "r", "p", "p32", "state", "flag") + (("ax",) if self.with_ax else ())
        out = {}
        for k in names:
            a = getattr(self, k).cpu().numpy()
            out[k] = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
        return out

    def check_guards(self):
        torch.cuda.synchronize()
        for k in ("x", "r", "p", "p32", "fullstep") + (("ax",) if self.with_ax else ()):
            assert torch.all(getattr(self, k)[self.n:] == -77.0), k + ": written past n"
        assert torch.all(self.state[self.ns:] == -77.0) and torch.all(self.out[self.ns:] == -77.0)


def _system(n):
    rng = np.random.default_rng(n)
    d = rng.uniform(0.5, 2.0, n)
    U = rng.standard_normal((n, 4)) / np.sqrt(n)
    g = rng.standard_normal(n).astype(np.float32)
    return d, U, g


def _run(lib, n, d, U, g, damping, tol, iters, with_ax=True):
    dd, UU = torch.as_tensor(d).cuda(), torch.as_tensor(U).cuda()
    cg = _Cg(lib, n, with_ax)
    cg.init(torch.as_tensor(-g.astype(np.float64)).cuda())
    for _ in range(iters):
        pv = cg.p32[:n].double()
        cg.update((dd * pv + UU @ (UU.T @ pv)).float(), damping, tol)
    return cg


@pytest.mark.parametrize("n", SIZES)
def test_cg_and_step_match_oracle(n):
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, ptr, stream
    lib = _lib.load(require_gpu=True)
    d, U, g = _system(n)

    def A(v):
        return d * v + U @ (U.T @ v)

    b = -g.astype(np.float64)
    damping, tol, iters, max_kl = 0.1, 1e-10, 10, 0.01
    cg = _run(lib, n, d, U, g, damping, tol, iters)
    x, ax, fullstep, out, state = cg.x, cg.ax, cg.fullstep, cg.out, cg.state
    gt = torch.as_tensor(g).cuda()
    call("mrl_trpo_step_ax", ptr(ax), ptr(x), ptr(gt), ctypes.c_double(max_kl), n, ptr(fullstep), ptr(out), stream())
    torch.cuda.synchronize()
    cg.check_guards()
    xw, its, shs, lm, ngx = _oracle(A, b, damping, iters, tol, max_kl, g)
    xd = x[:n].cpu().numpy()
    o = out[:4].cpu().numpy()
    assert int(state[2].item()) == its
    np.testing.assert_allclose(xd, xw, rtol=1e-6, atol=1e-9 * np.abs(xw).max())
    np.testing.assert_allclose(o[0], shs, rtol=1e-6)
    np.testing.assert_allclose(o[1], lm, rtol=1e-6)
    np.testing.assert_allclose(o[2], ngx, rtol=1e-6)
    np.testing.assert_allclose(o[3], ngx / lm, rtol=1e-6)
    np.testing.assert_allclose(fullstep[:n].cpu().numpy(), xw / lm, rtol=1e-6, atol=1e-9 * np.abs(xw / lm).max())
    # mrl_trpo_step: the same scaling from a float32 Fisher product of the final x
    # (trpo.py:119-124), against the oracle's 0.5 x.(fvp + damping x) on its own x
    dd, UU = torch.as_tensor(d).cuda(), torch.as_tensor(U).cuda()
    xs = x[:n]
    fvp = (dd * xs + UU @ (UU.T @ xs)).float()
    full2 = torch.full_like(fullstep, -77.0)
    out2 = torch.full((4 + 64,), -77.0, dtype=torch.float64, device="cuda")
    call("mrl_trpo_step", ptr(fvp), ptr(x), ptr(gt), ctypes.c_double(damping), ctypes.c_double(max_kl), n, ptr(full2),
         ptr(out2), stream())
    torch.cuda.synchronize()
    assert torch.all(full2[n:] == -77.0) and torch.all(out2[4:] == -77.0)
    shs2 = 0.5 * xw.dot(A(xw).astype(np.float32).astype(np.float64) + damping * xw)
    lm2 = np.sqrt(shs2 / max_kl)
    o2 = out2[:4].cpu().numpy()
    np.testing.assert_allclose(o2[0], shs2, rtol=1e-6)
    np.testing.assert_allclose(o2[1], lm2, rtol=1e-6)
    np.testing.assert_allclose(o2[2], ngx, rtol=1e-6)
    np.testing.assert_allclose(o2[3], ngx / lm2, rtol=1e-6)
    np.testing.assert_allclose(full2[:n].cpu().numpy(), xw / lm2, rtol=1e-6, atol=1e-9 * np.abs(xw / lm2).max())


@pytest.mark.parametrize("n", ONE_PER_PATH)
def test_cg_is_reproducible_and_ax_is_optional(n):
    """Two runs of the same case agree bit for bit (every path sums in a fixed order), and
    ax == NULL (allowed in init and update) changes nothing else: x, r, p, p32, the state
    with its block partials and the flag are the same bits."""
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    d, U, g = _system(n)
    first = _run(lib, n, d, U, g, 0.1, 1e-10, 10)
    first.check_guards()
    s0 = first.snapshot()
    s1 = _run(lib, n, d, U, g, 0.1, 1e-10, 10).snapshot()
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    no_ax = _run(lib, n, d, U, g, 0.1, 1e-10, 10, with_ax=False)
    assert torch.all(no_ax.ax == -77.0)
    s2 = no_ax.snapshot()
    for k in s2:
        np.testing.assert_array_equal(s0[k], s2[k], err_msg=k)


@pytest.mark.parametrize("n", ONE_PER_PATH)
def test_cg_early_exit_freezes_every_buffer(n):
    """A diagonal operator with three eigenvalues: rdotr drops below tol at the third update
    and nowhere near it before (tests/test_vector_ops_host.py), so flag[0] = 1 and state[2] = 3
    whatever the summation order; two further updates with a garbage Fisher product must then
    leave x, r, p, p32, ax and the whole state (block partials included) bit-identical."""
    from modular_rl_amd import _lib
    from tests import vector_ops_np as V
    lib = _lib.load(require_gpu=True)
    d, g, b, tol = V.three_eigen_system(n, n)
    damping = 0.1
    dd = torch.as_tensor(d).cuda()
    cg = _Cg(lib, n)
    cg.init(torch.as_tensor(b).cuda())
    for k in range(3):
        assert int(cg.flag[0].item()) == 0 and int(cg.state[2].item()) == k
        cg.update((dd * cg.p32[:n].double()).float(), damping, tol)
    assert int(cg.flag[0].item()) == 1 and int(cg.state[2].item()) == 3
    before = cg.snapshot()
    for junk in (float("nan"), 1e30):
        cg.update(torch.full((n,), junk, dtype=torch.float32, device="cuda"), damping, tol)
    after = cg.snapshot()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    cg.check_guards()
    xw, its, _, _, _ = _oracle(lambda v: d * v, b, damping, 10, tol, 0.01, g)
    assert its == 3
    np.testing.assert_allclose(cg.x[:n].cpu().numpy(), xw, rtol=1e-6, atol=1e-9 * np.abs(xw).max())
