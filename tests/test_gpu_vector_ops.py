"""Direct GPU checks of the flat-vector layer (csrc/vector_ops.hip, csrc/gae.hip): the slab
reductions, the moments, the standardisation and the grid-stride elementwise kernels, each
at the smallest sizes on either side of every branch of its dispatch (row-group switch at
256 rows, narrow / wide fp64 reduction at 16 columns, unroll trips and tails, one block /
several blocks, the 2048- and 1024-block grid caps) against the references and the
derived bounds of tests/vector_ops_np.py.  tests/test_vector_ops_host.py shows on the CPU
that those bounds reject the subtly wrong version of each operation."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vector_ops_np as V

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


def _api():
    from modular_rl_amd import _lib
    _lib.load(require_gpu=True)
    return _lib.call, _lib.ptr, _lib.stream


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------ slab reductions
def _check_reduce(name, np_dtype, rows, cols, cast32):
    call, ptr, stream = _api()
    rng = np.random.default_rng(1000 * rows + cols)
    slab = V.cancel_rows(rng, rows, cols).astype(np_dtype)
    if np_dtype is np.float64:  # use the width: fp64 noise below the float32 grid
        slab += rng.standard_normal((rows, cols)) * 2.0 ** -30
    want, asum = V.reduce_rows_ref(slab)
    bound = V.sum_bound(rows, asum, want if cast32 else None)
    d = _dev(slab)
    out = torch.full((cols + 64,), SENTINEL, dtype=d.dtype, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    call(name, ptr(d), rows, cols, ptr(out), ptr(one), stream())
    assert np.all(_host(out) == np_dtype(SENTINEL)), "a non-zero skip must leave out untouched"
    call(name, ptr(d), rows, cols, ptr(out), None, stream())
    got = _host(out).copy()
    assert np.all(got[cols:] == np_dtype(SENTINEL)), "written past cols"
    err = np.abs(got[:cols].astype(np.float64) - want)
    worst = int(np.argmax(err / bound))
    print(f"{name} rows={rows} cols={cols}: max err/bound {err[worst] / bound[worst]:.3g}")
    assert np.all(err <= bound), (worst, got[worst], want[worst], bound[worst])
    for skip in (zero, None):  # *skip == 0 is no skip; and two calls agree bit for bit
        out2 = torch.full_like(out, SENTINEL)
        call(name, ptr(d), rows, cols, ptr(out2), ptr(skip), stream())
        np.testing.assert_array_equal(_bits(_host(out2)), _bits(got))


@pytest.mark.parametrize("rows", [1, 3, 4, 31, 32, 33, 255, 256, 257, 383, 384, 1025])
def test_reduce_rows_f32(rows):
    """4 row groups below 256 rows, 16 from 256 up; the 8-way unrolled trip takes 32 or 128
    rows, so 31/32/33 and 383/384 sit on the first trip of each, 255 / 257 on the switch."""
    for cols in (1, 63, 64, 65, 5126):
        _check_reduce("mrl_reduce_rows_f32", np.float32, rows, cols, cast32=True)


@pytest.mark.parametrize("rows", [1, 3, 4, 31, 32, 33, 255, 256, 257, 1000])
def test_reduce_rows_f64(rows):
    """cols <= 16: one 256-thread block per column; above: the 4-group kernel, never run by
    the product (it only passes cols = 4)."""
    for cols in (1, 4, 16, 17, 64, 65):
        _check_reduce("mrl_reduce_rows_f64", np.float64, rows, cols, cast32=False)


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262144, 262149])
def test_moments_and_centered(n, with_b):
    """One block / two blocks, the 1024-block grid cap (262144 fills it, 262149 starts the
    second trip of the stride loop), b given and NULL, and the centred second pass with the
    centre of the first -- against exact sums; the workspace is exactly the advertised size."""
    from modular_rl_amd import _lib
    call, ptr, stream = _api()
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = V.cancel_vec(rng, n)
    b = V.unit_noise(rng, n) if with_b else None
    da, db = _dev(a), (_dev(b) if with_b else None)
    wsb = int(lib.mrl_moments_workspace_bytes(n))
    assert wsb % 8 == 0 and wsb == 16 * min((n + 255) // 256, 1024)
    ws = torch.full((wsb // 8 + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    out0 = torch.full((3 + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    out1 = torch.full((3 + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    call("mrl_moments", ptr(da), ptr(db), n, ptr(out0), ptr(ws), stream())
    m0 = _host(out0).copy()
    call("mrl_moments_centered", ptr(da), ptr(db), n, ptr(out0), ptr(out1), ptr(ws), stream())
    m1 = _host(out1).copy()
    w = _host(ws)
    assert np.all(w[wsb // 8:] == SENTINEL), "written past mrl_moments_workspace_bytes"
    assert not np.any(w[:wsb // 8] == SENTINEL), "a partial was left unwritten"
    for m, shift in ((m0, 0.0), (m1, m0[0] / m0[2])):
        assert m[2] == n and np.all(m[3:] == SENTINEL)
        s1, s2, asum, qsum = V.moments_ref(a, b, shift)
        b1, b2 = V.moments_bounds(n, asum, qsum)
        print(f"moments n={n} shift={shift:.3g}: err {abs(m[0] - s1):.3g} / {b1:.3g}, {abs(m[1] - s2):.3g} / {b2:.3g}")
        assert abs(m[0] - s1) <= b1, (m[0], s1, b1)
        assert abs(m[1] - s2) <= b2, (m[1], s2, b2)


# ------------------------------------------------------------------ standardize
def _standardize(x, two_pass):
    from modular_rl_amd import _lib
    call, ptr, stream = _api()
    n = x.size
    dx = _dev(x)
    ws = torch.zeros(int(_lib.load().mrl_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device="cuda")
    mom = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    call("mrl_moments", ptr(dx), None, n, ptr(mom[0]), ptr(ws), stream())
    if two_pass:
        call("mrl_moments_centered", ptr(dx), None, n, ptr(mom[0]), ptr(mom[1]), ptr(ws), stream())
    call("mrl_standardize", ptr(dx), n, ptr(mom[0]), ptr(mom[1]) if two_pass else None, stream())
    return _host(dx).astype(np.float64)


@pytest.mark.parametrize("n", [2, 257, 524291])
def test_standardize(n):
    """The product's sequence (moments, centred moments, standardize) on mean 1e4 / std 1
    data -- where a single-pass variance is measurably off, test_vector_ops_host.py -- and on
    mean 0 data, within half a float32 ulp plus the fp64 slack of numpy's float64
    (x - x.mean()) / x.std(); cmoments == NULL on the mean 0 data only (the header documents
    the cancellation otherwise); constant input is 0 / 0 = NaN as in numpy."""
    rng = np.random.default_rng(n)
    for mean in (1e4, 0.0):
        x = V.shifted_normal(rng, n, mean)
        err = np.abs(_standardize(x, True) - V.standardize_ref(x))
        bound = V.standardize_bound(x)
        print(f"standardize n={n} mean={mean}: max err/bound {np.max(err / bound):.3g}")
        assert np.all(err <= bound), int(np.argmax(err / bound))
    err = np.abs(_standardize(x, False) - V.standardize_ref(x))
    assert np.all(err <= V.standardize_bound(x, two_pass=False))
    const = np.full(n, 3.25, dtype=np.float32)
    assert np.all(np.isnan(V.standardize_ref(const)))
    for two_pass in (True, False):
        assert np.all(np.isnan(_standardize(const, two_pass)))


# ------------------------------------------------------------------ elementwise kernels
# 256 threads per block, at most 2048 blocks: 524288 elements fill the grid, 524291 start the
# second trip of the stride loop
ELEMENTWISE_N = [1, 255, 256, 257, 524288, 524291]


def _theta_and_step(n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    return a, b


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_axpy_cast_and_linesearch_candidates(n):
    call, ptr, stream = _api()
    a, b = _theta_and_step(n)
    da, db = _dev(a), _dev(b)
    out = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    call("mrl_axpy_cast", ptr(da), ptr(db), ctypes.c_double(0.3), n, ptr(out), stream())
    got = _host(out).copy()
    assert np.all(got[n:] == np.float32(SENTINEL))
    ok = V.matches_one_of(got[:n], V.axpy_cast_refs(a, b, 0.3))
    assert np.all(ok), int(np.argmin(ok))
    for (k0, K) in ((0, 1), (0, 10), (5, 3), (63, 1)):
        cand = torch.full((K * n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        call("mrl_linesearch_candidates", ptr(da), ptr(db), k0, K, n, ptr(cand), stream())
        c = _host(cand).copy()
        assert np.all(c[K * n:] == np.float32(SENTINEL))
        c = c[:K * n].reshape(K, n)
        np.testing.assert_array_equal(_bits(c), _bits(V.linesearch_ref(a, b, k0, K)))
        for k in range(K):  # the same arithmetic as one mrl_axpy_cast per candidate
            call("mrl_axpy_cast", ptr(da), ptr(db), ctypes.c_double(0.5 ** (k0 + k)), n, ptr(out), stream())
            np.testing.assert_array_equal(_bits(_host(out)[:n]), _bits(c[k]))


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_vf_target_and_cast_scale(n):
    call, ptr, stream = _api()
    rng = np.random.default_rng(n + 1)
    ret = (rng.standard_normal(n) * 100).astype(np.float32)
    vp = (rng.standard_normal(n) * 100).astype(np.float32)
    y = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    dret, dvp = _dev(ret), _dev(vp)
    call("mrl_vf_target", ptr(dret), ptr(dvp), ctypes.c_double(0.1), n, ptr(y), stream())
    got = _host(y)
    assert np.all(got[n:] == np.float32(SENTINEL))
    ok = V.matches_one_of(got[:n], V.vf_target_refs(ret, vp, 0.1))
    assert np.all(ok), int(np.argmin(ok))
    for scale in (-1.0, 1.0 / 3.0):
        o = torch.full((n + 64,), SENTINEL, dtype=torch.float64, device="cuda")
        call("mrl_cast_scale_f32_f64", ptr(dret), ctypes.c_double(scale), n, ptr(o), stream())
        got = _host(o)
        assert np.all(got[n:] == SENTINEL)
        np.testing.assert_array_equal(_bits(got[:n]), _bits(V.cast_scale_ref(ret, scale)))


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_adam_two_steps(n):
    """Two consecutive steps, so the second reads back the m / v the first wrote in place; each
    step is compared from the float32 state the device itself held before it."""
    call, ptr, stream = _api()
    rng = np.random.default_rng(n + 2)
    th = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, dtype=np.float32)
    v = np.zeros(n, dtype=np.float32)
    dth, dm, dv = (torch.cat([_dev(t), torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")])
                   for t in (th, m, v))
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 3e-4
    for t in (1, 2):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32)
        a_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        tw, mw, vw, (eth, em, ev) = V.adam_ref(th, g, m, v, a_t, b1, b2, eps)
        dg = _dev(g)
        call("mrl_adam_step", ptr(dth), ptr(dg), ptr(dm), ptr(dv), ctypes.c_double(a_t), ctypes.c_double(b1),
             ctypes.c_double(b2), ctypes.c_double(eps), n, stream())
        th, m, v = (_host(x).copy() for x in (dth, dm, dv))
        for x in (th, m, v):
            assert np.all(x[n:] == np.float32(SENTINEL))
        th, m, v = th[:n], m[:n], v[:n]
        for name, got, want, bound in (("m", m, mw, em), ("v", v, vw, ev), ("theta", th, tw, eth)):
            err = np.abs(got.astype(np.float64) - want)
            print(f"adam n={n} step {t} {name}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert np.all(err <= bound), (name, t, int(np.argmax(err - bound)))
        assert np.any(m != 0) and np.all(v >= 0)


def _gather(src_rows, idx):
    call, ptr, stream = _api()
    n, words = len(idx), src_rows.shape[1]
    dst = torch.full((n * words + 64,), -7, dtype=torch.int32, device="cuda")
    dsrc, didx = _dev(src_rows), _dev(np.asarray(idx, dtype=np.int64))
    call("mrl_gather_rows", ptr(dsrc), ptr(didx), n, 4 * words, ptr(dst), stream())
    got = _host(dst)
    assert np.all(got[n * words:] == -7)
    np.testing.assert_array_equal(got[:n * words].reshape(n, words), V.gather_rows_ref(src_rows, idx))


@pytest.mark.parametrize("row_bytes", [4, 44, 1508])
def test_gather_rows(row_bytes):
    """Rows of 1, 11 and 377 words; a permutation, one index repeated, reversed order; a few
    rows, and the fewest rows whose words pass the grid cap (2048 x 256 threads)."""
    words = row_bytes // 4
    for n in (1, 3, 257, 524288 // words + 3):
        assert n < 300 or (n - 3) * words <= 524288 < n * words
        rng = np.random.default_rng(n)
        src = rng.integers(-2 ** 31, 2 ** 31, (n + 5, words), dtype=np.int64).astype(np.int32)
        for idx in (rng.permutation(n + 5)[:n], np.full(n, n + 4), np.arange(n + 5)[::-1][:n]):
            _gather(src, idx)


def test_gather_rows_source_offsets_past_2_to_31_bytes():
    """Source rows whose byte offset idx * row_bytes needs more than 31 bits (and one just below
    for contrast): a 2.2 GB source left uninitialised except for the gathered rows."""
    call, ptr, stream = _api()
    words, rows = 377, 1_460_000
    assert rows * words * 4 > 2.2e9
    try:
        src = torch.empty(rows * words, dtype=torch.int32, device="cuda").view(rows, words)
    except RuntimeError as e:  # out of memory on a shared device
        pytest.skip(f"cannot allocate the 2.2 GB source: {e}")
    first_past = 2 ** 31 // (4 * words) + 1
    idx = np.array([rows - 1, 0, first_past, first_past - 2, rows - 2, first_past + 12345], dtype=np.int64)
    assert np.sum(idx * 4 * words >= 2 ** 31) == 4
    vals = np.random.default_rng(0).integers(-2 ** 31, 2 ** 31, (len(idx), words), dtype=np.int64).astype(np.int32)
    src[torch.as_tensor(idx).cuda()] = _dev(vals)
    dst = torch.full((len(idx) * words + 64,), -7, dtype=torch.int32, device="cuda")
    didx = _dev(idx)
    call("mrl_gather_rows", ptr(src), ptr(didx), len(idx), 4 * words, ptr(dst), stream())
    got = _host(dst)
    del src
    assert np.all(got[len(idx) * words:] == -7)
    np.testing.assert_array_equal(got[:len(idx) * words].reshape(len(idx), words), vals)
