"""CPU separation checks for tests/test_gpu_vector_ops.py and the CG early-exit cases of
tests/test_gpu_cg.py: on the inputs those GPU tests use, the bound of tests/vector_ops_np.py
rejects the subtly wrong twin of each operation (float32 accumulation, the single-pass
variance, a wrong CG iteration count) and accepts a correct fp64 restatement summed in
another order.  Plus the argument checks of the flat-vector entry points that return
before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import fma as F
from tests import vector_ops_np as V
from tests.test_gpu_cg import _oracle


# ------------------------------------------------------------------ row sums
@pytest.mark.parametrize("rows", [31, 32, 33, 255, 256, 257, 383, 384, 1000, 1025])
@pytest.mark.parametrize("cast32", [True, False])
def test_row_sum_bound_separates_float32_accumulation(rows, cast32):
    """At every row count of the GPU tests with enough rows to accumulate (from 31 up; with
    1 .. 4 rows float32 sums are exact or nearly so and nothing can tell them apart), fp64
    sums in two other orders stay inside the bound and float32 accumulation misses it in
    most columns, by more than three orders of magnitude in the median column."""
    x = V.cancel_rows(np.random.default_rng(rows), rows, 65)
    s, _ = V.reduce_rows_ref(x)
    bound = V.reduce_rows_bound(x, cast32)
    cast = (lambda v: np.float32(v).astype(np.float64)) if cast32 else (lambda v: v)
    for right in (x.astype(np.float64).sum(axis=0), V.sum_rows_pairwise(x)):
        assert np.all(np.abs(cast(right) - s) <= bound)
    wrong = np.abs(V.sum_rows_f32(x) - s) / bound
    assert np.mean(wrong > 1.0) > 0.9 and np.median(wrong) > 1e3, (np.mean(wrong > 1.0), np.median(wrong))


@pytest.mark.parametrize("n", [255, 256, 257, 262144, 262149])
@pytest.mark.parametrize("with_b", [True, False])
def test_moment_bounds_separate_float32_accumulation(n, with_b):
    """mrl_moments and mrl_moments_centered on the GPU test's data: numpy's fp64 sums are
    inside both bounds, float32 differences / accumulators outside both, for the plain and
    for the centred pass (centre = the first pass's mean)."""
    rng = np.random.default_rng(n)
    a = V.cancel_vec(rng, n)
    b = V.unit_noise(rng, n) if with_b else None
    for shift in (0.0, V.moments_f64(a, b)[0] / n):
        s1, s2, asum, qsum = V.moments_ref(a, b, shift)
        b1, b2 = V.moments_bounds(n, asum, qsum)
        r1, r2 = V.moments_f64(a, b, shift)
        assert abs(r1 - s1) <= b1 and abs(r2 - s2) <= b2
        w1, w2 = V.moments_f32(a, b, shift)
        assert abs(w1 - s1) > 3 * b1 and abs(w2 - s2) > 3 * b2, (abs(w1 - s1) / b1, abs(w2 - s2) / b2)


def test_moments_reference_is_exact():
    """moments_ref against rational arithmetic on a small case."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = V.cancel_vec(rng, 37), V.unit_noise(rng, 37)
    shift = 0.1234567891234567
    d = [Fraction(float(x)) - Fraction(float(y)) - Fraction(shift) for x, y in zip(a, b)]
    s1, s2, _, _ = V.moments_ref(a, b, shift)
    assert s1 == float(sum(d)) and s2 == float(sum(v * v for v in d))


# ------------------------------------------------------------------ standardize
@pytest.mark.parametrize("n", [2, 257, 524291])
def test_standardize_bound_admits_two_pass_forms(n):
    """Mean 1e4 / std 1 and mean 0 data of the GPU test: the two-pass form, with numpy's sums
    and with exact ones, cast to float32 as the device casts, meets the bound; so does the
    single-pass form on the mean-0 data under the single-pass bound."""
    rng = np.random.default_rng(n)
    fs = lambda v: math.fsum(v)  # noqa: E731
    for mean in (1e4, 0.0):
        x = V.shifted_normal(rng, n, mean)
        z, bound = V.standardize_ref(x), V.standardize_bound(x)
        for sum_fn in (np.sum, fs):
            out = np.float32(V.standardize_two_pass(x, sum_fn)).astype(np.float64)
            assert np.all(np.abs(out - z) <= bound)
    out = np.float32(V.standardize_single_pass(x)).astype(np.float64)
    assert np.all(np.abs(out - z) <= V.standardize_bound(x, two_pass=False))


def test_standardize_bound_rejects_single_pass_variance():
    """At n = 524291, mean 1e4, std 1 the single-pass E[x^2] - mean^2 from fp64 sums is off by
    ~1e-8 relative (sum x^2 ~ 5e13 carries ~1e-2 of rounding, mean^2 ~ 1e8 another 1e-8): a
    twelfth of float32 epsilon, two orders above the fp64 slack of the bound.  It misses the
    half-ulp bound in thousands of elements -- every cast that lands on the neighbouring
    float32 -- where the two-pass form misses none.  (At n = 2 and 257 the fp64 sums are
    still accurate to ~1e-11 and the two forms cannot be told apart in float32.)"""
    x = V.shifted_normal(np.random.default_rng(524291), 524291, 1e4)
    z, bound = V.standardize_ref(x), V.standardize_bound(x)
    single = V.standardize_single_pass(x)
    assert np.median(np.abs(single - z) / np.abs(z)) > 30 * np.median(V.standardize_slack(x) / np.abs(z))
    miss = np.abs(np.float32(single).astype(np.float64) - z) > bound
    assert miss.sum() > 1000, miss.sum()
    two = np.float32(V.standardize_two_pass(x)).astype(np.float64)
    assert not np.any(np.abs(two - z) > bound)


def test_standardize_constant_input_is_nan_in_the_reference():
    assert np.all(np.isnan(V.standardize_ref(np.full(7, 3.25, dtype=np.float32))))


# ------------------------------------------------------------------ elementwise
def test_power_of_two_axpy_is_the_same_fused_and_unfused():
    """The bit-equality reference of mrl_linesearch_candidates assumes a + 2^-j b rounds the
    same with and without contraction: checked with the correctly rounded fma for every
    stepfrac exponent 0 .. 63 on the GPU test's inputs."""
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4096).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 3, 4096)
    for j in range(64):
        f = 2.0 ** -j
        np.testing.assert_array_equal(F.fma(np.full_like(b, f), b, a), a + f * b)
    # and a general frac is not: the two admissible references of mrl_axpy_cast differ in fp64
    assert np.any(F.fma(np.full_like(b, 0.3), b, a) != a + 0.3 * b)


def test_one_of_references_rejects_a_float32_evaluation():
    """mrl_axpy_cast / mrl_vf_target: the float32 evaluation of the same formula (the wrong
    twin) is not among the admissible casts of the fp64 ones."""
    rng = np.random.default_rng(4)
    n = 4096
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n)
    wrong = a + np.float32(0.3) * b.astype(np.float32)
    ok = V.matches_one_of(wrong, V.axpy_cast_refs(a, b, 0.3))
    assert ok.mean() < 0.9
    assert np.all(V.matches_one_of(np.float32(a.astype(np.float64) + 0.3 * b), V.axpy_cast_refs(a, b, 0.3)))
    ret, vp = rng.standard_normal(n).astype(np.float32) * 100, rng.standard_normal(n).astype(np.float32) * 100
    wrong = ret * np.float32(0.1) + vp * np.float32(0.9)
    assert V.matches_one_of(wrong, V.vf_target_refs(ret, vp, 0.1)).mean() < 0.9


def test_adam_bound_admits_float32_and_rejects_a_misplaced_eps():
    """The float32 evaluation of the header's formula (what the kernel does, unfused) is inside
    the bounds; sqrt(v + eps) in place of sqrt(v) + eps -- the classic slip -- is outside."""
    rng = np.random.default_rng(6)
    n = 4096
    th, g = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-3).astype(np.float32)
    m, v = (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.random(n) * 1e-6).astype(np.float32)
    a_t, b1, b2, eps = 3e-4, 0.9, 0.999, 1e-8
    tw, mw, vw, (dth, dm, dv) = V.adam_ref(th, g, m, v, a_t, b1, b2, eps)
    f = np.float32
    mi = f(b1) * m + (f(1) - f(b1)) * g
    vi = f(b2) * v + (f(1) - f(b2)) * (g * g)
    ti = th - f(a_t) * mi / (np.sqrt(vi) + f(eps))
    assert mi.dtype == vi.dtype == ti.dtype == np.float32
    assert np.all(np.abs(mi - mw) <= dm) and np.all(np.abs(vi - vw) <= dv) and np.all(np.abs(ti - tw) <= dth)
    v0 = np.zeros(n, dtype=np.float32)  # first step: v' = (1 - b2) g^2, where eps matters most
    tw, mw, vw, (dth, _, _) = V.adam_ref(th, g, m, v0, a_t, b1, b2, 1e-4)
    wrong = th.astype(np.float64) - float(f(a_t)) * mw / np.sqrt(vw + float(f(1e-4)))
    assert np.mean(np.abs(wrong - tw) > dth) > 0.9


# ------------------------------------------------------------------ CG early exit
@pytest.mark.parametrize("n", [1025, 8193, 65537])
def test_three_eigenvalue_cg_stops_after_exactly_three(n):
    """The oracle's rdotr on the three-eigenvalue system is above tol after two iterations
    and below it after three, by four orders of magnitude either side: the iteration count
    is 3 at 1e4 tol and at 1e-4 tol as well, so the device's count cannot hinge on the
    order of its sums."""
    d, g, b, tol = V.three_eigen_system(n, n)
    A = lambda v: d * v  # noqa: E731
    for t in (tol * 1e-4, tol, tol * 1e4):
        assert _oracle(A, b, 0.1, 10, t, 0.01, g)[1] == 3
    assert len(np.unique(d)) == 3
    w = [float(b[d == e].dot(b[d == e])) for e in np.unique(d)]
    assert max(w) < 1.5 * min(w)  # comparable weight on each eigenspace


# ------------------------------------------------------------------ argument checks
X = ctypes.c_void_p(1 << 20)  # a non-NULL pointer nothing dereferences: every call below returns before a launch


def _lib():
    from modular_rl_amd import _lib as L
    return L, L.load()


def _each_null(fn, args, optional=()):
    """Every pointer argument NULL in turn (the others non-NULL): MRL_E_ARG, before any launch."""
    for i, a in enumerate(args):
        if a is X and i not in optional:
            rc = fn(*[None if j == i else b for j, b in enumerate(args)])
            assert rc == -1, (fn.__name__, i, rc)


def test_null_pointers_are_refused():
    L, lib = _lib()
    z = ctypes.c_double(0.5)
    _each_null(lib.mrl_cg_init, [X, 8, X, X, X, X, X, X, X, None], optional=(6,))
    _each_null(lib.mrl_cg_update, [X, z, z, 8, X, X, X, X, X, X, X, None], optional=(8,))
    _each_null(lib.mrl_trpo_step, [X, X, X, z, z, 8, X, X, None])
    _each_null(lib.mrl_trpo_step_ax, [X, X, X, z, 8, X, X, None])
    _each_null(lib.mrl_axpy_cast, [X, X, z, 8, X, None])
    _each_null(lib.mrl_linesearch_candidates, [X, X, 0, 1, 8, X, None])
    _each_null(lib.mrl_adam_step, [X, X, X, X, z, z, z, z, 8, None])
    _each_null(lib.mrl_gather_rows, [X, X, 8, 4, X, None])
    _each_null(lib.mrl_cast_scale_f32_f64, [X, z, 8, X, None])
    _each_null(lib.mrl_vf_target, [X, X, z, 8, X, None])
    _each_null(lib.mrl_standardize, [X, 8, X, X, None], optional=(3,))
    _each_null(lib.mrl_moments, [X, X, 8, X, X, None], optional=(1,))
    _each_null(lib.mrl_moments_centered, [X, X, 8, X, X, X, None], optional=(1, 3))
    _each_null(lib.mrl_reduce_rows_f32, [X, 8, 8, X, None, None])
    _each_null(lib.mrl_reduce_rows_f64, [X, 8, 8, X, None, None])
    assert b"null" in lib.mrl_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="launches on fake pointers: only where no device can run them")
def test_null_ax_is_not_an_argument_error():
    """ax == NULL passes the argument checks of init and update (what follows is the launch,
    which fails for want of a device here; tests/test_gpu_cg.py runs it on one)."""
    L, lib = _lib()
    z = ctypes.c_double(0.5)
    assert lib.mrl_cg_init(X, 8, X, X, X, X, None, X, X, None) != -1
    assert lib.mrl_cg_update(X, z, z, 8, X, X, X, X, None, X, X, None) != -1


def test_size_arguments_are_checked_before_any_launch():
    L, lib = _lib()
    for (k0, K) in ((0, 0), (0, -1), (-1, 1), (0, 65), (63, 2), (64, 1)):
        assert lib.mrl_linesearch_candidates(X, X, k0, K, 8, X, None) == -1, (k0, K)
        assert b"k0" in lib.mrl_last_error()
    for rb in (0, -4, 2, 6, 1507):
        assert lib.mrl_gather_rows(X, X, 8, rb, X, None) == -1, rb
    for n in (0, -1):
        assert lib.mrl_gather_rows(X, X, n, 44, X, None) == 0
        assert lib.mrl_moments(X, None, n, X, X, None) == -1
        assert lib.mrl_moments_centered(X, X, n, X, X, X, None) == -1
        assert lib.mrl_standardize(X, n, X, X, None) == 0
        assert lib.mrl_vf_target(X, X, ctypes.c_double(0.1), n, X, None) == 0
    for cols in (0, -1):
        assert lib.mrl_reduce_rows_f32(X, 8, cols, X, None, None) == 0
        assert lib.mrl_reduce_rows_f64(X, 8, cols, X, None, None) == 0
    assert lib.mrl_cg_state_doubles(65536) == 4
    assert lib.mrl_cg_state_doubles(65537) == 8 + 2 * 256
    assert lib.mrl_moments_workspace_bytes(1) == 16
    assert lib.mrl_moments_workspace_bytes(262144) == 1024 * 16 == lib.mrl_moments_workspace_bytes(262149)
    assert lib.mrl_moments_workspace_bytes(262144 - 256) == 1023 * 16
