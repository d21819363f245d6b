"""CPU checks behind tests/test_gpu_mlp_widths.py: the case list of tests/mlp_width_cases.py
reaches every width branch of the fused MLP kernels; its restated dispatch agrees with the
library where the library exports the same fact; the recorded floors are what
measure_floors() gives; the bound rejects subtly wrong twins of the VJP that differ only at
an edge; and a time-feature net without an observation column (n_in == 1 with ep_t) is
refused by every entry point before any launch."""
import ctypes

import numpy as np
import pytest

from oracle import trpo_np as T
from tests import mlp_width_cases as C

X = ctypes.c_void_p(1 << 20)  # a non-NULL pointer nothing dereferences: every call below returns before a launch
E_ARG = -1
HEAD = {"linear": 0, "softmax": 1, "gauss": 2}
PROB, LOSSES, SURRGRAD, VFLOSS, FVP = 0, 1, 2, 3, 4


def _lib():
    from modular_rl_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------ the case list
def test_case_list_reaches_every_width_branch():
    shapes = set(C.SHAPES)
    policy_O = {O for h, O, A, e in shapes if h != "linear" and not e}
    # the input layer's k-steps: every value, and both sides of each step
    assert {C.ks0p(O) for O in policy_O} == {4, 8, 12, 16} == {C.ks0p(O) for O in range(1, C.MAX_IN + 1)}
    for step in (8, 16, 24):
        assert {step, step + 1} <= policy_O and C.ks0p(step + 1) == C.ks0p(step) + 4 == C.ks0p(step - 1) + 4
    assert {1, 2, 3, 7, 15, 31, 32} <= policy_O  # the run-time shape's smallest, odd widths below a step, MAX_IN
    # the cached VJP's dispatch: all three kernels, without ep_t and with it; the fallback at both multiples of 16
    assert {C.vjp_kernel(O, True) for O in policy_O} == {"vjp16", "vjp16_wide", "vjp32"}
    assert {C.vjp_kernel(O, True) for O in C.EPT_NIN} == {"vjp16", "vjp16_wide", "vjp32"}
    assert {O for O in policy_O if C.vjp_kernel(O, True) == "vjp32"} == {16, 32}
    assert [C.vjp_kernel(O, True) for O in C.EPT_NIN] == ["vjp16", "vjp16", "vjp32", "vjp16_wide", "vjp32"]
    assert {C.vjp_kernel(O, False) for O in policy_O} == {"vjp32"}
    # the ones column (the bias gradient) in the last column of a 16-wide tile, narrow and wide
    assert C.vjp_kernel(15, True) == "vjp16" and C.vjp_kernel(31, True) == "vjp16_wide"
    # the head: both k-step counts either side of the step, MAX_OUT, and a gauss head of 16 columns
    for head in ("gauss", "softmax"):
        As = {A for h, O, A, e in shapes if h == head}
        assert {C.ks2(A) for A in As} == {1, 2} and {1, 4, 5, 7, C.MAX_OUT} <= As
        assert C.ks2(4) == 1 and C.ks2(5) == 2
    assert any(C.gh_of(A, h) == 16 for h, O, A, e in shapes)
    assert ("linear", 1, 1, False) in shapes
    # every (O, A) of the grid under both policy heads; the corners and the value nets at every row count
    for O in C.O_EDGES:
        for A in C.A_EDGES:
            assert ("gauss", O, A, False) in shapes and ("softmax", O, A, False) in shapes
    for h, O, A in C.CORNER_SHAPES:
        assert set(C.NS) <= set(C.SHAPES[(h, O, A, False)])
    for O in C.EPT_NIN:
        assert C.SHAPES[("linear", O, 1, True)] == C.NS
    # the corners meet every kernel and both head k-step counts
    assert {C.vjp_kernel(O, True) for O, A in C.CORNERS} == {"vjp16", "vjp16_wide", "vjp32"}
    assert {C.ks2(A) for O, A in C.CORNERS} == {1, 2}
    # no shape of the list is a static one: the one-pass Fisher product must decline all of them
    assert not any(C.fisher_hyb_fits(O, A, h) for h, O, A, e in shapes)
    assert len(C.CASES) == len(set(C.CASES)) <= 400


def test_structured_rows_are_nonzero_only_at_the_edge():
    for key in C.CASES:
        c = C.make_case(*key)
        g = c.G["struct"]
        nz = set(zip(*np.nonzero(g)))
        want = {(c.N - 1, c.A - 1)} | ({(c.N - 1, c.gh - 1)} if c.head == "gauss" else set())
        assert nz == want and g.dtype == np.float32 and c.G["dense"].shape == (c.N, c.gh)
        assert c.X.shape == (c.N, c.O) and c.obs.shape == (c.N, c.O - (c.ept is not None))
        if c.ept is not None:  # the time feature as the kernels form it: f32(ep_t / limit), in column n_obs
            np.testing.assert_array_equal(c.X[:, c.O - 1], (c.ept / C.EPT_LIMIT).astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ the library's own dispatch
def test_helpers_agree_with_the_library():
    L, lib = _lib()
    fixed = 2 * 32 * 64 + 64 + 64 + 2 * 8 * 32 + 16 + 2 * 32 * 64 + 2 * 4 * 64  # mlp_dims but the input layer
    shapes = [(h, O, A) for h, O, A, e in C.SHAPES] + [(h, O, A) for O, A, h in C.STATIC_POLICY]
    for h, O, A in shapes:
        d = L.MlpDesc(O, A, HEAD[h], 64, 2)
        assert lib.mrl_mlp_num_params(ctypes.byref(d)) == T.Spec(O, [64, 64], A, h).P, (h, O, A)
        assert lib.mrl_mlp_image_floats(ctypes.byref(d)) == 2 * 64 * C.ks0p(O) + fixed, (h, O, A)
        assert bool(lib.mrl_mlp_fisher_hyb_fits(ctypes.byref(d))) == C.fisher_hyb_fits(O, A, h), (h, O, A)
        for n in C.NS + [C.GRID_N, C.BF16_N]:
            assert lib.mrl_mlp_partial_rows(ctypes.byref(d), n) == C.grid_rows(n), (h, O, A, n)
            assert lib.mrl_mlp_slab_rows(ctypes.byref(d), n) == C.grid_rows(n), (h, O, A, n)
    assert [C.grid_rows(n) for n in (1, 128, 129, 256, 257)] == [4, 4, 8, 8, 12]
    assert sum(C.fisher_hyb_fits(O, A, h) for h, O, A in shapes) == 2


# ------------------------------------------------------------------ the bound
def test_recorded_floors_are_the_measured_ones():
    """FLOOR is measure_floors() rounded up to two digits (at most 10 % above); the f32
    matmuls' sum order may differ a little between CPUs, so the measured value may also sit
    up to 10 % above and 30 % below."""
    got = C.measure_floors()
    assert set(got) == set(C.FLOOR) == set(C.TOL)
    for k, v in got.items():
        assert 0.7 * C.FLOOR[k] <= v <= 1.1 * C.FLOOR[k], (k, v, C.FLOOR[k])
        assert C.TOL[k] == 4.0 * C.FLOOR[k]


def test_tanh_fast_restatement():
    x = np.concatenate([np.linspace(-12, 12, 4001), [-0.125, 0.125, 0.12499, 0.0, 100.0, -100.0]]).astype(np.float32)
    y = C.tanh_fast_f32(x)
    assert y.dtype == np.float32 and np.all(np.abs(y) <= 1) and y[-1] == -1 and y[-2] == 1 and y[-3] == 0
    assert np.max(np.abs(y - np.tanh(x.astype(np.float64)))) < 2e-7  # the header's abs. err ~1e-7
    small = np.abs(x) < 0.125
    np.testing.assert_allclose(y[small], np.tanh(x[small].astype(np.float64)), rtol=2e-7)


def _twins(c, name):
    """Subtly wrong VJPs of head rows c.G[name], each differing from the reference at one edge."""
    G = c.G[name].astype(np.float64)
    N, O, A = c.N, c.O, c.A
    sl = C.block_slices(O, A, c.head)
    good, _ = C.vjp_reference(c, G)
    g = G.copy()
    g[N - 1] = 0
    yield "row N-1 dropped", C.vjp_reference(c, g)[0]
    g = G.copy()
    g[N - 1] *= 2
    yield "row N-1 counted twice", C.vjp_reference(c, g)[0]
    v = good.copy()
    v[sl["W0"]].reshape(O, 64)[O - 1] = 0
    yield "column O-1 of gW0 zeroed", v
    v = good.copy()
    v[sl["b0"]] = good[sl["W0"]].reshape(O, 64)[O - 1]
    yield "b0 from column O-1", v
    g = G.copy()
    g[:, A - 1] = 0
    v = C.vjp_reference(c, g)[0]
    if c.head == "gauss":
        v[sl["ls"]] = good[sl["ls"]]
    yield "head column A-1 dropped", v
    if c.head == "gauss":
        v = good.copy()
        v[sl["ls"]][A - 1] = 0
        yield "log-std sum over A-1 columns", v


TWIN_CASES = [(h, O, A, n, False) for h, O, A in C.CORNER_SHAPES for n in (1, 33, 129)] + \
             [("linear", O, 1, n, True) for O in C.EPT_NIN for n in (1, 33, 129)]


def test_bound_rejects_the_wrong_twins():
    """Every twin misses TOL in every corner case it applies to, on the dense rows and on the
    structured ones; the float64 reference rounded to f32, and the f32 restatement, pass."""
    seen = set()
    for key in TWIN_CASES:
        c, ref = C.make_case(*key), C.reference(*key)
        for name in ("dense", "struct"):
            out = "vjp." + name
            assert C.within(c, out, ref[out][0].astype(np.float32), ref) == []
            assert C.within(c, out, C.f32_outputs(c)[out], ref) == []
            for twin, v in _twins(c, name):
                assert C.within(c, out, v, ref) != [], (key, name, twin)
                seen.add(twin)
    assert len(seen) == 6


def test_bound_rejects_a_poisoned_or_stray_entry():
    key = ("gauss", 15, 4, 33, False)
    c, ref = C.make_case(*key), C.reference(*key)
    good = ref["vjp.struct"][0].astype(np.float32)
    for i in (0, c.P - 1):
        v = good.copy()
        v[i] = np.nan
        assert C.within(c, "vjp.struct", v, ref) != []
    # the structured rows leave b2 and log-std entries of scale 0: those must be exact
    sl = C.block_slices(c.O, c.A, c.head)
    assert ref["vjp.struct"][1][sl["b2"]][0] == 0 and ref["vjp.struct"][1][sl["ls"]][0] == 0
    v = good.copy()
    v[sl["ls"]][0] = 1e-30
    assert C.within(c, "vjp.struct", v, ref) != []


# ------------------------------------------------------------------ n_obs == 0
def _io(L, n, ep_t=X):
    return L.RowsIO(X, ep_t, 200.0, n, 1.0, X, X, X, X, X, X, X, 0.0, 0.0, 0.0, 0, 0, None, None)


@pytest.mark.parametrize("n", [8, 0])
def test_time_feature_net_without_observations_is_refused(n):
    """n_in == 1 with ep_t leaves n_obs == 0, and the kernels' clamped column loads would read
    column -1: MRL_E_ARG from every entry point that takes ep_t, before the row count is looked
    at and before any launch (the pointers here are never dereferenced)."""
    L, lib = _lib()
    for head in ("linear", "gauss"):
        d = ctypes.byref(L.MlpDesc(1, 1, HEAD[head], 64, 2))
        io = ctypes.byref(_io(L, n))
        calls = {
            "mrl_mlp_vjp": lambda: lib.mrl_mlp_vjp(d, X, X, X, 200.0, X, n, X, None, None, None),
            "mrl_mlp_vjp cached": lambda: lib.mrl_mlp_vjp(d, X, X, X, 200.0, X, n, X, X, None, None),
            "mrl_mlp_vjp_bf16": lambda: lib.mrl_mlp_vjp_bf16(d, X, X, X, 200.0, X, n, X, None, None, None),
            "mrl_linesearch_eval": lambda: lib.mrl_linesearch_eval(d, 0, X, X, 0, 1, io, X, X, 1 << 30, X, 1 << 30, X, None),
        }
        for epi in (PROB, LOSSES, SURRGRAD, VFLOSS, FVP):
            calls[f"mrl_mlp_rows {epi}"] = lambda e=epi: lib.mrl_mlp_rows(d, e, X, X, X, X, io, None, None)
            calls[f"mrl_mlp_rows_bf16 {epi}"] = lambda e=epi: lib.mrl_mlp_rows_bf16(d, e, X, X, X, X, io, None, None)
            if epi != FVP:
                calls[f"mrl_mlp_rows_split {epi}"] = lambda e=epi: lib.mrl_mlp_rows_split(d, e, X, X, io, None, None)
        for name, f in calls.items():
            assert f() == E_ARG, (head, name)
            msg = lib.mrl_last_error()
            assert b"n_in >= 2" in msg and b"n_obs = 0" in msg, (head, name, msg)
        # the Fisher-product and one-launch entry points take no time feature at all
        assert lib.mrl_mlp_fvp_split(d, X, X, X, X, io, None, None) == E_ARG
        assert lib.mrl_mlp_fisher_hyb(d, X, X, X, X, X, io, X, None, None) == E_ARG
        assert lib.mrl_mlp_grad_hyb(d, X, X, X, io, X, None, None) == E_ARG


def test_time_feature_check_leaves_the_valid_forms_alone():
    """n_in == 1 without ep_t, and n_in == 2 with it, pass the check: with no rows the calls
    return MRL_OK (still before any launch)."""
    L, lib = _lib()
    for n_in, ep_t in ((1, None), (2, X)):
        d = ctypes.byref(L.MlpDesc(n_in, 1, HEAD["linear"], 64, 2))
        io = ctypes.byref(_io(L, 0, ep_t))
        assert lib.mrl_mlp_rows(d, PROB, X, X, X, X, io, None, None) == 0
        assert lib.mrl_mlp_rows_split(d, PROB, X, X, io, None, None) == 0
        assert lib.mrl_mlp_rows_bf16(d, PROB, X, X, X, X, io, None, None) == 0
        assert lib.mrl_mlp_vjp(d, X, X, ep_t, 200.0, X, 0, X, None, None, None) == 0
        assert lib.mrl_mlp_vjp_bf16(d, X, X, ep_t, 200.0, X, 0, X, None, None, None) == 0
