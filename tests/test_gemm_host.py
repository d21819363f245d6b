"""CPU checks behind tests/test_gpu_gemm.py: the case list of tests/gemm_cases.py reaches every
branch of mrl_gemm the suite had left unreached; its restated dispatch agrees with the library's
host-only queries; the recorded floors are what the restatements measure; the bound meets its
two conditions; and ``within`` accepts the reference and the restatements and rejects every
wrong twin, a poisoned entry, a stray value in a scale-0 entry and a disturbed sentinel."""
import ctypes
import functools

import numpy as np

from tests import gemm_cases as C

MODE_ID = {"f32": 0, "bf16": 1, "split": 2}
EPI_ID = {"store": 0, "tanh": 1, "dtanh": 2, "slab": 3}
X = ctypes.c_void_p(1 << 20)  # a non-NULL pointer nothing dereferences: the queries are host-only

# the small cases: every narrow-tile case, and the wide-tile slabs (130 x 130 outputs)
SMALL = [c for c in C.CASES if c.m <= 257]
WIDE_PROBE = [c for c in C.WIDE if c.mode != "bf16" and (c.at, c.bt) in ((0, 0), (1, 1))]


def _facts(cases):
    out = set()
    for c in cases:
        out |= C.branches(c)
    return out


# ------------------------------------------------------------------ the case list
def test_case_list_reaches_every_branch():
    assert len(C.CASES) == len(set(C.CASES)) <= 420
    for c in C.CASES:
        assert c.m <= 20353 and c.k <= 1287 and c.m * c.n <= 20353 * 70 + 7117 * 257
        assert not (c.ones and c.dual) and (c.epi == "slab" or not c.ones)
        assert C.k_ranges(C._ref_key(c)) == C.k_ranges(c)
    # both tile widths under every orientation and mode
    for o in C.ORIENTS:
        for mode in C.MODES:
            sel = [c for c in C.CASES if (c.at, c.bt) == o and c.mode == mode and c.epi != "slab"]
            assert {C.tile_n(c) for c in sel} == {32, 128}, (o, mode)
            wide = _facts(c for c in sel if C.tile_n(c) == 128)
            # the wide tile: interior and edge blocks, the FULL and the checked staging path,
            # the checked epilogue, remap on and off with a ragged grid
            assert {"interior", "edge", "full_out", "checked_out", "full_load", "remap+ragged", "noremap+ragged",
                    "m_edge1", "n_edge1", "n_edge44", "n_edge70", "full_then_ktail1"} <= wide, (o, mode, wide)
            if not o[0]:
                assert {"full_a_vector", "full_a_scalar", "va", "va_off_by_ld", "va_off_by_alignment"} <= wide, (o, mode)
            if o[1]:
                assert {"full_b_vector", "full_b_scalar", "vb", "vb_off_by_ld"} <= wide, (o, mode)
            if o == (1, 1):
                assert "vb_off_by_alignment" in wide
    # the wide shapes of the issue, either side of the 160-block threshold
    by_shape = {}
    for c in C.WIDE:
        by_shape.setdefault((c.m, c.n, c.k, c.shift != ""), []).append(c)
    assert len(by_shape) == 5 and all(len(v) == 12 for v in by_shape.values())
    want = {(20353, 70, 40, False): (128, (1, 160, 1), True), (20352, 70, 40, False): (32, (3, 159, 1), False),
            (6785, 300, 33, False): (128, (3, 54, 1), False), (7117, 257, 36, False): (128, (3, 56, 1), True),
            (7117, 257, 36, True): (128, (3, 56, 1), True)}
    for key, cs in by_shape.items():
        for c in cs:
            assert (C.tile_n(c), C.grid(c), C.remapped(c)) == want[key], (key, c)
    assert all(C.dims(c).lda == 40 for c in by_shape[(7117, 257, 36, False)] if not c.at)
    # the rotation: every epilogue, single / dual and bias / none under every orientation
    for o in C.ORIENTS:
        sel = [c for c in C.WIDE if (c.at, c.bt) == o]
        assert {c.epi for c in sel} == set(C.EPIS) and {c.dual for c in sel} == {0, 1} == {c.bias for c in sel}
        assert {c.mode for c in sel} == set(C.MODES)
    # the narrow tile: every M, N and K edge, several column tiles, both K tails, the full product twice
    narrow = [c for c in C.NARROW_COVER]
    assert all(C.tile_n(c) == 32 for c in narrow + C.NARROW_PRODUCT)
    assert {c.m for c in narrow} >= {1, 31, 32, 33, 127, 128, 129, 257}
    assert {c.n for c in narrow} >= {1, 31, 32, 33, 64, 65} and {c.k for c in narrow} >= {1, 3, 4, 5, 31, 32, 33, 64, 65, 100}
    assert any(C.grid(c)[0] == 3 for c in narrow)
    assert {"ktail1", "ktail31", "ktail0"} <= _facts(C.CASES)
    for m, n, k, pad in C.PRODUCT_SHAPES:
        sel = {c for c in C.NARROW_PRODUCT if (c.m, c.n, c.k) == (m, n, k)}
        assert len(sel) == 4 * 3 * 3 * 2 * 2
    # whole arms for f32 and split compute outside SLAB: a single product, no bias
    for mode in ("f32", "split"):
        sel = [c for c in C.CASES if c.mode == mode and c.epi != "slab"]
        assert any(not c.dual for c in sel) and any(not c.bias for c in sel)
        assert "full_a_scalar" in _facts(c for c in sel if C.tile_n(c) == 128)
    # slabs: the ones-row alone in its row tile and not, on the wide tile; the clamp, the exact
    # multiple, the short last slab, one slab; TN and NN; each with and without the ones-row
    for mode in C.MODES:
        sl = [c for c in C.SLABS if c.mode == mode]
        wide = [c for c in sl if C.tile_n(c) == 128]
        assert {(c.m, c.ones) for c in wide} == {(129, 1), (129, 0), (130, 1), (130, 0)}
        assert all(C.n_slabs(c) == 41 and C.grid(c) == (2, 2, 41) for c in wide)
        assert {"ones_alone", "ones_shared", "slab_last7", "slabs41"} <= _facts(wide)
        facts = _facts(c for c in sl if C.tile_n(c) == 32)
        assert {"slab_clamped", "slab_exact", "slab_last4", "slab_last8", "slabs1", "slabs2", "slabs3", "slabs4"} <= facts
        for o, mr, n, k, s in C.SLAB_SHAPES:
            assert {c.ones for c in sl if (c.at, c.bt, c.n, c.k, c.splits) == (*o, n, k, s)} == {0, 1}
        assert {(c.at, c.bt) for c in sl} == {C.TN, C.NN}
    for c in C.SLABS:
        d = C.dims(c)
        assert d.ldc > c.n and d.slab_stride > c.m * d.ldc
    assert C.slab_splits(40, 64) == 2 and C.slab_splits(96, 3) == 3 and C.slab_splits(1287, 41) == 41


def test_layouts_poison_what_no_launch_may_consume():
    seen = set()
    for c in SMALL + [c for c in WIDE_PROBE if c.mode == "f32"]:
        L, o = C.layout(c), C.case_operands(c)
        seen.add((c.pad, c.shift))
        for name, rows, ext, ld, off in (("A", L.a_rows, L.a_ext, L.lda, L.offa), ("B", L.b_rows, L.b_ext, L.ldb, L.offb)):
            for buf in (getattr(L, name), getattr(L, name + "2")):
                if buf is None:
                    continue
                body = buf[off:off + rows * ld].reshape(rows, ld)
                assert np.isfinite(body[:, :ext]).all() and np.isnan(body[:, ext:]).all()
                assert np.isnan(buf[:off]).all() and np.isnan(buf[off + rows * ld:]).all() and buf.size == off + (rows + C.GUARD) * ld
        A = L.A[L.offa:L.offa + L.a_rows * L.lda].reshape(L.a_rows, L.lda)[:, :L.a_ext]
        B = L.B[L.offb:L.offb + L.b_rows * L.ldb].reshape(L.b_rows, L.ldb)[:, :L.b_ext]
        assert np.array_equal(A.T if c.at else A, o.A) and np.array_equal(B.T if c.bt else B, o.B)
        if c.shift:
            assert (L.lda if c.shift == "a" else L.ldb) % 4 == 0
        if c.pad != "tight":
            assert L.ldh != L.ldc
        assert np.all(C.embed(c, C.reference(c)[0]).view(np.uint32)[~np.isin(np.arange(L.c_size), C.valid_index(c))] == C.SENT_BITS)
    assert seen >= {("tight", ""), ("pad3", ""), ("padv", ""), ("padv", "a"), ("padv", "b")}
    # exponents over the whole range, mantissas away from 0, H inside (-1, 1)
    o = C.operands(129, 33, 33)
    nz = np.abs(o.A[o.A != 0])
    assert nz.min() >= 2.0 ** -9 and nz.max() < 2.0 ** 8 and np.abs(o.H).max() < 1 and (o.A[1] == 0).all()


# ------------------------------------------------------------------ the library's own dispatch
def test_helpers_agree_with_the_library():
    from modular_rl_amd import _lib as L
    lib = L.load()
    for c in C.CASES:
        d = C.dims(c)
        desc = L.GemmDesc(m=c.m, n=c.n, k=c.k, a=X, lda=d.lda, a_trans=c.at, ones_row=c.ones, b=X, ldb=d.ldb, b_trans=c.bt,
                          epilogue=EPI_ID[c.epi], a2=X if c.dual else None, b2=X if c.dual else None, c=X, ldc=d.ldc,
                          bias=X if c.bias else None, h=X if c.epi == "dtanh" else None, ldh=d.ldh, splits=c.splits,
                          compute=MODE_ID[c.mode], slab_stride=d.slab_stride)
        assert lib.mrl_gemm_tile_n(ctypes.byref(desc)) == C.tile_n(c), c
        if c.epi == "slab":
            assert lib.mrl_gemm_slab_splits(c.k, c.splits) == C.n_slabs(c), c
    for k in (1, 5, 31, 32, 33, 40, 96, 100, 1287, 65536):
        for s in (0, 1, 2, 3, 4, 41, 64, 70000):
            assert lib.mrl_gemm_slab_splits(k, s) == C.slab_splits(k, s), (k, s)
    assert (MODE_ID["f32"], MODE_ID["bf16"], MODE_ID["split"]) == (L.COMPUTE_F32, L.COMPUTE_BF16, L.COMPUTE_SPLIT)
    assert [EPI_ID[e] for e in ("store", "tanh", "dtanh", "slab")] == [L.GEMM_STORE, L.GEMM_TANH, L.GEMM_DTANH, L.GEMM_SLAB]


# ------------------------------------------------------------------ the bound
@functools.lru_cache(maxsize=None)
def _sweep():
    """measure_floors() once for the two tests below: (the floors, the cases whose restatement
    ``within`` refuses)."""
    refused = []
    floors = C.measure_floors(lambda c, r: refused.append(c) if C.within(c, C.embed(c, r)) != [] else None)
    return floors, refused


def test_recorded_floors_are_the_measured_ones():
    """FLOOR is measure_floors() rounded up to two digits (at most 10 % above); the measured
    value may sit up to 10 % above and 30 % below (the window of test_mlp_widths_host.py)."""
    got, _ = _sweep()
    assert set(got) == set(C.FLOOR) == set(C.TOL) == {(m, e) for m in C.MODES for e in C.EPIS + ("slab",)}
    for k, v in got.items():
        assert 0.7 * C.FLOOR[k] <= v <= 1.1 * C.FLOOR[k], (k, v, C.FLOOR[k])
        assert C.TOL[k] == 4.0 * C.FLOOR[k]


def test_bound_meets_its_two_conditions():
    """tol never exceeds the a-priori bound of the case's term count, and equals TOL from 40
    terms on for every mode; it stays below half of the smallest single term a wrong twin
    removes, in units of the entry's scale."""
    capped = 0
    for c in C.CASES:
        t, ap = C.tol(c), C.apriori(c)
        assert t.shape == ap.shape == (C.n_slabs(c), 1, 1) and np.all(t <= ap) and np.all(t <= C.TOL[(c.mode, c.epi)])
        full = C.terms(c) >= 40
        assert np.all(t[full] == C.TOL[(c.mode, c.epi)])
        capped += int(np.any(t < C.TOL[(c.mode, c.epi)]))
    assert 0 < capped < len(C.CASES)
    seen = set()
    for c in SMALL + WIDE_PROBE:
        for name, _, removed in C.twins(c):
            if removed is not None:
                assert float(C.tol(c).max()) < 0.5 * removed, (c, name, removed)
                seen.add(name)
    assert seen == {"last k dropped", "second product missing on the last K tile", "ones-row one k past its slab",
                    "a k counted in two adjacent slabs"}


def test_bound_accepts_the_reference_and_the_restatements():
    """Every case: the restatement (seen during the floor measurement) and the float64
    reference rounded to f32 are within the bound."""
    assert _sweep()[1] == []
    for c in sorted(C.CASES, key=lambda c: (c.m, c.n, c.k, c.ones, c.dual, c.mode)):
        ref, _ = C.reference(c)
        assert ref.shape == (C.n_slabs(c), c.m, c.n)
        assert C.within(c, C.embed(c, ref.astype(np.float32))) == [], c


TWINS = {"last k dropped", "last row of op(A) dropped", "last column of op(B) dropped",
         "second product missing on the last K tile", "bias shifted by one column", "H indexed with ldc",
         "ones-row one k past its slab", "a k counted in two adjacent slabs"}


def test_bound_rejects_the_wrong_twins():
    """Every twin misses the bound in every case it applies to: all the small cases, and the
    NN and TT exact-f32 and split cases of every wide shape."""
    seen = set()
    for c in SMALL + WIDE_PROBE:
        for name, v, _ in C.twins(c):
            assert C.within(c, C.embed(c, v)) != [], (c, name)
            seen.add(name)
    assert seen == TWINS


def test_bound_rejects_a_poisoned_stray_or_out_of_place_entry():
    seen_zero = 0
    for c in (C._case(129, 33, 33, C.ORIENTS[0], "f32", "store", pad="pad3"),
              C._case(129, 33, 33, C.ORIENTS[1], "split", "tanh", dual=1, pad="pad3"),
              C._case(129, 33, 33, C.ORIENTS[3], "bf16", "dtanh", pad="pad3"),
              C._case(34, 33, 100, C.TN, "f32", "slab", ones=1, splits=4, pad="pad3")):
        assert c in C.CASES
        ref, scale = C.reference(c)
        good = C.embed(c, ref.astype(np.float32))
        idx, d = C.valid_index(c), C.dims(c)
        assert C.within(c, good) == []
        for pos in (idx[0, 0, 0], idx[-1, -1, -1]):
            b = good.copy()
            b[pos] = np.nan
            assert C.within(c, b) != []
        # row 1 of op(A) is zero and the case has no bias: scale 0, exact
        assert np.all(scale[:, 1] == 0) and np.all(ref[:, 1] == 0)
        b = good.copy()
        b[idx[-1, 1, c.n - 1]] = 1e-30
        assert C.within(c, b) != []
        seen_zero += 1
        # one float past a row's last column, the first guard row, a slab gap, the last float
        outside = [idx[0, 0, c.n - 1] + 1, idx[-1, -1, -1] + 1, idx[-1, -1, 0] + d.ldc, d.c_size - 1]
        if c.epi == "slab":
            outside.append(idx[0, -1, -1] + C.SLAB_GAP)
        for pos in outside:
            for value in (0.0, np.float32(ref[0, 0, 0])):
                b = good.copy()
                b[pos] = value
                assert [p[0] for p in C.within(c, b)] == ["sentinel"], (c, pos)
        assert C.within(c, good[:-1]) != []
    assert seen_zero == 4
