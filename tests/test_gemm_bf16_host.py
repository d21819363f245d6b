"""The CPU side of the bf16-operand GEMM tests (tests/gemm_bf16_cases.py): the case list reaches
every branch named per kernel, the restated route agrees with hand-worked descriptors and with
the library's own query where no device is needed, the recorded floors reproduce, the float32
restatement passes ``within`` and every wrong twin fails it.  Nothing here runs on a device."""
import ctypes

import numpy as np
import pytest

from tests import gemm_bf16_cases as C

# what the case list must reach, per routed kernel family (``branches``)
REQUIRED = {
    "tiled": {"tile128", "tile32", "bk64", "bk32", "remap", "noremap", "single", "dual", "bias", "nobias", "store", "tanh",
              "dtanh", "f32out", "bf16out", "vec", "scalar", "vec_partial_run", "ldh_eq_ldc", "ldh_ne_ldc", "m_edge",
              "m_even", "n_edge", "n_even", "k0", "ktail", "kfull", "k_chunk_partial", "dual_ktail", "blocks>1", "intended",
              "declined_to_tiled"},
    "small": {"quarters1", "quarters2", "quarters3", "quarters4", "partial_quarter", "chunk_past_k", "rows_clamped",
              "cols_clamped", "block1", "blocks>1", "store", "tanh", "bias", "nobias", "f32out", "bf16out", "vec", "scalar",
              "vec_partial_run", "m_even", "n_even", "intended"},
    "stream": {"plan384", "plan512", "slices1", "slices2", "slices3", "slices4", "partial_slice", "last_step_masked",
               "last_step_read", "k_steps_of_zeros", "two_row_tiles", "one_row_tile", "idle_groups", "store", "tanh",
               "dtanh", "bias", "nobias", "f32out", "bf16out", "vec", "scalar", "ldh_eq_ldc", "ldh_ne_ldc", "lda_ld8",
               "lda_padded", "m_edge", "m_even", "n_edge", "n_even", "intended"},
    "big": {"single", "dual", "ntn1", "ntn2", "stages4", "stages8", "interior_dma", "edge_dma_only", "ktail",
            "k_chunk_partial", "two_row_tiles", "one_row_tile", "idle_blocks", "store", "tanh", "dtanh", "bias", "nobias",
            "f32out", "bf16out", "vec", "scalar", "vec_partial_run", "ldh_eq_ldc", "ldh_ne_ldc", "m_edge", "m_even",
            "n_edge", "n_even", "intended"},
    "tn_tiled": {"tile32", "tile128", "ones", "noones", "ones_alone", "ones_shared", "chunk_straddles_m_real",
                 "chunk_straddles_n", "k0", "slab_clamped", "slab_exact", "slab_ragged", "stage_ragged", "slabs1",
                 "slabs41", "ldc_tight", "ldc_padded", "intended"},
    "tn_big": {"ones", "noones", "rounds1", "rounds2", "slabs1", "slabs7", "slabs8", "slabs9", "stages<4", "stages>=4",
               "slab_exact", "slab_ragged", "stage_ragged", "ntm1", "ntm2", "ntn1", "ntn2", "ntn3", "m_edge", "n_edge",
               "ones_second_half_cut", "ldc_tight", "ldc_padded", "intended"},
}


def test_case_list_reaches_every_branch():
    seen = set()
    for c in C.CASES:
        seen |= C.branches(c)
    want = {f + ":" + b for f, bs in REQUIRED.items() for b in bs}
    assert want <= seen, sorted(want - seen)
    # the streaming cases the launcher must refuse: rows shorter than the plan's last k-step
    refused = [c for c in C.STREAM if C.family(C.route(c)) == "tiled"]
    assert {c.k for c in refused} == {257, 264, 300, 360, 385, 392, 440}  # ld8(367) = 368 and ld8(495) = 496 reach it
    assert all(C.dims(c).lda < (384 if c.k <= 384 else 512) - 16 for c in refused)
    # every other case runs the kernel it was written for
    assert all(C.family(C.route(c)) == c.kernel for c in C.CASES if c not in refused)
    # K = 0 only where the K loop is guarded
    assert {c.kernel for c in C.CASES if c.k == 0} == {"tiled", "tn_tiled"}
    assert sorted(c for g in C.GROUPS.values() for c in g) == sorted(C.CASES) and len(set(C.CASES)) == len(C.CASES)


def _nn(m, n, k, dual=0, epi="store", lds=0, ldx=0):
    return C.Case("nn", "", m, n, k, dual, 0, epi, 0, 0, 0, "tight", ldx, lds)


def _tn(mr, n, ones=1, lds=0):
    return C.Case("tn", "", mr + ones, n, 4096, 0, 0, "slab", 0, ones, 64, "tight", 0, lds)


D = C.DEFAULT_ENV
# (descriptor, CU count, thresholds, route), worked by hand from csrc/gemm_bf16*.hip
ROUTE_TABLE = [
    (_nn(70001, 512, 512), 256, D, "big"),                   # 16 stages, 2 column tiles of 32 blocks per XCD
    (_nn(70001, 512, 512), 0, D, "tiled128_bk64"),           # no CU count: neither persistent kernel
    (_nn(70001, 512, 512), 300, D, "tiled128_bk64"),         # not a multiple of 8: the same
    (_nn(70001, 512, 512), 304, D, "big"),                   # 38 blocks per XCD, whole groups of 2
    (_nn(70001, 10000, 512), 304, D, "tiled128_bk64"),       # 40 column tiles, 79 slices: more than 38 per XCD
    (_nn(70001, 10000, 512), 256, D, "tiled128_bk64"),
    (_nn(70001, 512, 512, dual=1), 256, D, "big"),
    (_nn(70001, 512, 48), 256, D, "tiled128_bk64"),          # 2 stages: no multiple of 4; K <= 256: no streaming
    (_nn(70001, 512, 48, dual=1), 256, D, "big"),            # 4 stages
    (_nn(70001, 512, 0), 256, D, "tiled128_bk64"),           # no stage at all: the big kernel declines
    (_nn(70001, 512, 0, dual=1), 256, D, "tiled128_bk64"),
    (_nn(70001, 17, 512), 256, D, "tiled32_bk64"),
    (_nn(40000, 512, 376), 256, D, "stream384"),             # lda = 376 >= 368
    (_nn(40000, 512, 376), 0, D, "tiled128_bk64"),
    (_nn(40000, 512, 512), 256, D, "stream512"),
    (_nn(40000, 512, 300), 256, D, "tiled128_bk64"),         # lda = 304 < 368: the over-read shape
    (_nn(40000, 512, 300, ldx=64), 256, D, "stream384"),     # lda = 368
    (_nn(40000, 512, 495), 256, D, "stream512"),             # ld8(495) = 496 = 512 - 16: the shortest row that streams
    (_nn(40000, 512, 488), 256, D, "tiled128_bk64"),         # lda = 488 < 496
    (_nn(40000, 512, 376, dual=1), 256, D, "tiled128_bk64"),
    (_nn(40000, 4200, 376), 256, D, "tiled128_bk64"),        # 33 slices > 32 per XCD
    (_nn(1024, 512, 376), 256, D, "small"),
    (_nn(1024, 512, 376, epi="dtanh"), 256, D, "tiled128_bk64"),
    (_nn(1024, 512, 513), 256, D, "tiled128_bk64"),
    (_nn(70001, 512, 512, lds=81920), 256, D, "tiled128_bk64"),
    (_nn(70001, 512, 512, lds=65536), 256, D, "tiled128_bk32"),
    (_nn(70001, 17, 512, lds=65536), 256, D, "tiled32_bk64"),
    (_nn(70001, 17, 512, lds=40960), 256, D, "tiled32_bk32"),
    (_nn(300, 300, 128), 256, dict(C.TILED_ENV, MRL_GEMM_BIG_MIN_M=1), "big"),
    (_nn(300, 300, 0), 256, dict(C.TILED_ENV, MRL_GEMM_BIG_MIN_M=1), "tiled128_bk64"),
    (_nn(0, 300, 128), 256, D, "none"),
    (_tn(512, 512), 256, D, "tn_big"),
    (_tn(376, 512), 0, D, "tn_big"),                         # the TN kernels do not size by CUs
    (_tn(512, 512), 256, dict(D, MRL_GEMM_TN_BIG=0), "tn_tiled128"),
    (_tn(512, 512, lds=65536), 256, D, "tn_tiled128"),
    (_tn(300, 512), 256, D, "tn_tiled128"),                  # m_real not a multiple of 8
    (_tn(248, 512), 256, D, "tn_tiled128"),
    (_tn(512, 17, ones=0), 256, D, "tn_tiled32"),
]


@pytest.mark.parametrize("i", range(len(ROUTE_TABLE)))
def test_restated_route_agrees_with_hand_worked_table(i):
    c, ncu, env, want = ROUTE_TABLE[i]
    assert C.route(c, ncu, env) == want


def _desc(c):
    """The descriptor of a case with dummy non-null addresses: the route queries read no operand."""
    from modular_rl_amd import _lib
    d = C.dims(c)
    if c.kind == "nn":
        return _lib.GemmBf16Desc(m=c.m, n=c.n, k=c.k, a=0x1000, lda=d.lda, bt=0x1000, ldb=d.ldb, a2=0x1000 if c.dual else None,
                                 bt2=0x1000 if c.dual else None, c=0x1000, ldc=d.ldc, c_bf16=c.bf,
                                 epilogue=C.EPIS.index(c.epi), ldh=d.ldh, lds_limit=c.lds)
    return _lib.GemmBf16TnDesc(m=c.m, n=c.n, k=c.k, a=0x1000, lda=d.lda, b=0x1000, ldb=d.ldb, ones_row=c.ones,
                               splits=c.splits, slab=0x1000, slab_stride=d.slab_stride, ldc=d.ldc, lds_limit=c.lds)


def test_library_route_query_without_a_device(monkeypatch):
    """Where no device is visible cu_count() is 0 and the library's query must equal the restated
    route at ncu = 0, for every case under its own thresholds and for the hand-worked table."""
    import torch

    from modular_rl_amd import _lib
    lib = _lib.load()
    ncu = 0
    if torch.cuda.is_available():
        n = ctypes.c_int32(0)
        assert lib.mrl_device_cu_count(ctypes.byref(n)) == 0
        ncu = n.value
    assert lib.mrl_gemm_bf16_route(None) == -1 and lib.mrl_gemm_bf16_tn_route(None) == -1
    for c, env in [(c, C.env_of(c)) for c in C.CASES] + [(c, env) for c, _, env, _ in ROUTE_TABLE]:
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        q = lib.mrl_gemm_bf16_route if c.kind == "nn" else lib.mrl_gemm_bf16_tn_route
        assert q(ctypes.byref(_desc(c))) == C.ROUTE_ID[C.route(c, ncu, env)], C.case_id(c)


def test_floors_restatement_and_layout():
    """measure_floors() reproduces FLOOR to its rounding; on the way every restatement, embedded
    as a launch would leave it, is ``within``; embed / valid_index round-trip and the guards of
    the operand images are where ``layout`` says."""
    def visit(c, r):
        buf = C.embed(c, r)
        assert C.within(c, buf) == [], C.case_id(c)
        idx = C.valid_index(c)
        assert idx.shape == r.shape and np.array_equal(buf[idx], C.to_bits(c, r))
        sent = C.SENT16 if c.bf else C.SENT_BITS
        assert np.count_nonzero(buf != sent) <= r.size and buf.size - r.size == np.count_nonzero(
            np.delete(buf, idx.reshape(-1)) == sent)

    worst = C.measure_floors(visit)
    assert set(worst) == set(C.FLOOR)
    for key, v in worst.items():
        assert C.round_up2(v) == C.FLOOR[key], (key, v)
    assert all(C.tol(c).max() <= C.apriori(c).max() for c in C.CASES)


@pytest.mark.parametrize("c", [C.TILED[3], C.TILED[20], C.STREAM[2], C.BIG[9], C.TN_TILED[5], C.TN_BIG[4]], ids=C.case_id)
def test_layout_poisons_what_the_contract_does_not_promise(c):
    L = C.layout(c)
    G = C.GUARD
    for name, rows, ext, ld in (("A", c.m if c.kind == "nn" else c.k, c.k if c.kind == "nn" else L.mr, L.lda),
                                ("B", c.n if c.kind == "nn" else c.k, c.k if c.kind == "nn" else c.n, L.ldb)):
        img = getattr(L, name).reshape(rows + 2 * G, ld)
        assert np.all(img[:G] == C.NAN16) and np.all(img[G + rows:] == C.NAN16)
        assert np.all(img[G:G + rows, ext:] == (0 if c.kind == "nn" else C.NAN16))
        assert not np.isnan(C.from_bits16(img[G:G + rows, :ext])).any()
    if L.H is not None:
        img = L.H.reshape(c.m + 2 * G, L.ldh)
        assert np.all(img[:G] == C.NAN16) and np.all(img[G + c.m:] == C.NAN16) and np.all(img[G:G + c.m, c.n:] == C.NAN16)
    if L.bias is not None:
        assert np.isnan(L.bias[:C.BIAS_LEAD]).all() and np.isnan(L.bias[C.BIAS_LEAD + c.n:]).all()
    assert L.a_off % 8 == 0 and L.b_off % 8 == 0 and np.all(L.C == (C.SENT16 if c.bf else C.SENT_BITS))


TWIN_NAMES = {"last k dropped", "last row of A dropped", "last column of B dropped",
              "second product missing on the last K stage", "bias shifted by one column", "H indexed with ldc",
              "a k counted in two adjacent slabs", "ones-row one k past its slab", "ones-row column j written at j + 16",
              "a NaN in the last valid row"}


def test_every_twin_is_rejected():
    """Every wrong twin of every case fails ``within``; where a twin removes one term, the
    smallest such term is at least 8 x the case's f32 bound in scale units (for bf16 output the
    rounding term of the bound is relative to the entry, so the rejection itself is the check).
    A disturbed sentinel and an entry one bf16 ulp off beyond rounding fail too."""
    seen = set()
    for c in C.CASES:
        if c in (C.STREAM_TALL, C.BIG_TALL):  # the same code paths as their groups' small cases
            continue
        t = float(C.tol(c).max())
        for name, values, removed in C.twins(c):
            seen.add(name)
            assert C.within(c, C.embed(c, values)) != [], (C.case_id(c), name)
            if removed is not None:
                assert removed >= 8 * t, (C.case_id(c), name, removed, t)
        buf = C.embed(c, C.restatement(c))
        buf[0] ^= 1  # a guard row's first element
        assert C.within(c, buf)[0][0] == "sentinel"
    assert seen == TWIN_NAMES, TWIN_NAMES ^ seen


def test_bf16_output_bound_bites_at_one_ulp():
    """An entry of a bf16-output case one bf16 ulp further from the reference than its correct
    rounding is off by at least 1.5 ulp, a whole ulp above the rounding term of the bound: it
    fails, while the correctly rounded buffer passes."""
    for c in [c for c in C.CASES if c.bf and c.epi == "store" and not c.bias and c.k > 0][:6]:
        want, scale = C.reference(c)
        ratio = np.where(scale > 0, np.abs(want) / np.maximum(scale, 1e-300), 0)
        z, i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[z, i, j] > 0.01  # an entry without heavy cancellation: the ulp is visible in scale units
        buf = C.embed(c, C.restatement(c))
        assert C.within(c, buf) == []
        at = C.valid_index(c)[z, i, j]
        away = abs(float(C.from_bits16(buf[at]))) >= abs(want[z, i, j])  # bits + 1: one ulp larger in magnitude
        buf[at] = int(buf[at]) + (1 if away else -1)
        assert [b[0] for b in C.within(c, buf)] == ["slab %d" % z], C.case_id(c)
