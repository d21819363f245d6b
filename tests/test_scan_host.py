"""CPU checks behind tests/test_gpu_scan.py: the case list of tests/scan_cases.py reaches
every chunk length of the three blocked scan kernels (gae_scan_kernel, gae_full_kernel,
episode_stats_kernel), one to three segments and the three block geometries; every flag
layout puts its episode ends where it claims; the exact-value cases are exact; the batched
reference agrees with the reference algorithm's per-path form; the bound rejects the
subtly wrong twins of the scan.  Plus the argument checks and workspace sizes of mrl_gae
and mrl_episode_stats, which return before any launch."""
import ctypes

import numpy as np
import pytest

from oracle import trpo_np as T
from tests import scan_cases as C

X = ctypes.c_void_p(1 << 20)  # a non-NULL pointer nothing dereferences: every call below returns before a launch


# ------------------------------------------------------------------ the case list
def test_chunk_len_restates_the_dispatch():
    """chunk_len(T, 32, 32) of csrc/vector_host.h: L covers T in one 32-chunk segment up to
    T = 1024, and stays 32 above."""
    want = {1: (1, 32), 2: (33, 64), 4: (65, 128), 8: (129, 256), 16: (257, 512), 32: (513, 5000)}
    for L, (lo, hi) in want.items():
        for Tn in (lo, (lo + hi) // 2, hi):
            assert C.chunk_len(Tn) == L, (Tn, L)
    assert [C.n_segments(t) for t in (1, 1024, 1025, 2048, 2049)] == [1, 1, 2, 2, 3]
    assert [C.geometry(e) for e in (1, 16, 17, 125, 128, 144)] == ["plain"] * 3 + ["permuted_partial",
                                                                                    "permuted_full", "plain"]
    assert C.exact_fit(128, 144) and not C.exact_fit(128, 125) and not C.exact_fit(127, 144) and not C.exact_fit(2048, 16)


def test_case_list_reaches_every_branch():
    assert all(t in C.TS and e in C.ES for t, e in C.SHAPES) and len(set(C.SHAPES)) == len(C.SHAPES) <= 32
    assert max(t * e for t, e in C.SHAPES) == 2049 * 144
    reach = {"general": set(), "full": set(), "episode": set()}
    for t, e in C.SHAPES:
        reach[C.gae_kernel(t, e)].add(C.chunk_len(t))
        reach["episode"].add(C.chunk_len(t))
    for k, ls in reach.items():
        assert ls == set(C.LS), (k, sorted(ls))
    assert {C.n_segments(t) for t, _ in C.SHAPES} == {1, 2, 3}
    assert {C.geometry(e) for _, e in C.SHAPES} == set(C.GEOMETRIES)
    # the general kernel meets each geometry, the permutation a partial block and a second segment
    assert {C.geometry(e) for t, e in C.SHAPES if C.gae_kernel(t, e) == "general"} == set(C.GEOMETRIES)
    assert any(C.geometry(e) == "permuted_partial" and C.n_segments(t) == 3 for t, e in C.SHAPES)
    # a second segment of one row, and a last chunk of one row
    assert any(t % C.segment_len(t) == 1 for t, _ in C.SHAPES)
    # the exact-fit list: six L x three geometries, all taken by gae_full_kernel
    assert all(C.exact_fit(t, e) for t, e in C.EXACT_FIT_SHAPES)
    assert {(C.chunk_len(t), e) for t, e in C.EXACT_FIT_SHAPES} == {(L, e) for L in C.LS for e in (16, 128, 144)}
    assert [C.geometry(e) for e in (16, 128, 144)] == ["plain", "permuted_full", "plain"]  # 1, 8 and 9 blocks
    # the sentinel list: one ragged general case per L, and the exact-fit kernel
    rag = [(t, e) for t, e in C.SENTINEL_SHAPES if C.gae_kernel(t, e) == "general"]
    assert {C.chunk_len(t) for t, _ in rag} == set(C.LS)
    assert all(e % C.EB and t % C.segment_len(t) for t, e in rag)  # a partial block, a partial segment
    assert any(C.gae_kernel(t, e) == "full" for t, e in C.SENTINEL_SHAPES)
    assert any(C.n_segments(t) == 3 for t, _ in rag) and any(C.geometry(e) == "permuted_partial" for _, e in rag)


def test_every_layout_is_launched():
    """Columns cycle through the 17 layouts: each shape of 17 or more columns holds them all,
    and over the blocks of the 125-, 128- and 144-column shapes a layout meets several env slots."""
    n = len(C.LAYOUTS)
    assert n == 17 and len(set(C.LAYOUT_NAMES)) == n
    for t, e in C.SHAPES:
        got = {C.layout_of(t, e, c) for c in range(e)}
        assert len(got) == min(e, n), (t, e)
    slots = {(C.layout_of(128, 125, c), c % C.EB) for c in range(125)}
    assert min(sum(1 for (l, _) in slots if l == k) for k in range(n)) >= 7
    # the small shapes start the cycle at different layouts
    assert len({C.layout_of(t, 1, 0) for t, e in C.SHAPES if e == 1}) == 3


def _column(name, Tn):
    i = C.LAYOUT_NAMES.index(name)
    _, fn, kind = C.LAYOUTS[i]
    return fn(Tn, C.chunk_len(Tn), C.segment_len(Tn), np.random.default_rng(Tn + i), kind), kind


@pytest.mark.parametrize("Tn", sorted({t for t, _ in C.SHAPES}))
def test_layouts_put_their_ends_where_they_claim(Tn):
    L, S, nseg = C.chunk_len(Tn), C.segment_len(Tn), C.n_segments(Tn)
    chunks = [(s * S + c * L, min(s * S + c * L + L, Tn)) for s in range(nseg) for c in range(C.NC) if s * S + c * L < Tn]
    assert sum(hi - lo for lo, hi in chunks) == Tn
    for variant in ("trunc", "term"):
        def ends(name):
            f, kind = _column(f"{name}_{variant}", Tn)
            assert kind == (C.TRUNC if variant == "trunc" else C.TERM)
            assert f.dtype == np.uint8 and f.shape == (Tn,) and f[Tn - 1] & 1
            return f, kind, set(np.nonzero(f & 1)[0].tolist())

        f, kind, at = ends("none")
        assert at == {Tn - 1} and f[Tn - 1] == kind
        f, kind, at = ends("every")
        assert at == set(range(Tn)) and f[0] == kind
        assert all(int(f[t]) + int(f[t + 1]) == C.TRUNC + C.TERM for t in range(Tn - 1))  # alternating
        f, kind, at = ends("chunk_last")
        assert at == {hi - 1 for lo, hi in chunks if hi - lo == L} | {Tn - 1} and all(f[t] == kind for t in at)
        f, kind, at = ends("chunk_first")
        assert at == {lo for lo, hi in chunks} | {Tn - 1} and all(f[t] == kind for t in at)
        f, kind, at = ends("seg_edges")
        want = {Tn - 1}
        for s in range(nseg):
            if (s + 1) * S - 1 < Tn:
                want.add((s + 1) * S - 1)  # the segment's last row ...
            if s > 0:
                want.add(s * S)            # ... and the next one's first
        assert at == want and all(f[t] == kind for t in at)
        f, kind, at = ends("single")
        assert at == ({Tn - 2, Tn - 1} if Tn >= 2 else {0}) and all(f[t] == kind for t in at)
        f, kind, at = ends("random")
        assert all(f[t] == kind for t in at) and np.all(f[sorted(set(range(Tn)) - at)] == 0)
        if Tn >= 1023:
            assert 0.03 * Tn < len(at) < 0.15 * Tn  # density 0.08: more than 5 sigma either side at T = 1023
    f, _ = _column("random_mixed", Tn)
    assert set(np.unique(f).tolist()) <= {0, C.TRUNC, C.TERM} and f[Tn - 1] & 1
    if Tn >= 200:
        assert (f == C.TRUNC).sum() > 0 and (f == C.TERM).sum() > 0
    f, _ = _column("bit1_mid", Tn)
    assert set(np.unique(f).tolist()) <= {2, C.TRUNC, C.TERM} and f[Tn - 1] & 1
    assert Tn < 64 or (f == 2).sum() > Tn // 2
    f, _ = _column("open_final", Tn)
    assert f[Tn - 1] == 0 and C.closed(f[:, None])[Tn - 1, 0] == 1
    assert np.array_equal(C.closed(f[:, None])[:-1, 0], f[:-1])


def test_flags_are_deterministic_and_cover_the_edge_rows():
    """Two builds agree; at 2049 x 144 some column ends an episode on each kind of edge row,
    as a truncation and as a termination."""
    Tn, E = 2049, 144
    f = C.make_flags(Tn, E)
    assert np.array_equal(f, C.make_flags(Tn, E))
    L, S = C.chunk_len(Tn), C.segment_len(Tn)
    for kind in (C.TRUNC, C.TERM):
        for row in (L - 1, L, S - 1, S, 2 * S - 1, 2 * S, Tn - 2, Tn - 1):
            assert np.any(f[row] == kind), (kind, row)
    assert np.any(f[Tn - 1] == 0) and np.any(f == 2)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_exact_cases_are_exact(shape):
    """Integer inputs with gamma = lam = 1: every partial sum of either recurrence stays below
    2^24 (exact in fp64 and in the float32 cast), the moments below 2^53, and the reference
    is integer valued."""
    Tn, E = shape
    c = C.gae_case(Tn, E, "exact", 1.0, 1.0)
    for k in ("rew", "v"):
        assert np.all(c[k] == np.rint(c[k])) and np.abs(c[k]).max() <= 8
    assert c["m_adv"].max() < 2 ** 24 and c["m_ret"].max() < 2 ** 24
    for k in ("adv", "ret"):
        assert np.all(c[k] == np.rint(c[k])) and np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64))
    a = [int(x) for x in c["adv"].reshape(-1)]
    assert sum(abs(x) for x in a) < 2 ** 53 and sum(x * x for x in a) < 2 ** 53
    (s1, s2), (b1, b2) = C.adv_moments_ref(c["adv"].astype(np.float32))
    assert (s1, s2) == (float(sum(a)), float(sum(x * x for x in a)))
    ep = C.episode_case(Tn, E, "exact")
    R = [int(sum(int(x) for x in p)) for p in C.episodes(ep["rew"], ep["flags"])]
    assert sum(r * r for r in R) < 2 ** 53
    if R:
        assert ep["out"].tolist() == [len(R), sum(R), sum(r * r for r in R), max(R),
                                      sum(len(p) for p in C.episodes(ep["rew"], ep["flags"])),
                                      max(len(p) for p in C.episodes(ep["rew"], ep["flags"]))]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", [s for s in C.SHAPES if s[0] * s[1] <= 2049 * 17 or s == (1025, 125)], ids=C.shape_id)
def test_batched_reference_matches_the_per_path_form(shape):
    """oracle.trpo_np.gae_batched against compute_advantage's per-path arithmetic (`discount`
    of the rewards and of the b1-bootstrapped deltas, one path per flags & 1 run): inside the
    bound for the generic values and every parameter set, identical for the exact ones."""
    Tn, E = shape
    for family, params in (("generic", C.PARAMS), ("offset", C.PARAMS[:1]), ("exact", C.PARAMS[2:])):
        for gamma, lam in params:
            c = C.gae_case(Tn, E, family, gamma, lam)
            adv, ret = C.gae_per_path(c["rew"], c["v"], c["flags"], gamma, lam)
            if family == "exact":
                np.testing.assert_array_equal(adv, c["adv"])
                np.testing.assert_array_equal(ret, c["ret"])
            else:
                for got, k in ((adv, "adv"), (ret, "ret")):
                    err = np.abs(got - c[k])
                    assert np.all(err <= c[k + "_bound"]), C.worst(err, c[k + "_bound"], Tn, E, f"{k} {family} {gamma} {lam}")


def test_per_path_form_is_compute_advantage():
    """gae_per_path restates oracle.trpo_np.compute_advantage: the same numbers before its
    standardisation, on the paths of one column."""
    Tn, E = 200, 125
    c = C.gae_case(Tn, E, "generic", 0.995, 0.97)
    adv, _ = C.gae_per_path(c["rew"], c["v"], c["flags"], 0.995, 0.97)
    f = C.closed(c["flags"])
    paths = []
    for e in range(E):
        start = 0
        for t in np.nonzero(f[:, e] & 1)[0]:
            paths.append(dict(reward=c["rew"][start:t + 1, e].astype(np.float64), terminated=bool(f[t, e] & 2),
                              v=c["v"][start:t + 1, e].astype(np.float64), at=(start, t + 1, e)))
            start = t + 1
    T.compute_advantage(lambda p: p["v"], paths, 0.995, 0.97)
    got = np.zeros((Tn, E))
    for p in paths:
        lo, hi, e = p["at"]
        got[lo:hi, e] = p["advantage"]
    np.testing.assert_allclose(got, T.standardize(adv), rtol=1e-12, atol=1e-12)


def _wrong_twins(c, gamma, lam):
    """Subtly wrong scans of the same inputs: (name, adv, ret)."""
    r, v, f = c["rew"].astype(np.float64), c["v"].astype(np.float64), C.closed(c["flags"])
    last, term = (f & 1) > 0, (f & 2) > 0
    yield "truncation bootstraps 0", *T.gae_batched(r, v, last, last, gamma, lam)
    yield "termination bootstraps v", *T.gae_batched(r, v, last, np.zeros_like(last), gamma, lam)
    yield "bit 1 alone ends an episode", *T.gae_batched(r, v, (f & 3) > 0, term, gamma, lam)
    yield "float32 recurrences", *T.gae_batched(c["rew"], c["v"], last, term, np.float32(gamma), np.float32(lam))
    S = C.segment_len(r.shape[0])
    if r.shape[0] > S:  # the carry into the first segment dropped: an end forced on its last row
        cut = last.copy()
        cut[S - 1] = True
        yield "segment carry dropped", *T.gae_batched(r, v, cut, term, gamma, lam)
    a, q = T.gae_batched(r, v, last, term, gamma, lam)
    yield "constant offset", a + 1e-3, q + 1e-3
    yield "uniform scale", a * (1 + 1e-6), q * (1 + 1e-6)


@pytest.mark.parametrize("shape", [(200, 125), (2049, 15)], ids=C.shape_id)
def test_bound_rejects_the_wrong_twins(shape):
    """Each wrong twin misses the elementwise bound in adv or ret (the offset and the scale,
    which cancel in the standardised advantage, included); float32 recurrences miss it on
    the +1000 rewards."""
    Tn, E = shape
    gamma, lam = 0.995, 0.97
    for family in ("generic", "offset"):
        c = C.gae_case(Tn, E, family, gamma, lam)
        for name, a, q in _wrong_twins(c, gamma, lam):
            if name == "float32 recurrences" and family == "generic":
                continue
            miss = np.sum(np.abs(a - c["adv"]) > c["adv_bound"]) + np.sum(np.abs(q - c["ret"]) > c["ret_bound"])
            assert miss > 0, (name, family)
        ok = np.float32(c["adv"]).astype(np.float64)  # the right answer, rounded as the device rounds
        assert np.all(np.abs(ok - c["adv"]) <= c["adv_bound"])


# ------------------------------------------------------------------ argument checks
def _lib():
    from modular_rl_amd import _lib as L
    return L.load()


def _gae(lib, args, Tn=8, E=8):
    return lib.mrl_gae(args[0], args[1], args[2], Tn, E, ctypes.c_double(0.99), ctypes.c_double(0.95), args[3], args[4],
                       args[5], args[6], None)


def test_gae_argument_checks():
    lib = _lib()
    for i in range(7):
        assert _gae(lib, [None if j == i else X for j in range(7)]) == -1, i
        assert b"null" in lib.mrl_last_error()
    for Tn, E in ((0, 8), (8, 0), (-1, 8), (8, -1), (0, 0)):
        assert _gae(lib, [X] * 7, Tn, E) == 0, (Tn, E)
    for E in (524272, 524273, 1 << 20, 1 << 40):
        for Tn in (1, 1024, 5000):
            assert _gae(lib, [X] * 7, Tn, E) == -2, (Tn, E)
            assert b"mrl_gae" in lib.mrl_last_error() and b"too large" in lib.mrl_last_error()
    # a null pointer is refused before the shape is looked at
    assert _gae(lib, [None] + [X] * 6, 0, 0) == -1 and _gae(lib, [None] + [X] * 6, 8, 1 << 20) == -1


def test_episode_stats_argument_checks():
    lib = _lib()
    for i in range(4):
        a = [None if j == i else X for j in range(4)]
        assert lib.mrl_episode_stats(a[0], a[1], 8, 8, a[2], a[3], None) == -1, i
        assert b"null" in lib.mrl_last_error()
    for Tn, E in ((0, 8), (8, 0), (-1, 8), (8, -1)):
        assert lib.mrl_episode_stats(X, X, Tn, E, X, X, None) == -1, (Tn, E)
        assert b"empty" in lib.mrl_last_error()
    for E in (4194288, 4194289, 1 << 30, 1 << 40):
        assert lib.mrl_episode_stats(X, X, 8, E, X, X, None) == -2, E
        assert b"mrl_episode_stats" in lib.mrl_last_error() and b"too large" in lib.mrl_last_error()


def test_workspace_sizes():
    lib = _lib()
    for E in (0, -1, -100):
        assert lib.mrl_gae_workspace_bytes(1024, E) == 128
    for E in (1, 15, 16, 17, 63, 64, 65, 125, 128, 144, 4096, 524271):
        nb = -(-E // 16)
        want = -(-(nb * 16) // 64) * 64 + 64
        for Tn in (1, 1024, 2049):
            assert lib.mrl_gae_workspace_bytes(Tn, E) == want == C.gae_workspace_bytes(E), (Tn, E)
        assert lib.mrl_episode_stats_workspace_bytes(E) == nb * 64 == C.episode_stats_workspace_bytes(E), E
