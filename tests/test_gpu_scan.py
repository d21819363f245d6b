"""Direct GPU checks of the two blocked time-major scans, `mrl_gae` (csrc/gae.hip: the
general gae_scan_kernel and the exact-fit gae_full_kernel) and `mrl_episode_stats`
(csrc/episode_stats.hip), on the cases of tests/scan_cases.py: every chunk length of each
kernel, one to three segments, ragged T and E, the XCD block permutation with a full and
with a partial last block, and episode ends placed on the first / last rows of chunks and
segments as truncations and as terminations.  The raw advantage, return and moments are
compared with the fp64 reference under derived bounds (or bit for bit where the arithmetic
is exact); every output and workspace sits between sentinel guards.
tests/test_scan_host.py shows on the CPU that the list reaches those branches and that the
bounds reject the subtly wrong scans."""
import numpy as np
import pytest
import torch

from tests import scan_cases as C

pytestmark = pytest.mark.gpu


def _api():
    from modular_rl_amd import _lib
    return _lib.load(require_gpu=True), _lib.call, _lib.ptr, _lib.stream


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).cuda()  # a copy: the shared cases are read-only


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Guarded:
    """nbytes of device memory with C.GUARD bytes of 0xFF (a NaN pattern in fp32 and fp64)
    either side; the body holds the same sentinel, or zeros."""

    def __init__(self, nbytes, dtype, zero=False):
        self.nbytes = int(nbytes)
        self.buf = torch.full((2 * C.GUARD + self.nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        self.raw = self.buf[C.GUARD:C.GUARD + self.nbytes]
        if zero:
            self.raw.zero_()
        self.body = self.raw.view(dtype)

    def check(self, what):
        b = _host(self.buf)
        assert np.all(b[:C.GUARD] == 0xFF), f"{what}: written before its first byte"
        assert np.all(b[C.GUARD + self.nbytes:] == 0xFF), f"{what}: written past its {self.nbytes} bytes"

    def unwritten(self):
        """4-byte words of the body that still hold the sentinel."""
        return int((_host(self.raw).view(np.uint32) == 0xFFFFFFFF).sum())


def _run_gae(rew, v, flags, gamma, lam, calls=1, inputs_kept=False):
    """mrl_gae on [T, E] host arrays, every output and the workspace guarded.  Returns
    (adv [T, E] float32, ret, moments [3] float64); checks the guards, that every output
    word was written and that the completion ticket is back at 0."""
    lib, call, ptr, stream = _api()
    Tn, E = rew.shape
    d_rew, d_v, d_f = _dev(rew), _dev(v), _dev(flags)
    adv, ret = Guarded(Tn * E * 4, torch.float32), Guarded(Tn * E * 4, torch.float32)
    wsb = int(lib.mrl_gae_workspace_bytes(Tn, E))
    assert wsb == C.gae_workspace_bytes(E)
    ws = Guarded(wsb, torch.uint8, zero=True)  # zeroed, as include/mrl_hip.h requires
    moms = []
    for _ in range(calls):
        mom = Guarded(24, torch.float64)
        call("mrl_gae", ptr(d_rew), ptr(d_v), ptr(d_f), Tn, E, gamma, lam, ptr(adv.body), ptr(ret.body), ptr(mom.body),
             ptr(ws.body), stream())
        mom.check("moments")
        assert mom.unwritten() == 0, "moments not written"
        moms.append(_host(mom.body).copy())
    for g, what in ((adv, "adv"), (ret, "ret"), (ws, "workspace")):
        g.check(what)
    assert adv.unwritten() == 0 and ret.unwritten() == 0, "an output row was left unwritten"
    assert np.all(_host(ws.raw)[wsb - 64:] == 0), "the completion ticket did not return to 0"
    for m in moms[1:]:
        np.testing.assert_array_equal(_bits(m), _bits(moms[0]), err_msg="moments of repeated calls on one workspace")
    if inputs_kept:
        for d, h, what in ((d_rew, rew, "rew"), (d_v, v, "v"), (d_f, flags, "flags")):
            assert np.array_equal(_host(d).view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), f"{what} was written"
    return _host(adv.body).reshape(Tn, E).copy(), _host(ret.body).reshape(Tn, E).copy(), moms[0]


def _check_moments(mom, adv, Tn, E, what):
    """moments[2] is the row count exactly; the two sums are within moments_bounds of the exact
    sums of the adv rows the kernel returned."""
    assert mom[2] == Tn * E, (what, mom[2])
    (s1, s2), (b1, b2) = C.adv_moments_ref(adv)
    print(f"{what}: moments err/bound {abs(mom[0] - s1) / max(b1, 1e-300):.3g} {abs(mom[1] - s2) / max(b2, 1e-300):.3g}")
    assert abs(mom[0] - s1) <= b1 and abs(mom[1] - s2) <= b2, (what, mom, (s1, s2), (b1, b2))


# ------------------------------------------------------------------ GAE
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_gae_matches_reference(shape, monkeypatch):
    """The raw (unstandardised) advantage and the return against oracle.trpo_np.gae_batched,
    elementwise inside gae_bound, and the moments against the exact sums of the returned
    rows: three parameter sets (lam = 0 zeroes every map multiplier B; gamma = lam = 1 keeps
    them at 1), unit-scale rewards and rewards offset by +1000."""
    monkeypatch.delenv("MRL_GAE_GENERAL", raising=False)
    Tn, E = shape
    for family in ("generic", "offset"):
        for gamma, lam in C.PARAMS:
            c = C.gae_case(Tn, E, family, gamma, lam)
            adv, ret, mom = _run_gae(c["rew"], c["v"], c["flags"], gamma, lam)
            what = f"{C.gae_kernel(Tn, E)} L={C.chunk_len(Tn)} {Tn}x{E} {family} gamma={gamma} lam={lam}"
            for got, k in ((adv, "adv"), (ret, "ret")):
                err, bound = np.abs(got.astype(np.float64) - c[k]), c[k + "_bound"]
                with np.errstate(divide="ignore", invalid="ignore"):
                    print(f"{what} {k}: max err/bound {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3g}")
                assert np.all(err <= bound), C.worst(err, bound, Tn, E, f"{what} {k}")
            _check_moments(mom, adv, Tn, E, what)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_gae_exact_identities(shape, monkeypatch):
    """Zero tolerance.  Integer rewards and baselines with gamma = lam = 1: every fp64
    operation is exact in any association, so adv, ret and the three moments equal the
    reference bit for bit.  gamma = 0: ret is rew and adv is the float32 cast of the fp64
    rew - v, whatever the flags."""
    monkeypatch.delenv("MRL_GAE_GENERAL", raising=False)
    Tn, E = shape
    c = C.gae_case(Tn, E, "exact", 1.0, 1.0)
    adv, ret, mom = _run_gae(c["rew"], c["v"], c["flags"], 1.0, 1.0)
    for got, k in ((adv, "adv"), (ret, "ret")):
        want = c[k].astype(np.float32)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), C.worst(bad * 1.0, np.zeros(bad.shape), Tn, E, f"exact {k}")
    a = c["adv"].reshape(-1)
    np.testing.assert_array_equal(mom, np.array([a.sum(), (a * a).sum(), Tn * E]))  # integer sums below 2^53: exact
    for family, lam in (("generic", 0.97), ("generic", 0.0)):
        rew, v = C.make_values(Tn, E, family)
        adv, ret, mom = _run_gae(rew, v, C.make_flags(Tn, E), 0.0, lam)
        np.testing.assert_array_equal(_bits(ret), _bits(rew))
        np.testing.assert_array_equal(_bits(adv), _bits((rew.astype(np.float64) - v.astype(np.float64)).astype(np.float32)))
        _check_moments(mom, adv, Tn, E, f"gamma=0 {Tn}x{E}")


@pytest.mark.parametrize("shape", C.EXACT_FIT_SHAPES, ids=C.shape_id)
def test_gae_exact_fit_equals_general(shape, monkeypatch):
    """gae_full_kernel (its chunk multipliers B, C written as the precomputed gl^L, gamma^L)
    against gae_scan_kernel on the same inputs in one process (MRL_GAE_GENERAL is read at
    every call): adv, ret and the moments bit for bit, for every chunk length, 1 / 8 / 9
    blocks, the three parameter sets and all value families; three calls on one workspace
    leave the ticket at 0 and give the same moments (checked in _run_gae)."""
    Tn, E = shape
    assert C.exact_fit(Tn, E)
    flags = C.make_flags(Tn, E)
    for family in C.FAMILIES:
        rew, v = C.make_values(Tn, E, family)
        for gamma, lam in C.PARAMS:
            monkeypatch.delenv("MRL_GAE_GENERAL", raising=False)
            full = _run_gae(rew, v, flags, gamma, lam, calls=3)
            monkeypatch.setenv("MRL_GAE_GENERAL", "1")
            general = _run_gae(rew, v, flags, gamma, lam, calls=3)
            for f, g, k in zip(full, general, ("adv", "ret", "moments")):
                np.testing.assert_array_equal(_bits(f), _bits(g), err_msg=f"{k} {family} gamma={gamma} lam={lam}")


@pytest.mark.parametrize("shape", C.SENTINEL_SHAPES, ids=C.shape_id)
def test_gae_writes_stay_in_bounds(shape, monkeypatch):
    """adv, ret, moments and the workspace inside NaN-pattern buffers with 4 KB of guard either
    side: the guards are untouched, every output word is written, and rew / v / flags come
    back bit for bit -- a ragged shape per chunk length (masked stores of the general kernel)
    and the exact-fit kernel (buffer resources sized on the host), which is run both ways."""
    Tn, E = shape
    rew, v = C.make_values(Tn, E, "generic")
    flags = C.make_flags(Tn, E)
    for general in ((False, True) if C.exact_fit(Tn, E) else (False,)):
        if general:
            monkeypatch.setenv("MRL_GAE_GENERAL", "1")
        else:
            monkeypatch.delenv("MRL_GAE_GENERAL", raising=False)
        _run_gae(rew, v, flags, 0.995, 0.97, calls=2, inputs_kept=True)


# ------------------------------------------------------------------ episode statistics
def _run_episode_stats(rew, flags):
    """mrl_episode_stats with out (6 doubles) and the workspace guarded and pre-filled with the
    sentinel: a block partial left unwritten shows as NaN in the output."""
    lib, call, ptr, stream = _api()
    Tn, E = rew.shape
    d_rew, d_f = _dev(rew), _dev(flags)
    wsb = int(lib.mrl_episode_stats_workspace_bytes(E))
    assert wsb == C.episode_stats_workspace_bytes(E)
    out, ws = Guarded(48, torch.float64), Guarded(wsb, torch.float64)
    call("mrl_episode_stats", ptr(d_rew), ptr(d_f), Tn, E, ptr(out.body), ptr(ws.body), stream())
    out.check("out")
    ws.check("workspace")
    assert out.unwritten() == 0 and ws.unwritten() == 0
    assert np.array_equal(_host(d_rew).view(np.uint8), np.ascontiguousarray(rew).view(np.uint8)), "rew was written"
    assert np.array_equal(_host(d_f), flags), "flags was written"
    return _host(out.body).copy()


def _check_episode_stats(got, want, bound, what):
    names = ("count", "sum R", "sum R^2", "max R", "sum len", "max len")
    print(what, "got", got.tolist(), "err", np.abs(got - want).tolist(), "bound", bound.tolist())
    for i, n in enumerate(names):
        if bound[i] == 0:
            assert got[i] == want[i], (what, n, got[i], want[i])
        else:
            assert abs(got[i] - want[i]) <= bound[i], (what, n, got[i], want[i], bound[i])


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_episode_stats_matches_reference(shape):
    """All six outputs against math.fsum per episode: bit for bit on integer rewards; with
    float rewards the count and the lengths exactly and the reward sums and maximum inside
    sum_bound.  The columns with an unflagged final row leave their last run uncounted."""
    Tn, E = shape
    c = C.episode_case(Tn, E, "exact")
    _check_episode_stats(_run_episode_stats(c["rew"], c["flags"]), c["out"], np.zeros(6), f"exact {Tn}x{E}")
    for family in ("generic", "offset"):
        c = C.episode_case(Tn, E, family)
        _check_episode_stats(_run_episode_stats(c["rew"], c["flags"]), c["out"], c["bound"], f"{family} {Tn}x{E}")


@pytest.mark.parametrize("shape", [(31, 15), (200, 125), (1025, 128), (2049, 144)], ids=C.shape_id)
def test_episode_stats_open_runs_and_empty_batches(shape):
    """Every column's final row unflagged: the runs the batch leaves open are dropped (the
    counted episodes are fewer than with the final row flagged).  No end at all, with and
    without stray bit 1: (0, 0, 0, -inf, 0, 0)."""
    Tn, E = shape
    rew, _ = C.make_values(Tn, E, "exact")
    flags = C.make_flags(Tn, E)
    flags[-1] &= 2
    want, _ = C.episode_stats_ref(rew, flags)
    got = _run_episode_stats(rew, flags)
    _check_episode_stats(got, want, np.zeros(6), f"open {Tn}x{E}")
    assert want[0] < C.episode_stats_ref(rew, C.closed(flags))[0][0]
    for fill in (0, 2):
        got = _run_episode_stats(rew, np.full((Tn, E), fill, dtype=np.uint8))
        assert got.tolist() == [0.0, 0.0, 0.0, -np.inf, 0.0, 0.0], (fill, got)
