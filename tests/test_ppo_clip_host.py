"""Clipped-surrogate PPO without a GPU: the argument checks of the MRL_EPI_PPOCLIP epilogue per
entry point (they return before any launch, so the built library is all this needs), the
float64 oracle of tests/ppo_clip_np.py against torch autograd, the conditions the GPU tests'
inputs are chosen to meet, the recorded float32 floors re-measured, and the updater's
construction checks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import trpo_np as T
from tests import ppo_clip_np as C

_E_ARG, _E_UNSUPPORTED = -1, -2
_PTR = ctypes.c_void_p(0x1000)   # a non-null address no check dereferences
PPOCLIP = 8
ENTRIES = ["mrl_mlp_rows", "mrl_mlp_rows_bf16", "mrl_head_rows"]
CLIP_TEXT = "PPOCLIP needs a clip range in (0, 1)"


def _call(entry, epi=PPOCLIP, head=2, clip=0.2, n=8, theta=_PTR, **io_changes):
    """One rows entry point on a valid descriptor (11 -> 64 -> 64 -> 3; the value net 12 -> 1)
    with dummy non-null addresses: (status, mrl_last_error)."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert _lib.EPI_PPOCLIP == PPOCLIP
    n_out = 1 if head == _lib.HEAD_LINEAR else 3
    io = _lib.RowsIO(x=_PTR, ep_t=None, timestep_limit=1.0, n=n, inv_n_global=0.125, act=_PTR, adv=_PTR, oldprob=_PTR,
                     target=_PTR, out=_PTR, ghead=_PTR, partial=_PTR, kl_cutoff=clip, cache_mode=0, act_cache=None,
                     feat_out=None)
    for k, v in io_changes.items():
        setattr(io, k, v)
    if entry == "mrl_head_rows":
        rc = lib.mrl_head_rows(head, n_out, epi, _PTR, None, theta, None, ctypes.byref(io), None, None)
    elif entry == "mrl_mlp_rows_split":
        d = _lib.MlpDesc(12 if head == _lib.HEAD_LINEAR else 11, n_out, head, 64, 2)
        rc = lib.mrl_mlp_rows_split(ctypes.byref(d), epi, theta, _PTR, ctypes.byref(io), None, None)
    else:
        d = _lib.MlpDesc(12 if head == _lib.HEAD_LINEAR else 11, n_out, head, 64, 2)
        rc = getattr(lib, entry)(ctypes.byref(d), epi, theta, _PTR, _PTR, _PTR, ctypes.byref(io), None, None)
    return rc, lib.mrl_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("clip", [0.0, 1.0, -0.1, float("nan"), float("inf")])
@pytest.mark.parametrize("head", [1, 2])
def test_ppoclip_rejects_a_clip_range_outside_0_1(entry, clip, head):
    assert _call(entry, head=head, clip=clip) == (_E_ARG, CLIP_TEXT)


@pytest.mark.parametrize("entry", ENTRIES)
def test_ppoclip_shares_ppograds_argument_checks(entry):
    assert _call(entry, head=0) == (_E_ARG, "policy epilogue on a value net")
    for field in ("act", "adv", "oldprob", "partial"):
        assert _call(entry, head=1, **{field: None}) == (_E_ARG, "losses need act/adv/oldprob/partial"), field
    assert _call(entry, head=2, ghead=None) == (_E_ARG, "gradient epilogues need ghead")
    want = "DiagGauss needs logstd" if entry == "mrl_head_rows" else "DiagGauss needs theta (logstd)"
    assert _call(entry, head=2, theta=None) == (_E_ARG, want)


@pytest.mark.parametrize("entry", ENTRIES)
def test_epilogue_7_stays_unknown(entry):
    assert _call(entry, epi=7, head=1) == (_E_ARG, "unknown epilogue")


def test_rows_split_keeps_refusing_ppoclip():
    assert _call("mrl_mlp_rows_split", head=2) == (_E_UNSUPPORTED, "mrl_mlp_rows_split: PROB, LOSSES, SURRGRAD or VFLOSS")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("head", [1, 2])
def test_ppoclip_accepts_zero_rows(entry, head):
    """n = 0 with valid arguments: nothing to do, status 0 (mrl_head_rows checks the epilogue
    first: "unknown epilogue" before MRL_EPI_PPOCLIP existed)."""
    assert _call(entry, head=head, n=0)[0] == 0


def test_ppoclip_allows_cache_write():
    """A plain forward epilogue: MRL_CACHE_WRITE passes the cache-mode check (the next check
    that fails is the one asked for here, the clip range)."""
    for entry in ("mrl_mlp_rows", "mrl_mlp_rows_bf16"):
        assert _call(entry, clip=0.0, act_cache=_PTR, cache_mode=1) == (_E_ARG, CLIP_TEXT)
        assert _call(entry, act_cache=_PTR, cache_mode=2) == (_E_ARG, "MRL_CACHE_READ is for MRL_EPI_FVP")


# ------------------------------------------------------------------ the oracle against autograd
@pytest.mark.parametrize("head,A", [("softmax", 3), ("softmax", 8), ("gauss", 1), ("gauss", 3)])
def test_oracle_ghead_is_autograd_of_the_clipped_surrogate(head, A):
    """ghead = d/d(head rows) of -mean min(r A, clamp(r, 1 - eps, 1 + eps) A), float64 torch
    autograd, to 1e-12; the DiagGauss log-std columns against the per-row log-std gradient."""
    from tests.test_gpu_ppo_clip import reference
    n = 257
    c, z, ref, _ = reference("f32", head, A, n)
    lo, hi = C.clip_bounds(C.EPS)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    adv, op = torch.tensor(c["adv"]), torch.tensor(c["oldprob"])
    if head == "softmax":
        a = torch.tensor(c["act"].astype(np.int64))
        logp = torch.log_softmax(zt, dim=1)[torch.arange(n), a]
        oldlogp = torch.log(op[torch.arange(n), a])
        leaves = [zt]
    else:
        a = torch.tensor(c["act"])
        ls = torch.tensor(np.repeat(c["theta"][-A:][None, :], n, axis=0), requires_grad=True)  # a log-std row per row
        logp = (-0.5 * ((a - zt) / torch.exp(ls)) ** 2 - ls).sum(dim=1) - 0.5 * C.LOG2PI * A
        oldlogp = (-0.5 * ((a - op[:, :A]) / op[:, A:]) ** 2 - torch.log(op[:, A:])).sum(dim=1) - 0.5 * C.LOG2PI * A
        leaves = [zt, ls]
    r = torch.exp(logp - oldlogp)
    loss = -(1.0 / (n + 3)) * torch.minimum(r * adv, torch.clamp(r, lo, hi) * adv).sum()
    want = torch.cat(torch.autograd.grad(loss, leaves), dim=1).numpy()
    np.testing.assert_allclose(r.detach().numpy(), ref["ratio"], rtol=1e-12)
    assert np.abs(ref["ghead"] - want).max() <= 1e-12
    assert (want[ref["clipped"]] == 0).all() and ref["clipped"].any() and (~ref["clipped"]).any()


# ------------------------------------------------------------------ the inputs of the GPU tests
@functools.lru_cache(maxsize=None)
def _measured():
    from tests.test_gpu_ppo_clip import measure
    return measure()


def _pools():
    return [(h, A, C.POOL) for h, A in C.HEAD_WIDTHS] + [(h, A, C.BIG_N) for h, A in C.BIG_WIDTH.items()]


@pytest.mark.parametrize("entry", ["f32", "bf16", "head"])
def test_row_inputs_hold_every_regime_and_stay_clear_of_the_bounds(entry):
    """Per pool of rows (257 per head and width, of which the smaller cases are prefixes, and
    the grid-stride size), for the entry's own float64 reference: each of the four regimes
    holds at least 5 % of the rows, at most 1 % lie within DELTA of a clip bound."""
    from tests.test_gpu_ppo_clip import DELTA, reference
    for head, A, n in _pools():
        c, z, ref, _ = reference(entry, head, A, n)
        share = np.bincount(ref["regime"], minlength=4) / n
        assert share.min() >= C.MIN_SHARE, (entry, head, A, n, dict(zip(C.REGIME_NAMES, share)))
        band = (C.bound_distance(ref["ratio"], C.EPS) <= DELTA[f"{entry}.{head}"]).mean()
        assert band <= C.MAX_BAND_SHARE, (entry, head, A, n, band)


def test_recorded_floors_and_ratio_errors_are_the_restatements():
    """FLOOR and RATIO_ERR are what measure() gives: none recorded below the restatement's
    distance by more than the spread between numpy builds' expf / logf (1.5x)."""
    from tests.test_gpu_ppo_clip import FLOOR, RATIO_ERR
    got = _measured()
    assert set(got["floor"]) == set(FLOOR) and set(got["ratio"]) == set(RATIO_ERR)
    for k, v in got["floor"].items():
        assert np.isfinite(v) and v <= 1.5 * FLOOR[k], (k, v, FLOOR[k])
    for k, v in got["ratio"].items():
        assert np.isfinite(v) and v <= 1.5 * RATIO_ERR[k], (k, v, RATIO_ERR[k])


@pytest.mark.parametrize("entry", ["f32", "head"])
@pytest.mark.parametrize("head,A", [("softmax", 3), ("gauss", 3)])
def test_identity_inputs_clip_no_row_or_every_row(entry, head, A):
    from tests.test_gpu_ppo_clip import DELTA, TINY_EPS, identity_adv, reference
    c, z, ref, _ = reference(entry, head, A, 257)
    args = (head, z, c["theta"][-A:], c["act"])
    none = C.clip_rows(*args, identity_adv(ref, c, False), c["oldprob"], 0.999, 1.0)
    assert not none["clipped"].any()
    every = C.clip_rows(*args, identity_adv(ref, c, True), c["oldprob"], TINY_EPS, 1.0)
    assert every["clipped"].all()
    assert C.bound_distance(ref["ratio"], TINY_EPS).min() > DELTA[f"{entry}.{head}"]


@pytest.mark.parametrize("head,nin,nout", [("gauss", 11, 3), ("softmax", 4, 3)])
def test_update_twin_keeps_every_row_clear_of_the_bounds(head, nin, nout):
    """No row of any minibatch of the twin's update comes within 1e-3 of 1 -+ eps (a flipped row
    would be a discontinuity of the gradient, not a rounding difference), rows are clipped and
    kept, and both epochs run."""
    from tests.test_gpu_ppo_clip import UPDATE_CFG, update_twin
    spec, th, ob, act, adv, oldprob, (th_w, info, adam, margin) = update_twin(head, nin, nout)
    assert margin > 1e-3, margin
    reg = C.policy_rows(spec, th, ob, act, adv, oldprob, UPDATE_CFG["clip_param"], 1.0)["regime"]
    assert set(reg) == {0, 1, 2, 3}
    assert info["epochs_run"] == 2 and adam[2] == 6 and np.abs(th_w - th).max() > 0


def test_twin_stops_early_on_target_kl():
    from tests.test_gpu_ppo_clip import UPDATE_N, update_twin
    spec, th, ob, act, adv, oldprob, _ = update_twin("gauss", 11, 3)
    perms = [np.arange(UPDATE_N)] * 3
    assert C.clip_update(spec, th, ob, act, adv, oldprob, perms, minibatch_size=128, target_kl=1e-9)[1]["epochs_run"] == 1
    assert C.clip_update(spec, th, ob, act, adv, oldprob, perms, minibatch_size=128)[1]["epochs_run"] == 3


# ------------------------------------------------------------------ the updater's construction
class _Net:
    P, device = 10, "cpu"


@pytest.mark.parametrize("bad", [100, 0, -128, 129])
def test_updater_rejects_a_minibatch_size_that_is_no_multiple_of_128(bad):
    from modular_rl_amd._lib import MrlError
    from modular_rl_amd.ppo import PpoClipUpdater
    pol = type("Pol", (), {"net": _Net()})()
    with pytest.raises(MrlError, match="minibatch_size"):
        PpoClipUpdater(pol, dict(minibatch_size=bad))
    up = PpoClipUpdater(pol, dict(minibatch_size=256))
    assert up.cfg["clip_param"] == 0.2 and up.cfg["epochs"] == 10 and up.cfg["stepsize"] == 3e-4
    assert up.cfg["minibatch_size"] == 256 and up.cfg["target_kl"] == 0.0
    assert set(up.state_arrays()) >= {"adam_m", "adam_v", "adam_t"}


def test_agent_is_a_trpo_agent_with_the_updaters_options():
    from modular_rl_amd import agentzoo
    assert issubclass(agentzoo.PpoClipAgent, agentzoo.TrpoAgent)
    assert agentzoo.PpoClipAgent.updater_cls.__name__ == "PpoClipUpdater"
    names = [o[0] for o in agentzoo.PpoClipAgent.options]
    assert {"clip_param", "epochs", "stepsize", "minibatch_size", "target_kl"} <= set(names)
