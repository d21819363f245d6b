"""The small-net population rollout without a GPU: the float64 twin of any depth against the
64-64 twin, the zero-padding to 64-64, the parameter count and the LDS predicate of the C ABI,
the argument checks of mrl_pop_rollout_mlp before any launch, the exports and the command line."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cem_np, cem_small_np, pop_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -2
REQUIRED_SHAPES = [(), (10, 5), (16,), (7, 3, 5)]


def _ids(_lib):
    return {"CartPole-v0": _lib.ENV_CARTPOLE, "Hopper-v2": _lib.ENV_HOPPER, "Pendulum-v0": _lib.ENV_PENDULUM,
            "MountainCar-v0": _lib.ENV_MOUNTAINCAR, "Acrobot-v1": _lib.ENV_ACROBOT,
            "InvertedPendulum-v2": _lib.ENV_INVPENDULUM, "InvertedDoublePendulum-v2": _lib.ENV_INVDOUBLEPENDULUM}


_hid = pop_cases.hid_array


def test_forward_at_64_64_is_the_64_64_twin():
    """The general forward at [11, 64, 64, 3] against the three layers written out."""
    rng = np.random.default_rng(0)
    P = cem_np.num_params([11, 64, 64, 3], True)
    assert P == 5126
    th = rng.standard_normal((6, P))
    x = rng.standard_normal((6, 11))

    def written_out(t, r):
        W0, b0 = t[0:704].reshape(11, 64), t[704:768]
        W1, b1 = t[768:4864].reshape(64, 64), t[4864:4928]
        W2, b2 = t[4928:5120].reshape(64, 3), t[5120:5123]
        return np.tanh(np.tanh(r @ W0 + b0) @ W1 + b1) @ W2 + b2

    assert np.array_equal(cem_np.forward(th, x, [11, 64, 64, 3]), np.stack([written_out(th[i], x[i]) for i in range(6)]))
    assert np.array_equal(cem_np.forward(th[0], x, [11, 64, 64, 3]), np.stack([written_out(th[0], r) for r in x]))
    assert np.array_equal(cem_np.forward_64_64(th, x, 3), cem_np.forward(th, x, [11, 64, 64, 3]))
    # no hidden layer: x @ W + b
    W, b = rng.standard_normal((4, 2)), rng.standard_normal(2)
    lin = cem_small_np.forward(np.concatenate([W.ravel(), b]), x[:, :4], [4, 2])
    assert np.array_equal(lin, np.stack([r @ W + b for r in x[:, :4]]))


@pytest.mark.parametrize("n_in,n_out,gauss", [(11, 3, True), (4, 2, False)])
def test_padded_net_computes_the_small_net(n_in, n_out, gauss):
    """The extra units contribute tanh(0) = 0 times zero weights: the float64 sums gain exact
    zeros only, so the two forwards agree to the last bit up to the order numpy sums 64
    instead of 10 / 5 terms in (pairwise blocks): rtol 1e-13."""
    rng = np.random.default_rng(1)
    dims = [n_in, 10, 5, n_out]
    P = cem_small_np.num_params(dims, gauss)
    th = rng.standard_normal((5, P)).astype(np.float32)
    x = rng.standard_normal((5, n_in))
    pad = np.stack([cem_small_np.pad_to_64_64(t, n_in, (10, 5), n_out, gauss) for t in th])
    assert pad.dtype == np.float32 and pad.shape == (5, cem_small_np.num_params([n_in, 64, 64, n_out], gauss))
    np.testing.assert_allclose(cem_np.forward_64_64(pad, x, n_out), cem_small_np.forward(th, x, dims), rtol=1e-13, atol=1e-15)
    if gauss:
        assert np.array_equal(pad[:, -n_out:], th[:, -n_out:])
    (W0, _), (W1, _), _ = cem_np.split_theta(pad[0], [n_in, 64, 64, n_out])
    assert not W0[:, 10:].any() and not W1[10:, :].any() and not W1[:, 5:].any()


def test_num_params_and_fits():
    from modular_rl_amd import _lib
    lib = _lib.load()
    for env_id, kind in _ids(_lib).items():
        O, A, gauss = cem_small_np.ENVS[env_id]
        for hid in REQUIRED_SHAPES:
            want = cem_small_np.num_params([O, *hid, A], gauss)
            assert lib.mrl_pop_mlp_num_params(kind, _hid(hid), len(hid)) == want, (env_id, hid)
            assert lib.mrl_pop_rollout_mlp_fits(kind, _hid(hid), len(hid)) == 1, (env_id, hid)
    H, C = _lib.ENV_HOPPER, _lib.ENV_CARTPOLE
    assert lib.mrl_pop_mlp_num_params(H, _hid((10, 5)), 2) == 196
    assert lib.mrl_pop_mlp_num_params(C, _hid((10, 5)), 2) == 117
    assert lib.mrl_pop_mlp_num_params(H, None, 0) == 39
    assert lib.mrl_pop_mlp_num_params(H, _hid((64, 64)), 2) == 5126
    # not supported: 0
    for kind, hid in ((H, (64, 64, 64, 64)), (H, (65,)), (H, (10, 0)), (_lib.ENV_HUMANOID, (10, 5))):
        assert lib.mrl_pop_rollout_mlp_fits(kind, _hid(hid), len(hid)) == 0, (kind, hid)
    # 64 candidates of the 64-64 net are 1.3 MB: beyond one block's LDS
    assert lib.mrl_pop_rollout_mlp_fits(H, _hid((64, 64)), 2) == 0
    # bad arguments: negative
    assert lib.mrl_pop_rollout_mlp_fits(H, None, 2) == E_ARG and b"mrl_pop_rollout_mlp_fits" in lib.mrl_last_error()
    assert lib.mrl_pop_rollout_mlp_fits(H, _hid((10, 5)), -1) == E_ARG
    assert lib.mrl_pop_rollout_mlp_fits(3, _hid((10, 5)), 2) == E_ARG  # 3 is not an env
    assert lib.mrl_pop_mlp_num_params(H, None, 2) == E_ARG and b"mrl_pop_mlp_num_params" in lib.mrl_last_error()
    assert lib.mrl_pop_mlp_num_params(H, _hid((10, 5)), -1) == E_ARG
    assert lib.mrl_pop_mlp_num_params(H, _hid((10, 0)), 2) < 0
    assert lib.mrl_pop_mlp_num_params(7, _hid((10, 5)), 2) == E_ARG


_pop_call = functools.partial(pop_cases.pop_call, entry="mrl_pop_rollout_mlp")


def test_pop_rollout_mlp_argument_checks():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for null in ("d", "b", "thetas", "io"):
        rc, msg = _pop_call(lib, _lib, null=(null,))
        assert rc == E_ARG and msg.startswith(b"mrl_pop_rollout_mlp:"), null
    cases = [dict(n_envs=0), dict(n_envs=-3), dict(bufs=False), dict(ld=195), dict(ld=-1), dict(io_kw=dict(ret=None)),
             dict(io_kw=dict(stat=None)),
             dict(io_kw=dict(trace_steps=4)),                                       # steps without buffers
             dict(io_kw=dict(trace_steps=4, trace_obs=fake, trace_act=fake)),       # no trace_rew
             dict(io_kw=dict(trace_obs=fake, trace_act=fake, trace_rew=fake)),      # no trace_steps
             dict(io_kw=dict(trace_steps=-1)),
             dict(n_hid=-1), dict(null_hid=True, n_hid=2),
             dict(env=3)]
    for kw in cases:
        rc, msg = _pop_call(lib, _lib, **kw)
        assert rc == E_ARG and msg.startswith(b"mrl_pop_rollout_mlp:"), kw
    unsupported = [dict(env=_lib.ENV_HUMANOID), dict(hid=(64, 64, 64, 64)), dict(hid=(65,)), dict(hid=(10, 0)),
                   dict(hid=(10, -2))]
    for kw in unsupported:
        rc, msg = _pop_call(lib, _lib, **kw)
        assert rc == E_UNSUPPORTED and msg.startswith(b"mrl_pop_rollout_mlp:"), kw
    # a shape the predicate turns away: the message names the need and the limit
    assert lib.mrl_pop_rollout_mlp_fits(_lib.ENV_HOPPER, _hid((64, 64)), 2) == 0
    rc, msg = _pop_call(lib, _lib, hid=(64, 64), ld=5126)
    need = 2 * 11 * 8 + 5123 * 65 * 4 + 2 * 64 * 64 * 4
    assert rc == E_UNSUPPORTED and str(need).encode() in msg and str(160 * 1024).encode() in msg, msg


def test_exports_and_signatures():
    from modular_rl_amd import _lib
    _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mrl_pop_mlp_num_params", "mrl_pop_rollout_mlp_fits", "mrl_pop_rollout_mlp"):
        assert f" T {name}\n" in nm, name
        assert name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mrl_hip.h")).read()
    for name in ("mrl_pop_mlp_num_params(", "mrl_pop_rollout_mlp_fits(", "mrl_pop_rollout_mlp("):
        assert name in hdr


def test_run_cem_help_still_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_cem.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--hid_sizes" in r.stdout and "--extra_std" in r.stdout
