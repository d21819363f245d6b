"""The wave-per-candidate population rollout (mrl_pop_rollout_wave) without a GPU: the
parameter count and the shape predicate of the C ABI, the argument checks before any launch,
the exports, the command line, and the float64 twin of the forward at Humanoid's dims."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

from tests import cem_humanoid_np, cem_np, pop_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -2
PREFIX = b"mrl_pop_rollout_wave:"


_hid = pop_cases.hid_array


def test_num_params_at_humanoid_dims():
    from modular_rl_amd import _lib
    lib = _lib.load()
    assert lib.mrl_pop_mlp_num_params(_lib.ENV_HUMANOID, _hid((10, 5)), 2) == 3944
    assert cem_humanoid_np.num_params((10, 5)) == 3944
    for hid in ((), (64, 64), (7, 3, 5)):
        assert lib.mrl_pop_mlp_num_params(_lib.ENV_HUMANOID, _hid(hid), len(hid)) == cem_humanoid_np.num_params(hid)


def test_wave_fits():
    from modular_rl_amd import _lib
    lib = _lib.load()
    HM, HOP = _lib.ENV_HUMANOID, _lib.ENV_HOPPER
    for hid in ((), (10, 5), (64, 64), (7, 3, 5)):
        assert lib.mrl_pop_rollout_wave_fits(HM, _hid(hid), len(hid)) == 1, hid
    assert lib.mrl_pop_rollout_wave_fits(HM, None, 0) == 1
    assert lib.mrl_pop_rollout_wave_fits(HOP, _hid((10, 5)), 2) == 0
    for hid in ((65,), (4, 4, 4, 4), (10, 0)):
        assert lib.mrl_pop_rollout_wave_fits(HM, _hid(hid), len(hid)) == 0, hid
    assert lib.mrl_pop_rollout_wave_fits(3, _hid((10, 5)), 2) == E_ARG  # 3 is not an env
    assert b"mrl_pop_rollout_wave_fits" in lib.mrl_last_error()
    assert lib.mrl_pop_rollout_wave_fits(HM, _hid((10, 5)), -1) == E_ARG
    assert lib.mrl_pop_rollout_wave_fits(HM, None, 2) == E_ARG
    assert b"mrl_pop_rollout_wave_fits" in lib.mrl_last_error()
    # the existing entry points go on refusing Humanoid
    assert lib.mrl_pop_rollout_mlp_fits(HM, _hid((10, 5)), 2) == 0


_wave_call = functools.partial(pop_cases.pop_call, entry="mrl_pop_rollout_wave")


def test_pop_rollout_wave_argument_checks():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for null in ("d", "b", "thetas", "io"):
        rc, msg = _wave_call(lib, _lib, null=(null,))
        assert rc == E_ARG and msg.startswith(PREFIX), null
    cases = [dict(n_envs=0), dict(n_envs=-3), dict(bufs=False), dict(ld=3943), dict(ld=-1), dict(io_kw=dict(ret=None)),
             dict(io_kw=dict(len=None)), dict(io_kw=dict(flags=None)), dict(io_kw=dict(stat=None)),
             dict(io_kw=dict(trace_steps=4)),                                       # steps without buffers
             dict(io_kw=dict(trace_steps=4, trace_obs=fake, trace_act=fake)),       # no trace_rew
             dict(io_kw=dict(trace_obs=fake, trace_act=fake, trace_rew=fake)),      # no trace_steps
             dict(io_kw=dict(trace_steps=-1)),
             dict(n_hid=-1), dict(null_hid=True, n_hid=2),
             dict(env=3),
             dict(hid=(64, 64), ld=3944)]  # the 64-64 net has 29,393 parameters
    for kw in cases:
        rc, msg = _wave_call(lib, _lib, **kw)
        assert rc == E_ARG and msg.startswith(PREFIX), (kw, rc, msg)
    unsupported = [dict(env=_lib.ENV_HOPPER), dict(env=_lib.ENV_CARTPOLE), dict(hid=(64, 64, 64, 64)), dict(hid=(65,)),
                   dict(hid=(10, 0)), dict(hid=(10, -2))]
    for kw in unsupported:
        rc, msg = _wave_call(lib, _lib, **kw)
        assert rc == E_UNSUPPORTED and msg.startswith(PREFIX), (kw, rc, msg)


def test_exports_and_signatures():
    from modular_rl_amd import _lib
    _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "mrl_hip.h")).read()
    for name in ("mrl_pop_rollout_wave_fits", "mrl_pop_rollout_wave"):
        assert f" T {name}\n" in nm, name
        assert name in _lib.SIGNATURES
        assert name + "(" in hdr


def test_run_cem_help_still_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_cem.py"), "--env", "Humanoid-v2", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--hid_sizes" in r.stdout and "--extra_std" in r.stdout and "--batch_size" in r.stdout


def test_float64_twin_at_humanoid_dims():
    """cem_np.forward takes [376, ..., 17] as it is: against the layers written out, and
    the error bound is positive, finite and grows with c."""
    rng = np.random.default_rng(0)
    for hid in ((10, 5), (), (7, 3, 5)):
        dims = cem_humanoid_np.dims_of(hid)
        assert dims[0] == 376 and dims[-1] == 17
        P = cem_humanoid_np.num_params(hid)
        th = rng.standard_normal((3, P)) * 0.1
        x = np.clip(rng.standard_normal((3, 376)) * 3, -5, 5)
        z = cem_humanoid_np.forward(th, x, dims)
        for i in range(3):
            h, o = x[i], 0
            for l, (r, c) in enumerate(zip(dims[:-1], dims[1:])):
                W, b = th[i, o:o + r * c].reshape(r, c), th[i, o + r * c:o + r * c + c]
                o += r * c + c
                h = h @ W + b if l == len(dims) - 2 else np.tanh(h @ W + b)
            assert o + 17 == P
            assert np.array_equal(z[i], h)
        z1, t1 = cem_humanoid_np.forward_with_bound(th, x, dims, 1)
        z2, t2 = cem_humanoid_np.forward_with_bound(th, x, dims, 2)
        assert np.array_equal(z1, z) and np.array_equal(z2, z)
        assert np.all(t1 > 0) and np.all(np.isfinite(t2)) and np.all(t2 > t1)
        # an f32 forward in plain ascending order stays inside the bound
        h = x.astype(np.float32)
        zf = np.zeros((3, 17), dtype=np.float32)
        for i in range(3):
            v, o = h[i], 0
            for l, (r, c) in enumerate(zip(dims[:-1], dims[1:])):
                W = th[i, o:o + r * c].reshape(r, c).astype(np.float32)
                b = th[i, o + r * c:o + r * c + c].astype(np.float32)
                o += r * c + c
                acc = np.zeros(c, dtype=np.float32)
                for k in range(r):
                    acc = (acc + v[k] * W[k]).astype(np.float32)
                v = acc + b if l == len(dims) - 2 else np.tanh(acc + b).astype(np.float32)
            zf[i] = v
        z32, tol = cem_humanoid_np.forward_with_bound(th.astype(np.float32), h, dims, 2)
        assert np.all(np.abs(zf - z32) <= tol)
        assert cem_np.num_params(dims, True) == P
