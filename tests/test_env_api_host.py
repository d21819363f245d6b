"""The stand-alone env stepper / obs filter boundary without a GPU: argument checks of
mrl_env_reset, mrl_env_step and mrl_obfilter_update_apply (every invalid case returns
MRL_E_ARG with a message, before any HIP call), the workspace query, the ctypes layout
of mrl_env_io, and VecEnv's host-side errors."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def _lib_and_args():
    from modular_rl_amd import _lib
    lib = _lib.load()
    # non-null dummies: the checks run before any HIP call, nothing is dereferenced on the device
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    desc = _lib.RolloutDesc(_lib.ENV_HOPPER, 4, 1, 1000, 0, 0, 0, 0, 0)
    bufs = _lib.RolloutBufs(env_state=p, env_int=p)
    io = _lib.EnvIO(p, None, p, p, p, p, None)
    return _lib, lib, p, desc, bufs, io


def _expect_arg_error(lib, rc, needle):
    assert rc == E_ARG, (rc, needle)
    msg = lib.mrl_last_error().decode()
    assert msg and needle in msg, (msg, needle)


def _copy(s, **kw):
    c = type(s)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(s), ctypes.sizeof(s))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("entry", ["mrl_env_reset", "mrl_env_step"])
def test_env_entries_reject_bad_arguments(entry):
    _lib, lib, p, desc, bufs, io = _lib_and_args()
    fn = getattr(lib, entry)
    tail = (None,) if entry == "mrl_env_reset" else (1, None)
    by = ctypes.byref

    def call(d, b, i):
        return fn(d, b, i, *tail)

    _expect_arg_error(lib, call(None, by(bufs), by(io)), "desc")
    _expect_arg_error(lib, call(by(desc), None, by(io)), "bufs")
    _expect_arg_error(lib, call(by(desc), by(bufs), None), "io")
    _expect_arg_error(lib, call(by(_copy(desc, n_envs=0)), by(bufs), by(io)), "n_envs")
    _expect_arg_error(lib, call(by(_copy(desc, n_envs=-3)), by(bufs), by(io)), "n_envs")
    _expect_arg_error(lib, call(by(_copy(desc, env_id=3)), by(bufs), by(io)), "env_id")
    _expect_arg_error(lib, call(by(_copy(desc, env_id=-1)), by(bufs), by(io)), "env_id")
    _expect_arg_error(lib, call(by(desc), by(_copy(bufs, env_state=None)), by(io)), "env_state")
    _expect_arg_error(lib, call(by(desc), by(_copy(bufs, env_int=None)), by(io)), "env_int")
    _expect_arg_error(lib, call(by(desc), by(bufs), by(_copy(io, obs=None))), "obs")
    if entry == "mrl_env_step":
        for f in ("act", "rew", "flags", "ep_t"):
            _expect_arg_error(lib, call(by(desc), by(bufs), by(_copy(io, **{f: None}))), f)


def test_obfilter_rejects_bad_arguments():
    _lib, lib, p, *_ = _lib_and_args()
    fn = lib.mrl_obfilter_update_apply
    good = dict(state=p, dim=11, x=p, n_rows=4, update=1, clip=5.0, out=p, workspace=p)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["state"], a["dim"], a["x"], a["n_rows"], a["update"], a["clip"], a["out"], a["workspace"], None)

    _expect_arg_error(lib, call(state=None), "state")
    _expect_arg_error(lib, call(dim=0), "dim")
    _expect_arg_error(lib, call(dim=-4), "dim")
    _expect_arg_error(lib, call(x=None), "x")
    _expect_arg_error(lib, call(n_rows=0), "n_rows")
    _expect_arg_error(lib, call(n_rows=-1), "n_rows")
    _expect_arg_error(lib, call(out=None), "out")
    assert lib.mrl_obfilter_workspace_bytes(4, 11) > 0  # the query says it needs one
    _expect_arg_error(lib, call(workspace=None), "workspace")
    _expect_arg_error(lib, call(workspace=None, update=0), "workspace")


@pytest.mark.parametrize("dim", [4, 11, 376])
def test_obfilter_workspace_query(dim):
    _, lib, *_ = _lib_and_args()
    prev = 0
    for n in (1, 7, 63, 64, 65, 130, 1024, 4096, 1 << 20):
        b = lib.mrl_obfilter_workspace_bytes(n, dim)
        assert b > 0 and b >= prev, (n, dim, b, prev)
        prev = b
    assert lib.mrl_obfilter_workspace_bytes(65, dim) > lib.mrl_obfilter_workspace_bytes(64, dim)
    for n, d in ((0, dim), (-5, dim), (64, 0), (64, -1)):
        assert lib.mrl_obfilter_workspace_bytes(n, d) <= 0


def test_env_io_layout_matches_c(tmp_path):
    from modular_rl_amd import _lib
    fields = [f for f, _ in _lib.EnvIO._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mrl_hip.h"
#define P(F) printf(#F " %zu\\n", offsetof(mrl_env_io, F));
int main(void) {
  printf("sizeof %zu\\n", sizeof(mrl_env_io));
  """ + " ".join(f"P({f})" for f in fields) + """
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    out = dict(l.rsplit(" ", 1) for l in lines if l)
    assert fields == ["act", "mask", "obs", "rew", "flags", "ep_t", "final_obs"]
    assert int(out["sizeof"]) == ctypes.sizeof(_lib.EnvIO)
    for f in fields:
        assert int(out[f]) == getattr(_lib.EnvIO, f).offset, f


def test_vecenv_unknown_env_is_a_value_error():
    from modular_rl_amd.envs import VecEnv
    with pytest.raises(ValueError):
        VecEnv("nope", 4)


def test_vecenv_without_gpu_raises_mrl_error(monkeypatch):
    from modular_rl_amd import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # the refusal itself, on any machine
    from modular_rl_amd.envs import VecEnv, make
    from modular_rl_amd.filters import BatchZFilter
    with pytest.raises(_lib.MrlError):
        VecEnv("CartPole-v0", 4)
    with pytest.raises(_lib.MrlError):
        make("CartPole-v0").reset()
    with pytest.raises(_lib.MrlError):
        BatchZFilter(4, 4)
