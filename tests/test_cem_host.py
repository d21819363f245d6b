"""The cross-entropy method without a GPU: the float64 twin against the reference's own
generator (golden), the option table, the C ABI of the new entry points (layout, exports,
argument checks before any launch) and the command line."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cem_np, pop_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cem.npz")
E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_twin_reproduces_the_reference_generator(golden, tag):
    g = {k[2:]: v for k, v in golden.items() if k.startswith(tag + "_")}
    batch, n_iter, elite_frac, initial_std, extra_std, decay = g["cfg"]
    out = cem_np.cem_replay(g["pops"], g["ys"], g["th0"], int(batch), elite_frac, initial_std, extra_std, decay)
    assert len(out) == int(n_iter) == 6
    for it, info in enumerate(out):
        np.testing.assert_allclose(info["th"], g["th"][it], rtol=1e-12, atol=0)
        np.testing.assert_allclose(info["std"], g["std"][it], rtol=1e-12, atol=0)
        np.testing.assert_allclose(info["ymean"], g["ymean"][it], rtol=1e-12, atol=0)
    if tag == "b":  # the extra-std schedule is live for 3 iterations, then off
        assert np.all(g["std"][1] > np.sqrt(0.25 * (1 - 1 / 3.0)) - 1e-12)


def test_options_match_the_reference_table(golden):
    from modular_rl_amd.cem import CEM_OPTIONS, n_elite_of
    assert [o[0] for o in CEM_OPTIONS] == list(golden["option_names"])
    assert [o[1].__name__ for o in CEM_OPTIONS] == list(golden["option_types"])
    np.testing.assert_array_equal([float(o[2]) for o in CEM_OPTIONS], golden["option_defaults"])
    # n_elite = int(np.round(batch * frac)): banker's rounding, as the reference
    assert n_elite_of(200, 0.2) == 40 and cem_np.n_elite_of(200, 0.2) == 40
    assert n_elite_of(25, 0.1) == 2 and cem_np.n_elite_of(25, 0.1) == 2


def test_pop_io_layout_and_exports(tmp_path):
    from modular_rl_amd import _lib
    _lib.load()
    fields = [f[0] for f in _lib.PopIO._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mrl_hip.h\"\nint main(void) {\n"
                     "  printf(\"size %zu\\n\", sizeof(mrl_pop_io));\n"
                     + "".join(f"  printf(\"{f} %zu\\n\", offsetof(mrl_pop_io, {f}));\n" for f in fields)
                     + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines() if l)
    assert int(out["size"]) == ctypes.sizeof(_lib.PopIO)
    for f in fields:
        assert int(out[f]) == getattr(_lib.PopIO, f).offset, f
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mrl_pop_rollout", "mrl_cem_sample", "mrl_cem_refit", "mrl_cem_refit_workspace_bytes"):
        assert f" T {name}\n" in nm, name
        assert name in _lib.SIGNATURES


_pop_call = functools.partial(pop_cases.pop_call, entry="mrl_pop_rollout")


def test_pop_rollout_argument_checks():
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for null in ("d", "b", "pol", "thetas", "io"):
        rc, msg = _pop_call(lib, _lib, null=(null,))
        assert rc == E_ARG and msg, null
    cases = [dict(n_envs=0), dict(n_envs=-3), dict(bufs=False), dict(ld=5125), dict(ld=-1), dict(io_kw=dict(ret=None)),
             dict(io_kw=dict(stat=None)),
             dict(io_kw=dict(trace_steps=4)),                                       # steps without buffers
             dict(io_kw=dict(trace_steps=4, trace_obs=fake, trace_act=fake)),       # no trace_rew
             dict(io_kw=dict(trace_obs=fake, trace_act=fake, trace_rew=fake)),      # no trace_steps
             dict(io_kw=dict(trace_steps=-1))]
    for kw in cases:
        rc, msg = _pop_call(lib, _lib, **kw)
        assert rc == E_ARG and b"mrl_pop_rollout" in msg, kw
    unsupported = [dict(env=_lib.ENV_HUMANOID, pol=_lib.MlpDesc(376, 17, _lib.HEAD_GAUSS, 64, 2)),
                   dict(pol=_lib.MlpDesc(11, 3, _lib.HEAD_GAUSS, 32, 1)),          # hid_sizes=[32]
                   dict(pol=_lib.MlpDesc(11, 3, _lib.HEAD_SOFTMAX, 64, 2)),
                   dict(pol=_lib.MlpDesc(12, 3, _lib.HEAD_GAUSS, 64, 2)),
                   dict(env=_lib.ENV_CARTPOLE)]                                     # Hopper's net on CartPole
    for kw in unsupported:
        rc, msg = _pop_call(lib, _lib, **kw)
        assert rc == E_UNSUPPORTED and b"mrl_pop_rollout" in msg, kw


def test_the_argument_checks_come_in_one_order_on_all_three_entries():
    """Calls with two faults each: the first failed check of the ladder names itself, with the
    entry point's own prefix -- null desc, null bufs, the entry's own check (null policy desc /
    n_hid < 0, null hid_sizes), null thetas, null io, unknown env, n_envs, bufs.env_state /
    env_int, io.ret / len / flags / stat, trace_steps, the partly set trace; then the net's
    shape, then ld_theta."""
    from modular_rl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    POP, MLP, WAVE = "mrl_pop_rollout", "mrl_pop_rollout_mlp", "mrl_pop_rollout_wave"
    partly = "the trace is only partly set (trace_steps, trace_obs, trace_act, trace_rew)"
    for entry in (POP, MLP, WAVE):
        own = dict(null=("b", "pol")) if entry == POP else dict(null=("b",), n_hid=-1)
        rows = [(dict(null=("d", "io")), "null desc"),
                (dict(null=("thetas",), n_envs=0), "null thetas"),
                (own, "null bufs"),
                (dict(io_kw=dict(trace_steps=-1, ret=None)), "null io.ret / len / flags / stat"),
                (dict(io_kw=dict(trace_steps=4, trace_obs=fake), env=3), "desc.env_id: unknown env"),
                (dict(io_kw=dict(trace_steps=4, trace_obs=fake), n_envs=0), "desc.n_envs <= 0"),
                (dict(io_kw=dict(trace_steps=4, trace_obs=fake)), partly),
                (dict(ld=pop_cases.ENTRIES[entry][1] - 1), "ld_theta is neither 0 nor >= the parameter count")]
        for kw, what in rows:
            rc, msg = pop_cases.pop_call(lib, _lib, entry, **kw)
            assert (rc, msg) == (E_ARG, f"{entry}: {what}".encode()), (entry, kw, rc, msg)
    # the entry's own check sits between null bufs and null thetas
    for kw, what in ((dict(null=("pol", "thetas")), "mrl_pop_rollout: null policy desc"),):
        assert pop_cases.pop_call(lib, _lib, POP, **kw) == (E_ARG, what.encode()), kw
    for entry in (MLP, WAVE):
        for kw, what in ((dict(n_hid=-1, null_hid=True, null=("thetas",)), "n_hid < 0"),
                         (dict(n_hid=2, null_hid=True, null=("thetas",)), "null hid_sizes")):
            assert pop_cases.pop_call(lib, _lib, entry, **kw) == (E_ARG, f"{entry}: {what}".encode()), (entry, kw)
    # the shape, after the ladder and before ld_theta: each entry's own env test comes before the widths
    one = [(MLP, dict(env=_lib.ENV_HUMANOID, hid=(65,), ld=1),
            "mrl_pop_rollout_mlp: Humanoid is not supported (the thread-per-env envs only)"),
           (WAVE, dict(env=_lib.ENV_HOPPER, hid=(65,), ld=1), "mrl_pop_rollout_wave: the wave-per-env envs only (Humanoid)"),
           (MLP, dict(hid=(65,), ld=1), "mrl_pop_rollout_mlp: a hidden width outside [1, 64]"),
           (WAVE, dict(hid=(65,), ld=1), "mrl_pop_rollout_wave: a hidden width outside [1, 64]"),
           (MLP, dict(hid=(4, 4, 4, 4), ld=1), "mrl_pop_rollout_mlp: more than 3 hidden layers"),
           (WAVE, dict(hid=(4, 4, 4, 4), ld=1), "mrl_pop_rollout_wave: more than 3 hidden layers"),
           (POP, dict(env=_lib.ENV_HUMANOID, ld=1),
            "mrl_pop_rollout: Humanoid is not supported (the thread-per-env envs only)")]
    for entry, kw, what in one:
        assert pop_cases.pop_call(lib, _lib, entry, **kw) == (E_UNSUPPORTED, what.encode()), (entry, kw)


def test_cem_sample_and_refit_argument_checks():
    from modular_rl_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    sample = lambda mean=f, std=f, P=7, N=5, th=f, ld=7: lib.mrl_cem_sample(mean, std, P, N, 1, 0, th, ld, None)
    for kw in (dict(mean=None), dict(std=None), dict(th=None), dict(P=0), dict(N=0), dict(ld=6)):
        assert sample(**kw) == E_ARG and b"mrl_cem_sample" in lib.mrl_last_error(), kw
    refit = lambda th=f, ld=7, N=5, P=7, ys=f, ne=2, m=f, v=f, idx=f, ws=f: lib.mrl_cem_refit(
        th, ld, N, P, ys, ne, m, v, idx, ws, None)
    for kw in (dict(th=None), dict(ys=None), dict(m=None), dict(v=None), dict(idx=None), dict(ws=None), dict(ld=6),
               dict(N=0), dict(P=0), dict(ne=0), dict(ne=6), dict(ne=-1)):
        assert refit(**kw) == E_ARG and b"mrl_cem_refit" in lib.mrl_last_error(), kw
    assert lib.mrl_cem_refit_workspace_bytes(24, 7) >= 24 * 4
    assert lib.mrl_cem_refit_workspace_bytes(0, 7) == 0


def test_run_cem_help_lists_the_cem_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_cem.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--batch_size", "--n_iter", "--elite_frac", "--initial_std", "--extra_std", "--std_decay_time",
                "--timestep_limit", "--parallel", "--hid_sizes", "--filter", "--env", "--agent"):
        assert opt in r.stdout, opt


@pytest.mark.parametrize("start", [0, 37])
def test_merge_of_candidate_partials_is_the_stat_of_all_rows(start):
    """merge_stat_partials over per-candidate (count, mean, M2) partials, an empty one among
    them, equals the two-pass stat of all rows at once -- from an empty state and on top of
    an earlier one.  Both sides are fp64 over a few hundred rows of O(1) values: rounding is
    ~1e-14 relative on M2 and absolute on the means, so rtol 1e-10 / atol 1e-12 leave margin."""
    from modular_rl_amd.cem import merge_stat_partials
    rng = np.random.default_rng(start)
    O = 4
    chunks = [rng.normal(1.0, 2.0, size=(n, O)) for n in (start, 5, 1, 40, 17, 200) if n]
    state = np.zeros(2 + 2 * (O + 1))
    if start:
        first = cem_np.welford_partial(chunks[0])
        state[0], state[1] = first[0], 9.0
        state[2:2 + O], state[2 + O + 1:2 + O + 1 + O] = first[1:1 + O], first[1 + O:]
        state[2 + O], state[2 + 2 * O + 1] = 0.25, 3.0  # the reward slots stay untouched
    rest = chunks[1:] if start else chunks
    stat = [cem_np.welford_partial(c) for c in rest]
    stat.insert(2, np.zeros(1 + 2 * O))  # a candidate that took no step
    out = merge_stat_partials(state, np.array(stat), O)
    want = cem_np.welford_partial(np.concatenate(chunks))
    assert out[0] == want[0] and out[1] == state[1]
    np.testing.assert_allclose(out[2:2 + O], want[1:1 + O], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out[2 + O + 1:2 + 2 * O + 1], want[1 + O:], rtol=1e-10, atol=1e-12)
    assert out[2 + O] == state[2 + O] and out[2 + 2 * O + 1] == state[2 + 2 * O + 1]
