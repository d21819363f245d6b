"""The population rollouts' test harness (helper, not collected): one traced run, one replay
check, the two action checks and the failing C call, shared by the tests of the three entry
points -- mrl_pop_rollout (64-64), mrl_pop_rollout_mlp (small nets), mrl_pop_rollout_wave
(Humanoid-v2)."""
import ctypes

import numpy as np

from tests import cem_np

KEYS = ("ret", "len", "flags", "stat", "trace_obs", "trace_act", "trace_rew")
# check_actions_bound's tolerance is cem_humanoid_np.forward_with_bound's: per output the f32
# accumulation bound c (din + 2) u (sum |x W| + |b|), u = 2^-24, carried through the layers.
# c = 1 is the first-order bound of din products, din - 1 sums and the bias in any order; c = 2
# covers what first order leaves out -- gamma_n = n u / (1 - n u) against n u, the products of
# an input's error with a rounding error -- and the float64 twin's own rounding (2^-53 per
# operation), all far below one more first-order term.
C_BOUND = 2


def run_traced(env_id, hid, n, seed, limit, thetas, filter_state=None, shared=False, cls=None):
    """One traced call of the rollout that serves (env_id, hid) -- envs.population_rollout, or
    the class a test names: (outputs as numpy copies, the rollout object)."""
    import torch
    from modular_rl_amd.envs import population_rollout
    pop = (cls or population_rollout)(env_id, n, seed=seed, timestep_limit=limit, hid_sizes=hid)
    th = torch.as_tensor(thetas).cuda()
    out = (pop.evaluate if shared else pop)(th, filter_state=filter_state, trace_steps=pop.limit)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}, pop


def traced_rows(out, most=400):
    """The first `most` raw observation rows of a traced run, in (step, env) order."""
    L = out["len"]
    return np.concatenate([out["trace_obs"][t][L > t] for t in range(int(L.max()))])[:most]


def filter_state_for(env_id, rows):
    """A BatchZFilter state after a few hundred traced observation rows (n >= 2)."""
    import torch
    from modular_rl_amd.filters import BatchZFilter
    f = BatchZFilter(cem_np.ENVS[env_id][0], len(rows))
    f(torch.as_tensor(rows).cuda(), update=True)
    torch.cuda.synchronize()
    assert f.n >= 2
    return f.state.clone()


def check_replay(env_id, n, seed, out, limit):
    """The traced actions through a VecEnv (same seed, no auto-reset) give the traced raw
    observations and rewards bit for bit, the same length and terminated bit; ret is the
    fp64 step-order sum of the traced rewards; stat is the Welford partial of the rows."""
    import torch
    from modular_rl_amd.envs import VecEnv
    O = cem_np.ENVS[env_id][0]
    env = VecEnv(env_id, n, seed=seed, auto_reset=False)
    obs = env.reset().cpu().numpy().copy()
    L = out["len"]
    assert L.min() >= 1 and L.max() <= limit
    alive = np.ones(n, dtype=bool)
    ret = [0.0] * n
    for t in range(int(L.max())):
        assert np.array_equal(obs[alive], out["trace_obs"][t][alive]), t
        ob, rew, done, info = env.step(torch.as_tensor(out["trace_act"][t]).cuda())
        obs, rew = ob.cpu().numpy().copy(), rew.cpu().numpy()
        term = info["terminated"].cpu().numpy()
        assert np.array_equal(rew[alive], out["trace_rew"][t][alive]), t
        for i in np.nonzero(alive)[0]:
            ret[i] += float(out["trace_rew"][t][i])
            ended = term[i] or t + 1 >= limit
            assert ended == (L[i] == t + 1), (t, i)
            if ended:
                assert bool(out["flags"][i] & 2) == bool(term[i]), (t, i)
                alive[i] = False
    assert not alive.any()
    assert np.array_equal(np.array(ret), out["ret"])
    assert np.all(out["flags"] & 1)
    for i in range(n):
        rows = out["trace_obs"][:L[i], i]
        want = cem_np.welford_partial(rows)
        # A column that is exactly constant over the episode (Humanoid's body masses in cinert,
        # the world body's zeros; any column of a one-step episode): its exact partial is known
        # -- mean the value, M2 0 -- and Welford's recurrence gives exactly that (dlt = 0 from
        # the second row on), while the two-pass twin rounds the mean of n equal values and
        # returns M2 ~ 1e-28 for 0, which no rtol with atol 0 takes.  Those entries are held to
        # the exact value, bit for bit; every other entry to the two-pass twin at rtol 1e-9.
        const = np.ptp(rows, axis=0) == 0
        want[1:1 + O][const] = rows[0][const]
        want[1 + O:][const] = 0.0
        assert np.array_equal(out["stat"][i][1:1 + O][const], rows[0][const]), i
        assert not out["stat"][i][1 + O:][const].any(), i
        np.testing.assert_allclose(out["stat"][i], want, rtol=1e-9, atol=0, err_msg=str(i))
        assert out["stat"][i].shape == (1 + 2 * O,)


def _live_rows(env_id, hid, thetas, out, filter_state):
    """Per step: (t, live envs, their float64 thetas, their filtered f32-rounded observations)."""
    fs = None if filter_state is None else filter_state.cpu().numpy()
    L = out["len"]
    th64 = np.asarray(thetas, dtype=np.float64)
    for t in range(int(L.max())):
        live = np.nonzero(L > t)[0]
        yield t, live, (th64[live] if th64.ndim == 2 else th64), cem_np.filter_obs(out["trace_obs"][t][live], fs)


def check_actions(env_id, hid, thetas, out, filter_state):
    """The lane kernels' form: every traced (raw obs, action) pair against the float64 forward
    at rtol 1e-4 / atol 1e-5; a discrete action wherever the top two logits are 1e-4 apart,
    with at most 1 % of the rows skipped."""
    gauss = cem_np.ENVS[env_id][2]
    dims = cem_np.dims_of(env_id, hid)
    rows, skipped = 0, 0
    for t, live, th, x in _live_rows(env_id, hid, thetas, out, filter_state):
        z = cem_np.forward(th, x, dims)
        rows += len(live)
        if gauss:
            np.testing.assert_allclose(out["trace_act"][t][live], z, rtol=1e-4, atol=1e-5, err_msg=str(t))
        else:
            srt = np.sort(z, axis=1)
            clear = (srt[:, -1] - srt[:, -2]) >= 1e-4
            skipped += int((~clear).sum())
            assert np.array_equal(out["trace_act"][t][live][clear], np.argmax(z, axis=1)[clear]), t
    print(env_id, list(hid), "filtered" if filter_state is not None else "raw", "rows", rows,
          "skipped (top-two logits closer than 1e-4)", skipped)
    assert skipped <= 0.01 * rows
    return rows, skipped


def check_actions_bound(env_id, hid, thetas, out, filter_state):
    """The derived-bound form: every traced (raw obs, action) row against the float64 forward,
    within cem_humanoid_np.forward_with_bound at C_BOUND."""
    from tests import cem_humanoid_np
    dims = cem_np.dims_of(env_id, hid)
    rows, worst = 0, 0.0
    for t, live, th, x in _live_rows(env_id, hid, thetas, out, filter_state):
        z, tol = cem_humanoid_np.forward_with_bound(th, x, dims, C_BOUND)
        err = np.abs(out["trace_act"][t][live].astype(np.float64) - z)
        rows += len(live)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (t, float((err / tol).max()))
    print(env_id, list(hid), "filtered" if filter_state is not None else "raw", "rows", rows, "worst error / bound",
          worst)
    return rows


def hid_array(hid):
    return (ctypes.c_int32 * max(len(hid), 1))(*hid)


# entry point -> (default env, default ld_theta: the parameter count of the default net there)
ENTRIES = {"mrl_pop_rollout": ("ENV_HOPPER", 5126), "mrl_pop_rollout_mlp": ("ENV_HOPPER", 196),
           "mrl_pop_rollout_wave": ("ENV_HUMANOID", 3944)}


def pop_call(lib, _lib, entry, env=None, n_envs=4, pol=None, hid=(10, 5), n_hid=None, null_hid=False, ld=None,
             null=(), io_kw=None, bufs=True):
    """One of the three entry points with fake non-null pointers (never dereferenced: every
    check precedes the launch, and every case the tests build fails a check): (return code,
    mrl_last_error()).  `pol` goes to mrl_pop_rollout, `hid` / `n_hid` / `null_hid` to the
    other two; `null` names the pointer arguments passed as NULL."""
    env_name, ld_default = ENTRIES[entry]
    env = getattr(_lib, env_name) if env is None else env
    fake = ctypes.c_void_p(0x1000)
    d = _lib.RolloutDesc(env, n_envs, 1, 0, 0, 0, 0, 0, 0)
    b = _lib.RolloutBufs(env_state=fake if bufs else None, env_int=fake)
    pol = pol or _lib.MlpDesc(11, 3, _lib.HEAD_GAUSS, 64, 2)
    io = _lib.PopIO(fake, fake, fake, fake)
    for k, v in (io_kw or {}).items():
        setattr(io, k, v)
    args = dict(d=ctypes.byref(d), b=ctypes.byref(b), pol=ctypes.byref(pol), thetas=fake, io=ctypes.byref(io))
    for k in null:
        args[k] = None
    if entry == "mrl_pop_rollout":
        net = (args["pol"],)
    else:
        net = (None if null_hid else hid_array(hid), len(hid) if n_hid is None else n_hid)
    rc = getattr(lib, entry)(args["d"], args["b"], *net, args["thetas"], ld_default if ld is None else ld, None,
                             args["io"], None)
    return rc, lib.mrl_last_error()
