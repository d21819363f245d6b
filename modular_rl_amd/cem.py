"""Noisy cross-entropy method (`cem.py` of the reference) on the device.

``cem`` keeps the reference generator's arithmetic (`cem.py:10-50`), quirks included:
``n_elite = int(np.round(batch_size * elite_frac))``; ``th_std`` starts as
``ones * initial_std`` and afterwards holds the elite *variance*; ``sample_std =
sqrt(th_std + extra_std**2 * max(1 - it / std_decay_time, 0))``.  What changes is where it
runs: the population is drawn by ``mrl_cem_sample`` (Philox, domain 2, one stream per
candidate and generation) instead of ``np.random.randn``, the objective ``f`` is *batched*
-- it takes the whole device ``[N, P]`` population and returns the ``[N]`` returns -- and the
elite mean / variance come from ``mrl_cem_refit``.  The population never leaves the device;
the host sees ``ys`` and the two ``[P]`` vectors per generation.

``run_cem_algorithm`` is the reference's driver (`cem.py:73-97`) with a
``PopulationRollout`` as the objective: every candidate's episode runs in one launch
(``mrl_pop_rollout`` for the 64-64 net, ``mrl_pop_rollout_mlp`` for the agent's other
``hid_sizes``, the reference battery's 10,5 among them; ``mrl_pop_rollout_wave``, a wave per
candidate, on Humanoid-v2 -- ``envs.population_rollout`` picks).  Observation filter: the reference pushes every observation of every
candidate into one shared ``ZFilter`` in serial order (with ``parallel=1`` each worker
updates a private copy that is never merged).  Here the filter is *frozen* during a
generation -- all candidates of a generation see the same normalisation -- and the
candidates' Welford partials are Chan-merged into it, in candidate order, after the
generation; the first generation (empty filter) runs on raw observations clipped to +-5.
"""
import numpy as np
import torch

from . import _lib
from .misc_utils import update_default_config

CEM_OPTIONS = [
    ("batch_size", int, 200, "Number of episodes per batch"),
    ("n_iter", int, 200, "Number of iterations"),
    ("elite_frac", float, 0.2, "fraction of parameter settings used to fit pop"),
    ("initial_std", float, 1.0, "initial standard deviation for parameters"),
    ("extra_std", float, 0.0, "extra stdev added"),
    ("std_decay_time", float, -1.0, "number of timesteps that extra stdev decays over. negative => n_iter/2"),
    ("timestep_limit", int, 0, "maximum length of trajectories"),
    ("parallel", int, 0, "collect trajectories in parallel (accepted and ignored: the population runs on the device)"),
]


def n_elite_of(batch_size, elite_frac):
    return int(np.round(batch_size * elite_frac))  # cem.py:32 (banker's rounding)


def sample_std_of(th_std, extra_std, iteration, std_decay_time):
    extra_var_multiplier = max((1.0 - iteration / float(std_decay_time)), 0)  # cem.py:38
    return np.sqrt(th_std + np.square(extra_std) * extra_var_multiplier)      # cem.py:40


def sample_population(th_mean, sample_std, n, seed, generation, out=None, device="cuda"):
    """``[n, P]`` float32 device population of one generation (``mrl_cem_sample``)."""
    dev = torch.device(device)
    mean = torch.as_tensor(np.asarray(th_mean, dtype=np.float64)).to(dev)
    std = torch.as_tensor(np.asarray(sample_std, dtype=np.float64)).to(dev)
    P = mean.numel()
    if out is None:
        out = torch.empty(int(n), P, dtype=torch.float32, device=dev)
    _lib.call("mrl_cem_sample", _lib.ptr(mean), _lib.ptr(std), P, int(n), int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(generation), _lib.ptr(out), P, _lib.stream())
    return out


def refit(thetas, ys, n_elite):
    """Elite mean, variance (ddof 0) and indices of a device population (``mrl_cem_refit``):
    ``(mean [P], var [P], elite_idx [n_elite])`` as float64 / int32 device tensors."""
    lib = _lib.load(require_gpu=True)
    N, P = thetas.shape
    dev = thetas.device
    ys = torch.as_tensor(ys, dtype=torch.float64).to(dev).contiguous()
    mean = torch.empty(P, dtype=torch.float64, device=dev)
    var = torch.empty(P, dtype=torch.float64, device=dev)
    idx = torch.empty(max(int(n_elite), 1), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.mrl_cem_refit_workspace_bytes(N, P)), 4) // 4, dtype=torch.int32, device=dev)
    _lib.call("mrl_cem_refit", _lib.ptr(thetas), int(thetas.stride(0)), N, P, _lib.ptr(ys), int(n_elite),
              _lib.ptr(mean), _lib.ptr(var), _lib.ptr(idx), _lib.ptr(ws), _lib.stream())
    return mean, var, idx


def cem(f, th_mean, batch_size, n_iter, elite_frac, initial_std=1.0, extra_std=0.0, std_decay_time=1.0, seed=0,
        thetas=None):
    """Noisy cross-entropy method (`cem.py:10-50`): yields ``{"ys", "th", "ymean", "std"}``
    per iteration.  ``f``: the batched objective, device ``[N, P]`` float32 -> ``[N]``.
    ``thetas``: optional sequence of per-generation populations used instead of sampling."""
    n_elite = n_elite_of(batch_size, elite_frac)
    th_mean = np.asarray(th_mean, dtype=np.float64)
    th_std = np.ones(th_mean.size) * initial_std
    pop = None
    for iteration in range(n_iter):
        sample_std = sample_std_of(th_std, extra_std, iteration, std_decay_time)
        if thetas is not None:
            pop = torch.as_tensor(np.asarray(thetas[iteration]), dtype=torch.float32).to("cuda").contiguous()
        else:
            pop = sample_population(th_mean, sample_std, batch_size, seed, iteration, out=pop)
        ys_dev = torch.as_tensor(f(pop), dtype=torch.float64).to(pop.device).reshape(-1)
        assert ys_dev.shape == (pop.shape[0],)
        mean, var, _ = refit(pop, ys_dev, n_elite)
        ys = ys_dev.cpu().numpy()
        th_mean = mean.cpu().numpy()
        th_std = var.cpu().numpy()
        yield {"ys": ys, "th": th_mean, "ymean": ys.mean(), "std": sample_std}


def merge_stat_partials(state, stat, obs_dim):
    """Chan-merge the per-candidate Welford partials ``stat [N, 1 + 2 obs_dim]`` (count,
    mean, M2) into a ZFilter ``state`` (n_obs, n_rew, M[obs_dim + 1], S[obs_dim + 1]) in
    candidate order; float64 numpy, returns the new state."""
    st = np.array(state, dtype=np.float64, copy=True)
    O, D = int(obs_dim), int(obs_dim) + 1
    n, M, S = st[0], st[2:2 + O].copy(), st[2 + D:2 + D + O].copy()
    for row in np.asarray(stat, dtype=np.float64):
        nb, mb, m2b = row[0], row[1:1 + O], row[1 + O:1 + 2 * O]
        if nb <= 0:
            continue
        nn = n + nb
        delta = mb - M
        newM = M + (delta * nb) / nn
        S = S + m2b + delta * (mb - newM) * nb
        M, n = newM, nn
    st[0], st[2:2 + O], st[2 + D:2 + D + O] = n, M, S
    return st


def run_cem_algorithm(env, agent, usercfg=None, callback=None):
    """`cem.py:73-97`: CEM over the agent's flat parameters with whole-episode returns."""
    from .envs import population_rollout
    cfg = update_default_config(CEM_OPTIONS, usercfg)
    cfg.update(usercfg or {})
    # after the merge: a command line always carries the option's own default (-1.0), and the
    # reference's order (cem.py:75-76) lets that overwrite n_iter / 2 again, so its extra
    # variance grows by the generation instead of decaying
    if cfg["std_decay_time"] < 0:
        cfg["std_decay_time"] = cfg["n_iter"] / 2
    print("cem config", {k: cfg[k] for k in sorted(cfg) if np.ndim(cfg[k]) == 0 or isinstance(cfg[k], (list, str))})
    seed = int(cfg.get("seed", 0) or 0)
    hid = tuple(getattr(getattr(agent.policy, "net", None), "hid_sizes", None) or (64, 64))
    pop = population_rollout(env, cfg["batch_size"], seed=seed, timestep_limit=cfg["timestep_limit"] or None,
                             hid_sizes=hid)
    if pop.P != agent.get_flat().size:
        raise _lib.MrlError(f"run_cem_algorithm: the agent's {agent.get_flat().size} parameters are not the "
                            f"{pop.P} of the env's tanh MLP with hid_sizes={list(hid)}")
    use_filter = agent.filter_state is not None

    def objective(thetas):
        out = pop(thetas, filter_state=agent.filter_state if use_filter else None)
        objective.last = out
        return out["ret"]

    th_mean = agent.get_flat()
    for info in cem(objective, th_mean, cfg["batch_size"], cfg["n_iter"], cfg["elite_frac"], cfg["initial_std"],
                    cfg["extra_std"], cfg["std_decay_time"], seed=seed):
        out = objective.last
        info["len"] = out["len"].cpu().numpy()
        if use_filter:
            merged = merge_stat_partials(agent.filter_state.cpu().numpy(), out["stat"].cpu().numpy(), env.obs_dim)
            agent.filter_state.copy_(torch.as_tensor(merged))
        agent.set_from_flat(info["th"])
        if callback is not None:
            callback(info)
        ps = np.linspace(0, 100, 5)
        rows = [ps, np.percentile(info["ys"].ravel(), ps), np.percentile(info["std"].ravel(), ps)]
        print("\n".join("  ".join("%12.5g" % v for v in r) for r in rows))
