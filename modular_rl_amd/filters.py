"""Running-stat filters (`filters.py` / `running_stat.py` of the reference).

The agent's ZFilter state lives on the device in the collector's ``filter_state``
(n, mean, M2 in fp64; obs dims then the reward), updated inside the fused rollout
kernel.  ``DeviceZFilter`` is the agent-facing view of that state with the
reference's ``ZFilter`` call semantics for single observations
(`filters.py:30-38`: push, then (x - mean)/(std + 1e-8), clip) -- a host-side
convenience for the per-observation API, not part of the batched hot path.
"""
import numpy as np
import torch


class BatchZFilter:
    """The reference's ``ZFilter`` (filters.py:17-40) over batches of observation rows on
    the device (``mrl_obfilter_update_apply``), in the rollout's own arithmetic: the rows
    of a call are pushed as one Chan merge, then normalised and clipped.

    ``f(obs, update=True)`` takes float64 ``[n, obs_dim]`` rows (``n <= n_rows``, e.g.
    ``VecEnv.obs``) and returns float32 ``[n, obs_dim]``; the returned tensor belongs to the
    filter and is overwritten by the next call.  ``state`` starts the running stat from a
    Collector's ``filter_state[:FS]`` (cloned, so a trained agent is evaluated with
    ``update=False`` without disturbing its filter).
    """

    def __init__(self, obs_dim, n_rows, clip=5.0, state=None, device="cuda"):
        from . import _lib
        lib = _lib.load(require_gpu=True)
        self.obs_dim, self.n_rows, self.clip = int(obs_dim), int(n_rows), float(clip)
        if self.obs_dim <= 0 or self.n_rows <= 0:
            raise ValueError("obs_dim and n_rows must be positive")
        dev = torch.device(device)
        FS = 2 + 2 * (self.obs_dim + 1)  # n_obs, n_rew, M[obs_dim + 1], S[obs_dim + 1]
        if state is None:
            self.state = torch.zeros(FS, dtype=torch.float64, device=dev)
        else:
            self.state = torch.as_tensor(state, dtype=torch.float64).to(dev).clone().contiguous()
            if tuple(self.state.shape) != (FS,):
                raise ValueError(f"state must hold {FS} doubles (n_obs, n_rew, M, S), got {tuple(self.state.shape)}")
        nbytes = int(lib.mrl_obfilter_workspace_bytes(self.n_rows, self.obs_dim))
        if nbytes <= 0:
            raise ValueError("obs_dim / n_rows out of range")
        self._ws = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        self._out = torch.zeros(self.n_rows, self.obs_dim, dtype=torch.float32, device=dev)

    def __call__(self, obs, update=True):
        from . import _lib
        x = torch.as_tensor(obs, dtype=torch.float64).to(self.state.device).contiguous()
        if x.dim() != 2 or x.shape[1] != self.obs_dim or not 0 < x.shape[0] <= self.n_rows:
            raise ValueError(f"obs must be [n <= {self.n_rows}, {self.obs_dim}], got {tuple(x.shape)}")
        out = self._out[:x.shape[0]]
        _lib.call("mrl_obfilter_update_apply", _lib.ptr(self.state), self.obs_dim, _lib.ptr(x), int(x.shape[0]),
                  int(bool(update)), self.clip, _lib.ptr(out), _lib.ptr(self._ws), _lib.stream())
        return out

    @property
    def n(self):
        return float(self.state[0])

    @property
    def mean(self):
        return self.state[2:2 + self.obs_dim].cpu().numpy()

    @property
    def var(self):
        n, D = self.n, self.obs_dim + 1
        M, S = self.mean, self.state[2 + D:2 + D + self.obs_dim].cpu().numpy()
        return S / (n - 1) if n > 1 else np.square(M)

    @property
    def std(self):
        return np.sqrt(self.var)


class DeviceZFilter:
    def __init__(self, agent, which, demean=True, destd=True, clip=10.0):
        self.agent, self.which = agent, which
        self.demean, self.destd, self.clip = demean, destd, clip

    def _state(self):
        col = self.agent._filter_owner()
        if col is None:
            raise RuntimeError("the filter state is created with the agent's first collector (make_collector)")
        return col

    @property
    def rs(self):
        return self

    @property
    def n(self):
        (n, _, _), (nr, _, _) = self._state().filter_stats()
        return n if self.which == "obs" else nr

    @property
    def mean(self):
        (_, m, _), (_, mr, _) = self._state().filter_stats()
        return m if self.which == "obs" else mr

    @property
    def var(self):
        (_, _, v), (_, _, vr) = self._state().filter_stats()
        return v if self.which == "obs" else vr

    @property
    def std(self):
        return np.sqrt(self.var)

    def __call__(self, x, update=True):
        col = self._state()
        fs = col.filter_state[:col.FS].cpu().numpy()
        D = (col.FS - 2) // 2
        cols = list(range(D - 1)) if self.which == "obs" else [D - 1]
        ci = 0 if self.which == "obs" else 1
        x = np.asarray(x, dtype=np.float64)
        if update:  # RunningStat.push (running_stat.py:10-20)
            n = fs[ci] + 1
            M, S = fs[2:2 + D][cols], fs[2 + D:2 + 2 * D][cols]
            if n == 1:
                M = np.array(x, dtype=np.float64).reshape(M.shape)
            else:
                old = M.copy()
                M = old + (x.reshape(M.shape) - old) / n
                S = S + (x.reshape(M.shape) - old) * (x.reshape(M.shape) - M)
            fs[ci] = n
            fs[2:2 + D][cols] = M
            fs[2 + D:2 + 2 * D][cols] = S
            col.filter_state[:col.FS].copy_(torch.as_tensor(fs))
        n = fs[ci]
        M, S = fs[2:2 + D][cols], fs[2 + D:2 + 2 * D][cols]
        var = S / (n - 1) if n > 1 else np.square(M)
        y = x.reshape(M.shape) if M.shape else x
        if self.demean:
            y = y - M
        if self.destd:
            y = y / (np.sqrt(var) + 1e-8)
        if self.clip:
            y = np.clip(y, -self.clip, self.clip)
        return y.reshape(np.shape(x))
