// Stand-alone env stepper (mrl_env_reset, mrl_env_step) and obs filter (mrl_obfilter_*): the
// envs and the ZFilter of the rollout without a policy, on the rollout's own device functions
// (rollout_device.h), so the same inputs give the rollout's bits.
#include "rollout_host.h"

namespace mrl {

// ------------------------------------------------------------------ stand-alone env stepper
// The envs without a policy: mrl_env_reset / mrl_env_step drive the same state buffers
// (env_state, env_int) with the caller's actions, one launch per call.  Same device
// functions as the rollout kernels; raw fp64 observation rows [E, obs_dim], row-major.
// Thread per env with one wave per block (the per-env step is a latency chain: the waves
// spread over the CUs); Humanoid wave per env like hm_reset_kernel / hm_act_kernel, beside
// which its two kernels are compiled (hm_env_*_kernel, rollout_layered.hip).
template <int ENV>
__global__ __launch_bounds__(64) void env_reset_kernel(RollArgs a, mrl_env_io io) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS;
  const int E = a.d.n_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E || (io.mask != nullptr && io.mask[e] == 0)) return;
  double s[EC::NS];
  reset_env<ENV>(a, e, s);
#pragma unroll
  for (int i = 0; i < EC::NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
  double* orow = io.obs + (int64_t)e * O;
  EC::obs_out(s, [&](int k, double v) { orow[k] = v; });
}

template <int ENV>
__global__ __launch_bounds__(64) void env_step_kernel(RollArgs a, mrl_env_io io, int auto_reset) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, NS = EC::NS, A = EC::ACT;
  const int E = a.d.n_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = a.b.env_state[(int64_t)i * E + e];
  double rew = 0.0;
  bool done = false;
  if constexpr (EC::DISCRETE) {
    EC::step(s, reinterpret_cast<const int32_t*>(io.act)[e], rew, done);
  } else {
    float av[A];
#pragma unroll
    for (int q = 0; q < A; ++q) av[q] = reinterpret_cast<const float*>(io.act)[(int64_t)e * A + q];
    EC::step(s, av, rew, done);
  }
  const int ept = a.b.env_int[e];
  bool term, last;
  env_step_flags<ENV>(a, ept, done, term, last);
  io.ep_t[e] = ept;
  io.rew[e] = rew;
  io.flags[e] = (uint8_t)((last ? 1 : 0) | (term ? 2 : 0));
  if (last && io.final_obs != nullptr) {
    double* frow = io.final_obs + (int64_t)e * O;
    EC::obs_out(s, [&](int k, double v) { frow[k] = v; });
  }
  if (last && auto_reset) reset_env<ENV>(a, e, s);
  else a.b.env_int[e] = ept + 1;
#pragma unroll
  for (int i = 0; i < NS; ++i) a.b.env_state[(int64_t)i * E + e] = s[i];
  double* orow = io.obs + (int64_t)e * O;
  EC::obs_out(s, [&](int k, double v) { orow[k] = v; });
}

// ------------------------------------------------------------------ stand-alone obs filter
// ZFilter (filters.py:17-40) over a batch of row-major fp64 rows x[n_rows, dim], in the
// layered rollout's arithmetic (col_partial, merge_records_column, lrollout_obs_kernel's
// normalisation), so the same rows in the same order give the same bits as mrl_rollout_obs.
// state = [n_obs, n_rew, M[dim+1], S[dim+1]], one copy updated in place: the merge
// (obfilter_merge_kernel, one thread per column) writes its own M, S and stages n, the
// mean and the denominator of every column in the workspace; the apply kernel reads only
// the staged values and stores n, so no block reads what another writes.
// workspace: records [nb][2 + 2 (dim + 1)] | mean [dim] | den [dim] | n
__global__ __launch_bounds__(RB) void obfilter_partials_kernel(const double* __restrict__ x, int64_t n_rows, int dim,
                                                               double* __restrict__ rec) {
  __shared__ double red[8][LCOLS];
  const int64_t r0 = (int64_t)blockIdx.x * ENVS_PER_BLOCK;
  const int nvalid = (int)(n_rows - r0 < ENVS_PER_BLOCK ? n_rows - r0 : ENVS_PER_BLOCK);
  const int c = threadIdx.x & (LCOLS - 1), g = threadIdx.x >> 5;
  const int k = blockIdx.y * LCOLS + c;
  const int D = dim + 1, RS = 2 + 2 * D;  // the rollout's record layout (the reward column unused)
  double* r = rec + (int64_t)blockIdx.x * RS;
  const double* col = x + r0 * dim + (k < dim ? k : 0);
  double mean, t2;
  col_partial([&](int row) { return col[(int64_t)row * dim]; }, nvalid, k < dim, red, c, g, mean, t2);
  if (g == 0 && k < dim) {
    r[2 + k] = mean;
    r[2 + D + k] = t2;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    r[0] = (double)nvalid;
    r[1] = 0.0;
  }
}

__global__ __launch_bounds__(LCOLS) void obfilter_merge_kernel(double* __restrict__ state, int dim, int nb, int update,
                                                               double* __restrict__ ws) {
  const int k = blockIdx.x * LCOLS + threadIdx.x;
  if (k >= dim) return;
  const int D = dim + 1, RS = 2 + 2 * D;
  double* stage = ws + (int64_t)nb * RS;
  double n, M, S;
  if (update) {
    merge_records_column(ws, nb, RS, D, k, false, state, n, M, S);
  } else {
    n = state[0];
    M = state[2 + k];
    S = state[2 + D + k];
  }
  const double var = n > 1.0 ? S / (n - 1.0) : M * M;  // running_stat.py:27
  stage[k] = M;
  stage[dim + k] = sqrt(var) + 1e-8;
  if (k == 0) stage[2 * dim] = n;
  if (update) {
    state[2 + k] = M;
    state[2 + D + k] = S;
  }
}

__global__ __launch_bounds__(RB) void obfilter_apply_kernel(const double* __restrict__ x, int64_t n_rows, int dim,
                                                            double clip, const double* __restrict__ stage,
                                                            float* __restrict__ out, double* n_out) {
  __shared__ double fmean[LCOLS], fden[LCOLS];
  const int kbase = blockIdx.y * LCOLS;
  if (threadIdx.x < LCOLS && kbase + (int)threadIdx.x < dim) {
    fmean[threadIdx.x] = stage[kbase + threadIdx.x];
    fden[threadIdx.x] = stage[dim + kbase + threadIdx.x];
  }
  if (n_out != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *n_out = stage[2 * dim];
  __syncthreads();
  // thread (row = tid / 4 of the block's 64, 8 consecutive columns of the chunk)
  constexpr int G = RB / ENVS_PER_BLOCK, CPT = LCOLS / G;
  const int64_t row = (int64_t)blockIdx.x * ENVS_PER_BLOCK + threadIdx.x / G;
  if (row >= n_rows) return;
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int kl = (threadIdx.x % G) * CPT + q, k = kbase + kl;
    if (k < dim) {
      double v = x[row * dim + k];
      v = v - fmean[kl];
      v = v / fden[kl];
      v = v < -clip ? -clip : (v > clip ? clip : v);
      out[row * dim + k] = (float)v;
    }
  }
}

}  // namespace mrl

using namespace mrl;

extern "C" {

// the stand-alone stepper's arguments: checked before any HIP call
static int check_env(const char* who, const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const mrl_env_io* io) {
  const char* what = nullptr;
  if (!d) what = "null desc";
  else if (!b) what = "null bufs";
  else if (!io) what = "null io";
  else if (!env_known(d->env_id)) what = "desc.env_id: unknown env";
  else if (d->n_envs <= 0) what = "desc.n_envs <= 0";
  else if (!b->env_state) what = "null bufs.env_state";
  else if (!b->env_int) what = "null bufs.env_int";
  else if (!io->obs) what = "null io.obs";
  if (!what) return OK;
  return fail(E_ARG, std::string(who) + ": " + what);
}

int mrl_env_reset(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const mrl_env_io* io, void* stream) {
  int rc = check_env("mrl_env_reset", d, b, io);
  if (rc) return rc;
  RollArgs a = make_args(d, b);
  const dim3 genv((d->n_envs + 63) / 64);
  if (d->env_id == MRL_ENV_HUMANOID) launch_hm_env_reset(a, *io, (hipStream_t)stream);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, env_reset_kernel, genv, dim3(64), 0, (hipStream_t)stream, a, *io);
  return hip_check(hipGetLastError(), "mrl_env_reset");
}

int mrl_env_step(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const mrl_env_io* io, int32_t auto_reset,
                 void* stream) {
  int rc = check_env("mrl_env_step", d, b, io);
  if (rc) return rc;
  if (!io->act) return fail(E_ARG, "mrl_env_step: null io.act");
  if (!io->rew) return fail(E_ARG, "mrl_env_step: null io.rew");
  if (!io->flags) return fail(E_ARG, "mrl_env_step: null io.flags");
  if (!io->ep_t) return fail(E_ARG, "mrl_env_step: null io.ep_t");
  RollArgs a = make_args(d, b);
  const int ar = auto_reset != 0;
  const dim3 genv((d->n_envs + 63) / 64);
  if (d->env_id == MRL_ENV_HUMANOID) launch_hm_env_step(a, *io, ar, (hipStream_t)stream);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, env_step_kernel, genv, dim3(64), 0, (hipStream_t)stream, a, *io, ar);
  return hip_check(hipGetLastError(), "mrl_env_step");
}

// rows per launch dimension: blocks of 64 rows in grid.x
static constexpr int64_t OBF_MAX_ROWS = (int64_t)0x7fffffff * 32;
static constexpr int32_t OBF_MAX_DIM = 65535 * LCOLS;

int64_t mrl_obfilter_workspace_bytes(int64_t n_rows, int32_t dim) {
  if (n_rows <= 0 || n_rows > OBF_MAX_ROWS || dim <= 0 || dim > OBF_MAX_DIM) return -1;
  return (env_blocks(n_rows) * (2 + 2 * ((int64_t)dim + 1)) + 2 * (int64_t)dim + 1) * (int64_t)sizeof(double);
}

int mrl_obfilter_update_apply(double* state, int32_t dim, const double* x, int64_t n_rows, int32_t update,
                              double clip, float* out, void* workspace, void* stream) {
  if (!state) return fail(E_ARG, "mrl_obfilter_update_apply: null state");
  if (dim <= 0 || dim > OBF_MAX_DIM) return fail(E_ARG, "mrl_obfilter_update_apply: dim out of range");
  if (n_rows <= 0 || n_rows > OBF_MAX_ROWS) return fail(E_ARG, "mrl_obfilter_update_apply: n_rows out of range");
  if (!x) return fail(E_ARG, "mrl_obfilter_update_apply: null x");
  if (!out) return fail(E_ARG, "mrl_obfilter_update_apply: null out");
  if (!(clip > 0.0)) return fail(E_ARG, "mrl_obfilter_update_apply: clip must be positive");
  if (!workspace) return fail(E_ARG, "mrl_obfilter_update_apply: null workspace (mrl_obfilter_workspace_bytes)");
  const int64_t nb = env_blocks(n_rows);
  const unsigned chunks = (unsigned)((dim + LCOLS - 1) / LCOLS);
  double* ws = reinterpret_cast<double*>(workspace);
  double* stage = ws + nb * (2 + 2 * ((int64_t)dim + 1));
  hipStream_t s = (hipStream_t)stream;
  if (update)
    hipLaunchKernelGGL(obfilter_partials_kernel, dim3((unsigned)nb, chunks), dim3(RB), 0, s, x, n_rows, dim, ws);
  hipLaunchKernelGGL(obfilter_merge_kernel, dim3(chunks), dim3(LCOLS), 0, s, state, dim, (int)nb, update != 0, ws);
  hipLaunchKernelGGL(obfilter_apply_kernel, dim3((unsigned)nb, chunks), dim3(RB), 0, s, x, n_rows, dim, clip, stage,
                     out, update ? state : nullptr);
  return hip_check(hipGetLastError(), "mrl_obfilter_update_apply");
}

}  // extern "C"
