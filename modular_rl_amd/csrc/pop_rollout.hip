// Population rollout of the cross-entropy method (mrl_pop_rollout): the step between cem.hip's
// mrl_cem_sample and mrl_cem_refit.
//
// Cross-entropy method (cem.py:10-50, 64-68): N parameter vectors, one whole episode each,
// env e driven by theta row e under the deterministic policy (agentzoo.py:116-123).  One
// launch runs every episode to its end.
//
// Layout: a lane per candidate, one wave per block.  The physics (the envs' step, the
// functions of env_step_kernel: the same bits) runs at full lane use; the policy forward is
// 64 independent fmaf chains.  Every lane needs its OWN weights, row-major [N, P] in memory, so
// lane-strided reads would touch 64 lines per load: instead the wave streams theta in chunks of
// 64 consecutive floats -- lane l loads float 64 ci + l of each of the wave's 64 rows (one
// 256 B run per row, coalesced), writes them transposed into an LDS tile (stride 65:
// conflict-free both ways) and every lane reads back its own candidate's 64 weights.  The flat
// Keras order makes every chunk one unit of work: W0 row k, b0, W1 row k, b1, 64 W2 entries,
// b2.  Chunk ci + 1 is in flight (registers) while chunk ci is consumed.
// Lanes whose episode ended keep loading and computing (the chunk loads are cooperative) with
// their stores masked until the wave's last episode ends; the loop is bounded by the step
// counter.  No block waits on another and nothing is accumulated across lanes: the results do
// not depend on scheduling.
// The argument block is pop_rollout_device.h's, the argument checks pop_rollout_host.h's.  The
// episode protocol (frozen filter, filter / clip / cast, Welford, traces, action and step,
// result stores) is written out here as in the other lane kernel: DESIGN 5g has the folds tried.
#include "pop_rollout_host.h"

namespace mrl {

constexpr int POP_LD = POP_W + 1;  // LDS tile stride in floats

template <int ENV>
__global__ __launch_bounds__(POP_W) void pop_rollout_kernel(RollArgs a, PopArgs p) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, A = EC::ACT, NS = EC::NS, D = O + 1;
  constexpr int PU = HID * (O + 66 + A) + A;  // floats of theta the forward reads (all but logstd)
  constexpr int NC = O + 67 + A;              // chunks of 64 floats covering them
  static_assert(mlp_dims(O, A, 0).P == PU, "flat theta layout");
  static_assert(A <= HID, "the b2 chunk holds the head biases");
  __shared__ float tile[POP_W * POP_LD];
  __shared__ float h1s[HID * POP_W];
  __shared__ float xs[O * POP_W];
  __shared__ double fmean[O], fden[O];
  const int N = a.d.n_envs;
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * POP_W;
  const int e = e0 + lane;
  const int nrows = N - e0 < POP_W ? N - e0 : POP_W;  // >= 1: the grid is ceil(N / 64)
  const float* __restrict__ th0 = p.thetas + (int64_t)e0 * p.ld;

  // frozen filter: mrl_obfilter_update_apply(update = 0); below two observations (or no state)
  // mean 0 / denominator 1, which leaves the observation bit for bit.  Written out, like the
  // rest of the episode below: load-bearing, every fold into a shared function
  // moved this kernel's register allocation for some env
  if (lane < O) {
    double M = 0.0, den = 1.0;
    if (p.fstate != nullptr && p.fstate[0] >= 2.0) {
      const double n = p.fstate[0];
      M = p.fstate[2 + lane];
      den = sqrt(p.fstate[2 + D + lane] / (n - 1.0)) + 1e-8;
    }
    fmean[lane] = M;
    fden[lane] = den;
  }

  // row pointers step by ld from one per-lane pointer (the last block, if it holds fewer than
  // 64 rows, re-reads its last row); ld passes through an empty asm so the 64 row addresses
  // are formed at each fetch and not kept live across the whole step loop
  float nxt[POP_W];
  auto fetch = [&](int ci) {
    const int off = HID * ci + lane;
    const bool in = off < PU;
    int64_t ldv = p.ld;
    asm volatile("" : "+s"(ldv));
    const float* q = th0 + off;
#pragma unroll
    for (int c = 0; c < POP_W; ++c) {
      nxt[c] = in ? *q : 0.f;
      q += c + 1 < nrows ? ldv : 0;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int c = 0; c < POP_W; ++c) tile[lane * POP_LD + c] = nxt[c];
    __syncthreads();
  };

  bool active = e < N;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (active) reset_env<ENV>(a, e, s);
  double ret = 0.0, wn = 0.0, wmean[O], wm2[O];
#pragma unroll
  for (int k = 0; k < O; ++k) wmean[k] = wm2[k] = 0.0;
  int len = 0;
  bool terminated = false;
  fetch(0);
  __syncthreads();  // fmean / fden

  for (int t = 0; t < p.limit; ++t) {
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;  // wave-uniform
    double o[O];
    EC::obs(s, o);
#pragma unroll
    for (int k = 0; k < O; ++k) {  // the lane's own column of xs: no barrier needed
      double v = o[k] - fmean[k];
      v = v / fden[k];
      xs[k * POP_W + lane] = (float)(v < -5.0 ? -5.0 : (v > 5.0 ? 5.0 : v));
    }
    if (active) {
      wn += 1.0;
#pragma unroll
      for (int k = 0; k < O; ++k) {
        const double dlt = o[k] - wmean[k];
        wmean[k] += dlt / wn;
        wm2[k] += dlt * (o[k] - wmean[k]);
      }
      if (t < p.io.trace_steps) {
        double* orow = p.io.trace_obs + ((int64_t)t * N + e) * O;
#pragma unroll
        for (int k = 0; k < O; ++k) orow[k] = o[k];
      }
    }
    // ---- policy forward, chunk by chunk
    float acc[HID];
#pragma unroll
    for (int j = 0; j < HID; ++j) acc[j] = 0.f;
    for (int k = 0; k < O; ++k) {  // chunks 0 .. O-1: W0 row k
      commit();
      fetch(k + 1);
      const float xk = xs[k * POP_W + lane];
#pragma unroll
      for (int j = 0; j < HID; ++j) acc[j] = fmaf(xk, tile[j * POP_LD + lane], acc[j]);
      __syncthreads();
    }
    commit();  // chunk O: b0
    fetch(O + 1);
#pragma unroll
    for (int j = 0; j < HID; ++j) {
      h1s[j * POP_W + lane] = tanhf(acc[j] + tile[j * POP_LD + lane]);
      acc[j] = 0.f;
    }
    __syncthreads();
    for (int k = 0; k < HID; ++k) {  // chunks O+1 .. O+64: W1 row k
      commit();
      fetch(O + 2 + k);
      const float hk = h1s[k * POP_W + lane];
#pragma unroll
      for (int j = 0; j < HID; ++j) acc[j] = fmaf(hk, tile[j * POP_LD + lane], acc[j]);
      __syncthreads();
    }
    commit();  // chunk O+65: b1
    fetch(O + 66);
#pragma unroll
    for (int j = 0; j < HID; ++j) acc[j] = tanhf(acc[j] + tile[j * POP_LD + lane]);
    __syncthreads();
    float z[A];
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] = 0.f;
#pragma unroll
    for (int cc = 0; cc < A; ++cc) {  // chunks O+66 .. O+65+A: W2 entries 64 cc .. 64 cc + 63 ([64, A] row-major)
      commit();
      fetch(O + 67 + cc);
#pragma unroll
      for (int j = 0; j < HID; ++j) {
        const int i = HID * cc + j;
        z[i % A] = fmaf(acc[i / A], tile[j * POP_LD + lane], z[i % A]);
      }
      __syncthreads();
    }
    commit();  // chunk NC-1: b2
    fetch(0);  // the next step's first chunk, in flight across the physics
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] += tile[q * POP_LD + lane];
    __syncthreads();
    static_assert(O + 67 + A == NC, "chunk count");

    // ---- deterministic action, env step
    if (active) {
      double rew = 0.0;
      bool done = false;
      if constexpr (EC::DISCRETE) {
        int act = 0;
#pragma unroll
        for (int q = 1; q < A; ++q)
          if (z[q] > z[act]) act = q;
        if (t < p.io.trace_steps) reinterpret_cast<int32_t*>(p.io.trace_act)[(int64_t)t * N + e] = act;
        EC::step(s, act, rew, done);
      } else {
        if (t < p.io.trace_steps) {
          float* arow = reinterpret_cast<float*>(p.io.trace_act) + ((int64_t)t * N + e) * A;
#pragma unroll
          for (int q = 0; q < A; ++q) arow[q] = z[q];
        }
        EC::step(s, z, rew, done);
      }
      if (t < p.io.trace_steps) p.io.trace_rew[(int64_t)t * N + e] = rew;
      ret += rew;
      len = t + 1;
      terminated = done || (t + 1 >= EC::MAX_STEPS);
      if (terminated || t + 1 >= p.limit) active = false;
    }
  }

  if (e < N) {
    p.io.ret[e] = ret;
    p.io.len[e] = len;
    p.io.flags[e] = (uint8_t)(1 | (terminated ? 2 : 0));
    double* st = p.io.stat + (int64_t)e * (1 + 2 * O);
    st[0] = wn;
#pragma unroll
    for (int k = 0; k < O; ++k) {
      st[1 + k] = wmean[k];
      st[1 + O + k] = wm2[k];
    }
    a.b.env_int[e] = len;
#pragma unroll
    for (int i = 0; i < NS; ++i) a.b.env_state[(int64_t)i * N + e] = s[i];
  }
}

}  // namespace mrl

using namespace mrl;

extern "C" int mrl_pop_rollout(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const mrl_mlp_desc* pol,
                               const float* thetas, int64_t ld_theta, const double* filter_state,
                               const mrl_pop_io* io, void* stream) {
  const char* what = pop_check_args(d, b, pol ? nullptr : "null policy desc", thetas, io);
  if (what) return fail(E_ARG, std::string("mrl_pop_rollout: ") + what);
  if (d->env_id == MRL_ENV_HUMANOID)
    return fail(E_UNSUPPORTED, "mrl_pop_rollout: Humanoid is not supported (the thread-per-env envs only)");
  const EnvInfo ei = env_info(d->env_id);
  const bool gauss = pol->head == MRL_HEAD_GAUSS, softmax = pol->head == MRL_HEAD_SOFTMAX;
  if (pol->n_hidden != HID || pol->n_layers != 2 || pol->n_in != ei.obs || pol->n_out != ei.act ||
      !(ei.discrete ? softmax : gauss))
    return fail(E_UNSUPPORTED, "mrl_pop_rollout: the policy must be the env's 64-64 net (hid_sizes [64, 64], "
                               "n_in = obs_dim, n_out = act_dim, softmax / Gauss head)");
  const int64_t P = mlp_dims(ei.obs, ei.act, gauss).P;
  if (ld_theta != 0 && ld_theta < P) return fail(E_ARG, "mrl_pop_rollout: ld_theta is neither 0 nor >= the parameter count");
  RollArgs a = make_args(d, b);
  PopArgs p;
  pop_fill(p, d, thetas, ld_theta, filter_state, io);
  const dim3 grid((d->n_envs + POP_W - 1) / POP_W);
  MRL_DISPATCH_THREAD_ENV(d->env_id, pop_rollout_kernel, grid, dim3(POP_W), 0, (hipStream_t)stream, a, p);
  return hip_check(hipGetLastError(), "mrl_pop_rollout");
}
