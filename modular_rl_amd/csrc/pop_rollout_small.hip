// Population rollout for small policy nets (mrl_pop_rollout_mlp): the cross-entropy method's
// objective for a tanh MLP obs -> hid_sizes -> act whose whole population tile fits one block's
// LDS -- the reference's CEM battery runs hid_sizes 10,5 (193 forward floats on Hopper-v2).
//
// Layout: a lane per candidate, one wave per block, as pop_rollout.hip.  What differs is where
// theta lives.  There a candidate's 5 k weights are re-streamed from memory every step; here the
// wave reads its 64 rows once -- lane l loads float p0 + l of each row (one coalesced run per
// row) -- and writes them transposed into a [PU][65] LDS tile: the write of row c touches
// words (p0 + l) 65 + c, bank p0 + l + c (mod 32, per 32-lane group): 32 different banks; the
// step loop's read of parameter p touches p 65 + lane: 32 different banks.  After the load's one
// barrier the step loop reads no theta from memory and needs no barrier: the activations are
// [width][64] LDS columns, one per lane, written and read by that lane alone (a wave's LDS
// operations complete in issue order).  Hidden widths are run-time values.
//
// The arithmetic is pop_rollout.hip's: per output j, acc = 0, acc = fmaf(x_k, W[k][j], acc)
// for k ascending, acc + b_j, tanhf on hidden layers; the same fp64 filter expressions and cast;
// the same physics (EnvC<>, reset_env).  A 10-5 net zero-padded to 64-64 gives the same bits in
// both kernels.
//
// The argument block is pop_rollout_device.h's, the argument checks pop_rollout_host.h's.  The
// episode protocol (frozen filter, filter / clip / cast, Welford, traces, action and step,
// result stores) is written out here as in the other lane kernel: DESIGN 5g has the folds tried.
#include "pop_rollout_host.h"

namespace mrl {

constexpr int PS_W = POP_W;      // candidates per block (one wave)
constexpr int PS_LD = PS_W + 1;  // LDS tile stride in floats
constexpr int PS_JB = 4;         // outputs accumulated per pass over a layer's inputs

// dynamic LDS of a block: the frozen filter (mean, denominator), the theta tile, two
// activation buffers.  The launch and mrl_pop_rollout_mlp_fits both go through here.
inline size_t ps_filter_bytes(int obs) { return (size_t)2 * obs * sizeof(double); }
inline size_t ps_tile_bytes(const PopSmallShape& net) { return (size_t)net.PU * PS_LD * sizeof(float); }
inline size_t ps_lds_bytes(const PopSmallShape& net) {
  return ps_filter_bytes(net.sh.dims[0]) + ps_tile_bytes(net) + (size_t)2 * net.maxw * PS_W * sizeof(float);
}

template <int ENV>
__global__ __launch_bounds__(PS_W) void pop_rollout_small_kernel(RollArgs a, PopSmallArgs p) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, A = EC::ACT, NS = EC::NS, D = O + 1;
  extern __shared__ __attribute__((aligned(16))) double ps_dyn[];
  double* fmean = ps_dyn;
  double* fden = ps_dyn + O;
  float* tile = reinterpret_cast<float*>(ps_dyn + 2 * O);
  const int PU = p.net.PU, n_hid = p.net.sh.n_hid;
  float* buf0 = tile + (size_t)PU * PS_LD;
  float* buf1 = buf0 + p.net.maxw * PS_W;
  const int N = a.d.n_envs;
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * PS_W;
  const int e = e0 + lane;
  const int nrows = N - e0 < PS_W ? N - e0 : PS_W;  // >= 1: the grid is ceil(N / 64)
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

  // theta, once: 64 floats of every row per pass, eight rows in flight (the last block, if it
  // holds fewer than 64 rows, re-reads its last row for the lanes without a candidate)
  for (int p0 = 0; p0 < PU; p0 += PS_W) {
    const int q = p0 + lane;
    const bool in = q < PU;
    for (int c0 = 0; c0 < PS_W; c0 += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = c0 + i < nrows ? c0 + i : nrows - 1;
        v[i] = in ? th0[(int64_t)c * p.ld + q] : 0.f;
      }
      if (in)
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[q * PS_LD + c0 + i] = v[i];
    }
  }

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
  __syncthreads();  // fmean / fden, the tile: the only barrier

  const float* tl = tile + lane;  // the lane's own candidate: parameter p at tl[p * PS_LD]
  for (int t = 0; t < p.limit; ++t) {
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;  // wave-uniform
    double o[O];
    EC::obs(s, o);
#pragma unroll
    for (int k = 0; k < O; ++k) {
      double v = o[k] - fmean[k];
      v = v / fden[k];
      buf0[k * PS_W + lane] = (float)(v < -5.0 ? -5.0 : (v > 5.0 ? 5.0 : v));
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
    // ---- policy forward: layer l reads xin [din][64], writes xout [dout][64]
    float* xin = buf0 + lane;
    float* xout = buf1 + lane;
    int off = 0;
    for (int l = 0; l <= n_hid; ++l) {
      const int din = p.net.sh.dims[l], dout = p.net.sh.dims[l + 1];
      const float* Wl = tl + off * PS_LD;            // W[k][j] at Wl[(k dout + j) PS_LD]
      const float* bl = Wl + din * dout * PS_LD;
      for (int j0 = 0; j0 < dout; j0 += PS_JB) {
        // PS_JB outputs per pass over the inputs (one x read per PS_JB weights); a ragged
        // last group recomputes output dout - 1 and drops the copies
        int jj[PS_JB];
        float acc[PS_JB];
#pragma unroll
        for (int i = 0; i < PS_JB; ++i) {
          jj[i] = j0 + i < dout ? j0 + i : dout - 1;
          acc[i] = 0.f;
        }
#pragma unroll 4  // four inputs' LDS reads in flight per wait: a lone wave has nothing else to hide them
        for (int k = 0; k < din; ++k) {
          const float xk = xin[k * PS_W];
#pragma unroll
          for (int i = 0; i < PS_JB; ++i) acc[i] = fmaf(xk, Wl[(k * dout + jj[i]) * PS_LD], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < PS_JB; ++i) {
          const float zb = acc[i] + bl[jj[i] * PS_LD];
          if (j0 + i < dout) xout[(j0 + i) * PS_W] = l < n_hid ? tanhf(zb) : zb;
        }
      }
      off += din * dout + dout;
      float* const written = xout;
      xout = xin;
      xin = written;
    }
    float z[A];
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] = xin[q * PS_W];

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

extern "C" int64_t mrl_pop_mlp_num_params(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid) {
  if (!env_known(env_id)) return fail(E_ARG, "mrl_pop_mlp_num_params: unknown env");
  if (const char* what = pop_check_hid(hid_sizes, n_hid)) return fail(E_ARG, std::string("mrl_pop_mlp_num_params: ") + what);
  for (int l = 0; l < n_hid; ++l)  // a count, not a launch: any number of layers, any width from 1 up
    if (hid_sizes[l] < 1) return fail(E_ARG, "mrl_pop_mlp_num_params: a hidden width < 1");
  const EnvInfo ei = env_info(env_id);
  return pop_num_params(ei, pop_forward_floats(ei, hid_sizes, n_hid));
}

extern "C" int32_t mrl_pop_rollout_mlp_fits(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid) {
  PopSmallShape sh;
  const char* what = nullptr;
  const int rc = pop_net_shape(env_id, hid_sizes, n_hid, false, sh, what);
  if (rc == E_ARG) return fail(E_ARG, std::string("mrl_pop_rollout_mlp_fits: ") + what);
  if (rc) return 0;
  return ps_lds_bytes(sh) <= LDS_PER_BLOCK ? 1 : 0;
}

extern "C" int mrl_pop_rollout_mlp(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const int32_t* hid_sizes,
                                   int32_t n_hid, const float* thetas, int64_t ld_theta, const double* filter_state,
                                   const mrl_pop_io* io, void* stream) {
  const char* what = pop_check_args(d, b, pop_check_hid(hid_sizes, n_hid), thetas, io);
  if (what) return fail(E_ARG, std::string("mrl_pop_rollout_mlp: ") + what);
  PopSmallArgs p;
  const int rc = pop_net_shape(d->env_id, hid_sizes, n_hid, false, p.net, what);
  if (rc) return fail(rc, std::string("mrl_pop_rollout_mlp: ") + what);
  const size_t lds = ps_lds_bytes(p.net);
  if (lds > LDS_PER_BLOCK)
    return fail(E_UNSUPPORTED, "mrl_pop_rollout_mlp: 64 candidates of this net need " + std::to_string(lds) +
                                   " bytes of LDS, a block has " + std::to_string(LDS_PER_BLOCK));
  if (ld_theta != 0 && ld_theta < pop_num_params(env_info(d->env_id), p.net.PU))
    return fail(E_ARG, "mrl_pop_rollout_mlp: ld_theta is neither 0 nor >= the parameter count");
  RollArgs a = make_args(d, b);
  pop_fill(p, d, thetas, ld_theta, filter_state, io);
  const dim3 grid((d->n_envs + PS_W - 1) / PS_W);
  MRL_DISPATCH_THREAD_ENV(d->env_id, pop_rollout_small_kernel, grid, dim3(PS_W), lds, (hipStream_t)stream, a, p);
  return hip_check(hipGetLastError(), "mrl_pop_rollout_mlp");
}
