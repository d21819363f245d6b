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
#include "rollout_host.h"

namespace mrl {

constexpr int PS_W = 64;              // candidates per block (one wave)
constexpr int PS_LD = PS_W + 1;       // LDS tile stride in floats
constexpr int PS_MAX_HID = 3;         // hidden layers
constexpr int PS_MAX_WIDTH = 64;      // units per hidden layer
constexpr int PS_JB = 4;              // outputs accumulated per pass over a layer's inputs
constexpr size_t PS_LDS_LIMIT = 160 * 1024;  // one block's LDS on gfx950

struct PopSmallShape {
  int n_hid;
  int dims[PS_MAX_HID + 2];  // obs, hid_sizes..., act
  int PU;                    // floats of theta the forward reads (all but logstd)
  int maxw;                  // widest layer, input and head included
};

struct PopSmallArgs {
  const float* thetas;
  int64_t ld;
  const double* fstate;
  mrl_pop_io io;
  int limit;  // steps an episode may take: min(timestep_limit or MAX_STEPS, MAX_STEPS)
  PopSmallShape sh;
};

// dynamic LDS of a block: the frozen filter (mean, denominator), the theta tile, two
// activation buffers.  The launch and mrl_pop_rollout_mlp_fits both go through here.
inline size_t ps_filter_bytes(int obs) { return (size_t)2 * obs * sizeof(double); }
inline size_t ps_tile_bytes(const PopSmallShape& sh) { return (size_t)sh.PU * PS_LD * sizeof(float); }
inline size_t ps_lds_bytes(const PopSmallShape& sh) {
  return ps_filter_bytes(sh.dims[0]) + ps_tile_bytes(sh) + (size_t)2 * sh.maxw * PS_W * sizeof(float);
}

template <int ENV>
__global__ __launch_bounds__(PS_W) void pop_rollout_small_kernel(RollArgs a, PopSmallArgs p) {
  using EC = EnvC<ENV>;
  constexpr int O = EC::OBS, A = EC::ACT, NS = EC::NS, D = O + 1;
  extern __shared__ __attribute__((aligned(16))) double ps_dyn[];
  double* fmean = ps_dyn;
  double* fden = ps_dyn + O;
  float* tile = reinterpret_cast<float*>(ps_dyn + 2 * O);
  const int PU = p.sh.PU, n_hid = p.sh.n_hid;
  float* buf0 = tile + (size_t)PU * PS_LD;
  float* buf1 = buf0 + p.sh.maxw * PS_W;
  const int N = a.d.n_envs;
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * PS_W;
  const int e = e0 + lane;
  const int nrows = N - e0 < PS_W ? N - e0 : PS_W;  // >= 1: the grid is ceil(N / 64)
  const float* __restrict__ th0 = p.thetas + (int64_t)e0 * p.ld;

  // frozen filter: mrl_obfilter_update_apply(update = 0); below two observations (or no state)
  // mean 0 / denominator 1, which leaves the observation bit for bit
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
      const int din = p.sh.dims[l], dout = p.sh.dims[l + 1];
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

// the net's shape from the caller's arguments.  E_ARG: an unknown env, n_hid < 0, null
// hid_sizes with n_hid > 0; E_UNSUPPORTED: Humanoid, more than three hidden layers, a width
// outside [1, 64].  `what` names the failed check.
static int ps_shape(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid, PopSmallShape& sh, const char*& what) {
  if (!env_known(env_id)) return what = "desc.env_id: unknown env", E_ARG;
  if (n_hid < 0) return what = "n_hid < 0", E_ARG;
  if (n_hid > 0 && !hid_sizes) return what = "null hid_sizes", E_ARG;
  if (env_id == MRL_ENV_HUMANOID) return what = "Humanoid is not supported (the thread-per-env envs only)", E_UNSUPPORTED;
  if (n_hid > PS_MAX_HID) return what = "more than 3 hidden layers", E_UNSUPPORTED;
  for (int l = 0; l < n_hid; ++l)
    if (hid_sizes[l] < 1 || hid_sizes[l] > PS_MAX_WIDTH) return what = "a hidden width outside [1, 64]", E_UNSUPPORTED;
  const EnvInfo ei = env_info(env_id);
  sh.n_hid = n_hid;
  sh.dims[0] = ei.obs;
  for (int l = 0; l < n_hid; ++l) sh.dims[1 + l] = hid_sizes[l];
  sh.dims[n_hid + 1] = ei.act;
  for (int l = n_hid + 2; l < PS_MAX_HID + 2; ++l) sh.dims[l] = 0;
  sh.PU = 0;
  sh.maxw = 0;
  for (int l = 0; l <= n_hid; ++l) sh.PU += sh.dims[l] * sh.dims[l + 1] + sh.dims[l + 1];
  for (int l = 0; l <= n_hid + 1; ++l) sh.maxw = sh.dims[l] > sh.maxw ? sh.dims[l] : sh.maxw;
  return OK;
}

}  // namespace mrl

using namespace mrl;

extern "C" int64_t mrl_pop_mlp_num_params(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid) {
  if (!env_known(env_id)) return fail(E_ARG, "mrl_pop_mlp_num_params: unknown env");
  if (n_hid < 0) return fail(E_ARG, "mrl_pop_mlp_num_params: n_hid < 0");
  if (n_hid > 0 && !hid_sizes) return fail(E_ARG, "mrl_pop_mlp_num_params: null hid_sizes");
  const EnvInfo ei = env_info(env_id);
  int64_t P = 0, din = ei.obs;
  for (int l = 0; l < n_hid; ++l) {
    if (hid_sizes[l] < 1) return fail(E_ARG, "mrl_pop_mlp_num_params: a hidden width < 1");
    P += din * hid_sizes[l] + hid_sizes[l];
    din = hid_sizes[l];
  }
  P += din * ei.act + ei.act;
  return P + (ei.discrete ? 0 : ei.act);
}

extern "C" int32_t mrl_pop_rollout_mlp_fits(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid) {
  PopSmallShape sh;
  const char* what = nullptr;
  const int rc = ps_shape(env_id, hid_sizes, n_hid, sh, what);
  if (rc == E_ARG) return fail(E_ARG, std::string("mrl_pop_rollout_mlp_fits: ") + what);
  if (rc) return 0;
  return ps_lds_bytes(sh) <= PS_LDS_LIMIT ? 1 : 0;
}

extern "C" int mrl_pop_rollout_mlp(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const int32_t* hid_sizes,
                                   int32_t n_hid, const float* thetas, int64_t ld_theta, const double* filter_state,
                                   const mrl_pop_io* io, void* stream) {
  const char* what = nullptr;
  if (!d) what = "null desc";
  else if (!b) what = "null bufs";
  else if (n_hid < 0) what = "n_hid < 0";
  else if (n_hid > 0 && !hid_sizes) what = "null hid_sizes";
  else if (!thetas) what = "null thetas";
  else if (!io) what = "null io";
  else if (!env_known(d->env_id)) what = "desc.env_id: unknown env";
  else if (d->n_envs <= 0) what = "desc.n_envs <= 0";
  else if (!b->env_state) what = "null bufs.env_state";
  else if (!b->env_int) what = "null bufs.env_int";
  else if (!io->ret || !io->len || !io->flags || !io->stat) what = "null io.ret / len / flags / stat";
  else if (io->trace_steps < 0) what = "io.trace_steps < 0";
  else {
    const bool any = io->trace_obs || io->trace_act || io->trace_rew || io->trace_steps > 0;
    const bool all = io->trace_obs && io->trace_act && io->trace_rew && io->trace_steps > 0;
    if (any && !all) what = "the trace is only partly set (trace_steps, trace_obs, trace_act, trace_rew)";
  }
  if (what) return fail(E_ARG, std::string("mrl_pop_rollout_mlp: ") + what);
  PopSmallArgs p;
  const int rc = ps_shape(d->env_id, hid_sizes, n_hid, p.sh, what);
  if (rc) return fail(rc, std::string("mrl_pop_rollout_mlp: ") + what);
  const size_t lds = ps_lds_bytes(p.sh);
  if (lds > PS_LDS_LIMIT)
    return fail(E_UNSUPPORTED, "mrl_pop_rollout_mlp: 64 candidates of this net need " + std::to_string(lds) +
                                   " bytes of LDS, a block has " + std::to_string(PS_LDS_LIMIT));
  const EnvInfo ei = env_info(d->env_id);
  const int64_t P = p.sh.PU + (ei.discrete ? 0 : ei.act);
  if (ld_theta != 0 && ld_theta < P)
    return fail(E_ARG, "mrl_pop_rollout_mlp: ld_theta is neither 0 nor >= the parameter count");
  RollArgs a = make_args(d, b);
  p.thetas = thetas;
  p.ld = ld_theta;
  p.fstate = filter_state;
  p.io = *io;
  p.limit = d->timestep_limit > 0 && d->timestep_limit < ei.max_steps ? d->timestep_limit : ei.max_steps;
  const dim3 grid((d->n_envs + PS_W - 1) / PS_W);
  MRL_DISPATCH_THREAD_ENV(d->env_id, pop_rollout_small_kernel, grid, dim3(PS_W), lds, (hipStream_t)stream, a, p);
  return hip_check(hipGetLastError(), "mrl_pop_rollout_mlp");
}
