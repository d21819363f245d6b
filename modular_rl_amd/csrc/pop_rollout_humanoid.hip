// Population rollout for the wave-per-env envs (mrl_pop_rollout_wave): the cross-entropy
// method's objective on Humanoid-v2.  pop_rollout.hip and pop_rollout_small.hip are "a lane per
// candidate" and call EnvC<ENV>::step per thread; Humanoid is stepped by one wave per env with
// its state in LDS (humanoid.h), so here a candidate is a WAVE: hm_pop_rollout_kernel<WPB> is
// persistent for the whole episode, with the block set-up of the other hm_* kernels (hm_block,
// hm_load_tables, MRL_LAUNCH_HM, hm_wpb()).
//
// Per wave: hm::reset from (seed, env_offset + e, episodes started) as hm_env_reset_kernel, then
// one loop whose body is  forward | [reward of the step that ended; observation, Welford,
// frozen filter, policy forward, ctrl] | accelerations | integrate  with the bracket taken every
// FRAME_SKIP-th pass: ONE forward site and ONE accelerations site, so the loop fits the
// instruction cache (the pass-counter shape of hm_act_kernel).  The wave holds forward() of the
// current state when a step starts, which is what a step kernel loads from the kinematics cache:
// the same bits, so a VecEnv of the same seed replays a traced call bit for bit.
//
// Barriers: the block's frozen filter (mean, denominator: one copy per block) is written before
// the tables' barrier and read-only afterwards; after that barrier there is NO block barrier --
// the waves of a block end their episodes at different steps (WAVE_SYNC only; waves past N pass
// the tables' barrier, then return).
//
// The 376 observation columns are split over the lanes, k = lane + 64 i (six per lane): the
// Welford partial (count, mean, M2: the small kernel's expressions per column) lives in
// registers, the trace row is written 64 consecutive doubles at a time.
//
// Policy forward: the tanh MLP 376 -> hid_sizes -> 17 (at most three hidden layers of 1 .. 64
// units), theta (flat Keras order, mrl_pop_mlp_num_params) read from memory every step.  Every
// product is an f32 fmaf.  The summation order is fixed:
//   layer 0   (376 inputs) lane l takes the inputs k = l, l + 64, ... ascending into one
//             accumulator per output from 0.f (a lane without a sixth input adds nothing); the
//             64 partials of output j are summed by wave_sumf -- the xor butterfly, offsets 32,
//             16, 8, 4, 2, 1 -- outputs ascending, HP_JB at a time; then + b_j
//   layer >=1 lane j is output j: acc = fmaf(h_k, W[k][j], acc) from 0.f for k ascending; + b_j
//   tanhf on hidden layers, none on the head; the action is the head (the Gauss mean).
// Nothing depends on scheduling or on where theta lies: the same inputs give the same bits on
// every call, and ld_theta = 0 (one shared theta) the bits of N copies.
// f32 values go to LDS through an identity DPP move (rows_epilogue.h st_head's idiom): an LDS
// op must not read a packed-f32 VALU result within 8 wait states.
//
// The frozen filter's column, filter / clip / cast and the Welford update are
// pop_rollout_device.h's, as in the lane kernels; the argument checks pop_rollout_host.h's.
#include "pop_rollout_host.h"

namespace mrl {

constexpr int HP_MAX_WIDTH = POP_MAX_WIDTH;  // units per hidden layer: one lane per unit
constexpr int HP_JB = 8;          // layer-0 outputs accumulated per pass over a lane's inputs
constexpr int HP_CPL = (HM_OBS + 63) / 64;  // observation columns per lane

// a wave's own LDS beside its hm::Wave: the raw observation, the filtered one, two activation rows
struct HmPopWave {
  double od[HM_OBS];
  float x[HP_CPL * 64];
  float h[2][HP_MAX_WIDTH];
};
static_assert(sizeof(HmPopWave) % 8 == 0 && sizeof(hm::Wave) % 8 == 0, "the dynamic LDS is an array of doubles");

// dynamic LDS of a launch: (WPB = 4) the states, then the block's filter, then the waves' rows
inline size_t hm_pop_lds_bytes(int wpb, int) {
  return hm_lds_state(wpb, 0) + (size_t)2 * HM_OBS * sizeof(double) + (size_t)wpb * sizeof(HmPopWave);
}
static_assert(sizeof(hm::Shared) + 4 * sizeof(hm::Wave) + 2 * HM_OBS * sizeof(double) + 4 * sizeof(HmPopWave) <=
                  LDS_PER_BLOCK,
              "four candidates per block exceed the LDS");

__device__ __forceinline__ void hp_st_lds(float* p, float v) { *p = dpp_f<0xE4>(v); }

// the head row of theta `th` on the filtered observation X.x: lane j < 17 returns z_j
__device__ inline float hp_policy(const HmPopArgs& p, const float* __restrict__ th, HmPopWave& X, int lane) {
  constexpr int O = HM_OBS;
  const int n_hid = p.sh.n_hid;
  float xv[HP_CPL];
#pragma unroll
  for (int i = 0; i < HP_CPL; ++i) xv[i] = lane + 64 * i < O ? X.x[lane + 64 * i] : 0.f;
  float val = 0.f;
  int off = 0;
  for (int l = 0; l <= n_hid; ++l) {
    const int din = p.sh.dims[l], dout = p.sh.dims[l + 1];
    const float* __restrict__ Wl = th + off;  // W[k][j] at Wl[k dout + j]
    const float* __restrict__ bl = Wl + din * dout;
    const float* hin = X.h[(l + 1) & 1];
    if (l == 0) {
      for (int j0 = 0; j0 < dout; j0 += HP_JB) {
        // a ragged last group recomputes output dout - 1 and drops the copies
        int jj[HP_JB];
        float acc[HP_JB];
#pragma unroll
        for (int q = 0; q < HP_JB; ++q) {
          jj[q] = j0 + q < dout ? j0 + q : dout - 1;
          acc[q] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < HP_CPL; ++i) {
          const int k = lane + 64 * i;
          if (k < O) {
            const float* wr = Wl + k * dout;
#pragma unroll
            for (int q = 0; q < HP_JB; ++q) acc[q] = fmaf(xv[i], wr[jj[q]], acc[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < HP_JB; ++q) {
          const float sum = wave_sumf(acc[q]);
          if (lane == j0 + q && j0 + q < dout) val = sum + bl[jj[q]];
        }
      }
    } else {
      const int j = lane < dout ? lane : dout - 1;
      float acc = 0.f;
#pragma unroll 4
      for (int k = 0; k < din; ++k) acc = fmaf(hin[k], Wl[k * dout + j], acc);
      val = acc + bl[j];
    }
    if (l < n_hid) {
      val = tanhf(val);
      if (lane < dout) hp_st_lds(&X.h[l & 1][lane], val);
      WAVE_SYNC();
    }
    off += din * dout + dout;
  }
  return val;
}

template <int WPB>
__global__ __launch_bounds__(64 * WPB) void hm_pop_rollout_kernel(RollArgs a, HmPopArgs p) {
  __shared__ hm::Shared S;
  extern __shared__ __attribute__((aligned(16))) double hm_dyn[];
  int e, lane;
  hm::Wave& W = hm_block<WPB>(e, lane);
  constexpr int O = HM_OBS, A = HM_ACT, D = O + 1;
  const int N = a.d.n_envs;
  double* const fmean = hm_dyn + (WPB == 1 ? 0 : WPB * (sizeof(hm::Wave) / 8));
  double* const fden = fmean + O;
  const int wave = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  HmPopWave& X = reinterpret_cast<HmPopWave*>(fden + O)[wave];

  // the frozen filter: one copy per block, written by all its waves before the tables' barrier
  for (int k = threadIdx.x; k < O; k += 64 * WPB) {
    double M, den;
    pop_frozen_filter(p.fstate, D, k, M, den);
    fmean[k] = M;
    fden[k] = den;
  }
  hm_load_tables<WPB>(S, lane);
  if (e >= N) return;  // after the tables' barrier, the block's only one

  const float* __restrict__ th = p.thetas + (int64_t)e * p.ld;
  const uint32_t w = (uint32_t)a.b.env_int[N + e];
  hm::reset(W, lane, a.d.seed, (uint32_t)(a.d.env_offset + e), (uint64_t)w);
  double ret = 0.0, wn = 0.0, wmean[HP_CPL], wm2[HP_CPL], x_before = 0.0;
#pragma unroll
  for (int i = 0; i < HP_CPL; ++i) wmean[i] = wm2[i] = 0.0;
  int len = 0, t = 0, sub = 0;
  bool terminated = false, first = true;

  // pass `sub` of step t: sub = 0 starts the step from forward() of its state (and closes the
  // step before), every pass is one substep
  for (;;) {
    hm::forward(W, S, lane);
    if (sub == 0) {
      if (!first) {
        double rew;
        bool done;
        hm::reward_done(W, lane, x_before, rew, done);
        if (t < p.io.trace_steps && lane == 0) p.io.trace_rew[(int64_t)t * N + e] = rew;
        ret += rew;
        len = t + 1;
        terminated = done || (t + 1 >= EnvC<MRL_ENV_HUMANOID>::MAX_STEPS);
        ++t;
        if (terminated || t >= p.limit) break;
      }
      first = false;
      x_before = W.com[0];
      hm::observation(W, S, lane, [&](int k, double v) { X.od[k] = v; });
      WAVE_SYNC();
      const bool tr = t < p.io.trace_steps;
      double* const orow = p.io.trace_obs + ((int64_t)t * N + e) * O;
      wn += 1.0;
#pragma unroll
      for (int i = 0; i < HP_CPL; ++i) {
        const int k = lane + 64 * i;
        if (k < O) {
          const double o = X.od[k];
          if (tr) orow[k] = o;
          welford_add(o, wn, wmean[i], wm2[i]);
          X.x[k] = pop_filtered(o, fmean[k], fden[k]);
        }
      }
      WAVE_SYNC();
      const float z = hp_policy(p, th, X, lane);
      if (lane < A) {
        if (tr) reinterpret_cast<float*>(p.io.trace_act)[((int64_t)t * N + e) * A + lane] = z;
        W.s[HM_NQ + HM_NV + lane] = (double)z;
      }
      WAVE_SYNC();
    }
    hm::accelerations(W, S, lane);
    hm::integrate(W, lane);
    sub = sub + 1 == hm::FRAME_SKIP ? 0 : sub + 1;
  }

  // W holds forward() of the final state: the state rows and their kinematics cache
  if (lane == 0) {
    p.io.ret[e] = ret;
    p.io.len[e] = len;
    p.io.flags[e] = (uint8_t)(1 | (terminated ? 2 : 0));
    a.b.env_int[e] = len;
    a.b.env_int[N + e] = (int32_t)(w + 1);
  }
  double* st = p.io.stat + (int64_t)e * (1 + 2 * O);
  if (lane == 0) st[0] = wn;
#pragma unroll
  for (int i = 0; i < HP_CPL; ++i) {
    const int k = lane + 64 * i;
    if (k < O) {
      st[1 + k] = wmean[i];
      st[1 + O + k] = wm2[i];
    }
  }
  if (lane < HM_NS) a.b.env_state[(int64_t)lane * N + e] = W.s[lane];
  hm::save_kcache(W, a.b.env_state + (int64_t)HM_NS * N + (int64_t)e * HM_KCACHE, lane);
}

}  // namespace mrl

using namespace mrl;

// 1: a net this kernel takes; 0: another env or shape; E_ARG
extern "C" int32_t mrl_pop_rollout_wave_fits(int32_t env_id, const int32_t* hid_sizes, int32_t n_hid) {
  PopSmallShape sh;
  const char* what = nullptr;
  const int rc = pop_net_shape(env_id, hid_sizes, n_hid, true, sh, what);
  if (rc == E_ARG) return fail(E_ARG, std::string("mrl_pop_rollout_wave_fits: ") + what);
  return rc == OK ? 1 : 0;
}

extern "C" int mrl_pop_rollout_wave(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, const int32_t* hid_sizes,
                                    int32_t n_hid, const float* thetas, int64_t ld_theta, const double* filter_state,
                                    const mrl_pop_io* io, void* stream) {
  const char* what = pop_check_args(d, b, pop_check_hid(hid_sizes, n_hid), thetas, io);
  if (what) return fail(E_ARG, std::string("mrl_pop_rollout_wave: ") + what);
  PopSmallShape net;
  const int rc = pop_net_shape(d->env_id, hid_sizes, n_hid, true, net, what);
  if (rc) return fail(rc, std::string("mrl_pop_rollout_wave: ") + what);
  if (ld_theta != 0 && ld_theta < pop_num_params(env_info(d->env_id), net.PU))
    return fail(E_ARG, "mrl_pop_rollout_wave: ld_theta is neither 0 nor >= the parameter count");
  RollArgs a = make_args(d, b);
  HmPopArgs p;
  p.sh = net.sh;
  pop_fill(p, d, thetas, ld_theta, filter_state, io);
  MRL_LAUNCH_HM(hm_pop_rollout_kernel, hm_pop_lds_bytes, d->n_envs, (hipStream_t)stream, a, p);
  return hip_check(hipGetLastError(), "mrl_pop_rollout_wave");
}
