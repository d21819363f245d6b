// The fused rollout's filter statistics: a block's Welford partial of its envs' raw
// observations and rewards, its hand-off to the other blocks -- records in memory between step
// launches, data-tagged granules inside the persistent launch -- the merge of all blocks'
// partials into one batch, and the filtered observation of an env row.  Used by the kernels of
// rollout_kernels.h and by rollout.hip's finish kernel.
#pragma once
#include "rollout_device.h"

namespace mrl {

// per-block two-pass (mean, M2) partial of vals[ENVS_PER_BLOCK][D] (doubles in LDS):
// thread (k = tid/16, j = tid%16) covers envs j, j+16, ...; 16-lane butterflies.
// column k's (mean, M2) over the block's nvalid envs: lane j adds envs j, j + 16, j + 32,
// j + 48 in that order, then the 16-lane butterflies.  The four values are read from LDS
// together and kept for the M2 pass (one LDS round trip instead of eight dependent ones);
// a term past nvalid is skipped, as the loop over i < nvalid did
__device__ inline void block_moments(const double* vals, int nvalid, int D, int k, int j, double& mean, double& m2) {
  constexpr int Q = ENVS_PER_BLOCK / 16;
  const int kk = k < D ? k : D - 1;
  double v[Q];
  bool in[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = j + 16 * q;
    in[q] = k < D && i < nvalid;
    v[q] = vals[(i < nvalid ? i : 0) * D + kk];
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (in[q]) s += v[q];
  mean = nvalid > 0 ? div_count(sum16(s), (double)nvalid) : 0.0;
  double m = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (in[q]) {
      const double dv = v[q] - mean;
      m += dv * dv;
    }
  m2 = sum16(m);
}

// The 16 thread groups take columns K0 .. K0 + 15.  An env with more than COLS columns
// (HalfCheetah: 17 obs + the reward) makes a second pass with K0 = COLS, whose first groups
// take columns 16 .. D - 1 (the counts r[0], r[1] are column 0's, so the first pass's).
// K0 is a template argument: as a function argument, even one that is 0 everywhere, it
// changed the address arithmetic of every existing kernel.
constexpr int COLS = RB / 16;
constexpr int col_slots(int D) { return D > MAXD ? D : MAXD; }
template <int K0 = 0>
__device__ inline void publish_partial(const RollArgs& a, const double* vals, int nvalid, int D, bool with_rew,
                                       double* rec_out) {
  const int k = K0 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  double mean, m2;
  block_moments(vals, nvalid, D, k, j, mean, m2);
  if (k < D && j == 0) {
    double* r = rec_out + (int64_t)blockIdx.x * a.RS;
    r[2 + k] = mean;
    r[2 + D + k] = m2;
    if (k == 0) {
      r[0] = (double)nvalid;
      r[1] = with_rew ? (double)nvalid : 0.0;
    }
  }
}

// combine the per-block records of one column k into a batch (n, mean, M2):
// mean = sum n_b mean_b / n ; M2 = sum (M2_b + n_b (mean_b - mean)^2).
// Called by all 16 lanes of thread group k; every lane returns the same values.
// Lane j holds records j + 16q of a round (RB_MAX per lane, 128 blocks = 8192 envs).
constexpr int RB_MAX = 8;
template <int R>
struct RecRoundT {
  double rn[R], rm[R], rs[R];
  __device__ void load(const double* rec, int nb, int RS, int D, int O, int k, int j, int b0) {
    const bool isr = (k == O);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int b = b0 + j + 16 * q;
      const double* r = rec + (int64_t)(b < nb ? b : 0) * RS;
      rn[q] = b < nb ? r[isr ? 1 : 0] : 0.0;
      rm[q] = b < nb ? r[2 + k] : 0.0;
      rs[q] = b < nb ? r[2 + D + k] : 0.0;
    }
  }
  __device__ void accumulate(double& n, double& sm, double& raw) const {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      n += rn[q];
      sm += rn[q] * rm[q];
      raw += rs[q] + rn[q] * rm[q] * rm[q];
    }
  }
  // one-round batch (nb <= 16 * R): exact two-pass form from registers
  __device__ void batch(double& bn, double& bm, double& bs) const {
    double n = 0.0, sm = 0.0, raw = 0.0;
    accumulate(n, sm, raw);
    n = sum16(n);
    sm = sum16(sm);
    const double mean = n > 0.0 ? div_count(sm, n) : 0.0;
    double m2 = 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (rn[q] > 0.0) {
        const double dm = rm[q] - mean;
        m2 += rs[q] + rn[q] * dm * dm;
      }
    bn = n;
    bm = mean;
    bs = sum16(m2);
  }
};

using RecRound = RecRoundT<RB_MAX>;
// persistent rollout: 16 * RB_SMALL blocks (<= 4096 envs) gather in half the registers
constexpr int RB_SMALL = 4;

__device__ inline void batch_of_records(const double* rec, int nb, int RS, int D, int O, int k, int j, double& bn,
                                        double& bm, double& bs) {
  RecRound rr;
  if (nb <= 16 * RB_MAX) {
    rr.load(rec, nb, RS, D, O, k, j, 0);
    rr.batch(bn, bm, bs);
    return;
  }
  // many rounds: sum (M2_b + n_b mean_b^2) - n mean^2
  double n = 0.0, sm = 0.0, raw = 0.0;
  for (int b0 = 0; b0 < nb; b0 += 16 * RB_MAX) {
    rr.load(rec, nb, RS, D, O, k, j, b0);
    rr.accumulate(n, sm, raw);
  }
  n = sum16(n);
  sm = sum16(sm);
  const double mean = n > 0.0 ? div_count(sm, n) : 0.0;
  bn = n;
  bm = mean;
  bs = sum16(raw) - n * mean * mean;
}

// the filtered observation columns 4i + g of one env row (core.py:191-192: clip((o - mean)
// / (std + 1e-8), -5, 5)), as f32.  Every column's statistics are read from LDS before any
// arithmetic and the stores are left to the caller, so the (O + 3) / 4 divisions are
// independent chains rather than one LDS round trip + division per branchy store block
// (the same operations per value)
template <int ENV>
__device__ inline void filtered_obs(const double* s, int g, bool filter, const double* fmean, const double* fden,
                                    float* vf) {
  constexpr int O = EnvC<ENV>::OBS, NI = (O + 3) / 4;
  double o[O];
  EnvC<ENV>::obs(s, o);
  double v[NI], mu[NI], den[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    v[i] = o[4 * i];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (4 * i + q < O && g == q) v[i] = o[4 * i + q < O ? 4 * i + q : O - 1];
  }
  if (filter) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int kc = 4 * i + g, kk = kc < O ? kc : O - 1;
      mu[i] = fmean[kk];
      den[i] = fden[kk];
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      double x = v[i] - mu[i];
      x = x / den[i];
      v[i] = x < -5.0 ? -5.0 : (x > 5.0 ? 5.0 : x);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) vf[i] = (float)v[i];
}

// ------------------------------------------------------------------ persistent hand-off
// The persistent kernel runs the whole horizon in ONE launch (mrl_rollout_run): the nb blocks
// of the step kernel stay resident (one block per CU of the launch stream's CU set) and loop
// over t.  Weights, env state, episode counters and the running stat live in registers for all
// T steps; the only cross-block
// dependency of a step -- the Welford partials of the E raw observations (and rewards)
// that every block merges into its copy of the running stat -- is handed off in memory
// as data-tagged granules: each (block, column) partial is ONE 16-B granule {fp64 mean,
// fp64 M2} written by a single write-through (sc1) store, the step tag riding in M2's
// sign bit (M2 >= 0); a consumer polls the granules themselves with sc1 loads until
// every tag carries the step it waits for, so one memory round trip both signals and
// delivers (MI355X_MICROARCH.md, hand-offs: untorn 16-B sc1 granules).  Counts are not
// sent: every block knows each block's number of envs.  Two parities as between step
// launches: block b can only overwrite the parity-p granule of gather step s at step
// s+2 after every block's step-s+1 granules arrived, i.e. after every block has read
// step s; so a slot only ever holds step s or s-2 (or the launch's memset zeros), and
// one tag bit that alternates between consecutive writes of a slot -- tag(s) =
// ((s >> 1) & 1) ^ 1, never the memset's 0 for s = 0, 1 -- tells them apart.
// Bit-identical to the step kernels.
constexpr int SYNC_ABORT = 32;             // u32 word: a block gave up waiting (own 128-B line)
constexpr int64_t SYNC_HEAD_BYTES = 256;   // then the granules: [2 parities][D][nb] x 16 B
constexpr uint32_t SPIN_LIMIT = 1u << 22;  // polls (~seconds): a non-resident grid exits

typedef uint32_t gran_t __attribute__((ext_vector_type(4)));  // one 16-B granule

__device__ inline uint32_t step_tag(int s) { return (((uint32_t)s >> 1) & 1u) ^ 1u; }

struct Granules {
  __amdgpu_buffer_rsrc_t rsrc;
  int nb, D;
  __device__ Granules(uint32_t* sync, int nb_, int D_) : nb(nb_), D(D_) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(sync) + SYNC_HEAD_BYTES, 0,
                                             2 * D_ * nb_ * 16, 0x00020000);
  }
  __device__ uint32_t off(int parity, int k, int b) const { return (uint32_t)(((parity * D + k) * nb + b) * 16); }
  __device__ void put(int step, int k, int b, double mean, double m2) const {
    const uint64_t mb = (uint64_t)__double_as_longlong(mean);
    const uint64_t sb = ((uint64_t)__double_as_longlong(m2) & ~(1ull << 63)) | ((uint64_t)step_tag(step) << 63);
    gran_t g = {(uint32_t)mb, (uint32_t)(mb >> 32), (uint32_t)sb, (uint32_t)(sb >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(g, rsrc, off(step & 1, k, b), 0, 16);  // aux 16 = sc1
  }
  __device__ gran_t get(int step, int k, int b) const {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, off(step & 1, k, b), 0, 16);
  }
};
__device__ inline double g_mean(gran_t g) { return __longlong_as_double((long long)(((uint64_t)g.y << 32) | g.x)); }
__device__ inline double g_m2(gran_t g) {
  return __longlong_as_double((long long)((((uint64_t)(g.w & 0x7fffffffu)) << 32) | g.z));
}
__device__ inline bool g_tag_is(gran_t g, int step) { return (g.w >> 31) == step_tag(step); }

// the block's (mean, M2) partial of vals[nvalid][D] (publish_partial's arithmetic) as
// the granules of gather step `step`; lane 0 of column group k writes column k's
// (K0: publish_partial's column pass)
template <int K0 = 0>
__device__ inline void publish_granules(const Granules& gr, const double* vals, int nvalid, int step) {
  const int k = K0 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  double mean, m2;
  block_moments(vals, nvalid, gr.D, k, j, mean, m2);
  if (k < gr.D && j == 0) gr.put(step, k, blockIdx.x, mean, m2);
}

// column k's records of blocks b0 + jj + 16q as RecRound registers, polled until every
// granule carries gather step `step`'s tag; n_b is known (envs of block b; 0 for the
// reward column of the reset partial).  false: the grid gave up (some block never
// published).
template <int R, class Under>
__device__ inline bool gather_granules(const Granules& gr, RecRoundT<R>& rr, int step, int k, int jj, int b0, int E,
                                       bool rew_counted, uint32_t* sync, Under&& under) {
  const bool isr = (k == gr.D - 1);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int b = b0 + jj + 16 * q;
    rr.rn[q] = (b < gr.nb && (!isr || rew_counted)) ? (double)min(ENVS_PER_BLOCK, E - b * ENVS_PER_BLOCK) : 0.0;
  }
  uint32_t it = 0;
  while (true) {
    gran_t gq[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int b = b0 + jj + 16 * q;
      gq[q] = gr.get(step, k, b < gr.nb ? b : 0);
    }
    if (it == 0) under();  // independent work while the first poll's loads are in flight
    bool ready = true;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const bool in = b0 + jj + 16 * q < gr.nb;
      ready = ready && (!in || g_tag_is(gq[q], step));
      rr.rm[q] = in ? g_mean(gq[q]) : 0.0;
      rr.rs[q] = in ? g_m2(gq[q]) : 0.0;
    }
    if (ready) return true;
    __builtin_amdgcn_s_sleep(1);
    if ((++it & 255) == 0 &&
        (it > SPIN_LIMIT || __hip_atomic_load(sync + SYNC_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      __hip_atomic_store(sync + SYNC_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

}  // namespace mrl
