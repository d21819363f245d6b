// Advantage scan, its moments, standardisation and the value-function target.
//
// GAE (core.py:63-75 + misc_utils.py:9-27 `discount` via scipy lfilter): on
// time-major [T, E] rows the per-path reverse recurrences
//     adv_t = delta_t + gamma*lam*cont_t*adv_{t+1},  ret_t = r_t + gamma*cont_t*ret_{t+1}
// are linear, so each (chunk of L steps, env) is summarised as an affine map
// (A, B): adv_in = A + B*adv_out, and chunks compose by a parallel scan.
// One pass: r / v / flags are read once, adv / ret written once (17 B per row).
// Scans run in fp64 like lfilter; outputs are fp32.
#include <math.h>
#include <stdlib.h>

#include "../../include/mrl_hip.h"
#include "block_reduce.h"
#include "mrl_common.h"
#include "vector_host.h"

namespace mrl {

// One block owns GAE_EB envs over the whole horizon: thread (c, e) holds chunk c
// (GAE_L consecutive steps) of env e in registers, so every load of the scan is
// issued up front (a wave instruction covers 4 rows x 64 B) and r / v / flags are
// read from HBM exactly once.  Each chunk is summarised as the affine map of its
// recurrence, one wave per env composes the GAE_NC chunk maps with a reverse
// shuffle scan, and each thread re-runs its chunk from the carried-in value and
// writes adv / ret.  Horizons longer than GAE_NC * L run as segments from the
// last to the first, the carry held by the env's scan wave.
constexpr int GAE_EB = 16;               // envs per block: one 64 B row segment
constexpr int GAE_NC = 32;               // chunks per segment: one per lane of a half-wave (32) or wave (64)
static_assert(GAE_NC == 32 || GAE_NC == 64, "scan groups are half-waves or waves");
constexpr int GAE_THREADS = GAE_EB * GAE_NC;
constexpr int GAE_LMAX = 32;             // longest chunk (dispatch_chunk_len's largest)
constexpr int GAE_PITCH = GAE_EB + 1;    // LDS row pitch (doubles): 2-way conflicts at most

template <int L>
__global__ __launch_bounds__(GAE_THREADS) void gae_scan_kernel(const float* __restrict__ rew,
                                                               const float* __restrict__ v,
                                                               const uint8_t* __restrict__ flags, int64_t T,
                                                               int64_t E, double gamma, double lam,
                                                               float* __restrict__ adv, float* __restrict__ ret,
                                                               double* __restrict__ part) {
  __shared__ double sA[GAE_NC * GAE_PITCH], sB[GAE_NC * GAE_PITCH], sR[GAE_NC * GAE_PITCH],
      sC[GAE_NC * GAE_PITCH];
  __shared__ double red[2][GAE_THREADS / 64];
  const int tid = threadIdx.x;
  const int el = tid % GAE_EB, c = tid / GAE_EB;
  const int64_t blk = xcd_segment(blockIdx.x, gridDim.x);  // env segment of this block
  const int64_t e = blk * GAE_EB + el;
  const bool live = e < E;
  const double gl = gamma * lam;
  const int64_t S = (int64_t)GAE_NC * L;
  const int64_t nseg = (T + S - 1) / S;
  const int lane = tid & 63, wave = tid >> 6;
  const int sc = tid % GAE_NC, se = tid / GAE_NC;  // scan: a group of GAE_NC lanes = env slot se, lane = chunk sc
  double carry_a = 0.0, carry_r = 0.0;                    // held by the half-wave of env slot se
  double s1 = 0.0, s2 = 0.0;
  for (int64_t seg = nseg - 1; seg >= 0; --seg) {
    const int64_t t0 = seg * S + (int64_t)c * L;
    // uniform segment/block base + 32-bit per-lane offsets (S * E < 2^29, checked on the host)
    const int64_t base = seg * S * E + blk * GAE_EB;
    const float* rb = rew + base;
    const float* vb = v + base;
    const uint8_t* fb = flags + base;
    // branch-free loads: rows past T and envs past E read a clamped valid element
    // and are masked where they are used
    const int64_t rows = min(S, T - seg * S);  // rows of this segment
    const int elc = (int)min((int64_t)el, E - 1 - blk * GAE_EB);
    auto off = [&](int row) -> uint32_t {  // byte offset of (row, env) from the base, float elements
      const int rc = row < rows ? row : (int)rows - 1;
      return ((uint32_t)rc * (uint32_t)E + (uint32_t)elc) * 4u;
    };
    float rr[L], vv[L];
    uint8_t ff[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const uint32_t o = off(c * L + j);
      rr[j] = *(const float*)((const char*)rb + o);
      vv[j] = *(const float*)((const char*)vb + o);
      ff[j] = fb[o >> 2];
    }
    const int64_t tn = t0 + L;  // first row of the next chunk (may sit in the next segment)
    const float vnext = (live && tn < T) ? v[tn * E + e] : 0.f;
    // delta_t and the continuation flag of step j of this chunk
    auto step = [&](int j, bool& cont) -> double {
      const int64_t t = t0 + j;
      cont = !(ff[j] & 1) && (t + 1 < T);
      const double vt = (double)vv[j];
      const double vn = (j + 1 < L) ? (double)vv[j + 1 < L ? j + 1 : j] : (double)vnext;
      // bootstrap b1[t+1]: next baseline inside the episode, 0 if terminated, else b[-1] (core.py:73)
      const double boot = cont ? vn : ((ff[j] & 2) ? 0.0 : vt);
      return (double)rr[j] + gamma * boot - vt;
    };
    // chunk summary: adv_in = A + B * adv_out, ret_in = R + C * ret_out
    double A = 0.0, B = 1.0, R = 0.0, Cc = 1.0;
#pragma unroll
    for (int j = L - 1; j >= 0; --j) {
      if (t0 + j < T) {
        bool cont;
        const double d = step(j, cont);
        const double kk = cont ? 1.0 : 0.0;
        A = d + gl * kk * A;
        B = gl * kk * B;
        R = (double)rr[j] + gamma * kk * R;
        Cc = gamma * kk * Cc;
      }
    }
    sA[c * GAE_PITCH + el] = A;
    sB[c * GAE_PITCH + el] = B;
    sR[c * GAE_PITCH + el] = R;
    sC[c * GAE_PITCH + el] = Cc;
    __syncthreads();
    {
      // reverse inclusive scan of the maps of env slot se over its chunks (lane = chunk)
      double a = sA[sc * GAE_PITCH + se], b = sB[sc * GAE_PITCH + se];
      double r = sR[sc * GAE_PITCH + se], cc = sC[sc * GAE_PITCH + se];
#pragma unroll
      for (int off = 1; off < GAE_NC; off <<= 1) {
        const double a2 = __shfl_down(a, off), b2 = __shfl_down(b, off);
        const double r2 = __shfl_down(r, off), c2 = __shfl_down(cc, off);
        if (sc + off < GAE_NC) {
          a = a + b * a2;
          b = b * b2;
          r = r + cc * r2;
          cc = cc * c2;
        }
      }
      // exclusive: the composite of the later chunks, applied to the segment carry
      double xa = __shfl_down(a, 1), xb = __shfl_down(b, 1), xr = __shfl_down(r, 1), xc = __shfl_down(cc, 1);
      if (sc == GAE_NC - 1) { xa = 0.0; xb = 1.0; xr = 0.0; xc = 1.0; }
      const double in_a = xa + xb * carry_a, in_r = xr + xc * carry_r;
      const int l0 = lane & (64 - GAE_NC);  // the group's chunk 0 (lane 32 or 0 of a half-wave, 0 of a wave)
      const double a0 = __shfl(a, l0), b0 = __shfl(b, l0), r0 = __shfl(r, l0), c0 = __shfl(cc, l0);
      carry_a = a0 + b0 * carry_a;
      carry_r = r0 + c0 * carry_r;
      __syncthreads();  // every summary read before the carries overwrite them
      sA[sc * GAE_PITCH + se] = in_a;
      sR[sc * GAE_PITCH + se] = in_r;
    }
    __syncthreads();
    double a = sA[c * GAE_PITCH + el], r = sR[c * GAE_PITCH + el];
    float* ab = adv + base;
    float* tb = ret + base;
#pragma unroll
    for (int j = L - 1; j >= 0; --j) {
      if (live && t0 + j < T) {
        bool cont;
        const double dj = step(j, cont);
        const double kk = cont ? 1.0 : 0.0;
        a = dj + gl * kk * a;
        r = (double)rr[j] + gamma * kk * r;
        const float af = (float)a;
        const uint32_t o = off(c * L + j);
        *(float*)((char*)ab + o) = af;
        *(float*)((char*)tb + o) = (float)r;
        s1 += (double)af;
        s2 += (double)af * (double)af;
      }
    }
    __syncthreads();  // LDS reused by the next (earlier) segment
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
  }
  if (lane == 0) {
    red[0][wave] = s1;
    red[1][wave] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int w = 0; w < GAE_THREADS / 64; ++w) {
      t1 += red[0][w];
      t2 += red[1][w];
    }
    part[blk * 2 + 0] = t1;
    part[blk * 2 + 1] = t2;
  }
}

// The exact-fit form (round 6): T = GAE_NC * L (one segment) and E a multiple of GAE_EB
// -- the benchmark's 1024 x 4096.  Same per-row arithmetic and summation order as
// gae_scan_kernel, rebuilt for instruction count (that kernel issues ~100 instructions per
// row: per-lane bounds clamps, 64-bit address arithmetic per load, the delta recomputed
// in the second pass; at 16 K rows per CU its VALU time alone is ~10 us):
//  * no bounds: every load / store is a uniform row base (SGPR) + one per-lane 32-bit
//    offset fixed for the thread's chunk;
//  * loads issued in consumption order (the chunk's last step first), so the summary pass
//    starts on the first rows to land instead of the last;
//  * delta_t kept in registers (fp64) for the second pass; the chunk maps' multipliers
//    B, C are gl^L / gamma^L unless the chunk breaks (0): no per-row products;
//  * the moments' final sum rides in the last block to finish (a ticket counter; the
//    partials handed over as sc1 granules, MI355X_MICROARCH.md's hand-off table, row 1),
//    so there is no second launch.
typedef uint32_t gran4_t __attribute__((ext_vector_type(4)));  // one 16-B granule

template <int L>
__global__ __launch_bounds__(GAE_THREADS) void gae_full_kernel(const float* __restrict__ rew,
                                                               const float* __restrict__ v,
                                                               const uint8_t* __restrict__ flags, int64_t E,
                                                               double gamma, double lam, float* __restrict__ adv,
                                                               float* __restrict__ ret, double* __restrict__ part,
                                                               uint32_t* __restrict__ ticket,
                                                               double* __restrict__ moments, double count) {
  __shared__ double sA[GAE_NC * GAE_PITCH], sB[GAE_NC * GAE_PITCH], sR[GAE_NC * GAE_PITCH],
      sC[GAE_NC * GAE_PITCH];
  __shared__ double red[2][GAE_THREADS];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int el = tid % GAE_EB, c = tid / GAE_EB;
  const int64_t blk = xcd_segment(blockIdx.x, gridDim.x);
  const double gl = gamma * lam;
  const int lane = tid & 63, wave = tid >> 6;
  const int sc = tid % GAE_NC, se = tid / GAE_NC;
  // byte offset of (row c*L, env) -- the same for every step j of the chunk; step j adds
  // the uniform j * E * 4 to the base pointer (T * E * 4 < 2^31, checked on the host)
  const uint32_t E4 = (uint32_t)E * 4u;
  const uint32_t o4 = ((uint32_t)(c * L) * (uint32_t)E + (uint32_t)(blk * GAE_EB + el)) * 4u;
  const bool lastc = c == GAE_NC - 1;
  // buffer resources: per access one VGPR offset (o4) + the row's uniform SGPR offset
  const int nbytes = (int)(GAE_NC * L * E4);
  const __amdgpu_buffer_rsrc_t rr_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rew), 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t vv_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(v), 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ff_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(flags), 0, nbytes / 4, 0x00020000);
  float rr[L], vv[L];
  uint32_t ff[L];
#pragma unroll
  for (int j = L - 1; j >= 0; --j) {
    const uint32_t rowb = (uint32_t)j * E4;
    rr[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr_rs, o4, rowb, 0));
    vv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vv_rs, o4, rowb, 0));
    ff[j] = __builtin_amdgcn_raw_buffer_load_b8(ff_rs, o4 >> 2, rowb >> 2, 0);
  }
  // v of the next chunk's first row (the last chunk's is never used: t + 1 = T)
  const float vnext = __builtin_bit_cast(
      float, __builtin_amdgcn_raw_buffer_load_b32(vv_rs, lastc ? o4 : o4 + (uint32_t)L * E4, 0, 0));
  double glL = 1.0, gL = 1.0;  // B, C of an unbroken chunk: the products gae_scan_kernel forms
#pragma unroll
  for (int j = 0; j < L; ++j) {
    glL = gl * glL;
    gL = gamma * gL;
  }
  double dd[L];
  double A = 0.0, R = 0.0;
  bool brk = false;
  double vn = (double)vnext;
  uint32_t fl[(L + 15) / 16] = {};  // the flags again, 2 bits per step, for the second pass
#pragma unroll
  for (int j = L - 1; j >= 0; --j) {
    fl[j >> 4] |= ff[j] << (2 * (j & 15));
    const bool cont = !(ff[j] & 1u) && !(lastc && j == L - 1);
    const double vt = (double)vv[j], rj = (double)rr[j];
    // bootstrap b1[t+1]: next baseline inside the episode, 0 if terminated, else b[-1] (core.py:73)
    const double boot = cont ? vn : ((ff[j] & 2u) ? 0.0 : vt);
    const double d = rj + gamma * boot - vt;
    dd[j] = d;
    A = d + (cont ? gl : 0.0) * A;
    R = rj + (cont ? gamma : 0.0) * R;
    brk = brk || !cont;
    vn = vt;
  }
  sA[c * GAE_PITCH + el] = A;
  sB[c * GAE_PITCH + el] = brk ? 0.0 : glL;
  sR[c * GAE_PITCH + el] = R;
  sC[c * GAE_PITCH + el] = brk ? 0.0 : gL;
  __syncthreads();
  {
    // reverse inclusive scan of env slot se's chunk maps (lane = chunk): gae_scan_kernel's,
    // line for line, with a zero carry (x + y * 0.0 kept as written: it is not x for -0, inf
    // or NaN).  A fix to one copy goes into the other; shared as a function, both kernels
    // compile to other (equivalent) code, and this file keeps every kernel's code as it was.
    double a = sA[sc * GAE_PITCH + se], b = sB[sc * GAE_PITCH + se];
    double r = sR[sc * GAE_PITCH + se], cc = sC[sc * GAE_PITCH + se];
#pragma unroll
    for (int off = 1; off < GAE_NC; off <<= 1) {
      const double a2 = __shfl_down(a, off), b2 = __shfl_down(b, off);
      const double r2 = __shfl_down(r, off), c2 = __shfl_down(cc, off);
      if (sc + off < GAE_NC) {
        a = a + b * a2;
        b = b * b2;
        r = r + cc * r2;
        cc = cc * c2;
      }
    }
    double xa = __shfl_down(a, 1), xb = __shfl_down(b, 1), xr = __shfl_down(r, 1), xc = __shfl_down(cc, 1);
    if (sc == GAE_NC - 1) { xa = 0.0; xb = 1.0; xr = 0.0; xc = 1.0; }
    const double in_a = xa + xb * 0.0, in_r = xr + xc * 0.0;
    __syncthreads();
    sA[sc * GAE_PITCH + se] = in_a;
    sR[sc * GAE_PITCH + se] = in_r;
  }
  __syncthreads();
  double a = sA[c * GAE_PITCH + el], r = sR[c * GAE_PITCH + el];
  double s1 = 0.0, s2 = 0.0;
  const __amdgpu_buffer_rsrc_t adv_rs = __builtin_amdgcn_make_buffer_rsrc(adv, 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ret_rs = __builtin_amdgcn_make_buffer_rsrc(ret, 0, nbytes, 0x00020000);
#pragma unroll
  for (int j = L - 1; j >= 0; --j) {
    const bool cont = !((fl[j >> 4] >> (2 * (j & 15))) & 1u) && !(lastc && j == L - 1);
    a = dd[j] + (cont ? gl : 0.0) * a;
    r = (double)rr[j] + (cont ? gamma : 0.0) * r;
    const float af = (float)a;
    const uint32_t rowb = (uint32_t)j * E4;
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, af), adv_rs, o4, rowb, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, (float)r), ret_rs, o4, rowb, 0);
    s1 += (double)af;
    s2 += (double)af * (double)af;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
  }
  if (lane == 0) {
    red[0][wave] = s1;
    red[1][wave] = s2;
  }
  __syncthreads();
  const int64_t nb = gridDim.x;
  __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(part, 0, (int)(nb * 16), 0x00020000);
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int w = 0; w < GAE_THREADS / 64; ++w) {
      t1 += red[0][w];
      t2 += red[1][w];
    }
    // the block's partial as one sc1 granule, waited for, then the ticket (agent scope)
    const uint64_t b1 = (uint64_t)__double_as_longlong(t1), b2 = (uint64_t)__double_as_longlong(t2);
    const gran4_t g = {(uint32_t)b1, (uint32_t)(b1 >> 32), (uint32_t)b2, (uint32_t)(b2 >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(g, prs, (uint32_t)(blk * 16), 0, 16);  // aux 16 = sc1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t done = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = done == (uint32_t)(nb - 1);
  }
  __syncthreads();
  if (!is_last) return;
  // the last block: every partial through sc1 loads, summed in block order and then in
  // moments_final_kernel's tree (lds_tree_sum2), over GAE_THREADS lanes
  double t1 = 0.0, t2 = 0.0;
  for (int64_t i = tid; i < nb; i += GAE_THREADS) {
    const gran4_t g = __builtin_amdgcn_raw_buffer_load_b128(prs, (uint32_t)(i * 16), 0, 16);
    t1 += __longlong_as_double((long long)(((uint64_t)g.y << 32) | g.x));
    t2 += __longlong_as_double((long long)(((uint64_t)g.w << 32) | g.z));
  }
  lds_tree_sum2<GAE_THREADS>(t1, t2, red[0], red[1]);
  if (tid == 0) {
    moments[0] = red[0][0];
    moments[1] = red[1][0];
    moments[2] = count;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  }
}

// ------------------------------------------------------------------ moments
// per-block fp64 (sum, sumsq) of (a - b - shift) -> part[block][2]; shift = center[0] /
// center[2] (a previous pass's mean) or 0
__global__ void moments_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                               const double* __restrict__ center, double* __restrict__ part) {
  __shared__ double red[2][256];
  const double shift = center ? center[0] / center[2] : 0.0;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = (double)a[i] - (b ? (double)b[i] : 0.0) - shift;
    s1 += v;
    s2 += v * v;
  }
  lds_tree_sum2<256>(s1, s2, red[0], red[1]);
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = red[0][0];
    part[blockIdx.x * 2 + 1] = red[1][0];
  }
}

__global__ void moments_final_kernel(const double* __restrict__ part, int64_t nb, double count,
                                     double* __restrict__ moments) {
  __shared__ double red[2][256];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += 256) {
    s1 += part[i * 2];
    s2 += part[i * 2 + 1];
  }
  lds_tree_sum2<256>(s1, s2, red[0], red[1]);
  if (threadIdx.x == 0) {
    moments[0] = red[0][0];
    moments[1] = red[1][0];
    moments[2] = count;
  }
}

// mom = (sum, sumsq, n) of the first pass; cmom = (sum, sumsq, n) of (adv - mom[0]/mom[2]),
// the second pass of numpy's two-pass std (core.py:100-105): the centred sums do not
// cancel when |mean| >> std.  Without cmom the single-pass form is used.
__global__ void standardize_kernel(float* __restrict__ adv, int64_t n, const double* __restrict__ mom,
                                   const double* __restrict__ cmom) {
  const double mean0 = mom[0] / mom[2];
  double mean, var;
  if (cmom) {
    const double d = cmom[0] / cmom[2];  // residual of the shift (rounding of mean0)
    mean = mean0 + d;
    var = fmax(cmom[1] / cmom[2] - d * d, 0.0);
  } else {
    mean = mean0;
    var = fmax(mom[1] / mom[2] - mean * mean, 0.0);
  }
  const double stdv = sqrt(var);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    adv[i] = (float)(((double)adv[i] - mean) / stdv);
}

__global__ void vf_target_kernel(const float* __restrict__ ret, const float* __restrict__ vp, double mixfrac, int64_t n,
                                 float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = (float)((double)ret[i] * mixfrac + (double)vp[i] * (1.0 - mixfrac));
}

}  // namespace mrl

using namespace mrl;

extern "C" {

// workspace: [nb fp64 (sum, sumsq) block partials][pad to 64 B][u32 completion ticket]
static int64_t gae_ticket_offset(int64_t E) {
  const int64_t nb = (E + GAE_EB - 1) / GAE_EB;
  return (nb * 2 * (int64_t)sizeof(double) + 63) / 64 * 64;
}

int64_t mrl_gae_workspace_bytes(int64_t T, int64_t E) {
  (void)T;
  if (E <= 0) return 128;
  return gae_ticket_offset(E) + 64;
}

int mrl_gae(const float* rew, const float* vpred, const uint8_t* flags, int64_t T, int64_t E, double gamma, double lam,
            float* adv, float* ret, double* moments, void* workspace, void* stream) {
  if (!rew || !vpred || !flags || !adv || !ret || !moments || !workspace) return fail(E_ARG, "null pointer");
  if (T <= 0 || E <= 0) return OK;
  const int64_t nb = (E + GAE_EB - 1) / GAE_EB;
  if ((int64_t)GAE_NC * GAE_LMAX * (E + GAE_EB) >= ((int64_t)1 << 29))
    return fail(E_UNSUPPORTED, "mrl_gae: E too large for 32-bit segment offsets");
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int L = chunk_len(T, GAE_NC, GAE_LMAX);
  // MRL_GAE_GENERAL=1 (tests / A-B probes): the general kernel for every shape; read at
  // every call (the tests flip it between calls)
  const char* general_env = getenv("MRL_GAE_GENERAL");
  const bool general_only = general_env && general_env[0] == '1';
  if (!general_only && T == (int64_t)GAE_NC * L && E % GAE_EB == 0 && T * E * 4 < ((int64_t)1 << 31)) {
    // exact fit: one pass, the moments finished by the last block (gae_full_kernel)
    uint32_t* ticket = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + gae_ticket_offset(E));
    dispatch_chunk_len(L, [&](auto l) {
      hipLaunchKernelGGL(gae_full_kernel<l()>, dim3(nb), dim3(GAE_THREADS), 0, s, rew, vpred, flags, E, gamma, lam, adv,
                         ret, part, ticket, moments, (double)(T * E));
    });
    return hip_check(hipGetLastError(), "mrl_gae");
  }
  dispatch_chunk_len(L, [&](auto l) {
    hipLaunchKernelGGL(gae_scan_kernel<l()>, dim3(nb), dim3(GAE_THREADS), 0, s, rew, vpred, flags, T, E, gamma, lam,
                       adv, ret, part);
  });
  hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(256), 0, s, part, nb, (double)(T * E), moments);
  return hip_check(hipGetLastError(), "mrl_gae");
}

int mrl_standardize(float* adv, int64_t n, const double* moments, const double* cmoments, void* stream) {
  if (!adv || !moments) return fail(E_ARG, "null pointer");
  if (n <= 0) return OK;
  hipLaunchKernelGGL(standardize_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, adv, n, moments,
                     cmoments);
  return hip_check(hipGetLastError(), "mrl_standardize");
}

int mrl_vf_target(const float* ret, const float* vpred, double mixfrac, int64_t n, float* y, void* stream) {
  if (!ret || !vpred || !y) return fail(E_ARG, "null pointer");
  if (n <= 0) return OK;
  hipLaunchKernelGGL(vf_target_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, ret, vpred, mixfrac, n, y);
  return hip_check(hipGetLastError(), "mrl_vf_target");
}

int64_t mrl_moments_workspace_bytes(int64_t n) { return grid_for(n, 256, 1024) * 2 * (int64_t)sizeof(double); }

int mrl_moments_centered(const float* a, const float* b, int64_t n, const double* center, double* out,
                         void* workspace, void* stream) {
  if (!a || !out || !workspace) return fail(E_ARG, "null pointer");
  if (n <= 0) return fail(E_ARG, "mrl_moments: empty input");
  const int64_t g = grid_for(n, 256, 1024);
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(moments_kernel, dim3(g), dim3(256), 0, s, a, b, n, center, part);
  hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(256), 0, s, part, g, (double)n, out);
  return hip_check(hipGetLastError(), "mrl_moments");
}

int mrl_moments(const float* a, const float* b, int64_t n, double* out, void* workspace, void* stream) {
  return mrl_moments_centered(a, b, n, nullptr, out, workspace, stream);
}

}  // extern "C"
