// Batched lock-step rollout: E envs per GPU advance one step per launch, or the whole horizon
// in one persistent launch.
//
// Replaces the reference's serial per-step loop (core.py:182-221):
//     ob = agent.obfilt(ob)                 ZFilter, filters.py:30-38
//     action, {"prob"} = agent.act(ob)      StochPolicy.act, core.py:261-267
//     ob, rew, done, _ = env.step(action)   gym
//     agent.rewfilt(rew)                    stats only, core.py:198-199
//
// This unit is the fused 64-64 path: the training instantiations of the kernel templates of
// rollout_kernels.h (which tells what a step does), the kernels only this unit owns -- noise
// fill, image pack, finish, workspace clear -- and the C entry points.  The evaluation
// instantiations are rollout_eval.hip's.  The layered path is rollout_layered.hip, the
// stand-alone env stepper and obs filter env_api.hip, the population rollout cem.hip; what the
// units share is rollout_device.h (device code) and rollout_host.h (checks, dispatch).
#include "rollout_host.h"
#include "rollout_kernels.h"

namespace mrl {

// a whole iteration's sampling-noise rows (load_noise, rollout_device.h)
template <int ENV>
__global__ void noise_fill_kernel(RollArgs a, double* __restrict__ out) {
  using EC = EnvC<ENV>;
  constexpr int A = EC::ACT, P = EC::DISCRETE ? 1 : (A + 1) / 2;
  // grid (ceil(E * P / 256), min(T, 65535)): steps t = blockIdx.y + k * gridDim.y, no runtime
  // 64-bit division
  const int E = a.d.n_envs;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * P) return;
  const int c = i % P, e = i / P;
  for (int t = blockIdx.y; t < a.d.horizon; t += gridDim.y) {
    const int64_t row = (int64_t)t * E + e;
    const uint32_t gid = (uint32_t)(a.d.env_offset + e);
    const uint64_t w = (uint64_t)(*a.b.iteration) * (uint64_t)a.d.horizon + (uint64_t)t;
    double u0, u1;
    philox_uniform2(a.d.seed, 0, gid, w, (uint32_t)c, u0, u1);
    if constexpr (EC::DISCRETE) {
      out[row] = u0;
    } else {
      const double rad = sqrt(-2.0 * log(1.0 - u0));
      double sn, cn;
      sincos(2.0 * 3.141592653589793 * u1, &sn, &cn);
      out[row * A + 2 * c] = rad * cn;
      if (2 * c + 1 < A) out[row * A + 2 * c + 1] = rad * sn;
    }
  }
}

// rollout image: rimage_value (mlp_layout.h) of every element
// part p (0, 1, 2) of an f32 value's exact three-way bf16 split (mlp_split.hip)
__device__ inline float rb_part(float v, int p) {
  const __bf16 a = (__bf16)v;
  if (p == 0) return (float)a;
  const float r = v - (float)a;
  const __bf16 c = (__bf16)r;
  if (p == 1) return (float)c;
  return r - (float)c;
}

__global__ void rollout_pack_kernel(RDims r, MlpDims d, const float* __restrict__ th, float* __restrict__ out,
                                    int bf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < r.f32_size) {
    const float v = rimage_value(r, d, th, i);
    out[i] = (bf && i < r.b0) ? bf16r(v) : v;  // bf16 mode: the MFMA weights W0, W1
  } else if (i >= r.bs1 && i < r.size) {
    // split W1 fragments (fp32 mode): part p of the ba1 fragment elements, two per word
    const int rel = i - r.bs1, part = rel / (4 * 2 * 64 * 4), rr = rel % (4 * 2 * 64 * 4);
    const int frag = rr >> 2, q = rr & 3;
    const __bf16 lo = (__bf16)rb_part(rimage_bf16_elem(d, th, true, frag, 2 * q), part);
    const __bf16 hi = (__bf16)rb_part(rimage_bf16_elem(d, th, true, frag, 2 * q + 1), part);
    out[i] = __uint_as_float((uint32_t)__builtin_bit_cast(uint16_t, lo) |
                             ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16));
  } else if (i < r.size) {
    // bf16 fragments: two bf16 per word
    const bool l1 = i >= r.ba1;
    const int rel = i - (l1 ? r.ba1 : r.ba0), frag = rel >> 2, q = rel & 3;
    const __bf16 lo = (__bf16)rimage_bf16_elem(d, th, l1, frag, 2 * q);
    const __bf16 hi = (__bf16)rimage_bf16_elem(d, th, l1, frag, 2 * q + 1);
    out[i] = __uint_as_float((uint32_t)__builtin_bit_cast(uint16_t, lo) |
                             ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16));
  }
}

__global__ void rollout_finish_kernel(RollArgs a, int O) {
  const int D = O + 1, T = a.d.horizon;
  const double* fs_in = a.b.filter_state + (T & 1) * a.FS;
  double* fs_out = a.b.filter_state;
  const double* rec_in = a.b.records + (int64_t)(T & 1) * a.nb * a.RS;
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  // the last step's rewards still go through rewfilt (core.py:199); obs_T is never pushed
  double n = 0.0, M = 0.0, S = 0.0;
  if (g == 0) {
    n = fs_in[1];
    M = fs_in[2 + O];
    S = fs_in[2 + D + O];
    double bn, bm, bs;
    batch_of_records(rec_in, a.nb, a.RS, D, O, O, j, bn, bm, bs);
    chan_merge(n, M, S, bn, bm, bs);
  }
  // copy the obs stat when fs_in is the other buffer (T odd)
  double cp[(MAXD_L + RB - 1) / RB * 2 + 1];
  int nc = 0;
  if ((T & 1) != 0)
    for (int k = threadIdx.x; k < O; k += RB) {
      cp[nc++] = fs_in[2 + k];
      cp[nc++] = fs_in[2 + D + k];
    }
  const double n_obs = fs_in[0];
  __syncthreads();  // fs_in may alias fs_out (T even)
  if ((T & 1) != 0) {
    nc = 0;
    for (int k = threadIdx.x; k < O; k += RB) {
      fs_out[2 + k] = cp[nc++];
      fs_out[2 + D + k] = cp[nc++];
    }
    if (threadIdx.x == 0) fs_out[0] = n_obs;
  }
  if (g == 0 && j == 0) {
    fs_out[1] = n;
    fs_out[2 + O] = M;
    fs_out[2 + D + O] = S;
  }
  if (threadIdx.x == 0) *a.b.iteration += 1;
}

}  // namespace mrl

using namespace mrl;

extern "C" {

// Humanoid: the state (SoA [NS][E]) and then each env's kinematics cache (AoS [E][KCACHE],
// humanoid.h save_kcache) -- the forward kinematics of the stored state
int64_t mrl_env_state_doubles(int32_t env_id) {
  return env_info(env_id).ns + (env_id == MRL_ENV_HUMANOID ? HM_KCACHE : 0);
}
int64_t mrl_filter_doubles(int32_t env_id) { return filt_doubles(env_info(env_id).obs); }
int64_t mrl_record_doubles(int32_t env_id) { return filt_doubles(env_info(env_id).obs); }
int64_t mrl_rollout_blocks(int32_t n_envs) { return env_blocks(n_envs); }
int64_t mrl_rollout_noise_doubles(const mrl_rollout_desc* d) {
  if (!d || d->n_envs <= 0 || d->horizon <= 0) return -1;
  if (roll_eval(d)) return 0;  // the head's mode: no noise is drawn
  const EnvInfo ei = env_info(d->env_id);
  return (int64_t)d->horizon * d->n_envs * (ei.discrete ? 1 : ei.act);
}

int mrl_rollout_noise(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, double* out, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (!out) return fail(E_ARG, "null noise rows");
  if (roll_eval(d)) return fail(E_ARG, "mrl_rollout_noise: MRL_ROLLOUT_EVAL draws no noise");
  RollArgs a = make_args(d, b);
  const EnvInfo ei = env_info(d->env_id);
  const int64_t per_step = (int64_t)d->n_envs * (ei.discrete ? 1 : (ei.act + 1) / 2);
  MRL_DISPATCH_ENV(d->env_id, noise_fill_kernel, dim3((unsigned)((per_step + 255) / 256), (unsigned)(d->horizon < 65535 ? d->horizon : 65535)),
                   dim3(256), 0, (hipStream_t)stream, a, out);
  return hip_check(hipGetLastError(), "mrl_rollout_noise");
}

int mrl_rollout_reset(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (d->env_id == MRL_ENV_HUMANOID) return fail(E_UNSUPPORTED, "Humanoid runs on the layered rollout (mrl_rollout_reset_rows)");
  RollArgs a = make_args(d, b);
  if (roll_eval(d)) launch_rollout_reset_eval(a, (hipStream_t)stream);
  else MRL_DISPATCH_THREAD_ENV(d->env_id, rollout_reset_kernel, dim3(a.nb), dim3(RB), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "mrl_rollout_reset");
}

int64_t mrl_rollout_image_floats(const mrl_mlp_desc* pol) {
  if (!pol || pol->n_in <= 0 || pol->n_in > MAX_IN) return -1;
  return rollout_dims(pol->n_in).size;
}

int mrl_rollout_pack(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, float* rimage,
                     void* stream) {
  if (!d || !pol || !theta || !rimage) return fail(E_ARG, "null pointer");
  if (d->env_id == MRL_ENV_HUMANOID) return fail(E_UNSUPPORTED, "Humanoid runs on the layered rollout");
  int rc = check_fused_policy(d, pol);
  if (rc) return rc;
  const RDims r = rollout_dims(pol->n_in);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  hipLaunchKernelGGL(rollout_pack_kernel, dim3((r.size + 255) / 256), dim3(256), 0, (hipStream_t)stream, r, md, theta,
                     rimage, (int)(roll_compute(d) == MRL_COMPUTE_BF16));
  return hip_check(hipGetLastError(), "mrl_rollout_pack");
}

int64_t mrl_rollout_sync_bytes(const mrl_rollout_desc* d) {
  if (!d || d->n_envs <= 0) return -1;
  return SYNC_HEAD_BYTES + 2 * (int64_t)(env_info(d->env_id).obs + 1) * env_blocks(d->n_envs) * 16;
}

// Zeroes the hand-off workspace before a persistent launch (plain 16-B vector stores;
// the kernel boundary publishes them).  A kernel, not hipMemsetAsync: replayed from a
// captured hipGraph after other work had been launched eagerly, the memset node of
// ROCm 7.2 wrote a repeated 16-B pattern -- {int64 n, double 1/n}, bytes of a later
// eager launch's arguments -- instead of zeros.
__global__ __launch_bounds__(256) void sync_clear_kernel(uint4* __restrict__ p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The nb blocks fit one per CU of the launch stream (its CU mask) at this kernel's
// register use: the persistent launch may run (its blocks wait on each other, so the
// whole grid must be resident at once).  launch_cus > 0: the CUs of the stream a
// captured graph will replay on (the capture stream's mask says nothing about it);
// < 0: debug, no check.
static bool persistent_fits(int nb, hipStream_t s, int launch_cus) {
  if (launch_cus < 0) return true;
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return false;
  int cus = ncu;
  if (s != nullptr) {
    uint32_t mask[16] = {};
    const int words = (ncu + 31) / 32;
    if (words <= 16 && hipExtStreamGetCUMask(s, (uint32_t)words, mask) == hipSuccess) {
      cus = 0;
      for (int w = 0; w < words; ++w) cus += __builtin_popcount(mask[w]);
    }
  }
  if (launch_cus > 0) cus = min(launch_cus, ncu);
  return nb <= cus;
}

int mrl_rollout_run(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, const float* rimage,
                    const mrl_rollout_bufs* b, uint32_t* sync, int32_t persistent, void* stream) {
  int rc = check_fused_run(d, pol, theta, rimage, b);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  RollArgs a = make_args(d, b);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  const float* logstd = pol->head == MRL_HEAD_GAUSS ? theta + md.tls : nullptr;
  const bool bf = roll_compute(d) == MRL_COMPUTE_BF16, st = b->stamps != nullptr;
  if (roll_eval(d) && persistent) {
    launch_rollout_persistent_eval(a, bf, logstd, rimage, s);
    return hip_check(hipGetLastError(), "mrl_rollout_run");
  }
  if (!persistent || !sync || !persistent_fits(a.nb, s, d->launch_cus)) {
    rc = mrl_rollout_reset(d, b, stream);
    for (int32_t t = 0; t < d->horizon && rc == OK; ++t) rc = mrl_rollout_step(d, pol, theta, rimage, b, t, stream);
    return rc;
  }
  {
    const int64_t n16 = mrl_rollout_sync_bytes(d) / 16;  // SYNC_HEAD_BYTES + 16-B granules
    const int nblk = (int)std::min<int64_t>((n16 + 255) / 256, 256);
    hipLaunchKernelGGL(sync_clear_kernel, dim3(nblk), dim3(256), 0, s, reinterpret_cast<uint4*>(sync), n16);
  }
  // A plain launch: persistent_fits() guarantees one block per CU of the stream's CU
  // set, so every block becomes resident (kernels of other streams on those CUs finish
  // on their own), and the step hand-off polls are bounded (SPIN_LIMIT).  A cooperative
  // launch made HIP keep a runtime-owned queue that its teardown destroyed after an
  // attached rocprofv3 had finalised: the profiled process crashed at exit.
  dispatch_thread_env(d->env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      dispatch_bool(st, [&](auto ST) {
        hipLaunchKernelGGL((rollout_persistent_kernel<env(), BF(), ST()>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage,
                           sync);
      });
    });
  });
  return hip_check(hipGetLastError(), "mrl_rollout_run");
}

int mrl_rollout_step(const mrl_rollout_desc* d, const mrl_mlp_desc* pol, const float* theta, const float* rimage,
                     const mrl_rollout_bufs* b, int32_t t, void* stream) {
  int rc = check_fused_run(d, pol, theta, rimage, b);
  if (rc) return rc;
  if (t < 0 || t >= d->horizon) return fail(E_ARG, "t out of range");
  RollArgs a = make_args(d, b);
  const MlpDims md = mlp_dims(pol->n_in, pol->n_out, pol->head == MRL_HEAD_GAUSS);
  const float* logstd = pol->head == MRL_HEAD_GAUSS ? theta + md.tls : nullptr;
  const bool bf = roll_compute(d) == MRL_COMPUTE_BF16;
  hipStream_t s = (hipStream_t)stream;
  if (roll_eval(d)) {
    launch_rollout_step_eval(a, bf, logstd, rimage, t, s);
    return hip_check(hipGetLastError(), "mrl_rollout_step");
  }
  dispatch_thread_env(d->env_id, [&](auto env) {
    dispatch_bool(bf, [&](auto BF) {
      hipLaunchKernelGGL((rollout_step_kernel<env(), BF()>), dim3(a.nb), dim3(RB), 0, s, a, logstd, rimage, t);
    });
  });
  return hip_check(hipGetLastError(), "mrl_rollout_step");
}

int mrl_rollout_finish(const mrl_rollout_desc* d, const mrl_rollout_bufs* b, void* stream) {
  int rc = check_roll(d, b);
  if (rc) return rc;
  if (roll_eval(d)) return OK;  // no reward partial to fold, and the noise's step base stays
  RollArgs a = make_args(d, b);
  hipLaunchKernelGGL(rollout_finish_kernel, dim3(1), dim3(RB), 0, (hipStream_t)stream, a, env_info(d->env_id).obs);
  return hip_check(hipGetLastError(), "mrl_rollout_finish");
}

}  // extern "C"
