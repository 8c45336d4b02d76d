// The coloured collect kernel (include/sactd3_noise.h: sactd3_rollout_collect_colored): k_collect_rollout_colored<KIND>, a text of its own
// beside collect_kernels.h, whose kernel stays letter for letter -- and so instruction for instruction -- what it was.  It serves the
// EXPLORE mode alone, so the random branch and its counters are gone, and takes e from the rollout's noise slab in place of the Philox
// block of stream 0x900: step t reads row t of z0 while t < wrap, then row t - wrap of z1 -- the slab's two slots, row stride S = n AC;
// the host has checked that every row read lies inside its slot (env.hip).  Everything else is the white kernel's step, operation for
// operation: observe, ev_actor_pass, SAC tanh(mean + e std) sc + bi / TD3 tanh(u) sc + bi + e (sc noise_std), env_step_body,
// env_write_record, the rollout's obs / actions behind step T - 1.  Same memory discipline: plain vector stores, every address derived
// from launch arguments and (t, i), never from data.
#pragma once
#include "collect_kernels.h"

struct CollectNoise {
  const float* z0; const float* z1;
  int wrap; long long S;
};
struct CollectLaunchColored : CollectLaunch { CollectNoise z; };      // (mode, lo, span unused)

// new device code: built without packed fp32 instructions (see noise_kernels.h; the host pass knows no such feature).  The attribute
// stands on the kernel, the text in a function it inlines: the HIP headers' helpers then inline into that function as usual.
#if defined(__HIP_DEVICE_COMPILE__)
#define COLLECT_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define COLLECT_NO_PK
#endif

#pragma clang fp contract(off)

template <int KIND>
__device__ __forceinline__ void collect_colored_body(EnvDev d, CollectLaunchColored p) {
  constexpr int OB = EnvTask<KIND>::OB, AC = EnvTask<KIND>::AC, NS = EnvTask<KIND>::NS;
  static_assert(OB <= 8 && AC <= 2, "Os rows are 8 floats, the head holds at most 4 outputs");
  __shared__ __attribute__((aligned(16))) float Os[HT_TILE * 8];
  __shared__ __attribute__((aligned(16))) float H1[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float H2[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float Ln[4 * HT_HID];
  __shared__ __attribute__((aligned(16))) float Whs[4 * HT_HID];
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const size_t n = (size_t)d.n;
  const int i = blockIdx.x * HT_TILE + row;
  const bool lead = sub == 0;
  const bool owner = lead && i < d.n;
  const EvalActor& A = p.A;
  const int nh = A.sac ? 2 * AC : AC;

  EvActorRegs<OB> R;
#pragma unroll
  for (int k = 0; k < OB; ++k) R.w1[k] = 0.f;
  R.b1c = 0.f; R.b2c[0] = R.b2c[1] = R.b2c[2] = R.b2c[3] = 0.f; R.W2 = A.P;
  ev_actor_load<OB>(A, nh, tid, R, Ln, Whs);

  // ---- the owner's env, in registers
  float s[4] = {0.f, 0.f, 0.f, 0.f}, g[2] = {0.f, 0.f};
  float bh[4] = {0.f, 0.f, 0.f, 0.f}, sc[AC], bi[AC];
#pragma unroll
  for (int j = 0; j < AC; ++j) { sc[j] = 1.f; bi[j] = 0.f; }
  if (owner) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = d.phys[j * n + i];
    env_goal<KIND>(p.env_seed, (uint32_t)i, d.episode[i], g);
#pragma unroll
    for (int m = 0; m < 4; ++m) bh[m] = m < nh ? A.P[A.bh + min(m, nh - 1)] : 0.f;
#pragma unroll
    for (int j = 0; j < AC; ++j) { sc[j] = A.scale[j]; bi[j] = A.bias[j]; }
  }

  for (int t = 0; t < p.T; ++t) {
    const size_t ti = (size_t)t * n + (size_t)i;
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    // 1. observe
    if (lead) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (owner) env_observe<KIND>(s, g, o);
      *(float4*)(Os + row * 8) = make_float4(o[0], o[1], o[2], o[3]);
      *(float4*)(Os + row * 8 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    // 2. - 5. the actor pass
    ev_actor_pass<OB>(R, Os, H1, H2, Ln, Whs, bh, A.ln, tid, u);
    // 6. the owner: action, env step, record
    if (owner) {
      const float* zr = (t < p.z.wrap ? p.z.z0 + (size_t)t * (size_t)p.z.S : p.z.z1 + (size_t)(t - p.z.wrap) * (size_t)p.z.S) + (size_t)i * AC;
      float a[AC], e[AC];
#pragma unroll
      for (int j = 0; j < AC; ++j) {
        e[j] = zr[j];
        if (A.sac) {
          const float u0 = u[j], u1 = u[AC + j];
          const float tt = tanhf(u1);
          const float log_std = -5.0f + 3.5f * (tt + 1.0f);
          const float sd = expf(log_std);
          const float x = u0 + e[j] * sd;
          a[j] = tanhf(x) * sc[j] + bi[j];
        } else {
          a[j] = tanhf(u[j]) * sc[j] + bi[j];
          a[j] = a[j] + e[j] * (sc[j] * p.noise_std);
        }
      }
      uint32_t araw[AC];
#pragma unroll
      for (int j = 0; j < AC; ++j) {
        araw[j] = __float_as_uint(a[j]);
        if (p.eps) p.eps[ti * AC + j] = e[j];
      }
      const EnvStepped st = env_step_body<KIND>(d, i, a, p.horizon, p.env_seed);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = st.nx[j];
      g[0] = st.g[0]; g[1] = st.g[1];
      float nx[OB];
      env_write_record<KIND>(st, araw, p.L, p.records + ti * (size_t)p.L.record_len, nx);
      if (t == p.T - 1) {
#pragma unroll
        for (int j = 0; j < OB; ++j) p.obs[(size_t)i * p.obs_ld + j] = nx[j];
#pragma unroll
        for (int j = 0; j < AC; ++j) p.actions[(size_t)i * p.actions_ld + j] = a[j];
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) COLLECT_NO_PK void k_collect_rollout_colored(EnvDev d, CollectLaunchColored p) {
  collect_colored_body<KIND>(d, p);
}
