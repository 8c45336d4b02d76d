// A training segment in one launch (include/sactd3_rollout_collect.h): k_collect_rollout<KIND>.
// The shape of k_eval_rollout (eval_kernels.h): one 256-thread workgroup owns a tile of up to 16 envs and loops over t = 0 .. T-1 by
// itself; thread 16 r of the block OWNS env r of the tile, alone reads and writes that env's words and keeps its state in registers
// between steps.  No workgroup reads what another wrote, nothing spins, every loop bound is a launch argument.
//
// Per step:
//   1. owners: o_t = env_observe(state) -> Os                                   } skipped, with their barriers, where the mode is RANDOM
//   2. - 5. ev_actor_pass (eval_kernels.h): THE actor pass, used, not restated   } (the mode is a launch argument: uniform over the grid)
//   6. owners: the action by `mode` -- RANDOM: what k_env_sample_actions would write, draws[i] advancing by one; EXPLOIT: the `mode` action
//      of k_eval_rollout's greedy branch; EXPLORE: SAC its `sample`, TD3 tanh(u) sc + bi, then + e (sc noise_std) (kernels.h: actor tail,
//      mode 2), e the draw of this feature's stream -- then env_step_body<KIND> with it and env_write_record<KIND> (env_kernels.h) to row
//      t n + i of the caller's slab: time-major, the ring order of T appends
// Behind step T-1 the owner leaves the rollout's `obs` (the observation to act on next) and `actions` (the last step's) as T choose +
// advance calls leave them.  Memory discipline as in env_kernels.h: plain vector stores, every address derived from launch arguments
// and (t, i), never from data.
#pragma once
#include "collect_rollout.h"
#include "eval_kernels.h"

#define SACTD3_STREAM_COLLECT 0x900u   // third counter word of every draw of this feature; words (collect_ctr, t, 0x900, element >> 2)

// the values of SACTD3_ROLLOUT_* (include/sactd3_rollout.h) the kernel serves
#define CL_RANDOM 0
#define CL_EXPLORE 1
#define CL_EXPLOIT 2

struct CollectLaunch {
  EvalActor A;            // A.eval_ctr: the feature's counter word, collect_ctr
  int T, horizon, mode;
  float noise_std;        // TD3's exploring action
  float lo, span;         // RANDOM: the bounds' low end and width, as k_env_sample_actions takes them
  uint64_t env_seed;
  EnvRec L;
  float* records;         // [T n][record_len]
  float* eps;             // [T][n][AC] or NULL
  float* obs; long long obs_ld;           // the rollout's buffers
  float* actions; long long actions_ld;
};

#pragma clang fp contract(off)

template <int KIND>
__global__ __launch_bounds__(256) void k_collect_rollout(EnvDev d, CollectLaunch p) {
  constexpr int OB = EnvTask<KIND>::OB, AC = EnvTask<KIND>::AC, NS = EnvTask<KIND>::NS;
  static_assert(OB <= 8 && AC <= 2, "Os rows are 8 floats, the head holds at most 4 outputs");
  __shared__ __attribute__((aligned(16))) float Os[EV_TILE * 8];
  __shared__ __attribute__((aligned(16))) float H1[EV_TILE * EV_AS];
  __shared__ __attribute__((aligned(16))) float H2[EV_TILE * EV_AS];
  __shared__ __attribute__((aligned(16))) float Ln[4 * EV_HID];
  __shared__ __attribute__((aligned(16))) float Whs[4 * EV_HID];
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const size_t n = (size_t)d.n;
  const int i = blockIdx.x * EV_TILE + row;
  const bool lead = sub == 0;
  const bool owner = lead && i < d.n;
  const EvalActor& A = p.A;
  const int nh = A.sac ? 2 * AC : AC;
  const bool acts = p.mode != CL_RANDOM;             // (uniform) the policy chooses: the actor pass runs
  const bool draws = p.mode == CL_EXPLORE;           // (uniform) ... with a draw of the feature's stream

  EvActorRegs<OB> R;
#pragma unroll
  for (int k = 0; k < OB; ++k) R.w1[k] = 0.f;
  R.b1c = 0.f; R.b2c[0] = R.b2c[1] = R.b2c[2] = R.b2c[3] = 0.f; R.W2 = A.P;
  if (acts) ev_actor_load<OB>(A, nh, tid, R, Ln, Whs);

  // ---- the owner's env, in registers
  float s[4] = {0.f, 0.f, 0.f, 0.f}, g[2] = {0.f, 0.f};
  float bh[4] = {0.f, 0.f, 0.f, 0.f}, sc[AC], bi[AC];
#pragma unroll
  for (int j = 0; j < AC; ++j) { sc[j] = 1.f; bi[j] = 0.f; }
  unsigned long long key = 0ull; uint32_t ctr = 0u, drawn = 0u;
  if (owner) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = d.phys[j * n + i];
    env_goal<KIND>(p.env_seed, (uint32_t)i, d.episode[i], g);
    if (acts) {
#pragma unroll
      for (int m = 0; m < 4; ++m) bh[m] = m < nh ? A.P[A.bh + min(m, nh - 1)] : 0.f;
#pragma unroll
      for (int j = 0; j < AC; ++j) { sc[j] = A.scale[j]; bi[j] = A.bias[j]; }
    } else {
      drawn = d.draws[i];
    }
    if (draws) { key = *A.seed; ctr = (uint32_t)*A.eval_ctr; }
  }

  for (int t = 0; t < p.T; ++t) {
    const size_t ti = (size_t)t * n + (size_t)i;
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    if (acts) {
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
    }
    // 6. the owner: action, env step, record
    if (owner) {
      float a[AC], e[AC];
      if (!acts) {
        const Philox4 rnd = philox4x32_10(drawn, (uint32_t)i, SACTD3_STREAM_ENV, 1u, (uint32_t)p.env_seed, (uint32_t)(p.env_seed >> 32));
#pragma unroll
        for (int j = 0; j < AC; ++j) { a[j] = p.lo + p.span * philox_u01(rnd.v[j]); e[j] = 0.f; }
        drawn = drawn + 1u;
        d.draws[i] = drawn;
      } else {
#pragma unroll
        for (int j = 0; j < AC; ++j) {
          e[j] = 0.f;
          if (draws) {
            const uint32_t el = (uint32_t)i * (uint32_t)AC + (uint32_t)j;
            const float4 z = philox_box_muller4(philox4x32_10(ctr, (uint32_t)t, SACTD3_STREAM_COLLECT, el >> 2, (uint32_t)key, (uint32_t)(key >> 32)));
            const uint32_t k = el & 3u;
            e[j] = k == 0u ? z.x : (k == 1u ? z.y : (k == 2u ? z.z : z.w));
          }
          if (A.sac && draws) {
            const float u0 = u[j], u1 = u[AC + j];
            const float tt = tanhf(u1);
            const float log_std = -5.0f + 3.5f * (tt + 1.0f);
            const float sd = expf(log_std);
            const float x = u0 + e[j] * sd;
            a[j] = tanhf(x) * sc[j] + bi[j];
          } else {
            a[j] = tanhf(u[j]) * sc[j] + bi[j];
            if (draws) a[j] = a[j] + e[j] * (sc[j] * p.noise_std);
          }
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
