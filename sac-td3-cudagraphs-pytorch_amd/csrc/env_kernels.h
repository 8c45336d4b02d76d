// The GPU-resident vector environments (include/sactd3_env.h): k_env_step<KIND>, k_env_step_rec<KIND> (both around the one env_step_body<KIND>),
// k_env_reset<KIND>, k_env_sample_actions.
// One thread per env, 256-thread blocks, plain C++ with vector stores.  No workgroup reads what another stores and there is
// no global counter: every counter is a per-env word, so a step is exactly one launch and the kernels are launch-bound by
// construction.
//
// Arithmetic: fp32, contraction off, ONE operation order -- the order of the expressions below, every product and sum
// parenthesised as written.  envs.py (HostVecEnv) restates these lines in numpy float32 and tests/env_model.py in float64.
// The physics is the textbook's: the torque-limited pendulum swing-up, and the cart-pole of Barto, Sutton & Anderson (1983)
// with a continuous force; and a 2-D point mass that has to reach a goal drawn per episode, paid -1 per step off the goal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

#define SACTD3_STREAM_ENV 0x500u   // third counter word of every env draw; fourth word: 0 = episode start, 1 = random action, 2 = goal

#define ENV_PENDULUM 0
#define ENV_CARTPOLE 1
#define ENV_POINTGOAL 2

// per-env words, struct of arrays: element i belongs to env i
struct EnvDev {
  float* phys;                  // [4][n] physical state, component-major
  int32_t* steps;               // steps taken in the running episode
  uint32_t* episode;            // index of the running episode
  float* ret;                   // running return
  uint32_t* draws;              // random actions drawn
  uint32_t* done_count;         // episodes finished
  double* ret_sum;              // sum of their returns
  unsigned long long* len_sum;  // sum of their lengths
  float* last_ret;              // the last finished episode
  int32_t* last_len;
  float* first_ret;             // the first episode finished since the reset
  int32_t* first_len;
  uint32_t* bad;                // non-finite actions replaced
  int n;
};

struct EnvOut {   // sactd3_env_out with the strides checked
  float* obs; long long obs_ld;
  float* final_obs; long long final_obs_ld;
  float* reward; long long reward_ld;
  uint8_t* terminated; long long terminated_ld;
  uint8_t* truncated; long long truncated_ld;
  uint8_t* ended; long long ended_ld;
};

// The task table, one line per task: observation and action widths, physical state words, the action bound, the default horizon.
// A new task is a line here, its KIND branches in the functions below and a case of env.hip's with_kind.
template <int KIND> struct EnvTask;
template <> struct EnvTask<ENV_PENDULUM> { static constexpr int OB = 3, AC = 1, NS = 2, HORIZON = 200; static constexpr float BOUND = 2.0f; };
template <> struct EnvTask<ENV_CARTPOLE> { static constexpr int OB = 4, AC = 1, NS = 4, HORIZON = 200; static constexpr float BOUND = 1.0f; };
template <> struct EnvTask<ENV_POINTGOAL> { static constexpr int OB = 6, AC = 2, NS = 4, HORIZON = 50; static constexpr float BOUND = 1.0f; };

#define ENV_PI      3.14159274f     // fl32(pi)
#define ENV_TWO_PI  6.28318548f     // fl32(2 pi)
#define ENV_INV_2PI 0.159154937f    // fl32(1 / (2 pi))
#define ENV_GOAL_THR 0.1f           // the point mass is on its goal within this distance (compared squared: one fp32 product)

#pragma clang fp contract(off)

// x - 2 pi floor((x + pi) / (2 pi)): [-pi, pi) up to the roundings of its three operations; x unchanged (exactly) where the floor is 0
__device__ __forceinline__ float env_angnorm(float x) {
  const float k = floorf((x + ENV_PI) * ENV_INV_2PI);
  return x - ENV_TWO_PI * k;
}

__device__ __forceinline__ float env_clamp(float x, float b) { return fminf(fmaxf(x, -b), b); }

// the first state of episode `ep` of env i
template <int KIND>
__device__ __forceinline__ void env_first_state(uint64_t seed, uint32_t i, uint32_t ep, float s[4]) {
  const Philox4 r = philox4x32_10(ep, i, SACTD3_STREAM_ENV, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u0 = philox_u01(r.v[0]), u1 = philox_u01(r.v[1]), u2 = philox_u01(r.v[2]), u3 = philox_u01(r.v[3]);
  if (KIND == ENV_PENDULUM) {
    s[0] = -ENV_PI + ENV_TWO_PI * u0;   // theta ~ U(-pi, pi)
    s[1] = -1.0f + 2.0f * u1;           // omega ~ U(-1, 1)
    s[2] = 0.0f; s[3] = 0.0f;
  } else if (KIND == ENV_CARTPOLE) {
    s[0] = -0.05f + 0.1f * u0; s[1] = -0.05f + 0.1f * u1; s[2] = -0.05f + 0.1f * u2; s[3] = -0.05f + 0.1f * u3;
  } else {
    s[0] = -1.0f + 2.0f * u0; s[1] = -1.0f + 2.0f * u1;   // x, y ~ U(-1, 1), at rest
    s[2] = 0.0f; s[3] = 0.0f;
  }
}

// the goal of episode `ep` of env i: not state, a pure function of (seed, i, ep).  (0, 0) for a task without one.
template <int KIND>
__device__ __forceinline__ void env_goal(uint64_t seed, uint32_t i, uint32_t ep, float g[2]) {
  g[0] = 0.0f; g[1] = 0.0f;
  if (KIND == ENV_POINTGOAL) {
    const Philox4 r = philox4x32_10(ep, i, SACTD3_STREAM_ENV, 2u, (uint32_t)seed, (uint32_t)(seed >> 32));
    g[0] = -1.0f + 2.0f * philox_u01(r.v[0]);
    g[1] = -1.0f + 2.0f * philox_u01(r.v[1]);
  }
}

// the thresholded squared distance of an achieved goal from a desired one: 0 on the goal, -1 off it
__device__ __forceinline__ float env_goal_reward(float ax, float ay, float gx, float gy) {
  const float d2 = ((ax - gx) * (ax - gx)) + ((ay - gy) * (ay - gy));
  return (d2 <= (ENV_GOAL_THR * ENV_GOAL_THR)) ? 0.0f : -1.0f;
}

template <int KIND>
__device__ __forceinline__ void env_observe(const float s[4], const float g[2], float* row) {
  if (KIND == ENV_PENDULUM) {
    row[0] = cosf(s[0]); row[1] = sinf(s[0]); row[2] = s[1];
  } else {
    row[0] = s[0]; row[1] = s[1]; row[2] = s[2]; row[3] = s[3];
    if (KIND == ENV_POINTGOAL) { row[4] = g[0]; row[5] = g[1]; }   // achieved goal: elements 0-1, desired goal: elements 4-5
  }
}

// one step of the physics: s -> s2, the reward, and whether s2 is terminal; `ua` is the clamped, finite action, `g` the running
// episode's goal
template <int KIND>
__device__ __forceinline__ void env_physics(const float s[4], const float* ua, const float g[2], float s2[4], float& reward, bool& terminal) {
  const float u = ua[0];
  if (KIND == ENV_PENDULUM) {
    const float th = s[0], w = s[1];
    const float thn = env_angnorm(th);
    const float cost = ((thn * thn) + (0.1f * (w * w))) + (0.001f * (u * u));
    const float acc = (15.0f * sinf(th)) + (3.0f * u);
    const float w2 = env_clamp(w + (acc * 0.05f), 8.0f);
    s2[0] = env_angnorm(th + (0.05f * w2));
    s2[1] = w2; s2[2] = 0.0f; s2[3] = 0.0f;
    reward = -cost;
    terminal = false;
  } else if (KIND == ENV_POINTGOAL) {
    const float vx = (0.8f * s[2]) + (0.2f * ua[0]);
    const float vy = (0.8f * s[3]) + (0.2f * ua[EnvTask<KIND>::AC - 1]);
    s2[0] = env_clamp(s[0] + (0.1f * vx), 1.0f);
    s2[1] = env_clamp(s[1] + (0.1f * vy), 1.0f);
    s2[2] = vx; s2[3] = vy;
    reward = env_goal_reward(s2[0], s2[1], g[0], g[1]);   // of the arrival state, against the running episode's goal
    terminal = false;
  } else {
    const float x = s[0], xd = s[1], th = s[2], thd = s[3];
    const float f = 10.0f * u;
    const float c = cosf(th), sn = sinf(th);
    const float temp = (f + ((0.05f * (thd * thd)) * sn)) / 1.1f;                 // (F + m l thd^2 sin) / (M + m)
    const float den = 0.5f * (1.33333337f - ((0.1f * (c * c)) / 1.1f));           // l (4/3 - m cos^2 / (M + m))
    const float thacc = ((9.8f * sn) - (c * temp)) / den;
    const float xacc = temp - (((0.05f * thacc) * c) / 1.1f);
    s2[0] = x + (0.02f * xd);
    s2[1] = xd + (0.02f * xacc);
    s2[2] = th + (0.02f * thd);
    s2[3] = thd + (0.02f * thacc);
    reward = 1.0f;
    terminal = (fabsf(s2[0]) > 2.4f) || (fabsf(s2[2]) > 0.20943951f);
  }
}

// the action as the physics takes it: a NaN or infinite component (every finite float passes) is replaced by 0 and never reaches
// the state, every component clamped to the bounds -> whether any component was replaced
template <int KIND>
__device__ __forceinline__ bool env_clean_action(const float* a, float* u) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < EnvTask<KIND>::AC; ++j) {
    float x = a[j];
    const bool b = !(fabsf(x) <= 3.40282347e38f);
    if (b) x = 0.0f;
    bad = bad || b;
    u[j] = env_clamp(x, EnvTask<KIND>::BOUND);
  }
  return bad;
}

// What one step of env i leaves for its kernel to write out.  The arrival state belongs to the goal the step started from.
struct EnvStepped {
  float s[4], g0[2];   // the state and the goal the step started from
  float fin[4];        // the arrival state
  float nx[4], g[2];   // the state the caller acts on next and its goal: the arrival, or behind an ended episode the next one's first
  float reward;
  bool terminal, truncated, ended;
};

// One step of env i, everything but the caller's outputs: the action cleaned, the physics, the flags, the episode books, the auto-reset
// and the new physical state.  `a`: the action as given.  The ONE statement of a step: both step kernels below are this plus their writes.
template <int KIND>
__device__ __forceinline__ EnvStepped env_step_body(const EnvDev& d, int i, const float* a, int horizon, uint64_t seed) {
  const size_t n = (size_t)d.n;
  EnvStepped r;
  float u[EnvTask<KIND>::AC];
  const bool bad = env_clean_action<KIND>(a, u);
#pragma unroll
  for (int j = 0; j < 4; ++j) r.s[j] = 0.0f;
#pragma unroll
  for (int j = 0; j < EnvTask<KIND>::NS; ++j) r.s[j] = d.phys[j * n + i];
  env_goal<KIND>(seed, (uint32_t)i, d.episode[i], r.g0);
  env_physics<KIND>(r.s, u, r.g0, r.fin, r.reward, r.terminal);
  const int t = d.steps[i] + 1;
  const float ret = d.ret[i] + r.reward;
  r.truncated = !r.terminal && t >= horizon;
  r.ended = r.terminal || r.truncated;
#pragma unroll
  for (int j = 0; j < 4; ++j) r.nx[j] = r.fin[j];
  r.g[0] = r.g0[0]; r.g[1] = r.g0[1];
  if (bad) d.bad[i] += 1u;
  if (r.ended) {
    const uint32_t ep = d.episode[i] + 1u;
    const uint32_t done = d.done_count[i];
    if (done == 0u) { d.first_ret[i] = ret; d.first_len[i] = t; }
    d.done_count[i] = done + 1u;
    d.ret_sum[i] += (double)ret;
    d.len_sum[i] += (unsigned long long)t;
    d.last_ret[i] = ret;
    d.last_len[i] = t;
    d.episode[i] = ep;
    env_first_state<KIND>(seed, (uint32_t)i, ep, r.nx);
    env_goal<KIND>(seed, (uint32_t)i, ep, r.g);
    d.steps[i] = 0;
    d.ret[i] = 0.0f;
  } else {
    d.steps[i] = t;
    d.ret[i] = ret;
  }
#pragma unroll
  for (int j = 0; j < EnvTask<KIND>::NS; ++j) d.phys[j * n + i] = r.nx[j];
  return r;
}

// `final_obs` is written before `obs`: a caller that hands one buffer for both finds `obs` in it
template <int KIND>
__global__ __launch_bounds__(256) void k_env_step(EnvDev d, const float* __restrict__ actions, long long act_ld, EnvOut o, int horizon,
                                                  uint64_t seed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  float a[EnvTask<KIND>::AC];
#pragma unroll
  for (int j = 0; j < EnvTask<KIND>::AC; ++j) a[j] = actions[(size_t)i * act_ld + j];
  const EnvStepped r = env_step_body<KIND>(d, i, a, horizon, seed);
  if (o.final_obs) env_observe<KIND>(r.fin, r.g0, o.final_obs + (size_t)i * o.final_obs_ld);
  if (o.reward) o.reward[(size_t)i * o.reward_ld] = r.reward;
  if (o.terminated) o.terminated[(size_t)i * o.terminated_ld] = r.terminal ? 1 : 0;
  if (o.truncated) o.truncated[(size_t)i * o.truncated_ld] = r.truncated ? 1 : 0;
  if (o.ended) o.ended[(size_t)i * o.ended_ld] = r.ended ? 1 : 0;
  env_observe<KIND>(r.nx, r.g, o.obs + (size_t)i * o.obs_ld);
}

// k_env_step that also emits env i's transition as record i of a caller slab in the engine's ring layout (include/sactd3.h:
// sactd3_rb_layout; include/sactd3_rollout.h):
//   [s (OB) | a (AC) | 0-pad to next_off][s'_stored (OB) | 0-pad to next_width][r, d][0-pad to record_len]
// s is env_observe of the state BEFORE the step (recomputed from phys: the caller's observation buffer is not read), a the action
// as given (its bits, not the clamped one), s'_stored the arrival observation where the step was truncated and otherwise the
// observation the caller acts on next (behind a termination: the auto-reset one), d = 1 iff terminated.  State, books, counters and
// `obs` are those of k_env_step: the same env_step_body.  One thread writes its whole record with 16-byte stores: the host side
// guarantees a 16-byte aligned slab and lengths that are multiples of four, and next_off >= OB + AC, next_width >= OB,
// record_len >= next_off + next_width + 2.
struct EnvRec { int record_len, next_off, next_width; };

// THE record of one step: what env_step_body left (`r`) and the action's bits as given (`araw`) -> the record at `row` (16-byte aligned,
// record_len floats), by the rule above, element by element through selects (no indexed local array), four elements per store.
// -> nx: the observation the caller acts on next.  Both kernels that emit records -- k_env_step_rec below, k_collect_rollout
// (collect_kernels.h) -- are env_step_body plus this.
template <int KIND>
__device__ __forceinline__ void env_write_record(const EnvStepped& r, const uint32_t* araw, const EnvRec& L, float* __restrict__ row, float* nx) {
  constexpr int OB = EnvTask<KIND>::OB, AC = EnvTask<KIND>::AC;
  float so[OB], fin[OB];
  env_observe<KIND>(r.s, r.g0, so);
  env_observe<KIND>(r.fin, r.g0, fin);
  env_observe<KIND>(r.nx, r.g, nx);
  const bool truncated = r.truncated;
  const int tail = L.next_off + L.next_width;
  const uint32_t rbits = __float_as_uint(r.reward), dbits = __float_as_uint(r.terminal ? 1.0f : 0.0f);
  uint4* __restrict__ rec = (uint4*)row;
  for (int c = 0; c < L.record_len / 4; ++c) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * c + k;
      uint32_t v = 0u;
#pragma unroll
      for (int j = 0; j < OB; ++j) v = (e == j) ? __float_as_uint(so[j]) : v;
#pragma unroll
      for (int j = 0; j < AC; ++j) v = (e == OB + j) ? araw[j] : v;
#pragma unroll
      for (int j = 0; j < OB; ++j) v = (e == L.next_off + j) ? __float_as_uint(truncated ? fin[j] : nx[j]) : v;
      v = (e == tail) ? rbits : v;
      v = (e == tail + 1) ? dbits : v;
      w[k] = v;
    }
    rec[c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_env_step_rec(EnvDev d, const float* __restrict__ actions, long long act_ld, EnvRec L,
                                                      float* __restrict__ records, float* __restrict__ obs, long long obs_ld, int horizon,
                                                      uint64_t seed) {
  constexpr int OB = EnvTask<KIND>::OB, AC = EnvTask<KIND>::AC;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  uint32_t araw[AC];
#pragma unroll
  for (int j = 0; j < AC; ++j) araw[j] = __float_as_uint(actions[(size_t)i * act_ld + j]);
  float a[AC];
#pragma unroll
  for (int j = 0; j < AC; ++j) a[j] = __uint_as_float(araw[j]);
  const EnvStepped r = env_step_body<KIND>(d, i, a, horizon, seed);
  float nx[OB];
  env_write_record<KIND>(r, araw, L, records + (size_t)i * (size_t)L.record_len, nx);
#pragma unroll
  for (int j = 0; j < OB; ++j) obs[(size_t)i * obs_ld + j] = nx[j];
}

template <int KIND>
__global__ __launch_bounds__(256) void k_env_reset(EnvDev d, float* __restrict__ obs, long long obs_ld, uint64_t seed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  const size_t n = (size_t)d.n;
  float s[4], g[2];
  env_first_state<KIND>(seed, (uint32_t)i, 0u, s);
  env_goal<KIND>(seed, (uint32_t)i, 0u, g);
#pragma unroll
  for (int j = 0; j < 4; ++j) d.phys[j * n + i] = s[j];
  d.steps[i] = 0; d.episode[i] = 0u; d.ret[i] = 0.0f; d.draws[i] = 0u;
  d.done_count[i] = 0u; d.ret_sum[i] = 0.0; d.len_sum[i] = 0ull; d.last_ret[i] = 0.0f; d.last_len[i] = 0; d.first_ret[i] = 0.0f; d.first_len[i] = 0; d.bad[i] = 0u;
  if (obs) env_observe<KIND>(s, g, obs + (size_t)i * obs_ld);
}

// ac_dim <= 4: dimension j of the draw takes word j
__global__ __launch_bounds__(256) void k_env_sample_actions(EnvDev d, float* __restrict__ actions, long long act_ld, int ac_dim, float lo,
                                                            float span, uint64_t seed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  const uint32_t j = d.draws[i];
  const Philox4 r = philox4x32_10(j, (uint32_t)i, SACTD3_STREAM_ENV, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
  float* row = actions + (size_t)i * act_ld;
  row[0] = lo + span * philox_u01(r.v[0]);
  if (ac_dim > 1) row[1] = lo + span * philox_u01(r.v[1]);
  if (ac_dim > 2) row[2] = lo + span * philox_u01(r.v[2]);
  if (ac_dim > 3) row[3] = lo + span * philox_u01(r.v[3]);
  d.draws[i] = j + 1u;
}
