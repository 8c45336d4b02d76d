// On-policy evaluation in one launch (include/sactd3_eval.h): k_eval_rollout<KIND>.
// One 256-thread workgroup owns a tile of up to 16 envs and loops over t = 0 .. T-1 by itself; thread 16 r of the block OWNS env r of the
// tile: it alone reads and writes that env's words (env_step_body), keeps its state in registers between steps and walks its rewards
// backwards at the end.  No workgroup reads what another wrote, nothing spins, every loop bound is a launch argument.
//
// Per step, between block barriers (LDS only: Os the tile's observations, H1 / H2 the two hidden layers' rows):
//   1. owners: o_t = env_observe(state) -> Os and the `obs` record
//   2. layer 1: thread c holds row c of W1 (K <= 8) and b1[c] in registers for the whole call: z1[r][c] for the 16 rows -> H1
//   3. thread (row = t >> 4, sub = t & 15) holds columns 4 sub + 64 q .. + 3: LayerNorm (two-pass, eps inside the root) + ReLU in place
//   4. layer 2 (K = 256) on the matrix cores: wave w owns columns 64 w .. 64 w + 63 as four 16 x 16 tiles, the tile's 16 envs are the 16
//      rows of v_mfma_f32_16x16x4f32; W2 (256 KB, above the LDS) is read through the cache every step, 16 bytes per lane and request,
//      64 contiguous bytes per weight row and request; + b2 -> H2
//   5. LayerNorm + ReLU of H2 in registers, the head (nh <= 4 outputs from LDS-resident Wh) as 16-lane sums -> the owner
//   6. owners: the action (policy_kernels.h: `mode`, or `sample` / `sample_logp` with the draw of this feature's stream), the records, then
//      env_step_body<KIND> with it -- cleaning, physics, flags, books, auto-reset: used, not restated
// Memory discipline as in env_kernels.h: plain vector stores, every address derived from launch arguments and (t, i), never from data.
#pragma once
#include "env_kernels.h"
#include "eval_rollout.h"

#define SACTD3_STREAM_EVAL 0x800u   // third counter word of every draw of this feature; words (eval_ctr, t, 0x800, element >> 2)
#define EV_HID 256
#define EV_AS 260                   // LDS row stride of the 256-wide rows: 16-byte aligned, odd in float4 units
#define EV_TILE 16

typedef float ev_f32x4 __attribute__((ext_vector_type(4)));

struct EvalLaunch {
  EvalActor A;
  int T, horizon, sample, soft;
  float gamma;
  uint64_t env_seed;
  float *obs, *actions, *eps, *reward, *logp, *rtg;
  uint8_t* live;
  float* ep_return; int32_t* ep_length; uint8_t* ep_terminated; float* g0;
  float* alpha;
};

#pragma clang fp contract(off)

// sum over the 16 lanes that share a row; every lane gets it
__device__ __forceinline__ float ev_sum16(float v) {
  v += __shfl_xor(v, 1, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 8, 16);
  return v;
}

// LayerNorm (ln == 0: identity) + ReLU of the 16 columns a thread holds of its row; g / be: the affine pair in LDS
__device__ __forceinline__ void ev_ln_relu(float4 v[4], const float* g, const float* be, int sub, int ln) {
  if (ln) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += (v[q].x + v[q].y) + (v[q].z + v[q].w);
    const float mean = ev_sum16(s) * (1.0f / EV_HID);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q].x -= mean; v[q].y -= mean; v[q].z -= mean; v[q].w -= mean;
      ss += ((v[q].x * v[q].x) + (v[q].y * v[q].y)) + ((v[q].z * v[q].z) + (v[q].w * v[q].w));
    }
    const float var = ev_sum16(ss) * (1.0f / EV_HID);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 gg = *(const float4*)(g + 4 * sub + 64 * q), bb = *(const float4*)(be + 4 * sub + 64 * q);
      v[q].x = (v[q].x * rstd) * gg.x + bb.x; v[q].y = (v[q].y * rstd) * gg.y + bb.y;
      v[q].z = (v[q].z * rstd) * gg.z + bb.z; v[q].w = (v[q].w * rstd) * gg.w + bb.w;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q].x = fmaxf(v[q].x, 0.f); v[q].y = fmaxf(v[q].y, 0.f); v[q].z = fmaxf(v[q].z, 0.f); v[q].w = fmaxf(v[q].w, 0.f); }
}

// What thread `tid` of a tile's workgroup keeps of the online actor for a whole call: row tid of W1 (K = OB <= 8) and b1[tid]; b2 of the four
// layer-2 columns it receives; where W2 lies.
template <int OB>
struct EvActorRegs {
  float w1[OB], b1c, b2c[4];
  const float* W2;
};

// once per call: R, and the LDS-resident operands -- Ln [4][256] = g1, be1, g2, be2; Whs [4][256] = the head's rows, zero beyond nh
template <int OB>
__device__ __forceinline__ void ev_actor_load(const EvalActor& A, int nh, int tid, EvActorRegs<OB>& R, float* Ln, float* Whs) {
  const float* __restrict__ P = A.P;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15;
#pragma unroll
  for (int k = 0; k < OB; ++k) R.w1[k] = P[A.W1 + tid * A.ld1 + k];
  R.b1c = P[A.b1 + tid];
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) R.b2c[tt] = P[A.b2 + wave * 64 + tt * 16 + r];
  Ln[tid] = P[A.g1 + tid]; Ln[EV_HID + tid] = P[A.be1 + tid]; Ln[2 * EV_HID + tid] = P[A.g2 + tid]; Ln[3 * EV_HID + tid] = P[A.be2 + tid];
#pragma unroll
  for (int m = 0; m < 4; ++m) Whs[m * EV_HID + tid] = m < nh ? P[A.Wh + min(m, nh - 1) * EV_HID + tid] : 0.f;
  R.W2 = P + A.W2;
}

// THE actor pass of one step, steps 2 to 5 of the list above, for the 16 rows of observations in Os (the caller's barrier stands behind
// their write): -> u[m], the head's output m of row tid >> 4 plus bh[m], in every lane of the row.  Three block barriers; every thread
// of the workgroup calls it.  k_eval_rollout and k_collect_rollout (collect_kernels.h) are this plus what they do with u.
template <int OB>
__device__ __forceinline__ void ev_actor_pass(const EvActorRegs<OB>& R, const float* Os, float* H1, float* H2, const float* Ln, const float* Whs,
                                              const float bh[4], int ln, int tid, float u[4]) {
  const int row = tid >> 4, sub = tid & 15;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
  // 2. layer 1, column tid
#pragma unroll
  for (int rr = 0; rr < EV_TILE; ++rr) {
    const float4 oa = *(const float4*)(Os + rr * 8), ob = *(const float4*)(Os + rr * 8 + 4);
    const float o[8] = {oa.x, oa.y, oa.z, oa.w, ob.x, ob.y, ob.z, ob.w};
    float z = R.b1c;
#pragma unroll
    for (int k = 0; k < OB; ++k) z += o[k] * R.w1[k];
    H1[rr * EV_AS + tid] = z;
  }
  __syncthreads();
  // 3. LayerNorm + ReLU of H1, in place (a thread rewrites the 16 elements it read)
  {
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *(const float4*)(H1 + row * EV_AS + 4 * sub + 64 * q);
    ev_ln_relu(v, Ln, Ln + EV_HID, sub, ln);
#pragma unroll
    for (int q = 0; q < 4; ++q) *(float4*)(H1 + row * EV_AS + 4 * sub + 64 * q) = v[q];
  }
  __syncthreads();
  // 4. layer 2: H2[16][64 wave .. + 63] = H1 W2^T + b2.  Lane (r, kq) feeds A[r][k] and B[k][col r] with k = 16 c + 4 kq + m for the
  //    m-th of four MFMAs (any order of k serves both operands alike); it receives D[4 kq + m'][col r].
  {
    float4 av[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) av[c] = *(const float4*)(H1 + r * EV_AS + 16 * c + 4 * kq);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int col = wave * 64 + tt * 16 + r;
      const float4* __restrict__ wrow = (const float4*)(R.W2 + (size_t)col * EV_HID + 4 * kq);
      float4 wv[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) wv[c] = wrow[4 * c];
      ev_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c].x, wv[c].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c].y, wv[c].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c].z, wv[c].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c].w, wv[c].w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) H2[(4 * kq + m) * EV_AS + col] = acc[m] + R.b2c[tt];
    }
  }
  __syncthreads();
  // 5. LayerNorm + ReLU of H2 in registers, the head
  {
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *(const float4*)(H2 + row * EV_AS + 4 * sub + 64 * q);
    ev_ln_relu(v, Ln + 2 * EV_HID, Ln + 3 * EV_HID, sub, ln);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float part = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 w = *(const float4*)(Whs + m * EV_HID + 4 * sub + 64 * q);
        part += ((v[q].x * w.x) + (v[q].y * w.y)) + ((v[q].z * w.z) + (v[q].w * w.w));
      }
      u[m] = ev_sum16(part) + bh[m];
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_eval_rollout(EnvDev d, EvalLaunch p) {
  constexpr int OB = EnvTask<KIND>::OB, AC = EnvTask<KIND>::AC, NS = EnvTask<KIND>::NS;
  static_assert(OB <= 8 && AC <= 2, "Os rows are 8 floats, the head holds at most 4 outputs");
  __shared__ __attribute__((aligned(16))) float Os[EV_TILE * 8];
  __shared__ __attribute__((aligned(16))) float H1[EV_TILE * EV_AS];
  __shared__ __attribute__((aligned(16))) float H2[EV_TILE * EV_AS];
  __shared__ __attribute__((aligned(16))) float Ln[4 * EV_HID];      // g1, be1, g2, be2
  __shared__ __attribute__((aligned(16))) float Whs[4 * EV_HID];     // the head's rows, zero beyond nh
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const size_t n = (size_t)d.n;
  const int i = blockIdx.x * EV_TILE + row;
  const bool lead = sub == 0;                // the thread that writes row `row` of Os
  const bool owner = lead && i < d.n;        // ... and owns env i
  const EvalActor& A = p.A;
  const float* __restrict__ P = A.P;
  const int nh = A.sac ? 2 * AC : AC;

  // ---- once per call: the parameters that stay in registers / LDS (ev_actor_load)
  EvActorRegs<OB> R;
  ev_actor_load<OB>(A, nh, tid, R, Ln, Whs);

  // ---- the owner's env, in registers
  float s[4] = {0.f, 0.f, 0.f, 0.f}, g[2] = {0.f, 0.f};
  float bh[4] = {0.f, 0.f, 0.f, 0.f}, sc[AC], bi[AC];
#pragma unroll
  for (int j = 0; j < AC; ++j) { sc[j] = 1.f; bi[j] = 0.f; }
  unsigned long long key = 0ull; uint32_t ctr = 0u; float alpha = 0.f;
  if (owner) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = d.phys[j * n + i];
    env_goal<KIND>(p.env_seed, (uint32_t)i, d.episode[i], g);
#pragma unroll
    for (int m = 0; m < 4; ++m) bh[m] = m < nh ? P[A.bh + min(m, nh - 1)] : 0.f;
#pragma unroll
    for (int j = 0; j < AC; ++j) { sc[j] = A.scale[j]; bi[j] = A.bias[j]; }
    if (p.sample) { key = *A.seed; ctr = (uint32_t)*A.eval_ctr; }
    if (A.log_alpha) alpha = expf(*A.log_alpha);
  }
  bool open = true, term = false;      // the call's episode: still running / ended by termination
  int L = 0;                           // its steps inside the call so far
  float ret = 0.f;

  for (int t = 0; t < p.T; ++t) {
    const size_t ti = (size_t)t * n + (size_t)i;
    // 1. observe
    if (lead) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (owner) {
        env_observe<KIND>(s, g, o);
        if (p.obs) {
#pragma unroll
          for (int k = 0; k < OB; ++k) p.obs[ti * OB + k] = o[k];
        }
      }
      *(float4*)(Os + row * 8) = make_float4(o[0], o[1], o[2], o[3]);
      *(float4*)(Os + row * 8 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    // 2. - 5. the actor pass -> the head's outputs
    float u[4];
    ev_actor_pass<OB>(R, Os, H1, H2, Ln, Whs, bh, A.ln, tid, u);
    // 6. the owner: action, records, env step
    if (owner) {
      float a[AC], e[AC];
      float lp = 0.f;
#pragma unroll
      for (int j = 0; j < AC; ++j) {
        e[j] = 0.f;
        if (A.sac && p.sample) {
          const uint32_t el = (uint32_t)i * (uint32_t)AC + (uint32_t)j;
          const float4 z = philox_box_muller4(philox4x32_10(ctr, (uint32_t)t, SACTD3_STREAM_EVAL, el >> 2, (uint32_t)key, (uint32_t)(key >> 32)));
          const uint32_t k = el & 3u;
          e[j] = k == 0u ? z.x : (k == 1u ? z.y : (k == 2u ? z.z : z.w));
          const float u0 = u[j], u1 = u[AC + j];
          const float tt = tanhf(u1);
          const float log_std = -5.0f + 3.5f * (tt + 1.0f);
          const float sd = expf(log_std);
          const float x = u0 + e[j] * sd;
          const float y = tanhf(x);
          a[j] = y * sc[j] + bi[j];
          const float dx = x - u0;
          float l = -(dx * dx) / (2.0f * sd * sd) - logf(sd) - 0.9189385332046727f;
          l -= logf(sc[j] * (1.0f - y * y) + 1e-6f);
          lp += l;
        } else {
          a[j] = tanhf(u[j]) * sc[j] + bi[j];
        }
      }
#pragma unroll
      for (int j = 0; j < AC; ++j) {
        if (p.actions) p.actions[ti * AC + j] = a[j];
        if (p.eps) p.eps[ti * AC + j] = e[j];
      }
      const EnvStepped st = env_step_body<KIND>(d, i, a, p.horizon, p.env_seed);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = st.nx[j];
      g[0] = st.g[0]; g[1] = st.g[1];
      if (p.reward) p.reward[ti] = st.reward;
      if (p.logp) p.logp[ti] = lp;
      if (p.live) p.live[ti] = open ? 1 : 0;
      A.rew[ti] = st.reward;
      if (p.soft) A.lp[ti] = lp;
      if (open) {
        ret = ret + st.reward;
        L = t + 1;
        if (st.ended) { open = false; term = st.terminal; }
      }
    }
  }

  // ---- the returns-to-go of the call's episode, walked backwards by its owner: one fp32 operation per line, in this order
  if (owner) {
    const int Le = open ? 0 : L;      // an episode still open at T has no return: rtg = 0 everywhere
    if (p.rtg)
      for (int t = Le; t < p.T; ++t) p.rtg[(size_t)t * n + i] = 0.f;
    float G = 0.f;
    if (Le > 0) {
      G = A.rew[(size_t)(Le - 1) * n + i];
      if (p.rtg) p.rtg[(size_t)(Le - 1) * n + i] = G;
      for (int t0 = Le - 2; t0 >= 0; t0 -= 8) {
        float rw[8], lq[8];      // eight steps' loads go out together
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int t = max(t0 - k, 0);
          rw[k] = A.rew[(size_t)t * n + i];
          lq[k] = p.soft ? A.lp[(size_t)(t + 1) * n + i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int t = t0 - k;
          if (t >= 0) {
            float B = G;
            if (p.soft) {
              const float pp = alpha * lq[k];
              B = G - pp;
            }
            const float q = p.gamma * B;
            G = rw[k] + q;
            if (p.rtg) p.rtg[(size_t)t * n + i] = G;
          }
        }
      }
    }
    if (p.ep_return) p.ep_return[i] = ret;
    if (p.ep_length) p.ep_length[i] = Le;
    if (p.ep_terminated) p.ep_terminated[i] = (!open && term) ? 1 : 0;
    if (p.g0) p.g0[i] = G;
    if (p.alpha && i == 0) p.alpha[0] = alpha;
  }
}
