// Device code of the candidate-scoring call (include/sactd3_action_values.h), a translation unit of its own inside libsactd3_hip.so
// (action_values.hip): it shares philox.h with engine.hip, and NetView (net_view.h) and the hidden tile's helpers (hidden_tile.h) with dormant.hip.
//
// k_action_values<N>: 256 threads; a workgroup owns 64 candidate rows = G = 64 / N observations with their N candidates, the four 16-row
//   tiles of v_mfma_f32_16x16x4f32, plus -- when data actions are given -- a fifth tile whose rows 0 .. G - 1 are the observations' data
//   actions (the rest zeros): both critics' W2 (256 KB each) are read once per workgroup for all of them.  Grid ceil(m N / 64).
//   1. candidates: thread e of (row, d) pairs builds the action component and its log-density element from the actor head's outputs (or
//      the bounds) and the draw -- the caller's, or lane element & 3 of the Philox block (av_ctr, row of the call, 0xC00, element >> 2) --
//      into LDS (A, El) and, where wanted, `cand` / `eps_out`; thread row then sums El over d ascending -> logp.
//   2. layer 1, the state's share, once per observation and critic: the packed observation rows walk through LDS in chunks of 64 floats;
//      thread c reads row c of W1 16 bytes at a time (words at or behind ob_dim, the action columns, replaced by zeros) and keeps
//      acc[k][g] += w s, k ascending from 0; zs[k][g][c] = acc + b1[c] stays in LDS (2 x 4 x 256 floats).
//   Then per critic k, in one LDS image H[80][260] (row stride 16-byte aligned and odd in float4 units: the MFMA operand reads are
//   conflict-free):
//   3. thread c: H[row][c] = zs[k][g(row)][c] + t, t = sum_d W1[c][ob_dim + d] A[row][d], d ascending from 0 (W1's action columns in
//      registers, A broadcast from LDS): a <= 32 products per candidate in place of ob_dim + a.
//   4. LayerNorm + ReLU in place, thread (row, sub) holding 16 columns: ht_ln_relu (hidden_tile.h).
//   5. layer 2 on the MFMA: wave w owns columns 64 w .. 64 w + 63 as four column tiles for each of the four (five) row tiles -- 16 (20)
//      accumulators of 4 registers live across K = 256; W2 through the cache, 16 bytes per lane.  A block barrier, then + b2 -> H in place.
//   6. LayerNorm + ReLU again, in registers, and the head: thread (row, sub) forms ((v0 w0 + v1 w1) + (v2 w2 + v3 w3)) over its four
//      float4 groups in ascending order, one fixed 16-lane butterfly adds the 16 partials, + bh -> Q[k][row] in LDS.
//   7. reductions: lane 0 of wave g walks the N candidates of observation g in ascending order, twice (maximum / sums, then the terms that
//      need the maximum and the mean): every order is the one the header states.  -> summary, best_index, best_action (copied from A:
//      bit for bit the candidate), cand_q.
//   Rows behind m repeat row m - 1 and store nothing.  No workgroup reads what another wrote, nothing spins, no atomics: a row's bits are
//   a pure function of (parameters, its observation, its draws, its data action).  Each workgroup leaves the number of its rows with a
//   non-finite input in bad[workgroup].
// k_av_finish: one workgroup; sums bad[0 .. groups) into the feature's counter and, behind the last launch of a call that drew
//   natively, advances av_ctr.
#pragma once
#include <hip/hip_runtime.h>

#include "action_values.h"
#include "philox.h"

#define AV_HR (AV_ROWS + AV_DROWS)   // rows of the LDS image
#define AV_XC 64                     // the observation walks through LDS in chunks of 64 floats

#include "hidden_tile.h"      // (action_values.hip includes this file where contraction is off and packed fp32 instructions are not formed)

__device__ __forceinline__ bool av_finite(float v) { return fabsf(v) < __builtin_inff(); }      // (false for a NaN too)

// min(q1, q2) that keeps a NaN of either
__device__ __forceinline__ float av_min2(float q1, float q2) { return (q1 == q1 && q2 == q2) ? fminf(q1, q2) : __uint_as_float(0x7FC00000u); }

template <int N>
__global__ __launch_bounds__(256) void k_action_values(AvArgs p) {
  static_assert(N == 16 || N == 32 || N == 64, "16, 32 or 64 candidates");
  constexpr int G = AV_ROWS / N;      // observations of a workgroup
  __shared__ __attribute__((aligned(16))) float H[AV_HR * HT_AS];         // the layer image; before it, El[64][32] of the candidates
  __shared__ __attribute__((aligned(16))) float Zs[2 * 4 * HT_HID];      // zs[k][g][c]
  __shared__ __attribute__((aligned(16))) float A[AV_HR * AV_MAXA];      // candidate (rows 0 .. 63) and data (64 ..) actions
  __shared__ __attribute__((aligned(16))) float Xs[4 * AV_XC];
  __shared__ float Lp[AV_ROWS], Mj[AV_ROWS], Q[2 * AV_HR];
  __shared__ int flag[4];
  const int tid = threadIdx.x, row16 = tid >> 4, sub = tid & 15;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
  const int a = p.a, ob = p.ob;
  const int o0 = blockIdx.x * G;                      // first observation of this workgroup, in the launch
  if (o0 >= p.m) return;                              // (block-uniform; the grid is cut to the rows)
  const bool data = p.actions != nullptr;             // (uniform) the fifth row tile is worked
  float* const El = H;
  if (tid < 4) flag[tid] = 0;
  __syncthreads();

  // ---- 1. candidates
  {
    const bool native = p.eps == nullptr;
    const unsigned long long seed = native ? *p.seed : 0ull;
    const unsigned ctr = native ? (unsigned)p.words[AV_W_CTR] : 0u;
    for (int idx = tid; idx < AV_ROWS * a; idx += 256) {
      const int row = idx / a, d = idx - row * a, g = row / N, j = row - g * N;
      const int og = o0 + g, oc = min(og, p.m - 1);
      const bool valid = og < p.m;
      const unsigned el = (unsigned)(j * a + d);
      float e;
      if (native) {
        const Philox4 blk = philox4x32_10(ctr, (uint32_t)(p.row0 + oc), AV_STREAM, el >> 2, (uint32_t)seed, (uint32_t)(seed >> 32));
        e = p.source == AV_SRC_UNIFORM ? philox_u01(ht_pick(blk, el & 3u)) : ht_pick(philox_box_muller4(blk), el & 3u);
      } else e = p.eps[(long)oc * p.eps_ld + el];
      float act, le;
      if (p.source == AV_SRC_UNIFORM) {
        const float lo = p.lo[d], hi = p.hi[d];
        act = lo + e * (hi - lo);
        le = -logf(hi - lo);
      } else if (p.sac) {
        const float mean = p.head[(long)oc * p.head_ld + d], log_std = p.head[(long)oc * p.head_ld + a + d];
        const float sc = p.scale[d], bi = p.bias[d];
        const float sd = expf(log_std);
        const float x = mean + e * sd;
        const float y = tanhf(x);
        act = y * sc + bi;
        const float dx = x - mean;
        le = -(dx * dx) / (2.0f * sd * sd) - logf(sd) - 0.9189385332046727f;
        le -= logf(sc * (1.0f - y * y) + 1e-6f);
      } else {
        const float mode = p.head[(long)oc * p.head_ld + d];
        act = fminf(fmaxf(mode + (e * p.sigma) * p.scale[d], p.lo[d]), p.hi[d]);
        le = 0.f;
      }
      A[row * AV_MAXA + d] = act;
      El[row * AV_MAXA + d] = le;
      if (!av_finite(e)) flag[g] = 1;                 // (every writer stores the same value)
      if (valid) {
        if (p.cand) p.cand[((long)og * N + j) * a + d] = act;
        if (p.eps_out) p.eps_out[(long)og * (N * a) + el] = e;
      }
    }
    for (int idx = tid; idx < AV_DROWS * a; idx += 256) {      // the data actions: row 64 + g; zeros behind G and without `actions`
      const int row = idx / a, d = idx - row * a;
      const int oc = min(o0 + min(row, G - 1), p.m - 1);
      float v = 0.f;
      if (data && row < G) {
        v = p.actions[(long)oc * p.actions_ld + d];
        if (!av_finite(v)) flag[row] = 1;
      }
      A[(AV_ROWS + row) * AV_MAXA + d] = v;
    }
  }
  __syncthreads();
  if (tid < AV_ROWS) {
    float s = 0.f;
    for (int d = 0; d < a; ++d) s += El[tid * AV_MAXA + d];
    Lp[tid] = s;
    const int g = tid / N, og = o0 + g;
    if (p.cand_logp && og < p.m) p.cand_logp[(long)og * N + (tid - g * N)] = s;
  }

  // ---- 2. the state's share of layer 1, once per observation and critic
  {
    float acc[2][G];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int g = 0; g < G; ++g) acc[k][g] = 0.f;
    const float* __restrict__ w1a = p.net[0].P + p.net[0].W1 + (size_t)tid * (size_t)p.net[0].ld1;
    const float* __restrict__ w1b = p.net[1].P + p.net[1].W1 + (size_t)tid * (size_t)p.net[1].ld1;
    for (int k0 = 0; k0 < ob; k0 += AV_XC) {
      __syncthreads();                                // (the chunk before is read; the first: El is summed before H is written again)
      if (row16 < G) {
        const int oc = min(o0 + row16, p.m - 1), kk = k0 + 4 * sub;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kk < p.ldo) v = *(const float4*)(p.x + (size_t)oc * (size_t)p.ldo + kk);      // (zeros behind ob_dim: the pack kernel's padding)
        *(float4*)(Xs + row16 * AV_XC + 4 * sub) = v;
        if (!(av_finite(v.x) && av_finite(v.y) && av_finite(v.z) && av_finite(v.w))) flag[row16] = 1;
      }
      __syncthreads();
#pragma unroll 4
      for (int i4 = 0; i4 < AV_XC / 4; ++i4) {
        const int kk = k0 + 4 * i4;
        if (kk < ob) {                                // (uniform; kk + 4 <= ld1: both are multiples of 4)
          float4 w[2];
          w[0] = *(const float4*)(w1a + kk);
          w[1] = *(const float4*)(w1b + kk);
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            if (kk + 1 >= ob) w[k].y = 0.f;
            if (kk + 2 >= ob) w[k].z = 0.f;
            if (kk + 3 >= ob) w[k].w = 0.f;
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const float4 s = *(const float4*)(Xs + g * AV_XC + 4 * i4);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              acc[k][g] += w[k].x * s.x; acc[k][g] += w[k].y * s.y; acc[k][g] += w[k].z * s.z; acc[k][g] += w[k].w * s.w;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float b1 = p.net[k].P[p.net[k].b1 + tid];
#pragma unroll
      for (int g = 0; g < G; ++g) Zs[(k * 4 + g) * HT_HID + tid] = acc[k][g] + b1;
    }
  }
  __syncthreads();

  // ---- 3. - 6. per critic
  for (int k = 0; k < 2; ++k) {
    const NetView Nn = k ? p.net[1] : p.net[0];      // (a select each: a dynamically indexed kernel argument would be copied to scratch memory)
    const int bh = k ? p.bh[1] : p.bh[0];
    const float* __restrict__ P = Nn.P;
    // 3. layer 1: the state's share + the action's
    {
      float4 wa[AV_MAXA / 4];
      const float* __restrict__ wrow = P + Nn.W1 + (size_t)tid * (size_t)Nn.ld1 + ob;
#pragma unroll
      for (int q = 0; q < AV_MAXA / 4; ++q)
        wa[q] = make_float4(4 * q < a ? wrow[min(4 * q, a - 1)] : 0.f, 4 * q + 1 < a ? wrow[min(4 * q + 1, a - 1)] : 0.f,
                            4 * q + 2 < a ? wrow[min(4 * q + 2, a - 1)] : 0.f, 4 * q + 3 < a ? wrow[min(4 * q + 3, a - 1)] : 0.f);
      const int nrows = data ? AV_HR : AV_ROWS;
      for (int row = 0; row < nrows; ++row) {
        const int g = row < AV_ROWS ? row / N : min(row - AV_ROWS, G - 1);
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < AV_MAXA / 4; ++q) {
          if (4 * q < a) {                            // (uniform; A holds what was stored for d < a alone: the rest is selected away)
            const float4 av = *(const float4*)(A + row * AV_MAXA + 4 * q);
            t += wa[q].x * av.x;
            if (4 * q + 1 < a) t += wa[q].y * av.y;
            if (4 * q + 2 < a) t += wa[q].z * av.z;
            if (4 * q + 3 < a) t += wa[q].w * av.w;
          }
        }
        H[row * HT_AS + tid] = Zs[(k * 4 + g) * HT_HID + tid] + t;
      }
    }
    __syncthreads();
    // 4. LayerNorm + ReLU of H1, in place (a thread rewrites the 16 elements it read)
#pragma unroll
    for (int rt = 0; rt < AV_HR / 16; ++rt) {
      if (rt < AV_ROWS / 16 || data) {
        ht_ln_relu_lds(H + (16 * rt + row16) * HT_AS, P + Nn.g1, P + Nn.be1, sub, p.ln);
      }
    }
    __syncthreads();
    // 5. layer 2: H2[rows][64 wave .. + 63] = H1 W2^T + b2
    {
      ht_f32x4 acc[AV_HR / 16][4];
#pragma unroll
      for (int rt = 0; rt < AV_HR / 16; ++rt)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[rt][tt] = ht_f32x4{0.f, 0.f, 0.f, 0.f};
      const float* __restrict__ w2 = P + Nn.W2 + (size_t)(wave * 64 + r) * HT_HID + 4 * kq;
#pragma unroll 2
      for (int c = 0; c < HT_HID / 16; ++c) {
        float4 wv[4], av[AV_HR / 16];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) wv[tt] = *(const float4*)(w2 + (size_t)tt * 16 * HT_HID + 16 * c);
#pragma unroll
        for (int rt = 0; rt < AV_HR / 16; ++rt)
          if (rt < AV_ROWS / 16 || data) av[rt] = *(const float4*)(H + (16 * rt + r) * HT_AS + 16 * c + 4 * kq);
#pragma unroll
        for (int rt = 0; rt < AV_HR / 16; ++rt)
          if (rt < AV_ROWS / 16 || data)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[rt][tt] = ht_mfma4(av[rt], wv[tt], acc[rt][tt]);
      }
      float b2c[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) b2c[tt] = P[Nn.b2 + wave * 64 + tt * 16 + r];
      __syncthreads();                                // every wave has read all of H1
#pragma unroll
      for (int rt = 0; rt < AV_HR / 16; ++rt)
        if (rt < AV_ROWS / 16 || data)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int m = 0; m < 4; ++m) H[(16 * rt + 4 * kq + m) * HT_AS + wave * 64 + tt * 16 + r] = acc[rt][tt][m] + b2c[tt];
    }
    __syncthreads();
    // 6. LayerNorm + ReLU of H2 in registers, and the head
    {
      float4 wh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) wh[q] = *(const float4*)(P + Nn.Wh + 4 * sub + 64 * q);
      const float bhv = P[bh];
#pragma unroll
      for (int rt = 0; rt < AV_HR / 16; ++rt) {
        if (rt < AV_ROWS / 16 || data) {
          float4 v[4];
          ht_load_row(H + (16 * rt + row16) * HT_AS, sub, v);
          ht_ln_relu(v, P + Nn.g2, P + Nn.be2, sub, p.ln);
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) s += ((v[q].x * wh[q].x) + (v[q].y * wh[q].y)) + ((v[q].z * wh[q].z) + (v[q].w * wh[q].w));
          const float tot = ht_sum16(s);
          if (sub == 0) Q[k * AV_HR + 16 * rt + row16] = tot + bhv;
        }
      }
    }
    __syncthreads();                                  // Q is complete; H is free for the next critic
  }

  // ---- 7. per candidate, then per observation
  if (tid < AV_ROWS) {
    const float q1 = Q[tid], q2 = Q[AV_HR + tid];
    Mj[tid] = av_min2(q1, q2);
    const int g = tid / N, og = o0 + g;
    if (p.cand_q && og < p.m) *(float2*)(p.cand_q + ((long)og * N + (tid - g * N)) * 2) = make_float2(q1, q2);
  }
  __syncthreads();
  if (lane == 0 && wave < G && o0 + wave < p.m) {
    const int g = wave, og = o0 + g;
    const float* mj = Mj + g * N;
    const float* lp = Lp + g * N;
    const float alpha = p.soft ? expf(*p.log_alpha) : 0.f;
    const float inv_n = 1.0f / N;
    float bm = mj[0], s = 0.f, lps = 0.f, sv = 0.f;
    int bi = 0, fin = 0;
    for (int j = 0; j < N; ++j) {
      const float m = mj[j];
      if (m > bm || (bm != bm && m == m)) { bm = m; bi = j; }
      s += m; lps += lp[j]; sv += m - alpha * lp[j];
      fin += av_finite(m) ? 1 : 0;
    }
    const float q_mean = s * inv_n;
    float es = 0.f, vs = 0.f;
    for (int j = 0; j < N; ++j) {
      const float m = mj[j], dm = m - q_mean;
      es += expf((m - bm) / p.tau);
      vs += dm * dm;
    }
    float* out = p.summary ? p.summary + (long)og * p.summary_ld : nullptr;
    if (out) {
      out[0] = bm;
      out[1] = q_mean;
      out[2] = bm + p.tau * logf(es * inv_n);
      out[3] = sqrtf(vs * inv_n);
      out[4] = p.soft ? sv * inv_n : q_mean;
      out[5] = data ? av_min2(Q[AV_ROWS + g], Q[AV_HR + AV_ROWS + g]) : __uint_as_float(0x7FC00000u);
      out[6] = lps * inv_n;
      out[7] = (float)fin;
    }
    if (p.best_index) p.best_index[og] = bi;
    if (p.best_action)
      for (int d = 0; d < a; ++d) p.best_action[(long)og * p.best_action_ld + d] = A[(g * N + bi) * AV_MAXA + d];
  }
  if (tid == 0) {
    int cnt = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) cnt += (flag[g] && o0 + g < p.m) ? 1 : 0;
    p.bad[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(256) void k_av_finish(int* words, const int* bad, int groups, int tick) {
  __shared__ int red[256];
  const int tid = threadIdx.x;
  if (blockIdx.x != 0) return;
  int c = 0;
  for (int i = tid; i < groups; i += 256) c += bad[i];
  red[tid] = c;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    words[AV_W_NONFINITE] += red[0];
    if (tick) words[AV_W_CTR] += 1;
  }
}
