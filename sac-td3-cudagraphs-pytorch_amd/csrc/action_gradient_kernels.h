// Device code of the action-gradient call (include/sactd3_action_gradient.h), a translation unit of its own inside libsactd3_hip.so
// (action_gradient.hip): the library's only backward pass outside engine.hip's update kernels, for rows of the caller's choosing.  The
// forward pieces are hidden_tile.h's (ht_ln_relu, ht_layer2, ht_mfma4, ht_sum16), as they stand; everything backward is this file's.
//
// k_action_gradient: 256 threads, one workgroup per 16-row tile (grid ceil(m / 16)), the two thread layouts of hidden_tile.h -- (row, sub)
//   for everything row-local, (wave, r, kq) for v_mfma_f32_16x16x4f32.  Both critics are worked one after the other in the same LDS: the
//   minimum, the cosine and the ascent step need both.  Rows behind m repeat row m - 1 and store nothing.
//   0. the tile's actions -> Act and Act0 (words at d >= a zeros); layer 1, the state's share, once: the caller's observation rows walk
//      through Xs in K chunks of 64 (4-byte reads: a caller's row has any stride and alignment; words at k >= ob_dim stored as zeros), W1
//      through the cache 16 bytes per lane with its words at k >= ob_dim -- the action columns and the pad -- replaced by zeros; eight
//      accumulators per lane (2 critics x 4 column tiles) live across the chunks; + b1 -> Zs[k].  Zs stays for every step.
//   Then `steps` + 1 forwards and max(steps, 1) backwards, per critic k:
//   F1 the action's share on the MFMA, K = a <= 32 as one or two groups of 16 (W1's action columns: 4-byte reads, they start at any
//      ob_dim; words at d >= a zeros on both operands): Z1 = Zs[k] + Act W1a^T, the image before LayerNorm.
//   F2 (row, sub): H = relu(LN(Z1)) (ht_ln_relu); Z1 stays.
//   F3 Z2 = H W2^T + b2 (ht_layer2: W2 through the cache, 16 bytes per lane), the image before LayerNorm.
//   F4 (row, sub): h2 = relu(LN(Z2)) in registers, Q_k = the row dot against w3 (the order of k_action_values: four products per float4
//      group, the groups ascending, one ht_sum16) + b3 -> Qs[k][row].  Where a backward follows: dY2 = w3 [h2 > 0], LayerNorm backward
//      with mean and rstd recomputed from Z2 by the forward's own operations (so the ReLU mask is the forward's, bit for bit)
//      -> dZ2 into H.
//   B1 dH1 = dZ2 W2 on the MFMA -- W2 used transposed: B[k = i][col = j] = W2[i][j], rows contiguous along the column index.  W2 is
//      fetched in 16-byte requests, a wave one whole 1 KB row per request, 16 rows (16 KB) at a time through the double-buffered slab
//      Sl[2][16][260]: slab s + 1 travels global -> registers while slab s feeds the MFMAs, then registers -> the other half, one block
//      barrier per slab.  A lane's B words are 4-byte LDS reads at bank 16 kq + r + const: conflict-free.  Each element of W2 is read
//      once per tile and critic in each direction.  -> dH1 into H (behind the last slab's barrier).
//   B2 (row, sub): dZ1 = the LayerNorm + ReLU backward of dH1 at Z1 -> H in place.
//   B3 dQ/da = dZ1 W1[:, ob_dim .. + a): one or two 16-column tiles; K = 256 is split over the four waves, partials -> Gp[wave]; and, at
//      the start actions and only when grad_obs is given, dQ/ds = dZ1 W1[:, 0 .. ob_dim): the ceil(ob_dim / 16) column tiles dealt to
//      the four waves in turn, K = 256 each, stored straight to the caller's array (64 contiguous bytes per 16 lanes).
//   B4 G[k][row][d] = (Gp0 + Gp1) + (Gp2 + Gp3), d < a; at the start actions -> `grad`.
//   Behind both critics, thread row < 16: at the start the norms, the cosine and Q_start; where a step follows, the header's ascent step
//   on Act (d ascending), the held count.  Nothing between steps touches global memory but parameter reads.
//   LDS (floats): Zs 2 x 16 x 260, Z1 / Z2 / H 16 x 260 each, Sl 2 x 16 x 260 (Xs [16][68] in 0. and Gp [4][16][32] in B3 / B4 live in
//   it), Act / Act0 16 x 32 each, G 2 x 16 x 32, Qs 32; flag 16 ints: 124 864 bytes.
//   Barriers of one critic and iteration: behind F1, F2, F3; behind the first slab's stores (it also stands behind F4's dZ2); one per
//   slab (16); behind the dH1 stores, B2 and B3.  Behind both critics one (G, Qs complete), and one behind the step (Act).  Every image is
//   next written behind a barrier that follows its last read: Z1 F1 <- B2; H F2 <- B3, F4 <- F3; Z2 F3 <- F4; Sl B1 <- B4.
//   No workgroup reads what another wrote, nothing spins, no atomics: a row's bits are a pure function of (parameters, its observation,
//   its action, steps, lr).  Each workgroup leaves the number of its rows with a non-finite input in bad[workgroup].
// k_ag_finish: one workgroup; sums bad[0 .. groups) into the feature's counter.
#pragma once
#include <hip/hip_runtime.h>

#include "action_gradient.h"

#include "hidden_tile.h"      // (action_gradient.hip includes this file where contraction is off and packed fp32 instructions are not formed)

#define AG_AS AG_MAXA      // row stride of Act / Act0 / G / Gp
#define AG_SR 16           // rows of W2 in one half of the slab

__device__ __forceinline__ bool ag_finite(float v) { return fabsf(v) < __builtin_inff(); }      // (false for a NaN too)

// Backward of ht_ln_relu for the 16 columns a thread (row, sub) holds of its row.  z: the image before LayerNorm; d: in, the gradient at
// the ReLU's output; out, the gradient at z.  mean, rstd, xhat and y are the forward's operations repeated, so y > 0 is the forward's
// mask; dz = rstd ((dx - mean(dx)) - xhat mean(dx xhat)), dx = dy g.  ln == 0: the mask alone.
__device__ __forceinline__ void ag_ln_relu_bwd(const float4 (&z)[4], float4 (&d)[4], const float* __restrict__ g, const float* __restrict__ be,
                                               int sub, int ln) {
  float v[16], dd[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[4 * q] = z[q].x; v[4 * q + 1] = z[q].y; v[4 * q + 2] = z[q].z; v[4 * q + 3] = z[q].w;
    dd[4 * q] = d[q].x; dd[4 * q + 1] = d[q].y; dd[4 * q + 2] = d[q].z; dd[4 * q + 3] = d[q].w;
  }
  if (!ln) {
#pragma unroll
    for (int i = 0; i < 16; ++i) dd[i] = v[i] > 0.f ? dd[i] : 0.f;
  } else {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += (v[4 * q] + v[4 * q + 1]) + (v[4 * q + 2] + v[4 * q + 3]);
    const float mean = ht_sum16(s) * (1.0f / HT_HID);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * q + i] -= mean;
      ss += ((v[4 * q] * v[4 * q]) + (v[4 * q + 1] * v[4 * q + 1])) + ((v[4 * q + 2] * v[4 * q + 2]) + (v[4 * q + 3] * v[4 * q + 3]));
    }
    const float var = ht_sum16(ss) * (1.0f / HT_HID);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 gg = *(const float4*)(g + 4 * sub + 64 * q), bb = *(const float4*)(be + 4 * sub + 64 * q);
      const float gq[4] = {gg.x, gg.y, gg.z, gg.w}, bq[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xh = v[4 * q + i] * rstd;
        const float y = xh * gq[i] + bq[i];
        v[4 * q + i] = xh;
        dd[4 * q + i] = y > 0.f ? dd[4 * q + i] * gq[i] : 0.f;
      }
      s1 += (dd[4 * q] + dd[4 * q + 1]) + (dd[4 * q + 2] + dd[4 * q + 3]);
      s2 += ((dd[4 * q] * v[4 * q]) + (dd[4 * q + 1] * v[4 * q + 1])) + ((dd[4 * q + 2] * v[4 * q + 2]) + (dd[4 * q + 3] * v[4 * q + 3]));
    }
    const float m1 = ht_sum16(s1) * (1.0f / HT_HID), m2 = ht_sum16(s2) * (1.0f / HT_HID);
#pragma unroll
    for (int i = 0; i < 16; ++i) dd[i] = rstd * ((dd[i] - m1) - v[i] * m2);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) d[q] = make_float4(dd[4 * q], dd[4 * q + 1], dd[4 * q + 2], dd[4 * q + 3]);
}

__device__ __forceinline__ void ag_store_row(float* h, int sub, const float4 (&v)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) *(float4*)(h + 4 * sub + 64 * q) = v[q];
}

__global__ __launch_bounds__(256) void k_action_gradient(AgArgs p) {
  __shared__ __attribute__((aligned(16))) float Zs[2 * HT_TILE * HT_AS];      // the state's share of layer 1, + b1, per critic
  __shared__ __attribute__((aligned(16))) float Z1[HT_TILE * HT_AS];          // layer 1 before LayerNorm (the critic in work)
  __shared__ __attribute__((aligned(16))) float Z2[HT_TILE * HT_AS];          // layer 2 before LayerNorm
  __shared__ __attribute__((aligned(16))) float H[HT_TILE * HT_AS];           // H1, then dZ2, dH1, dZ1
  __shared__ __attribute__((aligned(16))) float Sl[2 * AG_SR * HT_AS];        // the W2 slab; Xs in step 0, Gp in B3 / B4
  __shared__ __attribute__((aligned(16))) float Act[HT_TILE * AG_AS];         // the actions as they stand
  __shared__ __attribute__((aligned(16))) float Act0[HT_TILE * AG_AS];        // ... as they were given
  __shared__ __attribute__((aligned(16))) float G[2 * HT_TILE * AG_AS];       // dQ_k/da at Act
  __shared__ float Qs[2 * HT_TILE];
  __shared__ int flag[HT_TILE];
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
  const int a = p.a, ob = p.ob, steps = p.steps;
  const int r0 = blockIdx.x * HT_TILE;                // first row of this workgroup, in the launch
  if (r0 >= p.m) return;                              // (block-uniform; the grid is cut to the rows)
  float* const Xs = Sl;
  float* const Gp = Sl;
  if (tid < HT_TILE) flag[tid] = 0;
  __syncthreads();

  // ---- 0. the actions, and the state's share of layer 1 for both critics
  for (int idx = tid; idx < HT_TILE * AG_AS; idx += 256) {
    const int rr = idx / AG_AS, d = idx - rr * AG_AS;
    const float v = d < a ? p.actions[(size_t)min(r0 + rr, p.m - 1) * (size_t)p.actions_ld + d] : 0.f;
    Act[idx] = v; Act0[idx] = v;
    if (!ag_finite(v)) flag[rr] = 1;                  // (every writer stores the same value)
  }
  {
    ht_f32x4 acc[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) acc[k][tt] = ht_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ orow = p.obs + (size_t)min(r0 + row, p.m - 1) * (size_t)p.obs_ld;
    for (int k0 = 0; k0 < ob; k0 += HT_KC) {
      {
        const int kk = k0 + 4 * sub;
        const float4 x = make_float4(kk < ob ? orow[kk] : 0.f, kk + 1 < ob ? orow[kk + 1] : 0.f, kk + 2 < ob ? orow[kk + 2] : 0.f,
                                     kk + 3 < ob ? orow[kk + 3] : 0.f);
        *(float4*)(Xs + row * HT_XS + 4 * sub) = x;
        if (!(ag_finite(x.x) && ag_finite(x.y) && ag_finite(x.z) && ag_finite(x.w))) flag[row] = 1;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < HT_KC / 16; ++c) {
        if (k0 + 16 * c < ob) {      // (block-uniform: a group of 16 k at or behind ob_dim holds zeros on both sides)
          const int kb = k0 + 16 * c + 4 * kq;
          const float4 av = *(const float4*)(Xs + r * HT_XS + 16 * c + 4 * kq);
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const float* __restrict__ w1 = p.net[k].P + p.net[k].W1 + (size_t)(wave * 64 + r) * (size_t)p.net[k].ld1 + min(kb, p.net[k].ld1 - 4);
            float4 wv[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) wv[tt] = *(const float4*)(w1 + (size_t)tt * 16 * (size_t)p.net[k].ld1);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[k][tt] = ht_mfma4(av, ht_below(wv[tt], kb, ob, true), acc[k][tt]);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int col = wave * 64 + tt * 16 + r;
        const float b1 = p.net[k].P[p.net[k].b1 + col];
#pragma unroll
        for (int m = 0; m < 4; ++m) Zs[(k * HT_TILE + 4 * kq + m) * HT_AS + col] = acc[k][tt][m] + b1;
      }
  }
  __syncthreads();

  const int nb = steps > 0 ? steps : 1;               // backwards of the call
  const int ntile = a > 16 ? 2 : 1;                   // 16-column tiles of dQ/da
  float qs1 = 0.f, qs2 = 0.f, n1 = 0.f, n2 = 0.f, cosv = 0.f;      // (thread row < 16: its row's start values)
  int held = 0;
  for (int it = 0; it <= steps; ++it) {
    const bool bwd = it < nb;                         // (uniform)
    for (int k = 0; k < 2; ++k) {
      const NetView Nn = k ? p.net[1] : p.net[0];      // (a select each: a dynamically indexed kernel argument would be copied to scratch memory)
      const int bh = k ? p.bh[1] : p.bh[0];
      const float* __restrict__ P = Nn.P;
      // F1. layer 1: the state's share + the action's
      {
        ht_f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = ht_f32x4{0.f, 0.f, 0.f, 0.f};
        const float* __restrict__ wrow = P + Nn.W1 + (size_t)(wave * 64 + r) * (size_t)Nn.ld1 + ob;
#pragma unroll
        for (int c = 0; c < AG_MAXA / 16; ++c) {
          if (16 * c < a) {                           // (uniform)
            const int d0 = 16 * c + 4 * kq;
            const float4 av = *(const float4*)(Act + r * AG_AS + d0);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
              const float* __restrict__ w = wrow + (size_t)tt * 16 * (size_t)Nn.ld1;
              const float4 wv = make_float4(d0 < a ? w[min(d0, a - 1)] : 0.f, d0 + 1 < a ? w[min(d0 + 1, a - 1)] : 0.f,
                                            d0 + 2 < a ? w[min(d0 + 2, a - 1)] : 0.f, d0 + 3 < a ? w[min(d0 + 3, a - 1)] : 0.f);
              acc[tt] = ht_mfma4(av, wv, acc[tt]);
            }
          }
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int col = wave * 64 + tt * 16 + r;
#pragma unroll
          for (int m = 0; m < 4; ++m) Z1[(4 * kq + m) * HT_AS + col] = Zs[(k * HT_TILE + 4 * kq + m) * HT_AS + col] + acc[tt][m];
        }
      }
      __syncthreads();
      // F2. H = relu(LN(Z1))
      {
        float4 v[4];
        ht_load_row(Z1 + row * HT_AS, sub, v);
        ht_ln_relu(v, P + Nn.g1, P + Nn.be1, sub, p.ln);
        ag_store_row(H + row * HT_AS, sub, v);
      }
      __syncthreads();
      // F3. Z2 = H W2^T + b2
      {
        float b2c[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) b2c[tt] = P[Nn.b2 + wave * 64 + tt * 16 + r];
        ht_layer2(H, P + Nn.W2, b2c, Z2, wave, r, kq);
      }
      __syncthreads();
      // F4. the head; dZ2 -> H
      {
        float4 z[4], v[4], wh[4];
        ht_load_row(Z2 + row * HT_AS, sub, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[q] = z[q]; wh[q] = *(const float4*)(P + Nn.Wh + 4 * sub + 64 * q); }
        ht_ln_relu(v, P + Nn.g2, P + Nn.be2, sub, p.ln);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += ((v[q].x * wh[q].x) + (v[q].y * wh[q].y)) + ((v[q].z * wh[q].z) + (v[q].w * wh[q].w));
        const float tot = ht_sum16(s);
        if (sub == 0) Qs[k * HT_TILE + row] = tot + P[bh];
        if (bwd) {
          ag_ln_relu_bwd(z, wh, P + Nn.g2, P + Nn.be2, sub, p.ln);
          ag_store_row(H + row * HT_AS, sub, wh);
        }
      }
      if (!bwd) continue;
      // B1. dH1 = dZ2 W2, W2 turned through the slab
      {
        const float* __restrict__ w2 = P + Nn.W2 + (size_t)(tid >> 6) * HT_HID + 4 * (tid & 63);
        float* const st = Sl + (tid >> 6) * HT_AS + 4 * (tid & 63);
        float4 pre[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pre[u] = *(const float4*)(w2 + (size_t)(4 * u) * HT_HID);
#pragma unroll
        for (int u = 0; u < 4; ++u) *(float4*)(st + 4 * u * HT_AS) = pre[u];
        __syncthreads();                              // slab 0 and dZ2 are in place
        ht_f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = ht_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < HT_HID / AG_SR; ++s) {
          const float* cur = Sl + (s & 1) * (AG_SR * HT_AS) + 4 * kq * HT_AS + wave * 64 + r;
          const bool more = s + 1 < HT_HID / AG_SR;   // (uniform)
          if (more) {
#pragma unroll
            for (int u = 0; u < 4; ++u) pre[u] = *(const float4*)(w2 + (size_t)(AG_SR * (s + 1) + 4 * u) * HT_HID);
          }
          const float4 av = *(const float4*)(H + r * HT_AS + AG_SR * s + 4 * kq);
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            const float4 wv = make_float4(cur[16 * tt], cur[HT_AS + 16 * tt], cur[2 * HT_AS + 16 * tt], cur[3 * HT_AS + 16 * tt]);
            acc[tt] = ht_mfma4(av, wv, acc[tt]);
          }
          if (more) {
#pragma unroll
            for (int u = 0; u < 4; ++u) *(float4*)(st + ((s + 1) & 1) * (AG_SR * HT_AS) + 4 * u * HT_AS) = pre[u];
          }
          __syncthreads();
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int m = 0; m < 4; ++m) H[(4 * kq + m) * HT_AS + wave * 64 + tt * 16 + r] = acc[tt][m];
      }
      __syncthreads();
      // B2. dZ1, in place (a thread rewrites the 16 elements it read)
      {
        float4 z[4], d[4];
        ht_load_row(Z1 + row * HT_AS, sub, z);
        ht_load_row(H + row * HT_AS, sub, d);
        ag_ln_relu_bwd(z, d, P + Nn.g1, P + Nn.be1, sub, p.ln);
        ag_store_row(H + row * HT_AS, sub, d);
      }
      __syncthreads();
      // B3. dQ/da: this wave's quarter of K = 256 -> Gp[wave]; dQ/ds on request, at the start actions
      for (int t = 0; t < ntile; ++t) {
        const int d = 16 * t + r;
        const bool on = d < a;
        const float* __restrict__ wcol = P + Nn.W1 + ob + min(d, a - 1);
        ht_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const int c0 = wave * 64 + 16 * cc + 4 * kq;
          const float4 av = *(const float4*)(H + r * HT_AS + c0);
          const float4 wv = make_float4(on ? wcol[(size_t)c0 * (size_t)Nn.ld1] : 0.f, on ? wcol[(size_t)(c0 + 1) * (size_t)Nn.ld1] : 0.f,
                                        on ? wcol[(size_t)(c0 + 2) * (size_t)Nn.ld1] : 0.f, on ? wcol[(size_t)(c0 + 3) * (size_t)Nn.ld1] : 0.f);
          acc = ht_mfma4(av, wv, acc);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) Gp[(wave * HT_TILE + 4 * kq + m) * AG_AS + d] = acc[m];
      }
      if (it == 0 && p.grad_obs) {                    // (uniform)
        float4 av[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) av[c] = *(const float4*)(H + r * HT_AS + 16 * c + 4 * kq);
        float* const out = p.grad_obs + (size_t)k * (size_t)p.n * (size_t)ob;
        for (int t = wave; 16 * t < ob; t += 4) {     // (uniform in the wave)
          const int col = 16 * t + r;
          const float* __restrict__ wcol = P + Nn.W1 + min(col, ob - 1) + (size_t)(4 * kq) * (size_t)Nn.ld1;
          ht_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const float* __restrict__ w = wcol + (size_t)(16 * c) * (size_t)Nn.ld1;
            const float4 wv = make_float4(w[0], w[(size_t)Nn.ld1], w[2 * (size_t)Nn.ld1], w[3 * (size_t)Nn.ld1]);
            acc = ht_mfma4(av[c], wv, acc);
          }
          if (col < ob) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
              if (r0 + 4 * kq + m < p.m) out[(size_t)(r0 + 4 * kq + m) * (size_t)ob + col] = acc[m];
          }
        }
      }
      __syncthreads();
      // B4. the four partials, in one order
      for (int idx = tid; idx < HT_TILE * AG_AS; idx += 256) {
        const int rr = idx / AG_AS, d = idx - rr * AG_AS;
        float v = 0.f;
        if (d < a) v = (Gp[idx] + Gp[HT_TILE * AG_AS + idx]) + (Gp[2 * HT_TILE * AG_AS + idx] + Gp[3 * HT_TILE * AG_AS + idx]);
        G[k * HT_TILE * AG_AS + idx] = v;
        if (it == 0 && p.grad && d < a && r0 + rr < p.m) p.grad[((size_t)k * (size_t)p.n + (size_t)(r0 + rr)) * (size_t)a + d] = v;
      }
    }
    __syncthreads();                                  // G and Qs are complete
    if (tid < HT_TILE) {
      const float q1 = Qs[tid], q2 = Qs[HT_TILE + tid];
      const float* g1 = G + tid * AG_AS;
      const float* g2 = G + (HT_TILE + tid) * AG_AS;
      if (it == 0) {
        qs1 = q1; qs2 = q2;
        float s1 = 0.f, s2 = 0.f, dot = 0.f;
        for (int d = 0; d < a; ++d) { s1 += g1[d] * g1[d]; s2 += g2[d] * g2[d]; dot += g1[d] * g2[d]; }
        n1 = sqrtf(s1); n2 = sqrtf(s2);
        cosv = (n1 == 0.f || n2 == 0.f) ? 0.f : dot / (n1 * n2);
      }
      if (it < steps) {
        const float* g = q1 <= q2 ? g1 : g2;
        float s = 0.f;
        for (int d = 0; d < a; ++d) { const float gu = g[d] * p.scale[d]; s += gu * gu; }
        const float den = fmaxf(sqrtf(s), 1e-8f);
        bool h = false;
        for (int d = 0; d < a; ++d) {
          const float sc = p.scale[d], lo = p.lo[d], hi = p.hi[d];
          const float gu = g[d] * sc;
          const float t = Act[tid * AG_AS + d] + ((p.lr * gu) / den) * sc;
          h = h || t < lo || t > hi;
          Act[tid * AG_AS + d] = fminf(fmaxf(t, lo), hi);
        }
        held += h ? 1 : 0;
      }
    }
    __syncthreads();                                  // Act is in place for the next forward
  }

  if (tid < HT_TILE && r0 + tid < p.m) {
    const size_t gr = (size_t)(r0 + tid);
    const float qe1 = Qs[tid], qe2 = Qs[HT_TILE + tid];
    if (p.q_start) { p.q_start[gr * p.q_start_ld] = qs1; p.q_start[gr * p.q_start_ld + 1] = qs2; }
    if (p.q_end) { p.q_end[gr * p.q_end_ld] = qe1; p.q_end[gr * p.q_end_ld + 1] = qe2; }
    float mv = 0.f;
    for (int d = 0; d < a; ++d) {
      const float v = Act[tid * AG_AS + d];
      if (p.refined) p.refined[gr * p.refined_ld + d] = v;
      const float u = (v - Act0[tid * AG_AS + d]) / p.scale[d];
      mv += u * u;
    }
    if (p.summary) {
      float* out = p.summary + gr * p.summary_ld;
      out[0] = qs1 <= qs2 ? qs1 : qs2;
      out[1] = qe1 <= qe2 ? qe1 : qe2;
      out[2] = n1; out[3] = n2; out[4] = cosv;
      out[5] = sqrtf(mv);
      out[6] = (float)held;
      out[7] = 0.f;
    }
  }
  if (tid == 0) {
    int cnt = 0;
    for (int g = 0; g < HT_TILE; ++g) cnt += (flag[g] && r0 + g < p.m) ? 1 : 0;
    p.bad[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(64) void k_ag_finish(int* words, const int* bad, int groups) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int c = 0;
  for (int i = 0; i < groups; ++i) c += bad[i];
  words[AG_W_NONFINITE] += c;
}
