// Device code of the dormant-neuron scan and the ReDo recycler (include/sactd3_dormant.h), a translation unit of its own inside
// libsactd3_hip.so (dormant.hip): it shares philox.h with engine.hip and nothing else.
//
// k_dormant_compact: one workgroup.  The slots of idx that lie inside [0, len), in the order of idx, into `slots`, and their number V (and
//   n - V, the refused rows): thread t counts its contiguous share of idx, one thread turns the 256 counts into offsets, thread t writes
//   its share.  Everything behind it is cut from this list, so a scan's bits do not depend on refused rows standing among the valid ones.
// k_dormant_scan: the two hidden layers of the online nets over ring records (hidden_tile.h: the ring front end, LayerNorm + ReLU,
//   layer 2), and per neuron the sum of its activations.
//   Grid (min(ceil(n / 16), 128), nets), 256 threads, of which G = min(ceil(V / 16), 128) workgroups per net work: a pure function of the
//   valid rows.  Workgroup g walks the 16-row tiles g, g + G, ... of the checked list in that order and keeps, for the whole call,
//   thread c, the running sums of column c of both layers in registers.  Behind each LayerNorm + ReLU thread c adds rows 0 .. 15 of
//   column c in ascending order, skipping the rows behind V.  The sum is compensated (Kahan): a plain fp32 running sum over n rows
//   carries an error that grows with n, which the layers' own arithmetic does not; the order stays fixed, so the bits stay a pure
//   function of the inputs.
//   At the end: part[net][layer][g][c], plain vector stores.  No workgroup reads what another wrote, nothing spins, no atomics: the
//   bits are a pure function of (parameters, ring, the valid slots of idx in their order).
// k_dormant_finish: one workgroup per (net, layer).  Thread c sums the G partials of column c in ascending order (compensated) and divides by the
//   number V of valid rows; one fixed 256-wide pairwise tree gives the layer's sum; score = m_c / (sum / 256), 0 where the layer mean is
//   not positive or V == 0; dormant iff V > 0 and score <= tau.  -> scores, mask bytes, the pair's dormant count, the optional copy.
// k_redo_recycle: grid (16, 2 layers, nets); a workgroup owns 16 neurons of one (net, layer), wave w the neurons w, w + 4, ... of them.
//   For a marked neuron i the wave draws row i of the incoming weight -- element j is lane e & 3, e = i K + j, of philox_box_muller4 over
//   the counter words (epoch, matrix id, 0xA00, e >> 2) -- sums its squares (lane l: j = l, l + 64, ... ascending, then a fixed butterfly
//   over the 64 lanes), and stores g (c / |g|), c = sqrtf(min(1, K / 256)), 16 bytes per lane; a norm that is zero or not finite leaves
//   the row zero and is counted.  An element of a layer-2 row whose column is a marked layer-1 neuron is stored as 0 (the layer-1
//   workgroups store the same 0 there: whichever store lands last, the zero wins, in one launch).  Then bias 0, LayerNorm weight 1,
//   LayerNorm bias 0, the outgoing column 0, and Adam's two moments 0 at exactly those elements.
#pragma once
#include <hip/hip_runtime.h>

#include "dormant.h"
#include "philox.h"

#define SACTD3_STREAM_REDO 0xA00u   // third counter word of the recycler's draws (free beside 0x000 + site, 0x100 .. 0x900)

#include "hidden_tile.h"      // (dormant.hip includes this file where contraction is off and packed fp32 instructions are not formed)

// (a constant index each: a dynamically indexed kernel argument would be copied to scratch memory)
__device__ __forceinline__ NetView dm_pick(const NetView (&net)[DM_NETS], unsigned i) {
  NetView N = net[0];
  if (i == 1u) N = net[1];
  if (i == 2u) N = net[2];
  return N;
}

__global__ __launch_bounds__(256) void k_dormant_compact(DormantScanArgs p) {
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  if (blockIdx.x != 0) return;
  const int per = (p.n + 255) / 256, lo = min(tid * per, p.n), hi = min(lo + per, p.n);
  int c = 0;
  for (int r = lo; r < hi; ++r) {
    const long long raw = p.idx[(long)r * p.idx_ld];
    c += (raw >= 0 && raw < (long long)p.len) ? 1 : 0;
  }
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int t = cnt[i]; cnt[i] = run; run += t; }
    p.st.rows[0] = run;
    p.st.rows[1] = p.n - run;
  }
  __syncthreads();
  int o = cnt[tid];      // (at most n - (this share's valid rows): every store below lies inside [0, V))
  for (int r = lo; r < hi; ++r) {
    const long long raw = p.idx[(long)r * p.idx_ld];
    if (raw >= 0 && raw < (long long)p.len) p.st.slots[o++] = (int)raw;
  }
}

__global__ __launch_bounds__(256) void k_dormant_scan(DormantScanArgs p) {
  __shared__ __attribute__((aligned(16))) float Xs[HT_TILE * HT_XS];
  __shared__ __attribute__((aligned(16))) float H1[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float H2[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float Ln[4 * HT_HID];      // g1, be1, g2, be2
  __shared__ int okS[HT_TILE];
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
  if ((int)blockIdx.y >= p.nnets) return;
  const NetView N = dm_pick(p.net, blockIdx.y);
  const int V = min(max(p.st.rows[0], 0), p.n);      // k_dormant_compact's, one launch ahead on this stream
  const int g = blockIdx.x, ntiles = (V + HT_TILE - 1) / HT_TILE, G = min(ntiles, DM_MAXG);
  if (g >= G) return;                                // (block-uniform; k_dormant_finish reads the partials of [0, G) alone)

  float b1c[4], b2c[4];
  ht_ring_load(N, tid, Ln, b1c, b2c);
  float sum1 = 0.f, sum2 = 0.f;      // thread c = tid: column c of layer 1 / layer 2 over this workgroup's valid rows
  float cmp1 = 0.f, cmp2 = 0.f;      // ... and their compensation terms

  for (int tile = g; tile < ntiles; tile += G) {
    const bool ok = ht_ring_layer1(N, p.ring, p.rec_f, p.len, p.st.slots, V, tile, Xs, H1, b1c, tid);
    if (sub == 0) okS[row] = ok ? 1 : 0;
    __syncthreads();
    ht_ln_relu_lds(H1 + row * HT_AS, Ln, Ln + HT_HID, sub, p.ln);
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < HT_TILE; ++rr) {
      const float h = H1[rr * HT_AS + tid];
      if (okS[rr]) ht_kahan(sum1, cmp1, h);
    }
    ht_layer2(H1, N.P + N.W2, b2c, H2, wave, r, kq);
    __syncthreads();
    ht_ln_relu_lds(H2 + row * HT_AS, Ln + 2 * HT_HID, Ln + 3 * HT_HID, sub, p.ln);
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < HT_TILE; ++rr) {
      const float h = H2[rr * HT_AS + tid];
      if (okS[rr]) ht_kahan(sum2, cmp2, h);
    }
    __syncthreads();      // okS is written again by the next tile
  }

  p.st.part[(((size_t)N.id * 2 + 0) * DM_MAXG + g) * HT_HID + tid] = sum1;
  p.st.part[(((size_t)N.id * 2 + 1) * DM_MAXG + g) * HT_HID + tid] = sum2;
}

__global__ __launch_bounds__(256) void k_dormant_finish(DormantScanArgs p) {
  __shared__ float red[HT_HID];
  const int tid = threadIdx.x, layer = blockIdx.x;
  if ((int)blockIdx.y >= p.nnets || layer > 1) return;
  const int id = dm_pick(p.net, blockIdx.y).id, pair = 2 * id + layer;
  const int V = min(max(p.st.rows[0], 0), p.n), R = p.st.rows[1];
  const int tiles = (V + HT_TILE - 1) / HT_TILE, G = tiles < DM_MAXG ? tiles : DM_MAXG;
  float s = 0.f, cmp = 0.f;
  for (int g = 0; g < G; ++g) {
    ht_kahan(s, cmp, p.st.part[(((size_t)id * 2 + layer) * DM_MAXG + g) * HT_HID + tid]);
  }
  const float m = V > 0 ? s / (float)V : 0.f;
  red[tid] = m;
  __syncthreads();
  for (int w = HT_HID / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] = red[tid] + red[tid + w];
    __syncthreads();
  }
  const float mean = red[0] * (1.0f / HT_HID);
  const float score = (V > 0 && mean > 0.f) ? m / mean : 0.f;
  const bool dormant = V > 0 && score <= p.tau;
  const int count = __syncthreads_count(dormant ? 1 : 0);
  p.st.scores[pair * HT_HID + tid] = score;
  p.st.mask[pair * HT_HID + tid] = dormant ? 1 : 0;
  if (p.out) p.out[pair * HT_HID + tid] = score;
  if (tid == 0) {
    p.st.words[DM_W_COUNT + pair] = count;
    if (blockIdx.x == 0 && blockIdx.y == 0) {      // one thread of the launch: the rows are the same for every net
      p.st.words[DM_W_VALID] = V;
      p.st.words[DM_W_REFUSED] += R;
    }
  }
}

// element e of matrix `mat`'s redraw in recycle epoch `epoch`: see the header of this file
__device__ __forceinline__ float redo_normal(unsigned long long seed, unsigned epoch, unsigned mat, unsigned e) {
  const float4 z = philox_box_muller4(philox4x32_10(epoch, mat, SACTD3_STREAM_REDO, e >> 2, (uint32_t)seed, (uint32_t)(seed >> 32)));
  return ht_pick(z, e & 3u);
}

__global__ __launch_bounds__(256) void k_redo_recycle(RedoArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, layer = blockIdx.y;
  if ((int)blockIdx.z >= p.nnets || layer > 1) return;
  const NetView N = dm_pick(p.net, blockIdx.z);
  const uint8_t* __restrict__ mk = p.st.mask + (2 * N.id + layer) * HT_HID;
  const uint8_t* __restrict__ mk1 = p.st.mask + (2 * N.id) * HT_HID;      // the layer-1 mask: the columns of W2 that become 0
  const int K = layer ? HT_HID : N.K, ld = layer ? HT_HID : N.ld1;
  const int W = layer ? N.W2 : N.W1, b = layer ? N.b2 : N.b1, gm = layer ? N.g2 : N.g1, be = layer ? N.be2 : N.be1;
  const unsigned mat = 3u * (unsigned)N.id + (unsigned)layer;
  const float c = sqrtf(fminf(1.0f, (float)K / (float)HT_HID));
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q = 0; q < 4; ++q) {
    const int i = blockIdx.x * 16 + wave + 4 * q;
    if (!mk[i]) continue;      // (wave-uniform)
    const unsigned e0 = (unsigned)i * (unsigned)K;
    float ss = 0.f;
    for (int j = lane; j < K; j += 64) {
      const float z = redo_normal(p.seed, p.epoch, mat, e0 + (unsigned)j);
      ss += z * z;
    }
    ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
    ss += __shfl_xor(ss, 8); ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);
    const bool good = ss > 0.f && ss < __builtin_inff();      // (false for a NaN too)
    const float scale = good ? c / sqrtf(ss) : 0.f;
    for (int j = 4 * lane; j < ld; j += 256) {
      float w[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool drawn = good && j + t < K && !(layer && mk1[j + t]);
        w[t] = drawn ? redo_normal(p.seed, p.epoch, mat, e0 + (unsigned)(j + t)) * scale : 0.f;
      }
      const size_t at = (size_t)W + (size_t)i * ld + j;
      *(float4*)(N.P + at) = make_float4(w[0], w[1], w[2], w[3]);
      *(float4*)(N.M + at) = zero;
      *(float4*)(N.V + at) = zero;
    }
    if (lane == 0) {
      N.P[b + i] = 0.f; N.P[gm + i] = 1.f; N.P[be + i] = 0.f;
      N.M[b + i] = 0.f; N.M[gm + i] = 0.f; N.M[be + i] = 0.f;
      N.V[b + i] = 0.f; N.V[gm + i] = 0.f; N.V[be + i] = 0.f;
      atomicAdd(p.st.words + DM_W_RECYCLED, 1);
      if (!good) atomicAdd(p.st.words + DM_W_LEFT_ZERO, 1);
    }
    // the outgoing column: W2[:, i] behind layer 1, every head row's element i behind layer 2
    const int rows_out = layer ? N.nh : HT_HID;
    const size_t out0 = (size_t)(layer ? N.Wh : N.W2) + i;
    for (int rr = lane; rr < rows_out; rr += 64) {
      N.P[out0 + (size_t)rr * HT_HID] = 0.f; N.M[out0 + (size_t)rr * HT_HID] = 0.f; N.V[out0 + (size_t)rr * HT_HID] = 0.f;
    }
  }
}
