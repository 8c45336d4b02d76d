// Device code of the nearest-ring-rows call (include/sactd3_ring_knn.h): k_knn_scan<DP>, k_knn_finish, k_knn_count.  Compiled in
// ring_knn.hip with contraction off and no packed fp32: every sum below is one fixed sequence of fp32 operations.
//
// k_knn_scan<DP>: 256 threads, grid (ring slices) x (query tiles of 64).  A workgroup stages its 64 transformed queries once into LDS,
// zero-extended to a multiple of 16 columns, and each of its four waves streams 16-row ring tiles of the slice.  Lane (r, g) = (lane &
// 15, lane >> 4) of a wave fetches, per 16-column block C, the 16 bytes at columns 16 C + 4 g .. + 3 of ring row r of its tile where they
// lie in the record -- a wave's request is sixteen whole 64-byte lines -- up to four blocks (a chunk of 64 columns) in one batch in front
// of the MFMAs.  Word j of that float4 is the A operand of the j-th v_mfma_f32_16x16x4f32 of the block (row r, k = g), and the same word
// of the query tile's LDS row is its B operand (k = g, column r): the MFMA sums the four g, the chain over (C, j) is the accumulator's.
// Four accumulators per ring tile, one per 16-query column tile; |x'|^2 accumulates beside them on the VALU in the lane's own columns
// and is closed over the four g by shuffles, in the same order for every row.
//
// Selection without private arrays: in the MFMA output layout lane (r, g) holds, per column tile, the selectors of query column r
// against ring rows 4 g .. 4 g + 3.  Each query keeps its current k-th best (sel, slot) as a threshold in LDS; a lane compares its
// candidates against it and appends the survivors to the query's LDS queue (an LDS atomic hands out the place).  A round is one tile
// per wave, closed by a barrier: at most 64 appends per query.  When a queue has passed KNN_MERGE_AT entries behind a round, and once
// at the end of the slice, lane q of wave 0 merges queue q into the query's sorted k-list by insertion and publishes the new threshold;
// KNN_QCAP = KNN_MERGE_AT + 64 is therefore never exceeded.  A threshold only ever falls, so a stale read keeps a candidate too many,
// never drops one: the k-list at the end is THE k smallest (sel, slot) of the slice whatever the order of the appends.  Slots outside the
// range, the excluded slot and non-finite selectors are dropped at the compare.  No atomics on global memory, no workgroup reads
// another's output.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "ring_knn.h"

#define KNN_MERGE_AT 16
#define KNN_QCAP (KNN_MERGE_AT + 64)

typedef float knn_f32x4 __attribute__((ext_vector_type(4)));

// (key - c) * w: THE transform, of queries and ring rows alike, in the scan and in the finish
__device__ __forceinline__ float knn_tf(float v, float c, float w) { return (v - c) * w; }
// (sel, slot) order: the total order of the selection
__device__ __forceinline__ bool knn_less(float s, int l, float s2, int l2) { return s < s2 || (s == s2 && l < l2); }

// lane q (< 64) of wave 0: queue q into the sorted k-list q, then the threshold.  Everything indexed lives in LDS.
__device__ __forceinline__ void knn_merge(int q, int k, bool live, float* Lsel, int* Lslot, const float* Wsel, const int* Wslot,
                                          int* Wn, float* Tsel, int* Tslot) {
  int n = Wn[q];
  n = n < KNN_QCAP ? n : KNN_QCAP;
  for (int c = 0; c < n; ++c) {
    const float s = Wsel[c * KNN_QT + q];
    const int l = Wslot[c * KNN_QT + q];
    int j = k - 1;
    if (!knn_less(s, l, Lsel[j * KNN_QT + q], Lslot[j * KNN_QT + q])) continue;
    while (j > 0) {
      const float ps = Lsel[(j - 1) * KNN_QT + q];
      const int pl = Lslot[(j - 1) * KNN_QT + q];
      if (!knn_less(s, l, ps, pl)) break;
      Lsel[j * KNN_QT + q] = ps; Lslot[j * KNN_QT + q] = pl;
      --j;
    }
    Lsel[j * KNN_QT + q] = s; Lslot[j * KNN_QT + q] = l;
  }
  Wn[q] = 0;
  if (live) { Tsel[q] = Lsel[(k - 1) * KNN_QT + q]; Tslot[q] = Lslot[(k - 1) * KNN_QT + q]; }
}

template <int DP>      // the LDS image holds keys of up to DP columns (a multiple of 16)
__global__ __launch_bounds__(256) void k_knn_scan(KnnArgs p) {
  constexpr int QS = DP + 4;      // row stride of the query image
  __shared__ __attribute__((aligned(16))) float Qs[KNN_QT * QS];
  __shared__ float Cs[DP], Ws[DP];                                  // offset, scale (0 / 1 where not given)
  __shared__ float Lsel[KNN_MAXK * KNN_QT]; __shared__ int Lslot[KNN_MAXK * KNN_QT];      // the k-lists, [j][query]
  __shared__ float Wsel[KNN_QCAP * KNN_QT]; __shared__ int Wslot[KNN_QCAP * KNN_QT];      // the queues, [place][query]
  __shared__ float Tsel[KNN_QT]; __shared__ int Tslot[KNN_QT];      // thresholds
  __shared__ int Wn[KNN_QT], Ex[KNN_QT];                            // queue lengths; excluded slots
  __shared__ int flag[3], nbad;      // flag[rd % 3]: a queue passed KNN_MERGE_AT in round rd

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x, q0 = blockIdx.y * KNN_QT;
  const int mq = min(KNN_QT, p.m - q0), D = p.D, k = p.k;
  const int Dp = (D + 15) & ~15;      // (<= DP: the launcher's choice)

  for (int d = tid; d < Dp; d += 256) {
    Cs[d] = (d < D && p.offset) ? p.offset[d] : 0.f;
    Ws[d] = (d < D && p.scale) ? p.scale[d] : 1.f;
  }
  __syncthreads();
  for (int i = tid; i < KNN_QT * Dp; i += 256) {
    const int qi = i / Dp, d = i - qi * Dp;
    Qs[qi * QS + d] = (qi < mq && d < D) ? knn_tf(p.q[(long)(q0 + qi) * p.q_ld + d], Cs[d], Ws[d]) : 0.f;
  }
  if (tid < KNN_QT) {
    const bool live = tid < mq;
    Tsel[tid] = live ? INFINITY : -INFINITY;      // a column behind the last query keeps nothing
    Tslot[tid] = INT_MAX; Wn[tid] = 0;
    long long ex = (live && p.exclude) ? p.exclude[(long)(q0 + tid) * p.exclude_ld] : -1;
    Ex[tid] = (ex >= 0 && ex < INT_MAX) ? (int)ex : -1;
    for (int j = 0; j < KNN_MAXK; ++j) { Lsel[j * KNN_QT + tid] = INFINITY; Lslot[j * KNN_QT + tid] = INT_MAX; }
  }
  if (tid == 0) { flag[0] = flag[1] = flag[2] = 0; nbad = 0; }
  __syncthreads();

  const long s0 = p.first + (long)slice * p.slice_rows;
  const long s1 = min(s0 + (long)p.slice_rows, p.last);      // (s0 < s1: nslices = ceil(len / slice_rows))
  const int ntiles = (int)((s1 - s0 + 15) / 16);
  const int rounds = (ntiles + 3) / 4;
  const bool count_rows = p.count_rows && blockIdx.y == 0;

  for (int rd = 0; rd < rounds; ++rd) {
    const int t = rd * 4 + wave;
    if (t < ntiles) {      // (uniform in a wave)
      const long t0 = s0 + (long)t * 16;
      const long row = t0 + r;
      const float* xp = p.ring + (size_t)(row < s1 ? row : s1 - 1) * p.rec_f + 4 * g;      // a row behind the slice reads its last row, and is dropped below
      knn_f32x4 acc[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) acc[tt] = knn_f32x4{0.f, 0.f, 0.f, 0.f};
      float xn = 0.f;
      for (int c0 = 0; c0 < Dp; c0 += 64) {
        const int nb = min(4, (Dp - c0) >> 4);
        float4 xv[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) xv[b] = *(const float4*)(xp + c0 + (b < nb ? 16 * b : 0));      // (a block behind the key: the first again, unused)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (b < nb) {      // (uniform)
            const int d = c0 + 16 * b + 4 * g;
            float4 x;      // the transformed words; a word behind the key is the zero the query image holds there
            x.x = d + 0 < D ? knn_tf(xv[b].x, Cs[d + 0], Ws[d + 0]) : 0.f;
            x.y = d + 1 < D ? knn_tf(xv[b].y, Cs[d + 1], Ws[d + 1]) : 0.f;
            x.z = d + 2 < D ? knn_tf(xv[b].z, Cs[d + 2], Ws[d + 2]) : 0.f;
            x.w = d + 3 < D ? knn_tf(xv[b].w, Cs[d + 3], Ws[d + 3]) : 0.f;
            xn = xn + x.x * x.x; xn = xn + x.y * x.y; xn = xn + x.z * x.z; xn = xn + x.w * x.w;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
              const float4 qv = *(const float4*)&Qs[(16 * tt + r) * QS + d];
              acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, qv.x, acc[tt], 0, 0, 0);
              acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, qv.y, acc[tt], 0, 0, 0);
              acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, qv.z, acc[tt], 0, 0, 0);
              acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, qv.w, acc[tt], 0, 0, 0);
            }
          }
        }
      }
      // |x'|^2 of row r: the four column groups' partials in one order, the same in the four lanes of a row
      const float xr = (__shfl(xn, r) + __shfl(xn, r + 16)) + (__shfl(xn, r + 32) + __shfl(xn, r + 48));
      if (count_rows && g == 0 && row < s1 && !isfinite(xr)) atomicAdd(&nbad, 1);
      float xo[4];      // ... of the rows this lane holds selectors of
#pragma unroll
      for (int i = 0; i < 4; ++i) xo[i] = __shfl(xr, 4 * g + i);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int qi = 16 * tt + r;
        const float T = Tsel[qi];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sel = xo[i] - 2.f * acc[tt][i];
          const long ro = t0 + 4 * g + i;
          const int slot = (int)ro;
          if (ro < s1 && isfinite(sel) && (sel < T || (sel == T && slot < Tslot[qi])) && slot != Ex[qi]) {
            const int at = atomicAdd(&Wn[qi], 1);
            if (at < KNN_QCAP) { Wsel[at * KNN_QT + qi] = sel; Wslot[at * KNN_QT + qi] = slot; }
            if (at >= KNN_MERGE_AT) flag[rd % 3] = 1;
          }
        }
      }
    }
    __syncthreads();
    // flag[rd % 3] is written in round rd alone, in front of this barrier, and read here by every thread; thread 0 clears the one of
    // round rd - 1, which every thread has read in front of this barrier and no thread writes again before the next
    if (tid == 0) flag[(rd + 2) % 3] = 0;
    if (flag[rd % 3]) {      // (uniform)
      if (tid < KNN_QT) knn_merge(tid, k, tid < mq, Lsel, Lslot, Wsel, Wslot, Wn, Tsel, Tslot);
      __syncthreads();
    }
  }
  if (tid < KNN_QT) knn_merge(tid, k, tid < mq, Lsel, Lslot, Wsel, Wslot, Wn, Tsel, Tslot);
  __syncthreads();
  for (int i = tid; i < mq * k; i += 256) {
    const int qi = i / k, j = i - qi * k;
    const size_t at = ((size_t)slice * KNN_CHUNK + (q0 + qi)) * KNN_MAXK + j;
    p.part_sel[at] = Lsel[j * KNN_QT + qi];
    p.part_slot[at] = Lslot[j * KNN_QT + qi];
  }
  if (blockIdx.y == 0 && tid == 0) p.bad[slice] = nbad;
}

// One wave per query: the k smallest (sel, slot) of the slices' lists by k rounds of a wave-wide minimum above the last winner; their
// direct distances, one lane per winner, d ascending; a rank sort by (dist2, slot); the query's flags for k_knn_count.
__global__ __launch_bounds__(64) void k_knn_finish(KnnArgs p) {
  const int q = blockIdx.x, lane = threadIdx.x, D = p.D, k = p.k;
  const float* qp = p.q + (long)q * p.q_ld;
  int bad = 0;
  for (int d = lane; d < D; d += 64)
    bad |= !isfinite(knn_tf(qp[d], p.offset ? p.offset[d] : 0.f, p.scale ? p.scale[d] : 1.f));
  bad = __any(bad);
  const int nc = p.nslices * k;
  float ps = -INFINITY, mys = INFINITY;      // the last winner; this lane's winner (lane j: the j-th)
  int pl = -1, myl = INT_MAX;
  for (int j = 0; j < k; ++j) {
    float bs = INFINITY;
    int bl = INT_MAX;
    for (int c = lane; c < nc; c += 64) {
      const int sl = c / k, jj = c - sl * k;
      const size_t at = ((size_t)sl * KNN_CHUNK + q) * KNN_MAXK + jj;
      const float s = p.part_sel[at];
      const int l = p.part_slot[at];
      if (l != INT_MAX && knn_less(ps, pl, s, l) && knn_less(s, l, bs, bl)) { bs = s; bl = l; }
    }
    for (int w = 32; w >= 1; w >>= 1) {
      const float os = __shfl_xor(bs, w);
      const int ol = __shfl_xor(bl, w);
      if (knn_less(os, ol, bs, bl)) { bs = os; bl = ol; }
    }
    if (bl == INT_MAX) break;      // (uniform: every lane holds the minimum) fewer than k exist
    if (lane == j) { mys = bs; myl = bl; }
    ps = bs; pl = bl;
  }
  float dist = INFINITY;
  if (myl != INT_MAX) {      // (lanes 0 .. k - 1 at most)
    const float* xp = p.ring + (size_t)myl * p.rec_f;
    dist = 0.f;
    for (int d = 0; d < D; ++d) {
      const float c = p.offset ? p.offset[d] : 0.f, w = p.scale ? p.scale[d] : 1.f;
      const float df = knn_tf(qp[d], c, w) - knn_tf(xp[d], c, w);
      dist = dist + df * df;
    }
  }
  (void)mys;
  int rank = 0, found = 0;
  for (int j = 0; j < KNN_MAXK; ++j) {
    const float od = __shfl(dist, j);
    const int ol = __shfl(myl, j);
    if (j < k) {
      found += ol != INT_MAX;
      rank += (od < dist || (od == dist && (ol < myl || (ol == myl && j < lane)))) ? 1 : 0;
    }
  }
  if (lane < k) {
    const bool hit = !bad && myl != INT_MAX;
    if (p.index) p.index[(long)q * p.index_ld + (bad ? lane : rank)] = hit ? (long long)myl : -1ll;
    if (p.dist2) p.dist2[(long)q * p.dist2_ld + (bad ? lane : rank)] = bad ? NAN : dist;
  }
  if (lane == 0) p.qflags[q] = bad ? KNN_F_BADQ : (found < k ? KNN_F_SHORT : 0);
}

// one workgroup: the launch's flags and per-slice counts into the feature's words (no atomics: the only writer)
__global__ __launch_bounds__(256) void k_knn_count(KnnArgs p) {
  __shared__ int red[3][256];
  int a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < p.m; i += 256) { a += (p.qflags[i] & KNN_F_BADQ) ? 1 : 0; c += (p.qflags[i] & KNN_F_SHORT) ? 1 : 0; }
  if (p.count_rows)
    for (int i = threadIdx.x; i < p.nslices; i += 256) b += p.bad[i];
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x < 3) {
    int s = 0;
    for (int i = 0; i < 256; ++i) s += red[threadIdx.x][i];
    const int w = threadIdx.x == 0 ? KNN_W_BADQ : threadIdx.x == 1 ? KNN_W_BADROWS : KNN_W_SHORT;
    p.words[w] += s;
  }
}
