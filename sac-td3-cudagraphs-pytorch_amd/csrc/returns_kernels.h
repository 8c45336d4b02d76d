// Device code of the returns-to-go call (include/sactd3_returns.h): k_rtg_scan, k_rtg_carry, k_rtg_apply.  Compiled in returns.hip with
// contraction off and no packed fp32: every sum below is one fixed tree of fp32 operations.
//
// Work order.  The n rows of the range are laid out chain-major: chain c = age mod stride owns cnt(c) = ceil((n - c) / stride)
// consecutive positions, t = age div stride ascending, so with q = n / stride and rem = n % stride the first rem chains own q + 1
// positions and start at c (q + 1), the others own q and start at rem (q + 1) + (c - rem) q: position -> age is two divisions
// (rtg_age).  The successor of a position is the next position, and the last position of every chain has no successor, which closes
// its chain like any other break.  The whole problem is therefore ONE flat segmented reverse scan over n positions, with the same
// parallelism for 4 envs x 250 000 steps as for 4 096 envs x 256 steps.
//
// The scanned element is the flagged affine map (kind, M, B, U, L, last) of a run of positions as seen from its first one: kind = 0
// while every link of the run holds, else how the chain that starts there ends (RTG_TERMINATED / TRUNCATED / OPEN); B, U, L, last =
// discounted sum, plain sum, rows and last slot of that chain inside the run; M = gamma^L, the factor of whatever follows an open
// run.  rtg_join(l, r) = l when l is closed, else (r.kind, l.M r.M, l.B + l.M r.B, l.U + r.U, l.L + r.L, r.last): a broken link is the
// flag, never a multiplication by zero, so a non-finite reward stays inside its chain.
//
// k_rtg_scan: 256 threads per RTG_SPAN consecutive positions.
//   phase 0  a position's own slot and its successor's (its own where none exists: never an address outside the ring) into LDS, for
//            the span and for the one position in front of it, whose link decides RTG_START of the span's first position.
//   phase 1  the links at HBM rate: items (position, 16-byte chunk of s' against the successor's s) and (position, [r, d]) are dealt
//            flat over the threads, consecutive lanes on consecutive chunks of a record, RTG_U items = 2 RTG_U loads per lane in
//            flight before anything depends on one (nstep_body.inc, phase 1); a difference is or-ed into the position's LDS word.
//            Consecutive rows of a chain sit in one span, so a record's s and s' are fetched once each.
//   phase 2  a thread folds its RTG_PER positions in reverse in registers, the waves scan in reverse by shuffles, the four waves join
//            through LDS, and the thread walks its positions again behind what stands to its right.  Per position the local result
//            goes to scratch (the span's first position is the span's aggregate); ends, starts and non-finite rewards are counted.
// k_rtg_carry: one workgroup scans the spans' aggregates in reverse with the same code and leaves per span what follows it.
// k_rtg_apply: one thread per position joins the carry into a result still open at its span's end and scatters to the caller's
// arrays by slot.  No workgroup waits for another: the three launches are the joins.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "returns.h"

#define RTG_U 4          // link-phase items per thread and round: 2 * RTG_U 16-byte loads in flight
#define RTG_PIN(x) asm volatile("" : "+v"(x))

struct Rtg { int kind; float M, B, U; int L, last; };
__device__ __forceinline__ Rtg rtg_none() { return Rtg{0, 1.f, 0.f, 0.f, 0, -1}; }      // L == 0: "nothing here", the scan's identity
__device__ __forceinline__ Rtg rtg_join(const Rtg& l, const Rtg& r) {
  const bool keep = l.kind != 0 || r.L == 0, take = l.L == 0;
  const float t = l.M * r.B;
  Rtg o;
  o.kind = keep ? l.kind : r.kind;
  o.M = keep ? l.M : take ? r.M : l.M * r.M;
  o.B = keep ? l.B : take ? r.B : l.B + t;
  o.U = keep ? l.U : take ? r.U : l.U + r.U;
  o.L = keep ? l.L : l.L + r.L;
  o.last = keep ? l.last : r.last;
  return o;
}
__device__ __forceinline__ Rtg rtg_shfl_down(const Rtg& x, int off) {
  Rtg y;
  y.kind = __shfl_down(x.kind, off, 64); y.M = __shfl_down(x.M, off, 64); y.B = __shfl_down(x.B, off, 64);
  y.U = __shfl_down(x.U, off, 64); y.L = __shfl_down(x.L, off, 64); y.last = __shfl_down(x.last, off, 64);
  return y;
}
// `mine`: the join of a thread's own run, threads in position order.  -> the join of everything to the right of the thread inside
// the workgroup of 256, in one fixed order.  wave_s: four elements of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ Rtg rtg_right_of(const Rtg& mine, Rtg* wave_s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Rtg x = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const Rtg y = rtg_shfl_down(x, off);
    if (lane + off < 64) x = rtg_join(x, y);
  }
  if (lane == 0) wave_s[w] = x;
  Rtg nx = rtg_shfl_down(x, 1);
  if (lane == 63) nx = rtg_none();
  __syncthreads();
  Rtg t = rtg_none();
#pragma unroll
  for (int v = 3; v >= 1; --v)
    if (v > w) t = rtg_join(wave_s[v], t);
  return rtg_join(nx, t);
}

// age of position pos (0 <= pos < n)
__device__ __forceinline__ int rtg_age(const RtgArgs& p, int pos) {
  const unsigned q1 = (unsigned)p.q + 1u, head = (unsigned)p.rem * q1, qq = p.q > 0 ? (unsigned)p.q : 1u, u = (unsigned)pos;
  const bool front = u < head;
  const unsigned v = front ? u : u - head, d = front ? q1 : qq;
  const unsigned c = v / d, t = v - c * d;
  return (int)((front ? c : c + (unsigned)p.rem) + t * (unsigned)p.stride);
}
__device__ __forceinline__ int rtg_slot(const RtgArgs& p, int age) {
  const unsigned s = (unsigned)p.base + (unsigned)age;
  return (int)(s >= (unsigned)p.cap ? s - (unsigned)p.cap : s);
}
__device__ __forceinline__ bool rtg_differs(const float4& a, const float4& b, int c, int o) {
  bool d = false;
  d |= 4 * c + 0 < o && __float_as_uint(a.x) != __float_as_uint(b.x);
  d |= 4 * c + 1 < o && __float_as_uint(a.y) != __float_as_uint(b.y);
  d |= 4 * c + 2 < o && __float_as_uint(a.z) != __float_as_uint(b.z);
  d |= 4 * c + 3 < o && __float_as_uint(a.w) != __float_as_uint(b.w);
  return d;
}
// the link word of a position -> how a chain that ends there ends (0: the link holds)
__device__ __forceinline__ int rtg_kind(unsigned w) { return (w & 1u) ? RTG_TERMINATED : (w & 4u) ? RTG_OPEN : (w & 2u) ? RTG_TRUNCATED : 0; }

// the scratch arrays of RtgArgs: per position, then per span
struct RtgScratch { float *M, *B, *U, *cM, *cB, *cU; int *K, *L, *last, *cK, *cL, *clast; };
__device__ __forceinline__ RtgScratch rtg_scratch_of(const RtgArgs& p) {
  const size_t cap = (size_t)p.cap, nb = ((size_t)p.cap + RTG_SPAN - 1) / RTG_SPAN;
  float* cf = p.sf + 3 * cap; int* ci = p.si + 3 * cap;
  return RtgScratch{p.sf, p.sf + cap, p.sf + 2 * cap, cf, cf + nb, cf + 2 * nb, p.si, p.si + cap, p.si + 2 * cap, ci, ci + nb, ci + 2 * nb};
}

__global__ __launch_bounds__(256) void k_rtg_scan(RtgArgs p) {
  // row i of the tables is position p0 - 1 + i: row 0 is the position in front of the span
  __shared__ int sa_s[RTG_SPAN + 1], sb_s[RTG_SPAN + 1];      // a position's slot and its successor's (its own where none exists)
  __shared__ unsigned brk_s[RTG_SPAN + 1];                    // bit 0: flag != 0, bit 1: the bits differ, bit 2: no successor
  __shared__ float r_s[RTG_SPAN + 1];
  __shared__ Rtg wave_s[4];
  __shared__ unsigned cnt_s[5];
  const int p0 = blockIdx.x * RTG_SPAN;
  if (p0 >= p.n) return;                                      // (block-uniform; the host launches no such span)
  const int rows = min(RTG_SPAN, p.n - p0) + 1;
  if (threadIdx.x < 5) cnt_s[threadIdx.x] = 0u;

  // ---- phase 0
  for (int i = threadIdx.x; i < rows; i += 256) {
    const int pos = p0 - 1 + i;
    const bool in = pos >= 0;
    const int age = in ? rtg_age(p, pos) : 0;
    const bool succ = in && age < p.n - p.stride;             // age + stride < n
    const int sa = rtg_slot(p, age);
    sa_s[i] = sa; sb_s[i] = succ ? rtg_slot(p, age + p.stride) : sa;
    brk_s[i] = succ ? 0u : 4u; r_s[i] = 0.f;
  }
  __syncthreads();

  // ---- phase 1: per row co compare items (chunk c of s' against chunk c of the successor's s) and one [r, d] item
  {
    const int co = (p.o + 3) >> 2, ipr = co + 1;
    const int first = p0 == 0 ? ipr : 0;                      // row 0 stands for no position in front of the first span
    const int items = rows * ipr;
    for (int base = first + (int)threadIdx.x; base < items; base += 256 * RTG_U) {
      int row[RTG_U], ch[RTG_U]; bool on[RTG_U], cmp[RTG_U]; float4 a[RTG_U], b[RTG_U];
#pragma unroll
      for (int u = 0; u < RTG_U; ++u) {
        const int it = base + u * 256;
        on[u] = it < items;
        const int r = on[u] ? it / ipr : rows - 1, rem = on[u] ? it - r * ipr : co;
        row[u] = r; cmp[u] = rem < co; ch[u] = cmp[u] ? rem : 0;
        const int sa = sa_s[r], sb = sb_s[r];
        a[u] = p.ring[(long)sa * p.rec4 + (cmp[u] ? p.cx + ch[u] : p.cx + p.cn)];
        b[u] = p.ring[(long)sb * p.rec4 + ch[u]];
      }
#pragma unroll
      for (int u = 0; u < RTG_U; ++u) { RTG_PIN(a[u].x); RTG_PIN(a[u].y); RTG_PIN(a[u].z); RTG_PIN(a[u].w); RTG_PIN(b[u].x); RTG_PIN(b[u].y); RTG_PIN(b[u].z); RTG_PIN(b[u].w); }
#pragma unroll
      for (int u = 0; u < RTG_U; ++u) {
        if (!on[u]) continue;
        if (cmp[u]) {
          if (rtg_differs(a[u], b[u], ch[u], p.o)) atomicOr(&brk_s[row[u]], 2u);
        } else {
          r_s[row[u]] = a[u].x;
          if (!(a[u].y == 0.f)) atomicOr(&brk_s[row[u]], 1u);
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: thread j owns rows 1 + RTG_PER j .. of the tables
  const int i0 = 1 + RTG_PER * (int)threadIdx.x;
  Rtg e[RTG_PER];
  Rtg mine = rtg_none();
  unsigned c_term = 0, c_trunc = 0, c_open = 0, c_start = 0, c_bad = 0;
#pragma unroll
  for (int j = RTG_PER - 1; j >= 0; --j) {
    const int i = i0 + j;
    const bool in = i < rows;
    const int kind = in ? rtg_kind(brk_s[i]) : 0;
    const float r = in ? r_s[i] : 0.f;
    e[j] = in ? Rtg{kind, p.gamma, r, r, 1, sa_s[i]} : rtg_none();
    mine = rtg_join(e[j], mine);
    c_term += kind == RTG_TERMINATED; c_trunc += kind == RTG_TRUNCATED; c_open += kind == RTG_OPEN;
    c_bad += in && !(fabsf(r) <= FLT_MAX);
  }
  Rtg acc = rtg_right_of(mine, wave_s);
  const RtgScratch s = rtg_scratch_of(p);
#pragma unroll
  for (int j = RTG_PER - 1; j >= 0; --j) {
    const int i = i0 + j, pos = p0 - 1 + i;
    acc = rtg_join(e[j], acc);
    if (i >= rows) continue;
    const bool start = pos == 0 || rtg_kind(brk_s[i - 1]) != 0;      // (row 0 of the first span is never read: pos == 0 there)
    c_start += start;
    s.M[pos] = acc.M; s.B[pos] = acc.B; s.U[pos] = acc.U;
    s.K[pos] = acc.kind | (start ? RTG_START : 0); s.L[pos] = acc.L; s.last[pos] = acc.last;
  }
  if (c_term) atomicAdd(&cnt_s[RTG_W_TERMINATED], c_term);
  if (c_trunc) atomicAdd(&cnt_s[RTG_W_TRUNCATED], c_trunc);
  if (c_open) atomicAdd(&cnt_s[RTG_W_OPEN], c_open);
  if (c_start) atomicAdd(&cnt_s[RTG_W_START], c_start);
  if (c_bad) atomicAdd(&cnt_s[RTG_W_BADR], c_bad);
  __syncthreads();
  if (threadIdx.x < 5 && cnt_s[threadIdx.x]) atomicAdd(p.words + threadIdx.x, (unsigned long long)cnt_s[threadIdx.x]);
}

// one workgroup: span b's aggregate is the local result of its first position; carry[b] = the join of the spans behind b, in reverse
__global__ __launch_bounds__(256) void k_rtg_carry(RtgArgs p) {
  __shared__ Rtg wave_s[4];
  const RtgScratch s = rtg_scratch_of(p);
  const int nb = (p.n + RTG_SPAN - 1) / RTG_SPAN, per = (nb + 255) / 256;
  const int lo = min(nb, per * (int)threadIdx.x), hi = min(nb, lo + per);
  auto aggregate = [&](int b) {
    const size_t pos = (size_t)b * RTG_SPAN;
    return Rtg{s.K[pos] & 7, s.M[pos], s.B[pos], s.U[pos], s.L[pos], s.last[pos]};
  };
  Rtg mine = rtg_none();
  for (int b = hi - 1; b >= lo; --b) mine = rtg_join(aggregate(b), mine);
  Rtg acc = rtg_right_of(mine, wave_s);
  for (int b = hi - 1; b >= lo; --b) {
    s.cK[b] = acc.kind; s.cM[b] = acc.M; s.cB[b] = acc.B; s.cU[b] = acc.U; s.cL[b] = acc.L; s.clast[b] = acc.last;
    acc = rtg_join(aggregate(b), acc);
  }
}

__global__ __launch_bounds__(256) void k_rtg_apply(RtgArgs p) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= p.n) return;
  const RtgScratch s = rtg_scratch_of(p);
  const int b = pos / RTG_SPAN, word = s.K[pos];
  Rtg x{word & 7, s.M[pos], s.B[pos], s.U[pos], s.L[pos], s.last[pos]};
  // (an open result's chain goes on in the next span, so a carry stands there; a closed one's join returns it unchanged)
  const Rtg c{s.cK[b], s.cM[b], s.cB[b], s.cU[b], s.cL[b], s.clast[b]};
  x = rtg_join(x, c);
  const long slot = rtg_slot(p, rtg_age(p, pos));
  if (p.returns) p.returns[slot * p.returns_ld] = x.B;
  if (p.undiscounted) p.undiscounted[slot * p.undiscounted_ld] = x.U;
  if (p.length) p.length[slot * p.length_ld] = x.L;
  if (p.last) p.last[slot * p.last_ld] = x.last;
  if (p.ends) p.ends[slot * p.ends_ld] = x.kind | (word & RTG_START);
}
