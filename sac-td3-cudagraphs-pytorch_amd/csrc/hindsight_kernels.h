// Hindsight relabelling at staging (include/sactd3.h: sactd3_rb_sample_hindsight*): device code.  A translation unit of its own
// (hindsight.hip): it shares philox.h with engine.hip and nothing else -- the magic division and the slot arithmetic of nstep_kernels.h
// are restated below.
//
// k_hindsight_stage is k_batch_from_index with an episode walk in front of the copy and a goal substitution inside it: the "future"
// strategy of hindsight experience replay (Andrychowicz et al. 2017).  Per batch row b with start slot i0 (the definitions of the chain
// are those of nstep_kernels.h):
//   age(i)  = i while len < cap, else (i - cursor) mod cap
//   slot_j  = (i0 + j * stride) mod cap, which EXISTS iff age(i0) + j * stride < len
//   link j -> j+1 holds iff slot_{j+1} exists, the flag float of slot_j is 0, and the first o floats of slot_j's s' field equal, as
//            32-bit patterns, the first o floats of slot_{j+1}'s record
//   L       = 1 + the number of leading links that hold among links 0 .. window-2, 1 <= L <= window
//   draw    : Philox counter words (hctr, 0, 0x600, b); relabelled iff philox_u01(v0) < ratio, j = (v1 * L) >> 32.  With `choice`:
//             choice[b] < 0: not relabelled, else relabelled with j = min(choice[b], L - 1)
//   goal    = floats [ag_off, ag_off + G) of the s' field of slot_j, as bits (j = 0: the row's own arrival)
// and the slot receives X = [s|a] of slot_0 with floats [dg_off, dg_off + G) of s replaced, Xn = s' of slot_0 with the same floats
// replaced, done = the stored flag, rew = (acc <= thr * thr) ? 0 : -1 with acc the sum over c, in index order, of
// (ag'_c - g_c) * (ag'_c - g_c), ag' the achieved goal in slot_0's own s' -- every operation one fp32 rounding, no contraction.  A row
// that is not relabelled receives its record's bits: what k_batch_from_index leaves, reward included.
//
// Rules the kernel keeps (those of nstep_body.inc):
//   * all candidate slots of a row are arithmetic in i0: every load of a phase is issued before anything depends on one.
//   * a start index outside [0, len), and a candidate slot that does not exist, never become an address: the load goes to the row's
//     slot_0 (ring slot 0 for a refused row) and the link counts as broken.
//   * loads first, stores last in each phase; plain vector stores and LDS atomics only; the three counters take one global atomicAdd
//     per counted row.  No indexed local array: every array below is unrolled into registers.
// This file holds what the kernels share and the graph's draw, k_hindsight_draw_g.  The staging kernel's body is
// hindsight_stage_body.inc, which hindsight.hip includes into both of its forms, k_hindsight_stage and k_hindsight_stage_g: the same
// rules hold for the graph form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hindsight.h"
#include "philox.h"

#define SACTD3_STREAM_HINDSIGHT 0x600u   // third counter word of the relabelling draw
#define HS_U 4                           // link-phase items per thread and round: 2 * HS_U 16-byte loads in flight
#define HS_PIN(x) asm volatile("" : "+v"(x))

__device__ __forceinline__ unsigned hs_fast_div(unsigned n, unsigned d, unsigned magic) { return magic ? __umulhi(n, magic) : n / d; }
// slot_j of a row whose slot_0 is s0, for a j that exists (then j * stride < cap: one conditional subtraction is the modulo)
__device__ __forceinline__ int hs_slot(int s0, int j, int stride, int cap) {
  const long long t = (long long)s0 + (long long)j * (long long)stride;
  return (int)(t >= (long long)cap ? t - (long long)cap : t);
}
__device__ __forceinline__ bool hs_differs(const float4& a, const float4& b, int c, int o) {
  bool d = false;
  d |= 4 * c + 0 < o && __float_as_uint(a.x) != __float_as_uint(b.x);
  d |= 4 * c + 1 < o && __float_as_uint(a.y) != __float_as_uint(b.y);
  d |= 4 * c + 2 < o && __float_as_uint(a.z) != __float_as_uint(b.z);
  d |= 4 * c + 3 < o && __float_as_uint(a.w) != __float_as_uint(b.w);
  return d;
}
// element e of a chunk of the copy phase: the goal's float where e falls into [dg_off, dg_off + G) of a relabelled row
__device__ __forceinline__ float hs_pick(float v, int e, bool relabel, int dg_off, int G, const float* g) {
  const int c = e - dg_off;
  const bool in = relabel && c >= 0 && c < G;
  const float gv = g[in ? c : 0];
  return in ? gv : v;
}

// ---- the graph forms (sactd3_step_sampled with SACTD3_DRAW_HINDSIGHT): what varies between two replays of a captured graph is read from
// device memory through host-computed pointers -- this translation unit knows no struct of engine.hip's.  Every word is bounded before
// anything is derived from it, as engine.hip's dev_ring_len / dev_ring_cursor bound it: a stale word never becomes an address.
__device__ __forceinline__ int hs_dev_len(const int* ring_words, int cap) { return min(max(ring_words[0], 0), cap); }
__device__ __forceinline__ int hs_dev_cursor(const int* ring_words, int cap) { return min(max(ring_words[1], 0), max(cap - 1, 0)); }
struct alignas(32) HsSlots4 { long long s[4]; };

// The graph's draw: the uniform draw of sactd3_rb_sample_hindsight (k_mix_draw<false> with P = 0, m = 0), bit for bit -- word b & 3 of
// philox4x32_10(sample_ctr, 0, 0x100, b >> 2) keyed by the seed gives slot = (w * len) >> 32, four slots leave as one 32-byte store.
// One workgroup of 256 threads.  len is the device's, never below 1.  The kernel also carries the hindsight draw counter into the graph:
// every thread reads the sample counter and the master word in front of the barrier; behind it thread 0 advances the sample counter,
// leaves the old hindsight count in the snapshot word (k_hindsight_stage_g's hctr) and advances the master word.
__global__ __launch_bounds__(256) void k_hindsight_draw_g(HindsightDrawArgs p) {
  const unsigned long long seed = *p.seed;
  const unsigned ctr = (unsigned)*p.sample_ctr;
  const unsigned hcount = (unsigned)p.hs_words[HS_WORD_MASTER];
  const unsigned len = (unsigned)max(hs_dev_len(p.ring_words, p.cap), 1);
  __syncthreads();                        // every thread holds both counters: thread 0 may now advance them
  const int groups = (p.B + 3) >> 2;
  for (int q = threadIdx.x; q < groups; q += 256) {
    const Philox4 r = philox4x32_10(ctr, 0u, SACTD3_STREAM_INDEX, (unsigned)q, (unsigned)seed, (unsigned)(seed >> 32));
    HsSlots4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.s[k] = (long long)(unsigned)(((unsigned long long)r.v[k] * (unsigned long long)len) >> 32);
    *reinterpret_cast<HsSlots4*>(p.idx_out + 4 * (long)q) = o;
  }
  if (threadIdx.x == 0) {
    *p.sample_ctr = (int)(ctr + 1u);
    p.hs_words[HS_WORD_SNAPSHOT] = (int)hcount;
    p.hs_words[HS_WORD_MASTER] = (int)(hcount + 1u);
  }
}
