// The mixed draw (include/sactd3.h: sactd3_rb_pin, sactd3_rb_set_mix, sactd3_rb_sample_mixed): device code.
// Included by engine.hip behind nstep_kernels.h (the graph form reads the ring length through dev_ring_len).
//
// A pinned ring holds P rows that appends never overwrite, slots [0, P), and live rows behind them, slots [P, len).  A mixed batch takes
// its first m rows from the pinned rows and the other B - m from the live ones.  With w_b the 32-bit word that philox_index selects for
// batch row b at the current sample counter (stream SACTD3_STREAM_INDEX, counter words (sample_ctr, 0, 0x100, b >> 2), word b & 3):
//   b <  m:  slot = (w_b * P) >> 32
//   b >= m:  slot = P + ((w_b * (len - P)) >> 32)
// so P = 0, m = 0 gives the slots of sactd3_rb_sample, bit for bit.  The kernel only draws: it leaves the slots in an int64 array of the
// engine's own, which k_batch_from_index / k_batch_from_index_g then stage -- there is no second gather.
//
// One workgroup of 256 threads.  One philox4x32_10 call serves four consecutive batch rows, whose four slots leave as one 32-byte store
// (the array is padded to a multiple of four rows).  Every thread reads the sample counter in front of the barrier, thread 0 advances it
// behind the barrier: the draw ticks the counter itself, no k_tick launch follows it.
// What the pinned two-region ring does NOT have yet: n-step chains and priorities (their age formula and refresh assume one wrap point, at
// slot 0); the host refuses those calls while rows are pinned.
#pragma once

// the words of the mixed draw the device holds, on a line of their own (made at the first mixed draw).  Published by the host on the
// learner stream in front of a launch, and only when they differ from what was last published (two adjacent words: k_set_int2)
struct MixCtl {
  int pinned;         // P: ring slots [0, P) are never overwritten by an append
  int prior_rows;     // m: batch rows [0, m) are drawn from the pinned rows
  int pad[30];
};
static_assert(sizeof(MixCtl) == 128, "one line");

struct MixDrawArgs {
  DevCtl* ctl;                            // seed, sample counter (read, then advanced once)
  long long* idx_out;                     // [B rounded up to 4], 32-byte aligned
  int B, len, P, m;
};
struct alignas(32) MixSlots4 { long long s[4]; };

__device__ __forceinline__ void mix_draw_body(const MixDrawArgs p) {
  const unsigned long long seed = p.ctl->seed;
  const unsigned ctr = (unsigned)p.ctl->sample_ctr;
  __syncthreads();                        // every thread holds the counter: thread 0 may now advance it
  const unsigned range_p = (unsigned)p.P, range_l = (unsigned)(p.len - p.P);
  const int groups = (p.B + 3) >> 2;
  for (int q = threadIdx.x; q < groups; q += 256) {
    const Philox4 r = philox4x32_10(ctr, 0u, SACTD3_STREAM_INDEX, (unsigned)q, (unsigned)seed, (unsigned)(seed >> 32));
    MixSlots4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool prior = 4 * q + k < p.m;
      const unsigned long long span = prior ? range_p : range_l;
      o.s[k] = (long long)((prior ? 0u : (unsigned)p.P) + (unsigned)(((unsigned long long)r.v[k] * span) >> 32));
    }
    *reinterpret_cast<MixSlots4*>(p.idx_out + 4 * (long)q) = o;
  }
  if (threadIdx.x == 0) p.ctl->sample_ctr = (int)(ctr + 1u);
}
// One template, two instances, appended to kernel_instances.inc (as instances they are emitted behind every kernel that existed before).
// k_mix_draw<false>, the call form: len, P and m as the host holds them (it has checked them: every range that is drawn from holds a
// row); `mc` and `cap` are not read.
// k_mix_draw<true>, the graph form (prio_kernels.h: the graph forms): the ring length from DevCtl, P and m from MixCtl.  Every value is
// bounded before anything is derived from it and every range is at least 1: a stale word never becomes an address (the staging kernel
// behind it checks each slot against the ring length once more).  For the values the host has checked it leaves the call form's bits.
template <bool GRAPH>
__global__ __launch_bounds__(256) void k_mix_draw(MixDrawArgs p, const MixCtl* mc, int cap) {
  if (GRAPH) {
    const int len = max(dev_ring_len(p.ctl, cap), 1);
    const int P = min(max(mc->pinned, 0), len);
    p.m = min(max(mc->prior_rows, 0), p.B);
    if (P == 0) p.m = 0;                  // (no pinned row: every row is a live one)
    if (P == len) p.m = p.B;              // (no live row: every row is a pinned one)
    p.len = len; p.P = P;
  }
  mix_draw_body(p);
}
