// Proportional prioritised replay (Schaul et al. 2016, proportional variant, draws with replacement) as engine state: device code.
// Included by engine.hip behind kernels.h (its structs and helpers are used here).
//
// Structure: a flat two-level table.  leaf[slot] = p^alpha of ring slot `slot` (0 for a slot the ring has not filled), in groups of
// PRIO_G = 1024 consecutive slots; sums[g] = the sum of group g's leaves.  The top level is as wide as the ring needs (977 sums for a
// 1 M ring) and is walked 1024 sums at a time.  Both arrays are padded with zeros to a multiple of 1024 floats, so every thread of a
// 256-thread block can always load its float4.
//
// Rules every kernel here keeps:
//   * a group's sum is ALWAYS recomputed from its 1024 leaves by prio_scan, whose order depends on nothing but the position of a
//     value in the group -- never adjusted incrementally.  The table cannot drift, and two histories that reach the same leaves reach
//     the same sums bit for bit.
//   * no workgroup reads what another workgroup of the same launch stores (the per-XCD L2s are not coherent, a CU's L1 is never
//     refreshed: DESIGN.md).  A write-back runs one workgroup per batch row; it re-sums the group that holds its row's slot and
//     substitutes on the fly the new values of ALL batch rows that fall into that group, so whatever it reads of a leaf another
//     workgroup is rewriting is replaced by the same new value, and every workgroup that touches a group stores identical bits.
//   * leaves and sums leave their kernels as write-through stores (st1_wt): no line of either table is ever dirty in two L2s.
//   * a value read from device memory never becomes an address unchecked.
#pragma once

#define PRIO_G 1024            // leaves per group = 256 threads x one float4
#define PRIO_NONE 0x7fffffff

// the words the prioritised route keeps on the device, on a line of their own (made by sactd3_prio_enable)
struct PrioCtl {
  float max_prio;     // running maximum of the unscaled priorities (starts at 1): what a freshly appended row gets
  int draw_ctr;       // counter word of the SACTD3_STREAM_PRIO draws, bumped once per native sactd3_rb_sample_prioritized
  int refused;        // rows a write-back refused (bad index, bad priority, non-finite TD error), once per row and call
  // what the graph forms below (k_*_g) read here instead of taking it by value -- a captured graph would freeze it.  Published by the
  // host on the learner stream in front of the graph launch, and only when it differs from what was last published (two adjacent words)
  float beta;         // the exponent of the importance weights
  int inject;         // != 0: the draws use the injected uniforms (pt_u) and the draw counter stands still
  int pad[27];
};
static_assert(sizeof(PrioCtl) == 128, "one line");

// The graph forms (k_prio_draw_g, k_prio_weights_g, k_prio_update_g; nstep_kernels.h: k_batch_from_index_g, k_batch_from_index_nstep_g):
// second instances of the bodies below for launches that live inside a captured graph (sactd3_step_sampled).  They take the same
// argument struct and overwrite, before the body runs, the fields that change between two replays with what device memory holds: the
// ring length and cursor from DevCtl (every append path publishes them on the learner stream), beta and the injection switch from
// PrioCtl.  For the same values they leave the same bits as the by-value forms -- it is the same code.  What they read is bounded by
// the capacity before anything is derived from it; a length of 0 selects nothing: every row is refused and counted, nothing faults.
// A body is a __device__ function that takes the struct BY VALUE (by reference the by-value kernel's instructions come out in another
// order), or, where it leaves early, a textual include (*_body.inc): either way the by-value kernels keep their machine code.
__device__ __forceinline__ int dev_ring_len(const DevCtl* ctl, int cap) { return min(max(ctl->rb_len, 0), cap); }
__device__ __forceinline__ int dev_ring_cursor(const DevCtl* ctl, int cap) { return min(max(ctl->rb_cursor, 0), max(cap - 1, 0)); }

// Running sums of the block's 1024 values (thread t owns values 4t .. 4t+3, in v): returns the sum of everything in front of the
// thread's first value, `tot` = the sum of all 1024.  Fixed order: four values sequentially per thread, a Kogge-Stone scan of the 64
// thread sums of a wave, the four wave sums sequentially.  `ws` is LDS [4]; the caller keeps a barrier between two uses.
__device__ __forceinline__ float prio_scan(const float4 v, float* ws, float& tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s = ((v.x + v.y) + v.z) + v.w;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(s, d);
    if (lane >= d) s += t;
  }
  const float before = __shfl_up(s, 1);
  if (lane == 63) ws[wave] = s;
  __syncthreads();
  const float w0 = ws[0], w1 = ws[1], w2 = ws[2], w3 = ws[3];
  tot = ((w0 + w1) + w2) + w3;
  const float woff = wave == 0 ? 0.f : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : (w0 + w1) + w2));
  return woff + (lane ? before : 0.f);
}

// Among the block's 1024 values (positions base + 4t + k, only those below `limit` count): s_first = the first position whose running
// sum exceeds m AND whose value is positive, s_last = the last position whose value is positive.  The second condition makes the
// answer independent of how the parallel running sums round: a zero value is never selected, whatever they do.  Then the thread that
// owns the chosen position (s_first, else s_last) leaves the sum in front of it and its value in s_excl / s_val.  With exact sums
// (small integers) this is the first position whose inclusive running sum exceeds m.
struct PrioFind { int first, last; float excl, val; };
__device__ __forceinline__ PrioFind prio_find(const float4 v, float front, float m, int base, int limit, int* s_first, int* s_last,
                                               float* s_excl, float* s_val) {
  // (s_first / s_last were reset by thread 0 in front of prio_scan's barrier)
  const float vv[4] = {v.x, v.y, v.z, v.w};
  float ex[4], in[4];
  ex[0] = front; in[0] = front + vv[0];
  ex[1] = front + vv[0]; in[1] = front + (vv[0] + vv[1]);
  ex[2] = in[1]; in[2] = front + ((vv[0] + vv[1]) + vv[2]);
  ex[3] = in[2]; in[3] = front + (((vv[0] + vv[1]) + vv[2]) + vv[3]);
  const int p0 = base + 4 * (int)threadIdx.x;
  int first = PRIO_NONE, last = -1;
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    const bool pos = vv[k] > 0.f && p0 + k < limit;
    if (pos && last < 0) last = p0 + k;
    if (pos && in[k] > m) first = p0 + k;
  }
  if (first != PRIO_NONE) atomicMin(s_first, first);
  if (last >= 0) atomicMax(s_last, last);
  __syncthreads();
  PrioFind f;
  f.first = *s_first; f.last = *s_last;
  const int chosen = f.first != PRIO_NONE ? f.first : f.last;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (p0 + k == chosen) { *s_excl = ex[k]; *s_val = vv[k]; }
  __syncthreads();
  f.excl = *s_excl; f.val = *s_val;
  return f;
}

// sactd3_rb_sample_prioritized, launch 1 of 3: one workgroup per batch row b.  u_b comes from the injected array or from Philox
// (stream SACTD3_STREAM_PRIO, counter words (draw_ctr, 0, 0x300, b >> 2), word b & 3, philox_u01, kept below 1).  The workgroup walks the top level twice
// with ONE loop (first for the total T, then, with m = u_b * T -- a single fp32 multiply --, for the group that holds m), then the
// 1024 leaves of that group for the slot.  Every request of a step is out before its wait; the walk has one load site.
// Out: idx_out[b] = the slot (-1: nothing to draw from, T == 0), leaf_out[b] = its leaf, total_out[0] = T.
struct PrioDrawArgs {
  const float4* leaf4; const float4* sums4; int nch /* ceil(groups / 1024) */, ngroups, len;
  const float* u_inj;                     // NULL: native draws
  const DevCtl* ctl; const PrioCtl* pc;
  long long* idx_out; float* leaf_out; float* total_out;
};
__device__ __forceinline__ void prio_draw_body(const PrioDrawArgs p) {
  __shared__ float ws[4];
  __shared__ int s_first, s_last;
  __shared__ float s_excl, s_val;
  const int tid = threadIdx.x, b = blockIdx.x;
  const unsigned long long seed = p.ctl->seed;
  const unsigned ctr = (unsigned)p.pc->draw_ctr;
  // (no injection: the load reads the counter word instead -- an address that is always valid -- and a select drops the value)
  const float* const usrc = p.u_inj ? p.u_inj + b : reinterpret_cast<const float*>(&p.pc->draw_ctr);
  const float uin = *usrc;
  const Philox4 r = philox4x32_10(ctr, 0u, SACTD3_STREAM_PRIO, (unsigned)b >> 2, (unsigned)seed, (unsigned)(seed >> 32));
  const unsigned k4 = (unsigned)b & 3u;
  const unsigned word = k4 == 0 ? r.v[0] : (k4 == 1 ? r.v[1] : (k4 == 2 ? r.v[2] : r.v[3]));
  const float u = fminf(p.u_inj ? uin : philox_u01(word), 0x1.fffffep-1f);

  float carry = 0.f, T = 0.f, m = 0.f, resid = __builtin_huge_valf();
  int g = -1, glast = -1;
  for (int it = 0; it < 2 * p.nch; ++it) {
    const int c = it < p.nch ? it : it - p.nch;
    if (it == p.nch) { T = carry; m = __fmul_rn(u, T); carry = 0.f; }
    const float4 v = p.sums4[(long)c * 256 + tid];
    if (tid == 0) { s_first = PRIO_NONE; s_last = -1; }
    float tot;
    const float front = prio_scan(v, ws, tot);
    if (it >= p.nch && g < 0) {      // (block-uniform)
      const PrioFind f = prio_find(v, carry + front, m, c * PRIO_G, p.ngroups, &s_first, &s_last, &s_excl, &s_val);
      if (f.last >= 0) glast = f.last;
      if (f.first != PRIO_NONE) { g = f.first; resid = m - f.excl; }
    } else __syncthreads();
    carry += tot;
  }
  if (g < 0) g = glast;              // m at or beyond the last running sum (rounding): the last group that holds anything
  long long slot = -1; float lv = 0.f;
  if (g >= 0) {                      // (block-uniform)
    const float4 v = p.leaf4[(long)g * 256 + tid];
    if (tid == 0) { s_first = PRIO_NONE; s_last = -1; }
    float tot;
    const float front = prio_scan(v, ws, tot);
    const PrioFind f = prio_find(v, front, resid, g * PRIO_G, p.len, &s_first, &s_last, &s_excl, &s_val);
    const int chosen = f.first != PRIO_NONE ? f.first : f.last;
    if (chosen >= 0) { slot = chosen; lv = f.val; }
  }
  if (tid == 0) {
    p.idx_out[b] = slot; p.leaf_out[b] = lv;
    if (b == 0) p.total_out[0] = T;
  }
}
__global__ __launch_bounds__(256) void k_prio_draw(PrioDrawArgs p) { prio_draw_body(p); }
// (graph form: u_inj always names pt_u; the switch decides)
struct PrioDrawArgsG { PrioDrawArgs a; int cap; };
__global__ __launch_bounds__(256) void k_prio_draw_g(PrioDrawArgsG q) {
  PrioDrawArgs p = q.a;
  p.len = dev_ring_len(p.ctl, q.cap);
  if (!p.pc->inject) p.u_inj = nullptr;
  prio_draw_body(p);
}

// ... launch 2 of 3, one workgroup: the importance weights w_b = (N leaf_b / T)^(-beta) over the batch's largest (the row that holds
// the largest gets exactly 1: x / x), N = the ring length; beta == 0: exactly 1 everywhere; a row with nothing drawn: 0.  The raw
// values are parked in w[] by the thread that reads them back.  Thread 0 then advances the draw counter (native draws only).
// Launch 3 is k_batch_from_index on idx / w.
struct PrioWeightArgs { const long long* idx; const float* leaf; const float* total; float* w; int B; float n_rows, beta; int* ctr; };
__device__ __forceinline__ void prio_weights_body(const PrioWeightArgs p) {
  __shared__ int s_max;
  const int tid = threadIdx.x;
  if (tid == 0) s_max = 0;
  __syncthreads();
  const float T = p.total[0];
  float mx = 0.f;
  for (int b = tid; b < p.B; b += 256) {
    const long long ix = p.idx[b];
    const float lv = p.leaf[b];
    float raw = 0.f;
    if (ix >= 0 && lv > 0.f && T > 0.f) raw = p.beta == 0.f ? 1.f : powf(p.n_rows * lv / T, -p.beta);
    if (!(raw < __builtin_huge_valf())) raw = 0.f;      // (overflow of the power: the row trains with weight 0 rather than poison the batch)
    p.w[b] = raw;
    mx = fmaxf(mx, raw);
  }
  atomicMax(&s_max, __float_as_int(mx));                // (non-negative floats order as their bit patterns)
  __syncthreads();
  const float top = __int_as_float(s_max);
  for (int b = tid; b < p.B; b += 256) {
    const float raw = p.w[b];
    p.w[b] = top > 0.f ? raw / top : 0.f;
  }
  if (tid == 0 && p.ctr) *p.ctr += 1;
}
__global__ __launch_bounds__(256) void k_prio_weights(PrioWeightArgs p) { prio_weights_body(p); }
struct PrioWeightArgsG { PrioWeightArgs a; const DevCtl* ctl; PrioCtl* pc; int cap; };
__global__ __launch_bounds__(256) void k_prio_weights_g(PrioWeightArgsG q) {
  PrioWeightArgs p = q.a;
  p.n_rows = (float)dev_ring_len(q.ctl, q.cap);
  p.beta = q.pc->beta;
  p.ctr = q.pc->inject ? nullptr : &q.pc->draw_ctr;
  prio_weights_body(p);
}

// Rows the ring has just written (or, at sactd3_prio_enable, the rows it holds) enter at the current maximum priority: one workgroup
// per group that holds a slot of [lo0, hi0) or [lo1, hi1) (the second range: what an append wrote behind the wrap).  The workgroup sets
// the leaves of both ranges inside its group to max_prio^alpha and re-sums the group.  Two workgroups of one launch meet the same
// group only where both ranges reach into it; both then substitute both ranges and store identical bits.
struct PrioRefreshArgs {
  float* leaf; float* sums; const PrioCtl* pc; float alpha;
  int g0, n0, g1;                         // blocks [0, n0) -> groups g0 .., the others -> groups g1 ..
  int lo0, hi0, lo1, hi1;
};
__global__ __launch_bounds__(256) void k_prio_refresh(PrioRefreshArgs p) {
  __shared__ float ws[4];
  const int tid = threadIdx.x, x = blockIdx.x;
  const int g = x < p.n0 ? p.g0 + x : p.g1 + (x - p.n0);
  float4 v = reinterpret_cast<const float4*>(p.leaf)[(long)g * 256 + tid];
  const float mp = p.pc->max_prio;
  const float val = p.alpha == 1.f ? mp : powf(mp, p.alpha);
  const int p0 = g * PRIO_G + 4 * tid;
  float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = p0 + k;
    if ((s >= p.lo0 && s < p.hi0) || (s >= p.lo1 && s < p.hi1)) { vv[k] = val; st1_wt(p.leaf + s, val); }
  }
  float tot;
  prio_scan(make_float4(vv[0], vv[1], vv[2], vv[3]), ws, tot);
  if (tid == 0) st1_wt(p.sums + g, tot);
}

// The write-back (sactd3_prio_update_from_td: q != NULL, rows and TD errors of batch slot 0; sactd3_prio_update_device: the caller's
// idx / prio arrays), one workgroup per row b of the n.  Row j is accepted when its slot is inside [0, len) and its unscaled priority
// p_j is finite (TD form: p_j = max_k |q_k - y| + eps, both TD errors finite; caller form: p_j as given, >= 0); its new leaf is p_j^alpha
// (alpha == 1: p_j itself, no pow; p_j == 0: 0).  A refused row is counted by its own workgroup and touches nothing.
// The workgroup of an accepted row loads the 1024 leaves of its group, walks ALL n rows and substitutes the new leaf of every accepted
// row of the group -- where a slot occurs several times the highest batch position wins: an LDS 64-bit max over (position + 1, bits
// of the leaf) --, re-sums the group and stores the sum; the winner's workgroup stores the leaf.  max_prio takes the p of every
// accepted row (an integer max on the bits of non-negative floats, at the memory side: order cannot matter).
struct PrioUpdateArgs {
  float* leaf; float* sums; int n, len; float alpha, eps;
  const int* slot_idx; const float* q; const float* y; int B;             // TD form
  const long long* idx; long idx_ld; const float* prio; long prio_ld;     // caller form
  PrioCtl* pc;
};
__device__ __forceinline__ bool prio_row(const PrioUpdateArgs& p, int j, int& slot, float& pr) {
  bool ok;
  if (p.q) {
    const int s = p.slot_idx[j];
    const float q0 = p.q[j], q1 = p.q[p.B + j], yv = p.y[j];
    const float a0 = fabsf(q0 - yv), a1 = fabsf(q1 - yv);
    ok = s >= 0 && s < p.len && a0 < __builtin_huge_valf() && a1 < __builtin_huge_valf();      // (false for NaN)
    slot = ok ? s : 0;
    pr = fmaxf(a0, a1) + p.eps;
  } else {
    const long long raw = p.idx[(long)j * p.idx_ld];
    pr = p.prio[(long)j * p.prio_ld];
    ok = raw >= 0 && raw < (long long)p.len && pr >= 0.f && pr < __builtin_huge_valf();
    slot = ok ? (int)raw : 0;
  }
  return ok && pr < __builtin_huge_valf();
}
__device__ __forceinline__ float prio_leaf_value(float pr, float alpha) {
  return pr == 0.f ? 0.f : (alpha == 1.f ? pr : powf(pr, alpha));
}
// (the body lives in prio_update_body.inc, shared with the graph form below)
__global__ __launch_bounds__(256) void k_prio_update(PrioUpdateArgs p) {
#include "prio_update_body.inc"
}
struct PrioUpdateArgsG { PrioUpdateArgs a; const DevCtl* ctl; int cap; };
__global__ __launch_bounds__(256) void k_prio_update_g(PrioUpdateArgsG q) {
  PrioUpdateArgs p = q.a;
  p.len = dev_ring_len(q.ctl, q.cap);
#include "prio_update_body.inc"
}
