// N-step returns staged from the ring (include/sactd3.h: sactd3_rb_sample_nstep*): device code.
// Included by engine.hip behind prio_kernels.h (the graph form reads the ring's state through its helpers).
//
// k_batch_from_index_nstep is k_batch_from_index with a chain walk in front of the copy.  Per batch row with start slot i0:
//   age(i)  = i while len < cap, else (i - cursor) mod cap            (rows the slot is behind the oldest one)
//   slot_j  = (i0 + j * stride) mod cap, which EXISTS iff age(i0) + j * stride < len
//   link j -> j+1 holds iff slot_{j+1} exists, the flag float of slot_j is 0, and the first o floats of slot_j's s' field equal, as
//            32-bit patterns, the first o floats of slot_{j+1}'s record (-0.0 != +0.0, equal NaN patterns are equal)
//   k       = 1 + the number of leading links that hold, 1 <= k <= steps
//   R_0 = r_0, G_0 = 1, G_j = G_{j-1} * gamma, R_j = R_{j-1} + G_j * r_j     (each one correctly rounded fp32 operation, no fma: nstep_return)
// and the slot receives X = [s|a] of slot_0, Xn = s' of slot_{k-1}, rew = R_{k-1}, done = 1 - (1 - d_{k-1}) * G_{k-1} (d_0 itself for
// k = 1), so that every critic tail's `rw + (1 - dn) * gamma * q'` is the k-step target.  With steps == 1 the slot holds what
// k_batch_from_index leaves, bit for bit.
//
// Rules the kernel keeps:
//   * all candidate slots of a row are arithmetic in i0: every load of the link phase is issued before anything depends on one.
//   * a start index outside [0, len), and a candidate slot that does not exist, never become an address: the load goes to the row's
//     slot_0 (ring slot 0 for a refused row) and the link counts as broken.
//   * loads first, stores last in each phase; plain vector stores and LDS atomics only (the two counters take one global atomicAdd
//     per counted row, as k_batch_from_index's does).
#pragma once

#define NS_MAX 16       // steps <= NS_MAX
#define NS_ROWS 136     // rows a block's span may touch: the host sizes the span so (launch_batch_nstep)
#define NS_U 4          // link-phase items per thread and round: 2 * NS_U 16-byte loads in flight

struct NstepArgs {
  const float4* ring; int rec4, cx, cn, o; int B, len, cursor, cap;
  int steps, stride; float gamma;
  const long long* idx; long idx_ld;      // start slot of row r: idx[r * idx_ld]; NULL: the uniform draw of sactd3_rb_sample
  const float* w; long w_ld;              // weight of row r: w[r * w_ld] (NULL: 1)
  const DevCtl* ctl;                      // seed and sample counter of the uniform draw
  float4* X; float4* Xn; float* rew; float* done; int* slot_idx; float* wdst /* NULL: the slot carries no weights */;
  int* nk; int* nlast;                    // per batch row: chain length k (0: refused), ring slot of the chain's last row (-1)
  unsigned rec4_magic;                    // as GatherArgs
  int cpb;                                // chunks per thread, <= GATHER_CPT, and (cpb * 256) / rec4 + 2 <= NS_ROWS
  int* counters;                          // [0] rows cut short (k < steps), [1] rows refused
};

// slot_j of a row whose slot_0 is s0, for a j that exists (then j * stride < cap: one conditional subtraction is the modulo)
__device__ __forceinline__ int nstep_slot(int s0, int j, int stride, int cap) {
  const long long t = (long long)s0 + (long long)j * (long long)stride;
  return (int)(t >= (long long)cap ? t - (long long)cap : t);
}
__device__ __forceinline__ bool nstep_differs(const float4& a, const float4& b, int c, int o) {
  bool d = false;
  d |= 4 * c + 0 < o && __float_as_uint(a.x) != __float_as_uint(b.x);
  d |= 4 * c + 1 < o && __float_as_uint(a.y) != __float_as_uint(b.y);
  d |= 4 * c + 2 < o && __float_as_uint(a.z) != __float_as_uint(b.z);
  d |= 4 * c + 3 < o && __float_as_uint(a.w) != __float_as_uint(b.w);
  return d;
}

// R_{k-1} and the mask of a chain of k >= 1 rows with rewards r[0 .. k-1] and last flag dl, in the documented order.  Contraction is off
// for this block: every product and sum is one correctly rounded fp32 operation (the __f*_rn intrinsics alone are plain operators
// to the compiler, which would fuse them into fmas).
__device__ __forceinline__ void nstep_return(const float* r, float dl, int k, float gamma, float& R, float& m) {
#pragma clang fp contract(off)
  float G = 1.f, acc = r[0];
  for (int j = 1; j < k; ++j) {
    G = G * gamma;
    const float t = G * r[j];
    acc = acc + t;
  }
  const float keep = 1.f - dl, scaled = keep * G;
  R = acc;
  m = k == 1 ? dl : 1.f - scaled;
}

// (the body lives in nstep_body.inc, shared with the graph form below)
__global__ __launch_bounds__(256) void k_batch_from_index_nstep(NstepArgs p) {
#include "nstep_body.inc"
}
// The graph forms of the two staging kernels (prio_kernels.h: the graph forms): ring length and cursor as the device holds them.
__global__ __launch_bounds__(256) void k_batch_from_index_nstep_g(NstepArgs q) {
  NstepArgs p = q;
  p.len = dev_ring_len(p.ctl, p.cap);
  p.cursor = dev_ring_cursor(p.ctl, p.cap);
#include "nstep_body.inc"
}
struct IndexBatchArgsG { IndexBatchArgs a; const DevCtl* ctl; int cap; };
__global__ __launch_bounds__(256) void k_batch_from_index_g(IndexBatchArgsG q) {
  IndexBatchArgs p = q.a;
  p.len = dev_ring_len(q.ctl, q.cap);
#include "batch_from_index_body.inc"
}

// sactd3_nstep_info_device: the two per-row words of an n-step slot into the caller's int32 arrays (either may be NULL), one thread
// per row; nothing else is read, nothing else written.
struct NstepInfoArgs { const int* nk; const int* nlast; int B; int* k; long k_ld; int* last; long last_ld; };
__global__ __launch_bounds__(256) void k_nstep_info(NstepInfoArgs p) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.B) return;
  const int kv = p.nk[b], lv = p.nlast[b];
  if (p.k) p.k[(long)b * p.k_ld] = kv;
  if (p.last) p.last[(long)b * p.last_ld] = lv;
}
