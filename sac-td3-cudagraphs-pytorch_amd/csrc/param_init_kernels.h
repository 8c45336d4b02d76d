// Device code of the parameter initialiser (include/sactd3_init.h), a translation unit of its own inside libsactd3_hip.so
// (param_init.hip): it shares philox.h with engine.hip and nothing else.
//
// k_init_orth: torch.nn.init.orthogonal_ at gain 1 (agents/nets.py:35-47), one workgroup of 256 threads per weight matrix, every
//   matrix of a call in one launch.
//   draw    : weight [rows, cols] -> G [m, n], m = max(rows, cols), n = min(rows, cols), row-major in the scratch buffer.  Element
//             e = i n + j of matrix `id` in reset epoch E is lane e & 3 of philox_box_muller4 over the Philox block with counter words
//                 (E, id | attempt << 16, 0x700, e >> 2)
//             keyed by the seed; attempt = 0, see `redraw`.  A pure function of (seed, id, i, j, E): not of the launch, not of which
//             other matrices it holds.
//   columns : classical Gram-Schmidt applied twice, column by column, in fp32 with one summation order: the coefficient of column
//             i < j is thread i's sum over the rows in ascending order; a row's correction is its thread's sum over the columns in
//             ascending order; the squared norm is each thread's sum over its rows (t, t + 256, ...) and then a pairwise tree over the
//             256 partial sums.  The diagonal of R is the norm a column is divided by: positive by construction.
//   redraw  : a column whose squared norm behind the two projections is zero or not finite never divides: it is drawn again with
//             attempt + 1 in the second counter word, projected again, and counted in *redrawn; behind PI_MAX_REDRAW attempts it is
//             left zero (and counted once more).
//   out     : W = Q for rows >= cols, else Q^T; the pad columns [cols, ld) get 0.
// k_init_fanout: behind it, per family of nets: biases 0, LayerNorm weights 1, LayerNorm biases 0 (schema._init_net); the targets -- the
//   run-ahead ones too -- a bit copy of the online nets; Adam's m and v 0; one thread: the step words 0, the beta-power words {1, 1},
//   the temperature's {log alpha_init, 0, 0}.  16-byte vector stores from plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include "param_init.h"
#include "philox.h"

#define SACTD3_STREAM_INIT 0x700u   // third counter word of the initialiser's draws (free beside 0x000 + site, 0x100 .. 0x600)
#define PI_HID 256

// element e of matrix `id`'s G at `attempt`: see the header of this file
__device__ __forceinline__ float4 init_normal4(unsigned long long seed, unsigned epoch, unsigned id, unsigned attempt, unsigned q) {
  return philox_box_muller4(philox4x32_10(epoch, id | (attempt << 16), SACTD3_STREAM_INIT, q, (uint32_t)seed, (uint32_t)(seed >> 32)));
}
__device__ __forceinline__ float init_normal(unsigned long long seed, unsigned epoch, unsigned id, unsigned attempt, unsigned e) {
  const float4 z = init_normal4(seed, epoch, id, attempt, e >> 2);
  const unsigned k = e & 3u;      // (selects: a dynamically indexed array would live in scratch memory)
  return k == 0 ? z.x : (k == 1 ? z.y : (k == 2 ? z.z : z.w));
}

__global__ __launch_bounds__(256) void k_init_orth(InitOrthArgs p) {
#pragma clang fp contract(off)
  __shared__ float v[PI_MAX_TALL];
  __shared__ float c[PI_MAX_SHORT];
  __shared__ float red[256];
  const int t = threadIdx.x;
  InitMat M = p.m[0];
#pragma unroll
  for (int i = 1; i < PI_MAX_MATS; ++i) if ((int)blockIdx.x == i) M = p.m[i];      // (a constant index each: the argument stays in SGPRs)
  if ((int)blockIdx.x >= p.n) return;
  const int m = max(M.rows, M.cols), n = min(M.rows, M.cols);
  if (m > PI_MAX_TALL || n > PI_MAX_SHORT || n < 1) return;      // (the launcher refused these)
  float* G = p.scratch + M.scratch_off;
  const unsigned total = (unsigned)m * (unsigned)n;
  for (unsigned q = t; 4u * q < total; q += 256u) {
    const float4 z = init_normal4(p.seed, p.epoch, (unsigned)M.id, 0u, q);
    float* d = G + 4ul * q;
    d[0] = z.x;
    if (4u * q + 1u < total) d[1] = z.y;
    if (4u * q + 2u < total) d[2] = z.z;
    if (4u * q + 3u < total) d[3] = z.w;
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    unsigned attempt = 0;
    for (;;) {
      for (int r = t; r < m; r += 256)
        v[r] = attempt == 0 ? G[(long)r * n + j] : init_normal(p.seed, p.epoch, (unsigned)M.id, attempt, (unsigned)r * (unsigned)n + (unsigned)j);
      for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        if (t < j) {
          float s = 0.f;
#pragma unroll 8      // (eight loads in flight per thread; the sum keeps its order)
          for (int r = 0; r < m; ++r) s = fmaf(G[(long)r * n + t], v[r], s);
          c[t] = s;
        }
        __syncthreads();
        for (int r = t; r < m; r += 256) {
          const float* row = G + (long)r * n;
          float s = 0.f;
#pragma unroll 8
          for (int i = 0; i < j; ++i) s = fmaf(c[i], row[i], s);
          v[r] -= s;
        }
      }
      float s = 0.f;
      for (int r = t; r < m; r += 256) s = fmaf(v[r], v[r], s);      // (a thread reads the rows it wrote: no barrier in between)
      red[t] = s;
      __syncthreads();
      for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
      }
      const float nrm2 = red[0];
      __syncthreads();                                               // (red[] is written again by the next column)
      if (nrm2 > 0.f && nrm2 < __builtin_inff()) {      // (false for a NaN too)
        const float nrm = sqrtf(nrm2);
        for (int r = t; r < m; r += 256) G[(long)r * n + j] = v[r] / nrm;
        break;
      }
      if (t == 0) atomicAdd(p.redrawn, 1);
      if (attempt == PI_MAX_REDRAW) {
        for (int r = t; r < m; r += 256) G[(long)r * n + j] = 0.f;
        break;
      }
      ++attempt;
    }
    __syncthreads();      // column j, written to global memory by this workgroup, is read by all of it from here on
  }
  const bool tall = M.rows >= M.cols;
  const int cells = M.rows * M.ld;
  for (int x = t; x < cells; x += 256) {
    const int r = x / M.ld, cc = x - r * M.ld;
    M.dst[x] = cc < M.cols ? (tall ? G[(long)r * n + cc] : G[(long)cc * n + r]) : 0.f;
  }
}

__device__ __forceinline__ void init_fan_family(const InitFanFam& f) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const long chunks = (long)f.nets * (f.size / 4);
  for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < chunks; x += (long)gridDim.x * 256) {
    const int off = (int)((4 * x) % f.size);
    const bool weight = off < f.b1 || (off >= f.W2 && off < f.b2) || (off >= f.Wh && off < f.bh);
    const bool gamma = (off >= f.g1 && off < f.g1 + PI_HID) || (off >= f.g2 && off < f.g2 + PI_HID);
    float4* P = (float4*)f.P + x;
    const float4 cur = *P;      // (always loaded, then selected per lane: a select between the addresses would put the constants in scratch memory)
    const float fill = gamma ? 1.f : 0.f;
    const float4 w = make_float4(weight ? cur.x : fill, weight ? cur.y : fill, weight ? cur.z : fill, weight ? cur.w : fill);
    if (!weight) *P = w;
    ((float4*)f.T)[x] = w;
    if (f.T2) ((float4*)f.T2)[x] = w;
    if (f.T3) ((float4*)f.T3)[x] = w;
    ((float4*)f.M)[x] = zero;
    ((float4*)f.V)[x] = zero;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *f.t = 0; f.pw[0] = 1.0; f.pw[1] = 1.0; }
}
__global__ __launch_bounds__(256) void k_init_fanout(InitFanArgs p) {
  if (p.nf > 0) init_fan_family(p.f[0]);      // (a constant index each: a dynamically indexed argument would be copied to scratch memory)
  if (p.nf > 1) init_fan_family(p.f[1]);
  if (p.la && blockIdx.x == 0 && threadIdx.x == 0) {
    p.la[0] = p.la0; p.la[1] = 0.f; p.la[2] = 0.f;
    *p.t_l = 0; p.pw_l[0] = 1.0; p.pw_l[1] = 1.0;
  }
}
