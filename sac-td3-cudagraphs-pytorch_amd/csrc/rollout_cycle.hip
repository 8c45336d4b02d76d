// Device code of sactd3_rollout_cycle (include/sactd3_rollout_cycle.h) that did not exist before it: the graph form of the ring append,
// and its launchers, which engine.hip calls (rollout_cycle.h).  A translation unit of its own inside libsactd3_hip.so, as env.hip and
// hindsight.hip are: engine.hip gains no kernel.
#include <hip/hip_runtime.h>

#include "rollout_cycle.h"

// {len, cursor} as the launch found them, bounded before anything is derived from them; `bad`: one of the two was outside its range.
// The two adjacent words are ONE 8-byte load from device memory (the launcher checks the alignment), made once: a volatile load is
// neither split into two dependent round trips nor repeated behind the barrier of the publishing form.
struct RingWords { int len, cursor; bool bad; };
typedef const volatile __attribute__((address_space(1))) unsigned long long* gwords_p;
__device__ __forceinline__ RingWords ring_words_ld(const int* words, int cap) {
  const unsigned long long both = *(gwords_p)(uintptr_t)words;
  const int len = (int)(unsigned)both, cursor = (int)(unsigned)(both >> 32);
  RingWords w;
  w.len = min(max(len, 0), cap);
  w.cursor = min(max(cursor, 0), cap - 1);
  w.bad = w.len != len || w.cursor != cursor;
  return w;
}
__device__ __forceinline__ void ring_words_publish(const IngestArgsG& p, const RingWords& w) {
  int cursor = w.cursor + p.n;      // (< 2 cap: n <= cap)
  if (cursor >= p.cap) cursor -= p.cap;
  p.ring_words[0] = min(p.cap, w.len + p.n);
  p.ring_words[1] = cursor;
  if (w.bad) atomicAdd(p.clamped, 1);
}

// One thread per float4 chunk (16-byte load, 16-byte store), grid-stride beyond the grid; every thread reads the words before its
// first store, and no thread of a multi-block launch writes them (rollout_cycle.h: read, then publish).
__global__ __launch_bounds__(INGEST_G_BLOCK) void k_rb_ingest_g(IngestArgsG p) {
  const RingWords w = ring_words_ld(p.ring_words, p.cap);
  const int total = p.n * p.rec4;
  for (int g = blockIdx.x * INGEST_G_BLOCK + threadIdx.x; g < total; g += gridDim.x * INGEST_G_BLOCK) {
    const int row = g / p.rec4, c = g - row * p.rec4;
    int dst = w.cursor + row;      // (< 2 cap)
    if (dst >= p.cap) dst -= p.cap;
    p.ring[(long)dst * p.rec4 + c] = p.src[g];
  }
  if (p.publish) {      // uniform: the launch is one block, and all of its threads have read the words when the barrier opens
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x == 0) ring_words_publish(p, w);
  }
}
// behind a multi-block k_rb_ingest_g: the words are still what its blocks read
__global__ void k_rb_publish_g(IngestArgsG p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ring_words_publish(p, ring_words_ld(p.ring_words, p.cap));
}

static bool ingest_g_args_ok(const IngestArgsG& p) {
  return p.src && p.ring && p.ring_words && p.clamped && p.rec4 >= 1 && p.cap >= 1 && p.n >= 1 && p.n <= p.cap &&
         (long long)p.n * p.rec4 < (1ll << 31) && (uintptr_t)p.src % 16 == 0 && (uintptr_t)p.ring % 16 == 0 &&
         (uintptr_t)p.ring_words % 8 == 0;
}
hipError_t rb_ingest_g_launch(const IngestArgsG& p, unsigned blocks, hipStream_t stream) {
  if (!ingest_g_args_ok(p) || blocks < 1 || (p.publish && blocks != 1) || (p.publish != 0 && p.publish != 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rb_ingest_g, dim3(blocks), dim3(INGEST_G_BLOCK), 0, stream, p);
  return hipGetLastError();
}
hipError_t rb_publish_g_launch(const IngestArgsG& p, hipStream_t stream) {
  if (!ingest_g_args_ok(p) || p.publish) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rb_publish_g, dim3(1), dim3(1), 0, stream, p);
  return hipGetLastError();
}
