// What engine.hip knows of the returns-to-go call (returns.hip, returns_kernels.h; include/sactd3_returns.h is its C ABI): the argument
// struct, the sizes of its scratch and one host launcher.  Nothing else crosses between the translation units.
#pragma once
#include <hip/hip_runtime.h>

#define RTG_SPAN 2048        // positions of one k_rtg_scan workgroup (engine.hip asserts it against the C ABI's)
#define RTG_PER (RTG_SPAN / 256)      // consecutive positions one thread folds
// bits of a position's `ends` word (the C ABI's SACTD3_RTG_*; 0 while a chain is still open at the end of what was scanned)
enum { RTG_TERMINATED = 1, RTG_TRUNCATED = 2, RTG_OPEN = 4, RTG_START = 8 };
// device counters of the feature, 64-bit each (k_rtg_scan)
enum { RTG_W_TERMINATED = 0, RTG_W_TRUNCATED, RTG_W_OPEN, RTG_W_START, RTG_W_BADR, RTG_WORDS = 8 };

// spans a range of n rows is cut into, and the floats / ints of scratch a ring of `cap` slots needs (three arrays of each type per
// position, three of each per span)
static inline long rtg_spans(long n) { return (n + RTG_SPAN - 1) / RTG_SPAN; }
static inline size_t rtg_scratch(long cap) { return 3 * ((size_t)cap + (size_t)rtg_spans(cap)); }

struct RtgArgs {
  const float4* ring; int rec4, cx, cn, o;  // the ring, a record's float4 chunks, those of [s | a] and of s', ob_dim
  int n, base, cap, stride;                 // rows of the range; slot(age) = (base + age) mod cap; the chain stride
  int q, rem;                               // n / stride, n % stride: chains c < rem own q + 1 positions, the others q
  float gamma;
  // the feature's own memory: per position p the local result M, B, U | kind (with RTG_START), L, last, then per span the carry
  float* sf; int* si;                       // [3][cap] each, followed by [3][rtg_spans(cap)]
  unsigned long long* words;                // [RTG_WORDS]
  // the caller's arrays, indexed by ring slot (NULL: not wanted)
  float* returns; long returns_ld;
  float* undiscounted; long undiscounted_ld;
  int* length; long length_ld;
  int* last; long last_ld;
  int* ends; long ends_ld;
};

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launches: k_rtg_scan, the single-workgroup k_rtg_carry, k_rtg_apply.  rb_len: the ring rows that hold records.
hipError_t returns_launch(const RtgArgs& args, long rb_len, hipStream_t stream);
