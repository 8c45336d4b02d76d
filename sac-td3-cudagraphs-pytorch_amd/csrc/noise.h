// What engine.hip and env.hip know of the coloured-noise generator (noise.hip, noise_kernels.h; include/sactd3_noise.h is its C ABI): the
// argument struct, the host tables and one launcher.  Nothing else crosses between the translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NZ_MIN_LOG 6       // chunk lengths 2^6 .. 2^12
#define NZ_MAX_LOG 12
#define NZ_MAX_EPOCH 65536u      // the epoch shares the fourth counter word with the block index (<= 1024): epoch << 16

// One (beta, L) pair's device tables, as the host made them in float64 and rounded once (noise_tables).
//   amp [L / 2 + 1]  a_k of include/sactd3_noise.h
//   tw  [L / 2]      (cos, sin)(2 pi j / L): every twiddle of every pass is one of them
static inline size_t noise_amp_floats(int L) { return (size_t)((L / 2 + 1 + 3) & ~3); }      // (tw behind it stays 16-byte aligned)
static inline size_t noise_table_floats(int L) { return noise_amp_floats(L) + (size_t)L; }

struct NoiseArgs {
  const float* amp; const float2* tw;
  const unsigned long long* seed;      // the engine's seed, a device word: the Philox key
  unsigned chunk, epoch;
  int log_len, sequences;
  float* out; long long ld;            // element (t, q) at out[t ld + q]
};

// NULL where (beta, length) is a process of include/sactd3_noise.h, else the refusal's text
const char* noise_refusal(float beta, int length);
// the tables of (beta, L) into host[noise_table_floats(L)]: amp, then tw
void noise_tables(float beta, int L, float* host);
// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernel's address arithmetic holds; otherwise
// hipGetLastError() behind the launch of k_colored_noise: ceil(sequences / 2) workgroups of 256 threads.
hipError_t noise_launch(const NoiseArgs& args, hipStream_t stream);
