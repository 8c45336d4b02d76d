// The coloured-noise generator's translation unit: k_colored_noise<N> (noise_kernels.h), the host tables and the launcher engine.hip and
// env.hip call (noise.h).  A translation unit of its own inside libsactd3_hip.so, as dormant.hip and param_init.hip are: engine.hip gains
// no kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "noise_kernels.h"

const char* noise_refusal(float beta, int length) {
  if (!(beta >= 0.f && beta <= 2.f)) return "beta must be in [0, 2]";
  if (length < (1 << NZ_MIN_LOG) || length > (1 << NZ_MAX_LOG) || (length & (length - 1))) return "length must be a power of two in [64, 4096]";
  return nullptr;
}

// float64 throughout, rounded once: the device calls no powf, sinf or cosf
void noise_tables(float beta, int L, float* host) {
  const int H = L / 2;
  std::vector<double> v((size_t)H + 1);
  const double ex = -0.5 * (double)beta;
  for (int k = 1; k <= H; ++k) v[k] = 2.0 * std::pow((double)k, ex);
  v[0] = std::sqrt(2.0);                          // sqrt(2) w_1: the DC bin takes the weight of the lowest frequency
  v[H] = std::sqrt(2.0) * std::pow((double)H, ex);
  double ss = 0.0;
  for (int k = 0; k <= H; ++k) ss += v[k] * v[k];
  const double norm = std::sqrt(ss);
  for (size_t k = 0; k < noise_amp_floats(L); ++k) host[k] = k <= (size_t)H ? (float)(v[k] / norm) : 0.f;
  float* tw = host + noise_amp_floats(L);
  const double step = 2.0 * 3.14159265358979323846 / (double)L;
  for (int j = 0; j < H; ++j) { tw[2 * j] = (float)std::cos(step * j); tw[2 * j + 1] = (float)std::sin(step * j); }
}

template <int N>
static hipError_t launch_n(const NoiseArgs& p, hipStream_t stream) {
  hipLaunchKernelGGL(k_colored_noise<N>, dim3((unsigned)((p.sequences + 1) / 2)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t noise_launch(const NoiseArgs& p, hipStream_t stream) {
  // what the kernel's address arithmetic relies on; the engine's checks (sactd3_colored_noise_device) come first, these stand between
  // any caller and the launch
  if (!p.amp || !p.tw || ((uintptr_t)p.tw & 7u) || !p.seed || !p.out) return hipErrorInvalidValue;
  if (p.sequences < 1 || p.ld < (long long)p.sequences || p.epoch >= NZ_MAX_EPOCH) return hipErrorInvalidValue;
  switch (p.log_len) {
    case 6: return launch_n<6>(p, stream);
    case 7: return launch_n<7>(p, stream);
    case 8: return launch_n<8>(p, stream);
    case 9: return launch_n<9>(p, stream);
    case 10: return launch_n<10>(p, stream);
    case 11: return launch_n<11>(p, stream);
    case 12: return launch_n<12>(p, stream);
    default: return hipErrorInvalidValue;
  }
}
