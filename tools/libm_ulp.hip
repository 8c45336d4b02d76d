// Evaluates the three single-precision library functions of the squashed-Gaussian chain (tanhf, expf, logf; csrc/kernels.h:
// actor_tail_body, the head backward) on the device over dense sweeps of the ranges the chain reaches, and writes arguments and
// results as raw float32 to a file: tools/libm_ulp.py compares them with numpy float64 and records the worst ULP error per
// function in profiles/libm_ulp.json, the source of tests/bounds.py's LIBM_ULP.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/libm_ulp.hip -o tools/libm_ulp       (the engine Makefile's flags: no fast-math)
//   tools/libm_ulp <out.bin>
// File: int32 count n, then per function (tanh, exp, log) n arguments and n results.
//
// Behind them, the pieces of the engine's normal draws, EXHAUSTIVELY: philox_u01 (csrc/philox.h, included here) has only 2^24
// possible arguments x >> 8, so every piece is evaluated at u = philox_u01(i << 8), i = 0 .. 2^24 - 1.  The three arithmetic lines
// of philox_normal4 (csrc/kernels.h) are RESTATED here, not included -- kernels.h is the whole engine:
//     rad = sqrtf(-2.0f * 0.6931471805599453f * __builtin_amdgcn_logf(u))      (v_log_f32: log2)
//     __builtin_amdgcn_sinf(u), __builtin_amdgcn_cosf(u)                       (v_sin_f32 / v_cos_f32: argument in revolutions)
// and so are those of k_rb_fill, which uses the library instead:  t = 6.283185307179586f * u, sinf(t), cosf(t), logf(u),
// sqrtf(-2.f * logf(u)).
// File, continued: int32 count m = 2^24, then m results each of NOISE_FNS functions in the order of enum NoiseFn; for FN_T the
// result is t itself (the float64 reference is taken at that same fp32 t).  The arguments are not written: tools/libm_ulp.py
// recomputes philox_u01 in numpy float32, and FN_U carries the device's own u to check that against.
#include <hip/hip_runtime.h>

#include "../sac-td3-cudagraphs-pytorch_amd/csrc/philox.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t err_ = (x);                                                                         \
    if (err_ != hipSuccess) {                                                                      \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(err_));                                    \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

__global__ __launch_bounds__(256) void k_eval(const float* x, float* y, int n, int fn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  y[i] = fn == 0 ? tanhf(v) : (fn == 1 ? expf(v) : logf(v));
}

enum NoiseFn { FN_U = 0, FN_RAD, FN_SINREV, FN_COSREV, FN_T, FN_SINF, FN_COSF, FN_LOGF, FN_RAD_LIBM, NOISE_FNS };

__global__ __launch_bounds__(256) void k_noise(float* y, int m, int fn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float u = philox_u01((uint32_t)i << 8);
  const float t = 6.283185307179586f * u;
  float r;
  switch (fn) {
    case FN_U: r = u; break;
    case FN_RAD: r = sqrtf(-2.0f * 0.6931471805599453f * __builtin_amdgcn_logf(u)); break;
    case FN_SINREV: r = __builtin_amdgcn_sinf(u); break;
    case FN_COSREV: r = __builtin_amdgcn_cosf(u); break;
    case FN_T: r = t; break;
    case FN_SINF: r = sinf(t); break;
    case FN_COSF: r = cosf(t); break;
    case FN_LOGF: r = logf(u); break;
    default: r = sqrtf(-2.f * logf(u)); break;
  }
  y[i] = r;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <out.bin>\n", argv[0]);
    return 2;
  }
  const int n = 1 << 22;
  // tanh: +-16 linearly (2^22 points: 7.6e-6 apart), with the last quarter of the points spent on +-[7, 10.5], every 4th float or
  // denser, where the result first rounds to +-1;  exp: [-5, 2] linearly;  log: [1e-6, 8] geometrically (equal density per octave; logf(std) reaches e^2, the tanh correction 1e-6)
  std::vector<float> x(3 * (size_t)n), y(3 * (size_t)n);
  const int nlin = 3 * (n / 4), nsat = n - nlin;
  for (int i = 0; i < nlin; ++i) x[i] = (float)(-16.0 + 32.0 * (double)i / (nlin - 1));
  for (int i = 0; i < nsat; ++i) {
    const double m = 7.0 + 3.5 * (double)(i / 2) / (nsat / 2 - 1);
    x[nlin + i] = (float)((i & 1) ? -m : m);
  }
  for (int i = 0; i < n; ++i) x[n + i] = (float)(-5.0 + 7.0 * (double)i / (n - 1));
  const double l0 = std::log(1e-6), l1 = std::log(8.0);
  for (int i = 0; i < n; ++i) x[2 * (size_t)n + i] = (float)std::exp(l0 + (l1 - l0) * (double)i / (n - 1));
  float *dx = nullptr, *dy = nullptr;
  CHECK(hipMalloc(&dx, sizeof(float) * n));
  CHECK(hipMalloc(&dy, sizeof(float) * n));
  for (int fn = 0; fn < 3; ++fn) {
    CHECK(hipMemcpy(dx, x.data() + (size_t)fn * n, sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, fn);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(y.data() + (size_t)fn * n, dy, sizeof(float) * n, hipMemcpyDeviceToHost));
  }
  CHECK(hipFree(dx));
  CHECK(hipFree(dy));
  const int m = 1 << 24;
  std::vector<float> z((size_t)NOISE_FNS * m);
  float* dz = nullptr;
  CHECK(hipMalloc(&dz, sizeof(float) * m));
  for (int fn = 0; fn < NOISE_FNS; ++fn) {
    hipLaunchKernelGGL(k_noise, dim3((m + 255) / 256), dim3(256), 0, 0, dz, m, fn);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(z.data() + (size_t)fn * m, dz, sizeof(float) * m, hipMemcpyDeviceToHost));
  }
  CHECK(hipFree(dz));
  FILE* f = fopen(argv[1], "wb");
  if (!f) {
    perror(argv[1]);
    return 1;
  }
  bool ok = fwrite(&n, sizeof(int), 1, f) == 1;
  for (int fn = 0; fn < 3 && ok; ++fn)
    ok = fwrite(x.data() + (size_t)fn * n, sizeof(float), n, f) == (size_t)n && fwrite(y.data() + (size_t)fn * n, sizeof(float), n, f) == (size_t)n;
  ok = ok && fwrite(&m, sizeof(int), 1, f) == 1 && fwrite(z.data(), sizeof(float), z.size(), f) == z.size();
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    fprintf(stderr, "short write to %s\n", argv[1]);
    return 1;
  }
  printf("wrote %d points per library function and %d per noise piece to %s\n", n, m, argv[1]);
  return 0;
}
