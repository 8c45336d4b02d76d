// Worst absolute error of the device library's sinf and cosf over [-X, X], X just above pi, EXHAUSTIVELY: every float32 bit pattern
// 0 .. bits(X) with either sign (2.1e9 arguments).  The env kernels (csrc/env_kernels.h) call sinf / cosf on angles they keep in
// [-pi, pi]; tests/env_model.py propagates this figure through a step.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/libm_trig.hip -o tools/libm_trig       (the engine Makefile's flags: no fast-math)
//   tools/libm_trig <out.bin>
// The arguments are too many to take to the host, so each block keeps its worst |sinf(x) - sin((double)x)| and |cosf(x) - cos((double)x)|
// against the device's DOUBLE sin / cos and writes the argument and the float result it occurred at; tools/libm_trig.py recomputes the
// error of those candidates with numpy float64 and records that.
// File: int32 blocks, uint32 bits(X), then per function (sin, cos) `blocks` records of {float x, float got, double err}.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t err_ = (x);                                                                         \
    if (err_ != hipSuccess) {                                                                      \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(err_));                                    \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

struct Worst { float x, got; double err; };

#define BLOCKS 4096

// out: [2][BLOCKS]
__global__ __launch_bounds__(256) void k_trig(uint32_t top_bits, Worst* out) {
  __shared__ Worst sh[2][256];
  Worst w[2] = {{0.f, 0.f, -1.0}, {0.f, 1.f, -1.0}};
  const unsigned long long total = 2ull * ((unsigned long long)top_bits + 1ull);
  for (unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; k < total; k += (unsigned long long)BLOCKS * 256ull) {
    const uint32_t bits = (uint32_t)(k >> 1) | ((uint32_t)(k & 1ull) << 31);
    const float x = __uint_as_float(bits);
    const float s = sinf(x), c = cosf(x);
    const double es = fabs((double)s - sin((double)x)), ec = fabs((double)c - cos((double)x));
    if (es > w[0].err) { w[0].x = x; w[0].got = s; w[0].err = es; }
    if (ec > w[1].err) { w[1].x = x; w[1].got = c; w[1].err = ec; }
  }
  sh[0][threadIdx.x] = w[0];
  sh[1][threadIdx.x] = w[1];
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      for (int f = 0; f < 2; ++f)
        if (sh[f][threadIdx.x + half].err > sh[f][threadIdx.x].err) sh[f][threadIdx.x] = sh[f][threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[blockIdx.x] = sh[0][0];
    out[BLOCKS + blockIdx.x] = sh[1][0];
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <out.bin>\n", argv[0]);
    return 2;
  }
  const float top = 3.15f;      // above pi: a normalised angle exceeds pi by roundings only
  uint32_t top_bits;
  memcpy(&top_bits, &top, 4);
  Worst* d = nullptr;
  CHECK(hipMalloc(&d, sizeof(Worst) * 2 * BLOCKS));
  hipLaunchKernelGGL(k_trig, dim3(BLOCKS), dim3(256), 0, 0, top_bits, d);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<Worst> h(2 * BLOCKS);
  CHECK(hipMemcpy(h.data(), d, sizeof(Worst) * 2 * BLOCKS, hipMemcpyDeviceToHost));
  CHECK(hipFree(d));
  FILE* f = fopen(argv[1], "wb");
  if (!f) {
    perror(argv[1]);
    return 1;
  }
  const int blocks = BLOCKS;
  bool ok = fwrite(&blocks, sizeof(int), 1, f) == 1 && fwrite(&top_bits, sizeof(uint32_t), 1, f) == 1 &&
            fwrite(h.data(), sizeof(Worst), h.size(), f) == h.size();
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    fprintf(stderr, "short write to %s\n", argv[1]);
    return 1;
  }
  printf("wrote the worst sinf / cosf arguments of %d blocks over %llu arguments to %s\n", blocks, 2ull * ((unsigned long long)top_bits + 1ull), argv[1]);
  return 0;
}
