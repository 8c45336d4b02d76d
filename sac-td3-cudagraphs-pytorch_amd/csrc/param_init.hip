// The parameter initialiser's translation unit: its two kernels (param_init_kernels.h) and their launchers, which engine.hip calls
// (param_init.h).  A translation unit of its own inside libsactd3_hip.so, as env.hip and hindsight.hip are: engine.hip gains no kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "param_init_kernels.h"

// what the kernels' LDS arrays and address arithmetic rely on; the engine's checks (sactd3_init_params) come first, these stand between
// any caller and the launch
static bool mat_ok(const InitMat& m) {
  if (!m.dst || ((uintptr_t)m.dst & 15u) || m.rows < 1 || m.cols < 1 || m.ld < m.cols || m.id < 0 || m.id >= PI_MAX_MATS || m.scratch_off < 0) return false;
  const int tall = m.rows > m.cols ? m.rows : m.cols, small = m.rows > m.cols ? m.cols : m.rows;
  return tall <= PI_MAX_TALL && small <= PI_MAX_SHORT && (long)m.rows * m.ld < (1l << 31);
}

hipError_t param_init_orth_launch(const InitOrthArgs& p, hipStream_t stream) {
  if (p.n < 1 || p.n > PI_MAX_MATS || !p.scratch || !p.redrawn) return hipErrorInvalidValue;
  for (int i = 0; i < p.n; ++i)
    if (!mat_ok(p.m[i])) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_init_orth, dim3(p.n), dim3(256), 0, stream, p);
  return hipGetLastError();
}

static bool fam_ok(const InitFanFam& f) {
  const bool arrays = f.P && f.T && f.M && f.V && f.t && f.pw;
  const bool aligned = !(((uintptr_t)f.P | (uintptr_t)f.T | (uintptr_t)f.T2 | (uintptr_t)f.T3 | (uintptr_t)f.M | (uintptr_t)f.V) & 15u);
  const bool offsets = !((f.size | f.b1 | f.g1 | f.W2 | f.b2 | f.g2 | f.Wh | f.bh) & 3) && 0 < f.b1 && f.b1 <= f.g1 && f.g1 + PI_HID <= f.W2 &&
                       f.W2 < f.b2 && f.b2 <= f.g2 && f.g2 + PI_HID <= f.Wh && f.Wh < f.bh && f.bh < f.size;
  return arrays && aligned && offsets && f.nets >= 1 && f.nets <= 2;
}

hipError_t param_init_fanout_launch(const InitFanArgs& p, hipStream_t stream) {
  if (p.nf < 0 || p.nf > 2 || (p.nf == 0 && !p.la)) return hipErrorInvalidValue;
  if (p.la && (!p.t_l || !p.pw_l)) return hipErrorInvalidValue;
  long chunks = 1;
  for (int i = 0; i < p.nf; ++i) {
    if (!fam_ok(p.f[i])) return hipErrorInvalidValue;
    chunks = std::max(chunks, (long)p.f[i].nets * (p.f[i].size / 4));
  }
  const unsigned blocks = (unsigned)std::min<long>(1024, (chunks + 255) / 256);
  hipLaunchKernelGGL(k_init_fanout, dim3(blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}
