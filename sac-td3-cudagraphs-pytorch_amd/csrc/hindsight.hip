// Host side of the hindsight staging kernel (hindsight_kernels.h): its one launcher, which engine.hip calls (hindsight.h).
// A translation unit of its own inside libsactd3_hip.so, as env.hip is: engine.hip gains no kernel.
#include <hip/hip_runtime.h>

#include "hindsight_kernels.h"

hipError_t hindsight_stage_launch(const HindsightArgs& p, unsigned blocks, hipStream_t stream) {
  // what the kernel's tables and its address arithmetic rely on; the engine's checks (sactd3_hindsight_configure) come first, these
  // stand between any caller and the launch
  const bool geometry = p.ring && p.rec4 >= 1 && p.cx >= 1 && p.cn >= 1 && p.cx + p.cn < p.rec4 && p.o >= 1 && p.o <= 4 * p.cn && p.o <= 4 * p.cx;
  if (!geometry) return hipErrorInvalidValue;
  const bool ring = p.B >= 1 && p.cap >= 1 && p.len >= 1 && p.len <= p.cap && p.cursor >= 0 && p.cursor < p.cap;
  const bool goal = p.G >= 1 && p.G <= HS_MAX_GOAL && p.ag_off >= 0 && p.dg_off >= 0 && p.ag_off + p.G <= p.o && p.dg_off + p.G <= p.o;
  const bool walk = p.window >= 1 && p.window <= HS_MAX_WINDOW && p.stride >= 1;
  const bool span = p.cpb >= 1 && p.cpb <= HS_CPT && (256L * p.cpb) / p.rec4 + 2 <= HS_ROWS &&
                    (unsigned long long)blocks * 256ull * (unsigned long long)p.cpb >= (unsigned long long)p.B * (unsigned long long)p.rec4;
  const bool arrays = p.idx && p.idx_ld >= 1 && (!p.choice || p.choice_ld >= 1) && p.X && p.Xn && p.rew && p.done && p.slot_idx && p.offset &&
                      p.goal_slot && p.counters;
  if (!(ring && goal && walk && span && arrays) || blocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hindsight_stage, dim3(blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}
