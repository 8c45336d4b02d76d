// The hindsight translation unit: the two forms of the staging kernel around their one body, and the launchers of every hindsight
// kernel, which engine.hip calls (hindsight.h).  A translation unit of its own inside libsactd3_hip.so, as env.hip is: engine.hip
// gains no kernel.
#include <hip/hip_runtime.h>

#include "hindsight_kernels.h"

// The call form: len, cursor and hctr as the host holds them.  (The body lives in hindsight_stage_body.inc, shared with the graph form
// below, as nstep_body.inc is shared.)
__global__ __launch_bounds__(256) void k_hindsight_stage(HindsightArgs p) {
#pragma clang fp contract(off)
#include "hindsight_stage_body.inc"
}
// The graph form: len and cursor from the device's {rb_len, rb_cursor} words, hctr from the snapshot word k_hindsight_draw_g left, read
// once per block at entry and bounded before anything is derived from them; the config stays by value.  Always the native draw: there
// is no `choice` path.  For the values the host would have passed it leaves the call form's bits.
__global__ __launch_bounds__(256) void k_hindsight_stage_g(HindsightArgsG q) {
#pragma clang fp contract(off)
  HindsightArgs p = q.a;
  p.len = hs_dev_len(q.ring_words, p.cap);
  p.cursor = hs_dev_cursor(q.ring_words, p.cap);
  p.hctr = (unsigned)q.hs_words[HS_WORD_SNAPSHOT];
  p.choice = nullptr; p.choice_ld = 0;
#include "hindsight_stage_body.inc"
}

// what both staging kernels' tables and address arithmetic rely on, whoever holds len and cursor; the engine's checks
// (sactd3_hindsight_configure) come first, these stand between any caller and the launch
static bool stage_args_ok(const HindsightArgs& p, unsigned blocks) {
  const bool geometry = p.ring && p.rec4 >= 1 && p.cx >= 1 && p.cn >= 1 && p.cx + p.cn < p.rec4 && p.o >= 1 && p.o <= 4 * p.cn && p.o <= 4 * p.cx;
  if (!geometry) return false;
  const bool ring = p.B >= 1 && p.cap >= 1;
  const bool goal = p.G >= 1 && p.G <= HS_MAX_GOAL && p.ag_off >= 0 && p.dg_off >= 0 && p.ag_off + p.G <= p.o && p.dg_off + p.G <= p.o;
  const bool walk = p.window >= 1 && p.window <= HS_MAX_WINDOW && p.stride >= 1;
  const bool span = p.cpb >= 1 && p.cpb <= HS_CPT && (256L * p.cpb) / p.rec4 + 2 <= HS_ROWS &&
                    (unsigned long long)blocks * 256ull * (unsigned long long)p.cpb >= (unsigned long long)p.B * (unsigned long long)p.rec4;
  const bool arrays = p.idx && p.idx_ld >= 1 && (!p.choice || p.choice_ld >= 1) && p.X && p.Xn && p.rew && p.done && p.slot_idx && p.offset &&
                      p.goal_slot && p.counters;
  return ring && goal && walk && span && arrays && blocks >= 1;
}

hipError_t hindsight_stage_launch(const HindsightArgs& p, unsigned blocks, hipStream_t stream) {
  if (!stage_args_ok(p, blocks)) return hipErrorInvalidValue;
  const bool ring = p.len >= 1 && p.len <= p.cap && p.cursor >= 0 && p.cursor < p.cap;
  if (!ring) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hindsight_stage, dim3(blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t hindsight_draw_g_launch(const HindsightDrawArgs& p, hipStream_t stream) {
  const bool words = p.seed && p.sample_ctr && p.ring_words && p.hs_words;
  const bool out = p.idx_out && ((uintptr_t)p.idx_out & 31u) == 0;      // (four slots leave as one 32-byte store)
  if (!(words && out && p.B >= 1 && p.cap >= 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hindsight_draw_g, dim3(1), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t hindsight_stage_g_launch(const HindsightArgsG& g, unsigned blocks, hipStream_t stream) {
  // len and cursor are the device's: the kernel bounds them by a.cap.  No injected choices inside a graph.
  if (!stage_args_ok(g.a, blocks) || g.a.choice || !g.ring_words || !g.hs_words) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hindsight_stage_g, dim3(blocks), dim3(256), 0, stream, g);
  return hipGetLastError();
}
