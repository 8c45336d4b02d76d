// What engine.hip knows of the hindsight staging kernel (hindsight.hip, hindsight_kernels.h): its argument struct and its one host
// launcher.  Nothing else crosses between the two translation units.
#pragma once
#include <hip/hip_runtime.h>

#define HS_MAX_GOAL 8      // goal_dim <= HS_MAX_GOAL
#define HS_MAX_WINDOW 64   // window <= HS_MAX_WINDOW
#define HS_ROWS 136        // rows a block's span may touch: (cpb * 256) / rec4 + 2 <= HS_ROWS
#define HS_CPT 4           // 16-byte chunks per thread in the copy phase, cpb <= HS_CPT

struct HindsightArgs {
  const float4* ring; int rec4, cx, cn, o;      // the ring's geometry: chunks per record, of [s|a], of s'; floats of an observation
  int B, len, cursor, cap;
  int ag_off, dg_off, G; float thr, ratio; int window, stride;
  unsigned long long seed; unsigned hctr;       // the engine's seed and the number of native draws made before this one
  const long long* idx; long idx_ld;            // start slot of row b: idx[b * idx_ld]
  const int* choice; long choice_ld;            // NULL: the native draw.  Otherwise choice[b * choice_ld] < 0: not relabelled, else j = min(choice, L - 1)
  float4* X; float4* Xn; float* rew; float* done; int* slot_idx;
  int* offset; int* goal_slot;                  // per batch row: j (-1: not relabelled / refused), the goal's ring slot (-1)
  unsigned rec4_magic;                          // magic divisor of rec4 over [0, B * rec4], 0: divide
  int cpb;                                      // chunks per thread
  int* counters;                                // [0] rows relabelled, [1] rows refused, [2] rows whose relabelled reward is 0
};

// One launch of k_hindsight_stage over `blocks` blocks on `stream`.  hipErrorInvalidValue, and nothing is launched, where an argument is
// outside what the kernel's tables hold; otherwise hipGetLastError() behind the launch.
hipError_t hindsight_stage_launch(const HindsightArgs& args, unsigned blocks, hipStream_t stream);
