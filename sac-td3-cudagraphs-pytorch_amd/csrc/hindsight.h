// What engine.hip knows of the hindsight kernels (hindsight.hip, hindsight_kernels.h): their argument structs and one host launcher
// per kernel.  Nothing else crosses between the two translation units.
#pragma once
#include <hip/hip_runtime.h>

#define HS_MAX_GOAL 8      // goal_dim <= HS_MAX_GOAL
#define HS_MAX_WINDOW 64   // window <= HS_MAX_WINDOW
#define HS_ROWS 136        // rows a block's span may touch: (cpb * 256) / rec4 + 2 <= HS_ROWS
#define HS_CPT 4           // 16-byte chunks per thread in the copy phase, cpb <= HS_CPT
// The hindsight allocation of 32 device ints: [0, 3) the counters below; two adjacent words of its spare part carry the draw counter of
// the graph forms.  MASTER: native hindsight draws made, as the device counts them (the host publishes its own count in front of a graph
// launch when the two differ); SNAPSHOT: the count k_hindsight_draw_g found, which is the hctr of the k_hindsight_stage_g behind it.
#define HS_WORD_MASTER 16
#define HS_WORD_SNAPSHOT 17
#define HS_WORDS 32

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
// k_hindsight_stage_g: `a` without len, cursor, hctr and choice, which the kernel replaces -- len and cursor by the two adjacent device
// words {rb_len, rb_cursor} at ring_words, hctr by hs_words[HS_WORD_SNAPSHOT].  a.idx is what k_hindsight_draw_g wrote.
struct HindsightArgsG {
  HindsightArgs a;
  const int* ring_words;
  const int* hs_words;                          // the hindsight allocation (HS_WORDS ints)
};
// k_hindsight_draw_g: the device words it reads and advances, each through a pointer the host computed
struct HindsightDrawArgs {
  const unsigned long long* seed;               // the engine's seed
  int* sample_ctr;                              // the sample counter: read, then advanced once
  const int* ring_words;                        // {rb_len, rb_cursor}
  int* hs_words;                                // the hindsight allocation (HS_WORDS ints): MASTER read and advanced, SNAPSHOT written
  long long* idx_out;                           // [B rounded up to 4], 32-byte aligned
  int B, cap;
};

// One launch of k_hindsight_stage over `blocks` blocks on `stream`.  hipErrorInvalidValue, and nothing is launched, where an argument is
// outside what the kernel's tables hold; otherwise hipGetLastError() behind the launch.
hipError_t hindsight_stage_launch(const HindsightArgs& args, unsigned blocks, hipStream_t stream);
// The graph forms, with the same contract.  The host checks what it still can -- capacity, geometry, span, pointers; len and cursor are
// the device's, which the kernels bound themselves.
hipError_t hindsight_draw_g_launch(const HindsightDrawArgs& args, hipStream_t stream);
hipError_t hindsight_stage_g_launch(const HindsightArgsG& args, unsigned blocks, hipStream_t stream);
