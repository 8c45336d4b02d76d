// What engine.hip knows of the action-gradient call (action_gradient.hip, action_gradient_kernels.h; include/sactd3_action_gradient.h is
// its C ABI): the argument struct and one host launcher.  The two critics are described as NetView (net_view.h), as the scan, the
// feature rank and the candidate-scoring call describe their nets; nothing else crosses between the translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "net_view.h"

#define AG_MAXA 32         // action dimensions (the actor head kernels' limit): one or two 16-column MFMA tiles
#define AG_MAXSTEPS 16     // ascent steps of one call
#define AG_CHUNK 1024      // rows of one launch
#define AG_MAXWG (AG_CHUNK / HT_TILE)      // workgroups of one launch at most: one per 16-row tile
#define AG_SUMMARY 8       // floats per row of `summary` (engine.hip asserts it against the C ABI's)
// device words of the feature (k_ag_finish)
enum { AG_W_NONFINITE = 0 /* rows with a non-finite input so far */, AG_WORDS = 4 };

struct AgArgs {
  NetView net[2]; int bh[2];                // the two critics of `which` (P: their parameter block; M, V unused) and their head bias offsets
  int ob, a, ln;                            // widths; sactd3_config::layer_norm
  int m; long n;                            // rows of this launch; rows of the call (the plane stride of grad / grad_obs in rows)
  int steps; float lr;
  const float *scale, *lo, *hi;             // [a] the engine's action scale and bounds
  int* words; int* bad;                     // [AG_WORDS]; [AG_MAXWG] non-finite rows per workgroup of this launch (k_ag_finish sums them)
  // the caller's arrays, already moved to row 0 of this launch (outputs: NULL = not wanted)
  const float* obs; long obs_ld;
  const float* actions; long actions_ld;
  float* q_start; long q_start_ld;
  float* grad;                              // plane k at grad + k n a
  float* grad_obs;                          // plane k at grad_obs + k n ob
  float* refined; long refined_ld;
  float* q_end; long q_end_ld;
  float* summary; long summary_ld;
};

static inline int ag_groups(int m) { return (m + HT_TILE - 1) / HT_TILE; }

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launches: k_action_gradient, then the single-workgroup k_ag_finish.
hipError_t action_gradient_launch(const AgArgs& args, hipStream_t stream);
