// What engine.hip knows of the candidate-scoring call (action_values.hip, action_values_kernels.h; include/sactd3_action_values.h is its
// C ABI): the argument struct and one host launcher.  The two critics are described as NetView (net_view.h), as the scan and the
// feature-rank call describe their nets; nothing else crosses between the translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "net_view.h"

#define AV_ROWS 64         // candidate rows of one workgroup: four 16-row MFMA tiles = 64 / N observations with their N candidates
#define AV_DROWS 16        // ... and one more tile whose rows 0 .. 64 / N - 1 are the observations' data actions (worked only when given)
#define AV_MAXA 32         // action dimensions (the actor head kernels' limit)
#define AV_CHUNK 1024      // observation rows of one launch
#define AV_MAXWG 1024      // workgroups of one launch at most: AV_CHUNK * 64 / AV_ROWS
#define AV_SRC_POLICY 0    // `source`: SACTD3_AV_POLICY / SACTD3_AV_UNIFORM of the C ABI (engine.hip asserts the pair)
#define AV_SRC_UNIFORM 1
#define AV_STREAM 0xC00u   // third counter word of the native draws (free beside 0x000 + site, 0x100 .. 0xB00)
// device words of the feature (AvArgs::words)
enum { AV_W_CTR = 0 /* av_ctr: numbers the native draws */, AV_W_NONFINITE = 1 /* rows with a non-finite input so far */, AV_WORDS = 4 };

struct AvArgs {
  NetView net[2]; int bh[2];             // the two critics of `which` (P: their parameter block; M, V unused) and their head bias offsets
  int ob, a, ln;                            // widths; sactd3_config::layer_norm
  int m; long row0;                         // observation rows of this launch; the row of the call its row 0 is (numbers the native draws)
  int source, sac, soft;                    // SACTD3_AV_*; the actor is SAC's; column 4 is the soft value (SAC with POLICY)
  float sigma, tau;
  const float* x; int ldo;                  // [m][ldo] the launch's observations, packed and zero-padded (the pack kernel's)
  const float* head; int head_ld;           // [m][head_ld] the actor head's outputs: SAC mean | log_std, TD3 mode (POLICY only)
  const float *scale, *bias, *lo, *hi;      // [a] the engine's action scale, bias and bounds
  const float* log_alpha;                   // device word (read when `soft`)
  const unsigned long long* seed;           // the engine's Philox key
  int* words; int* bad;                     // [AV_WORDS]; [AV_MAXWG] non-finite rows per workgroup of this launch (k_av_finish sums them)
  int tick;                                 // k_av_finish advances av_ctr: behind the last launch of a call that drew natively
  // the caller's arrays, already moved to row 0 of this launch (NULL: not given / not wanted)
  const float* actions; long actions_ld;
  const float* eps; long eps_ld;
  float* summary; long summary_ld;
  int* best_index;
  float* best_action; long best_action_ld;
  float *cand, *cand_q, *cand_logp, *eps_out;
};

static inline int av_groups(int m, int candidates) { return (int)(((long)m * candidates + AV_ROWS - 1) / AV_ROWS); }

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launches: k_action_values<candidates>, then the single-workgroup k_av_finish.
hipError_t action_values_launch(const AvArgs& args, int candidates, hipStream_t stream);
