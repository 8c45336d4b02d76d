/*
 * sactd3_action_gradient.h -- the action (and observation) gradients of the twin critics on rows of the caller's choosing, on the device,
 * with a few steps of projected gradient ascent on min(Q1, Q2) inside the same kernel (libsactd3_hip.so; include it beside sactd3.h).  The
 * ABI version stays 1: two functions are added, nothing that existed changes.
 *
 * dQ/da is the quantity SAC and TD3 are built on (the actor follows it), and the library's forward questions -- sactd3_qvalues_device,
 * sactd3_policy_device, sactd3_action_values_device -- do not answer it.  Three uses: critic smoothness vitals (||dQ/da|| on replay rows
 * and the cosine between the twin critics' action gradients: a critic whose action gradient grows is a critic the actor is about to
 * exploit); gradient-refined acting (a few ascent steps from the policy's action, the gradient-based companion of best-of-N selection);
 * observation saliency dQ/ds.  Across ascent steps only the action's share of the first layer changes: the state's share is computed
 * once per row, and parameters, activations and the step loop stay in one workgroup.
 *
 * Q_k(s, a), k = 1, 2, is what sactd3_qvalues_device defines for the critics of `which` (LayerNorm two-pass with eps inside the root, the
 * identity with layer_norm == 0); the gradients are those of that float32 computation: ReLU passes where its output is > 0, LayerNorm
 * backward dz = rstd ((dx - mean(dx)) - xhat mean(dx xhat)), dx = dy g, with mean and rstd of the forward.
 *
 * One ascent step of a row (float32, one rounding per written operation, nothing contracted; sc / lo / hi = the engine's action scale and
 * bounds), steps times, starting from the given action:
 *   j    = Q1 <= Q2 ? 0 : 1                          (the critics at the action as it stands)
 *   gu_d = g_{j,d} * sc_d
 *   nrm  = sqrtf(sum_d gu_d * gu_d)
 *   a_d  = min(max(a_d + ((lr * gu_d) / fmaxf(nrm, 1e-8f)) * sc_d, lo_d), hi_d)
 * so `lr` is a distance in normalised action units per step and the step does not depend on the scale of Q.  The call runs steps + 1
 * forward passes and max(steps, 1) backward passes per row.  With steps == 0 `refined` is a bit copy of `actions` and `q_end` has the
 * bits of `q_start`; with lr == 0 a step leaves an action inside the bounds as it is (a negative zero becomes a positive one).
 *
 * summary[i][0 .. 7] (all sums over d ascending from 0, float32):
 *   0 min_k Q_k at the start (Q1 <= Q2 ? Q1 : Q2)
 *   1 min_k Q_k at the end
 *   2 ||g1||_2 = sqrtf(sum_d g1_d g1_d), at the start
 *   3 ||g2||_2
 *   4 (sum_d g1_d g2_d) / (||g1|| ||g2||), or 0 where a norm is 0
 *   5 sqrtf(sum_d ((refined_d - a_d) / sc_d)^2)
 *   6 the number of steps in which a component left [lo_d, hi_d] before the clamp held it there
 *   7 0
 * A row with a non-finite observation or action produces whatever the arithmetic gives; it is counted (stats), never a fault, and never
 * touches another row.  A row's outputs are the same bits whatever n is and whichever rows stand beside it.
 *
 * Semantics are those of sactd3_action_values_device: device pointers with any row stride at or above the width; eager launches on the
 * learner stream behind every update issued before, any n >= 1 in chunks of at most 1024 rows, no copy, no host wait;
 * SACTD3_SRC_ORDERED orders every given array both ways against `caller_stream`.  The call is invisible to training and acting: scratch
 * and control words of its own, made at its first use; no batch slot, noise buffer, acting scratch or counter of another feature is
 * touched, a precomputed opening pair of sactd3_step_period stays valid, and the call is allowed while sactd3_predict_begin is in flight.
 */
#ifndef SACTD3_ACTION_GRADIENT_H
#define SACTD3_ACTION_GRADIENT_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACTD3_AG_SUMMARY   8    /* floats per row of `summary` */
#define SACTD3_AG_MAX_STEPS 16   /* ascent steps of one call at most */

typedef struct sactd3_action_gradient_io {   /* device pointers, NULL = not wanted; *_ld row strides in elements */
  float* q_start;  int64_t q_start_ld;   /* out: [n, 2]         Q1, Q2 at the given actions                                      */
  float* grad;                           /* out: [2, n, a]      contiguous: dQ_k/da at the given actions                         */
  float* grad_obs;                       /* out: [2, n, ob_dim] contiguous: dQ_k/ds at the given actions (the wide layer-1
                                                                backward runs only when this is asked)                           */
  float* refined;  int64_t refined_ld;   /* out: [n, a]         the actions after `steps` ascent steps                           */
  float* q_end;    int64_t q_end_ld;     /* out: [n, 2]         Q1, Q2 at `refined`                                              */
  float* summary;  int64_t summary_ld;   /* out: [n, 8]                                                                          */
} sactd3_action_gradient_io;

/* Refusals, all in front of any launch, the engine left usable (SACTD3_EINVAL): a NULL handle, obs, actions or io; no output set; n < 1;
 * `steps` outside [0, 16]; lr not finite or negative (read only when steps > 0); an unknown `which` (SACTD3_Q_ONLINE | SACTD3_Q_TARGET)
 * or flag; a stride below its width; a pointer not on the engine's device. */
int sactd3_action_gradient_device(sactd3_engine* e, const float* obs, int64_t obs_ld, const float* actions, int64_t actions_ld,
                                  int n, int which, int steps, float lr, const sactd3_action_gradient_io* io,
                                  void* caller_stream, int flags);
/* out = {calls, rows, rows with a non-finite input so far, ascent steps run (steps x rows, summed over the calls), 0, 0, 0, 0}.
 * Device memory: [sync]. */
int sactd3_action_gradient_stats(sactd3_engine* e, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_ACTION_GRADIENT_H */
