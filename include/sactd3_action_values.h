/*
 * sactd3_action_values.h -- the twin critics at one state under N sampled candidate actions, on the device: best-of-N, the sampled soft
 * value and the gap to the data action (libsactd3_hip.so; include it beside sactd3.h).  The ABI version stays 1: two functions are added,
 * nothing that existed changes.
 *
 * What offline and offline-to-online RL ask of the critics first is what they think of actions the data does not contain: the gap
 * max_a Q(s, a) - Q(s, a_data) over sampled a (CQL's regulariser read as a diagnostic, Kumar et al. 2020), the sampled soft value
 * E_a[min Q - alpha log pi], the advantage of a data action over the policy's own samples (CRR / AWAC), acting by the best of N policy
 * samples (EMaQ, SfBC, IDQL).  All of them are one pass of both critics over [s | a_j], j < N, whose first layer splits into a share of the
 * state, the same for all j, and a share of the action: the call computes the first once per state.
 *
 * Candidates of row i, j < N, dimension d < a, from the draw e = eps[i][j a + d] (float32, one rounding per written operation;
 * sc / bi / lo / hi = the engine's action scale, bias and bounds):
 *   SACTD3_AV_POLICY, SAC   sd = expf(log_std), x = mean + e sd, y = tanhf(x), action = y sc + bi, dx = x - mean,
 *                           el = -(dx dx) / (2 sd sd) - logf(sd) - 0.9189385332046727f - logf(sc (1 - y y) + 1e-6f)
 *                           (mean, log_std: what sactd3_policy_device reports for the row -- the online actor); logp = sum_d el_d
 *   SACTD3_AV_POLICY, TD3   action = min(max(mode + (e sigma) sc, lo), hi), mode as sactd3_policy_device reports it; logp = 0
 *   SACTD3_AV_UNIFORM       action = lo + e (hi - lo), e uniform in [0, 1); logp = sum_d -logf(hi_d - lo_d)
 * logp sums d ascending from 0.  Each candidate is scored by both critics of `which` exactly as sactd3_qvalues_device defines Q
 * (LayerNorm two-pass with eps inside the root, the identity with layer_norm == 0); m_j = min(Q1_j, Q2_j).
 *
 * summary[i][0 .. 7]:
 *   0 q_max       max_j m_j; ties go to the lowest j, which is best_index[i] (a NaN m_j never wins; all NaN: index 0)
 *   1 q_mean      (sum_j m_j) / N, j ascending
 *   2 q_lme       q_max + tau logf((sum_j expf((m_j - q_max) / tau)) / N), j ascending
 *   3 q_std       sqrtf((sum_j (m_j - q_mean)^2) / N), j ascending
 *   4 soft_value  (sum_j (m_j - alpha logp_j)) / N with alpha = expf(log_alpha) read from device memory, for SAC with SACTD3_AV_POLICY;
 *                 every other case repeats q_mean
 *   5 q_data      min_k Q_k(s_i, actions_i); a quiet NaN when `actions` is NULL
 *   6 logp_mean   (sum_j logp_j) / N
 *   7 the number of candidates with a finite m_j
 * A row with a non-finite observation, data action or injected draw produces whatever the arithmetic gives; it is counted (stats), never
 * a fault, and never touches another row.  A row's outputs are the same bits whatever n is and whichever rows stand beside it.
 *
 * Draws: `eps` given -- they are read, nothing is drawn, no counter moves.  `eps` NULL -- native: Philox stream 0xC00 with the counter
 * words (av_ctr, row of the call, 0xC00, element >> 2), element = j a + d, lane element & 3 of the block; normals by the library's
 * Box-Muller for POLICY, philox_u01 of the word for UNIFORM.  av_ctr is a device word of this feature; it advances by one behind a call
 * that drew natively.  `eps_out` receives the draws used either way.
 *
 * Semantics are those of sactd3_qvalues_device / sactd3_policy_device: eager launches on the learner stream behind every update issued
 * before, any n >= 1 in chunks of at most 1024 rows, no copy, no host wait; SACTD3_SRC_ORDERED orders every given array both ways against
 * `caller_stream`.  The call is invisible to training and acting: scratch and control words of its own, made at its first use; no batch
 * slot, noise buffer, acting scratch or sample / noise / predict / policy counter is touched, a precomputed opening pair of
 * sactd3_step_period stays valid, and the call is allowed while sactd3_predict_begin is in flight.
 */
#ifndef SACTD3_ACTION_VALUES_H
#define SACTD3_ACTION_VALUES_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACTD3_AV_POLICY  0   /* candidates from the online actor */
#define SACTD3_AV_UNIFORM 1   /* candidates uniform inside the action bounds */
#define SACTD3_AV_SUMMARY 8   /* floats per row of `summary` */

typedef struct sactd3_action_values_io {   /* device pointers, NULL = not given / not wanted; *_ld row strides in elements */
  const float* actions; int64_t actions_ld;     /* in : [n, a]    data actions -> q_data                                          */
  const float* eps;     int64_t eps_ld;         /* in : [n, N*a]  injected draws (normals for POLICY, uniforms in [0,1) for UNIFORM) */
  float* summary;       int64_t summary_ld;     /* out: [n, 8]                                                                   */
  int32_t* best_index;                          /* out: [n]                                                                      */
  float* best_action;   int64_t best_action_ld; /* out: [n, a]    candidate best_index, bit for bit                              */
  float* cand;          /* out: [n, N, a] contiguous: every candidate action                                                     */
  float* cand_q;        /* out: [n, N, 2] Q1, Q2 of every candidate                                                              */
  float* cand_logp;     /* out: [n, N]                                                                                           */
  float* eps_out;       /* out: [n, N*a] the draws used                                                                          */
} sactd3_action_values_io;

/* Refusals, all in front of any launch, the engine left usable (SACTD3_EINVAL): a NULL handle, obs or io; no output set; n < 1;
 * `candidates` not 16, 32 or 64; an unknown `source`, `which` (SACTD3_Q_ONLINE | SACTD3_Q_TARGET) or flag; sigma not finite or negative
 * (read for TD3 with SACTD3_AV_POLICY only); tau not finite or <= 0; a stride below its width; a pointer not on the engine's device. */
int sactd3_action_values_device(sactd3_engine* e, const float* obs, int64_t obs_ld, int n, int candidates, int source, int which,
                                float sigma, float tau, const sactd3_action_values_io* io, void* caller_stream, int flags);
/* out = {calls, rows, calls that drew natively, rows with a non-finite input so far, av_ctr, 0, 0, 0}.  Device memory: [sync]. */
int sactd3_action_values_stats(sactd3_engine* e, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_ACTION_VALUES_H */
