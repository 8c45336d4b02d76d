/* On-policy evaluation in one launch: n envs of a sactd3_env rolled for T steps under an engine's online actor, with the trajectory, the
 * discounted returns-to-go of each env's episode and its summary left in device memory (device code: csrc/eval_kernels.h).
 *
 * One workgroup owns a tile of up to 16 envs and loops over the T steps by itself: observe -> actor MLP -> env step (the one
 * env_step_body of csrc/env_kernels.h) -> record.  No workgroup reads what another wrote; there is no grid barrier and no spin.
 *
 * Per step t and env i
 *   obs[t][i]      the observation of env i's state: the bits sactd3_env_step's `obs` would hold
 *   actions[t][i]  SACTD3_EVAL_GREEDY: tanh(mean) scale + bias (SAC), tanh(u) scale + bias (TD3): the `mode` of sactd3_policy_device
 *                  SACTD3_EVAL_SAMPLE (SAC): its `sample`, with logp[t][i] its `sample_logp` and eps[t][i] the draws: element i ac_dim + j
 *                  of the Philox stream 0x800 with counter words (eval_ctr, t, 0x800, element >> 2), keyed by the engine's seed; eval_ctr is
 *                  a device word of this feature that advances once per call that draws.  GREEDY: logp and eps are written as 0.
 *                  fp32 throughout; the action does not have sactd3_predict's bits (another summation order).
 *   reward[t][i]   of the step;  live[t][i] = 1 while the step belongs to "the call's episode" of env i -- the one it was in at t = 0
 * After step T - 1, per env, with L the number of steps of the call's episode inside the call if it ended there:
 *   rtg[L-1] = r[L-1];  for t = L-2 .. 0:  p = alpha logp[t+1] (soft only), B = rtg[t+1] - p (else rtg[t+1]), q = gamma B, rtg[t] = r[t] + q
 *   -- each one fp32 operation, in this order, never contracted; alpha = expf(log_alpha) is read once and written to `alpha` (0 for TD3).
 *   Steps outside the call's episode: rtg = 0, live = 0.  An episode still open at T: rtg = 0 everywhere, ep_length = 0, ep_terminated = 0.
 *   ep_return  the undiscounted fp32 sum of the call's episode's rewards inside the call, in step order (with reset == 1: the env's first_return)
 *   ep_length  L (0: still open);  ep_terminated  1 iff it ended by termination;  g0 = rtg[0]
 *
 * The launch goes on the engine's learner stream: it evaluates the parameters at that point of the call sequence.  The env's state and
 * the outputs are ordered against `caller_stream` by the two events of sactd3_predict_device (SACTD3_SRC_ORDERED; SACTD3_DST_ORDERED is
 * the same bit).  No host wait; no allocation after the first use (a later call that needs more reward scratch than any before it makes
 * a larger one).  The env is left, bit for bit, where sactd3_env_reset(seed) [reset == 1] plus T calls of sactd3_env_step with the recorded
 * actions leave it: state, books and counters.  The call is invisible to training and acting: no sample, noise, exploration or policy
 * counter moves, no engine state changes, a precomputed opening pair of sactd3_step_period stays valid.
 *
 * Refused with nothing changed (SACTD3_EINVAL, text in sactd3_last_error(engine)): a NULL handle or config; env and engine dims or devices
 * that differ; `steps` outside [0, 4096]; gamma outside [0, 1] or NaN; a mode other than the two; reset other than 0 / 1; SAMPLE or soft on a
 * TD3 engine; soft without SAMPLE; an output that is not memory of the device; an unknown flag. */
#ifndef SACTD3_EVAL_H
#define SACTD3_EVAL_H

#include "sactd3.h"
#include "sactd3_env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACTD3_EVAL_GREEDY 0
#define SACTD3_EVAL_SAMPLE 1
#define SACTD3_EVAL_MAX_STEPS 4096

typedef struct sactd3_eval_config {
  int32_t steps;    /* T in [1, 4096]; 0 = the env's horizon */
  int32_t mode;     /* SACTD3_EVAL_GREEDY = 0, SACTD3_EVAL_SAMPLE = 1 (SAC only) */
  int32_t reset;    /* 1: sactd3_env_reset(seed) first, books included; 0: go on from the env's state and books */
  int32_t soft;     /* 1: entropy terms in rtg (needs SAMPLE) */
  float gamma;      /* in [0, 1] */
  uint64_t seed;    /* used when reset == 1 */
} sactd3_eval_config;

typedef struct sactd3_eval_out {          /* device pointers, each may be NULL; time-major, contiguous */
  float *obs, *actions, *eps, *reward, *logp, *rtg;   /* [T][n][ob_dim | ac_dim | ac_dim | 1 | 1 | 1] */
  uint8_t *live;                                      /* [T][n] */
  float *ep_return; int32_t *ep_length; uint8_t *ep_terminated; float *g0;   /* [n]; g0 = rtg[0] */
  float *alpha;                                       /* [1] */
} sactd3_eval_out;

int sactd3_eval_rollout(sactd3_engine* engine, sactd3_env* env, const sactd3_eval_config* cfg, const sactd3_eval_out* out,
                        void* caller_stream, int flags /* SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED */);
/* out = {calls, env steps rolled, calls that drew, eval_ctr}; the last is a device word: waits for the engine's stream */
int sactd3_eval_stats(sactd3_engine* engine, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_EVAL_H */
