/*
 * sactd3_rollout_collect.h -- the part of include/sactd3_rollout.h that collects a whole training segment -- T env steps of all the
 * rollout's envs, each transition a packed ring record, all of them appended -- as ONE call and two launches.  It is included by
 * sactd3_rollout.h (behind its types) and declares nothing on its own: include that header.  The ABI version stays 1: two functions are
 * added, nothing that existed changes.
 *
 * A segment of T steps on the call sequence is T x (sactd3_rollout_choose, sactd3_rollout_advance): per step a pack kernel, two acting
 * kernels, an unpack kernel, the env step and the ring append.  sactd3_rollout_collect is one launch of k_collect_rollout
 * (csrc/collect_kernels.h) -- a workgroup per tile of 16 envs that loops over the T steps by itself: observe, the actor pass of
 * sactd3_eval_rollout, the action, the env step, the record -- followed by sactd3_rb_extend_records_device of the slab.
 *
 * The action of env i at step t, by `mode` (the values of sactd3_rollout_choose; SACTD3_ROLLOUT_REPEAT is refused):
 *   SACTD3_ROLLOUT_RANDOM   what sactd3_env_sample_actions would write: the env's own draw, whose per-env count advances by one per step.
 *                           The actor is not evaluated.  The call is bit for bit T x (choose(RANDOM), advance).
 *   SACTD3_ROLLOUT_EXPLOIT  the policy's `mode` action: tanh(mean) scale + bias (SAC), tanh(u) scale + bias (TD3) -- the bits of
 *                           sactd3_eval_rollout's SACTD3_EVAL_GREEDY from the same state and parameters.
 *   SACTD3_ROLLOUT_EXPLORE  SAC: the policy's `sample`, tanh(mean + e std) scale + bias.  TD3: tanh(u) scale + bias, then + e (scale
 *                           actor_noise_std), not clamped (the env cleans what it is given).  e: element i ac_dim + j of the Philox
 *                           stream 0x900 with counter words (collect_ctr, t, 0x900, element >> 2), keyed by the engine's seed; collect_ctr
 *                           is a device word of this feature that advances once per call that drew.
 *   fp32 throughout; a policy action does not have sactd3_predict's bits (another summation order).
 *
 * Outputs.  Record (t, i) is row t num_envs + i of `records` -- time-major, so that the ring holds the order of T appends and n-step
 * chains with stride = num_envs hold -- by the record rule of sactd3_rollout.h.  `eps` [steps][num_envs][ac_dim], if given, holds the
 * draws e, and 0 in the other two modes.  Behind the call the rollout's `obs` holds the observations to act on next and its `actions`
 * the last step's actions; the env's state, books and counters, the ring and sactd3_rollout_stats are where T choose + advance calls with
 * the recorded actions leave them (the rollout's own `records` buffer is not written).
 *
 * Streams.  The kernel and the append run on the engine's learner stream: the segment acts with the parameters at that point of the call
 * sequence.  The rollout's stream is ordered around the call once, with the two events of SACTD3_SRC_ORDERED.  No host wait; no
 * allocation after the first use.
 *
 * A HIP error behind the refusals (a failed launch or append: SACTD3_EHIP) is the one case in which the call is left half done: the
 * envs may have stepped while the ring and the rollout's counters have not moved.  The event pair is closed all the same, so the
 * rollout's stream stays ordered behind the learner's.
 *
 * Training does not see the call apart from the rows: no sample, noise, exploration or policy counter moves.  As an append it breaks
 * the run-ahead chain of sactd3_step_period, as sactd3_rb_extend does.
 */
#ifndef SACTD3_ROLLOUT_COLLECT_H
#define SACTD3_ROLLOUT_COLLECT_H

#ifndef SACTD3_ROLLOUT_H
#error "include sactd3_rollout.h: it declares the rollout handle and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SACTD3_COLLECT_MAX_STEPS 4096

/* `records`: [steps * num_envs][record_len] floats, contiguous, 16-byte aligned device memory; `eps`: [steps][num_envs][ac_dim] or NULL.
 * Refusals, all in front of any side effect (a refused call has launched, counted and moved nothing; text in sactd3_rollout_last_error):
 *   SACTD3_EINVAL  a NULL handle or slab; a slab that is misaligned or not memory of the handles' device; an `eps` that is not memory of that device; a mode other
 *                  than RANDOM, EXPLORE, EXPLOIT; `steps` outside [1, 4096]; steps * num_envs above the ring slots an append may use
 *                  (rb_capacity minus the pinned rows)
 *   SACTD3_ESTATE  an acting call is in flight (sactd3_predict_begin without its end) */
int sactd3_rollout_collect(sactd3_rollout* r, int mode, int steps, float* records, float* eps);
/* out = {calls, env steps (steps summed over the calls), calls that drew, collect_ctr}; the last is a device word: waits for the
 * engine's stream */
int sactd3_rollout_collect_stats(sactd3_rollout* r, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_ROLLOUT_COLLECT_H */
