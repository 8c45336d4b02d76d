/*
 * sactd3_rollout.h -- C ABI of the native rollout of libsactd3_hip.so: a GPU-resident vector env (include/sactd3_env.h) that
 * feeds an engine (include/sactd3.h) with no Python, no allocation and no tensor arithmetic per env step.
 *
 * This is the one header that knows both handles.  It adds nothing to either: the env step below is a second form of
 * sactd3_env_step that ALSO emits every env's transition as one packed ring record (csrc/env_kernels.h: k_env_step_rec), and the
 * rollout handle strings public calls of the two ABIs together -- sactd3_env_reset / sactd3_env_sample_actions,
 * sactd3_predict_device and sactd3_rb_extend_records_device -- on buffers the caller allocated once.
 *
 * Conventions (those of sactd3_env.h)
 *   - every function returns 0 or a negative SACTD3_E* code of sactd3.h and never throws; a NULL handle gives SACTD3_EINVAL;
 *     `sactd3_rollout_last_error` gives the text of the last failure on that rollout (NULL: of the last failed
 *     `sactd3_rollout_create` on this thread); `sactd3_rollout_env_step` reports through `sactd3_env_last_error` of its env;
 *   - every call enqueues and returns at once: no call here waits on the host;
 *   - device pointers are float32 arrays in the memory of the handles' device; `*_ld` is the distance between two rows in elements;
 *   - a rollout is not thread-safe, and while it exists its env and its engine's acting / ring calls belong to it.
 *
 * The record (sactd3_rb_layout of the engine, the first three values), in floats:
 *   [s (ob_dim) | a (ac_dim) | 0-pad to next_off][s'_stored (ob_dim) | 0-pad to next_width][r, d][0-pad to record_len]
 *   s          the observation of the state BEFORE the step, recomputed from the env's own state (the caller's buffer is not read)
 *   a          the action as given, bit for bit -- not the clamped one, and a NaN / infinite one as it came (it is counted in
 *              sactd3_env_stats.bad_actions and never reaches the state)
 *   s'_stored  the observation the step arrived at, before the reset, where the step was TRUNCATED; otherwise the observation the
 *              caller acts on next -- behind a termination the auto-reset one (the rule of the reference's rollout)
 *   r, d       the reward; 1.0f where the step terminated, else 0.0f
 *   every pad float is written as 0.
 */
#ifndef SACTD3_ROLLOUT_H
#define SACTD3_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#include "sactd3.h"
#include "sactd3_env.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sactd3_record_layout {
  int32_t record_len;   /* floats per record           (sactd3_rb_layout out[0]) */
  int32_t next_off;     /* offset of s'                (out[1]) */
  int32_t next_width;   /* padded width of s'          (out[2]) */
} sactd3_record_layout;

/* One vector step = one kernel launch, as sactd3_env_step: the same state, books, counters and `obs` [n, ob_dim] (what the caller
 * acts on next) -- and record i of `records` [n, record_len] (contiguous rows) holds env i's transition.  No engine is involved.
 * SACTD3_EINVAL: a NULL argument; act_ld < ac_dim or obs_ld < ob_dim; next_off < ob_dim + ac_dim; next_width < ob_dim;
 * record_len < next_off + next_width + 2; any of the three not a multiple of 4; `records` not 16-byte aligned or not device memory
 * of the env's device.  A refused call launches nothing. */
int sactd3_rollout_env_step(sactd3_env* env, const float* actions, int64_t act_ld, const sactd3_record_layout* layout,
                            float* records, float* obs, int64_t obs_ld, void* stream);

/* the caller's buffers, allocated once and alive as long as the rollout: device memory of the handles' device */
typedef struct sactd3_rollout_buffers {
  float* obs;      int64_t obs_ld;       /* [num_envs, ob_dim]  the observations to act on */
  float* actions;  int64_t actions_ld;   /* [num_envs, ac_dim]  the action in force */
  float* records;                        /* [num_envs, record_len] contiguous, 16-byte aligned: the step's transitions */
} sactd3_rollout_buffers;

enum {
  SACTD3_ROLLOUT_RANDOM = 0,   /* uniform inside the bounds, drawn by the env (sactd3_env_sample_actions) */
  SACTD3_ROLLOUT_EXPLORE = 1,  /* the policy's exploring action (sactd3_predict_device, explore = 1) */
  SACTD3_ROLLOUT_EXPLOIT = 2,  /* its greedy action (explore = 0) */
  SACTD3_ROLLOUT_REPEAT = 3    /* the action in force stays: nothing is launched, nothing counted */
};

typedef struct sactd3_rollout sactd3_rollout;

/* Binds `env` to `engine` on `stream` (a hipStream_t, NULL = the default stream: the stream the env's kernels run on and the
 * engine's calls are ordered against).  Neither handle is owned: destroy the rollout first.  SACTD3_EINVAL: a NULL argument or
 * buffer, a stride below its width, a misaligned `records`, the env's ob_dim / ac_dim differ from the engine's, the two handles
 * are on different devices, a buffer that is not memory of that device, num_envs > the engine's max_envs (a rollout that chunks is
 * not provided). */
int sactd3_rollout_create(sactd3_engine* engine, sactd3_env* env, const sactd3_rollout_buffers* buffers, void* stream,
                          sactd3_rollout** out);
void sactd3_rollout_destroy(sactd3_rollout* r);
const char* sactd3_rollout_last_error(const sactd3_rollout* r);

/* sactd3_env_reset(seed) into `obs` */
int sactd3_rollout_reset(sactd3_rollout* r, uint64_t seed);
/* the next action into `actions` by `mode` (SACTD3_ROLLOUT_*).  The policy modes are sactd3_predict_device(obs -> actions) with
 * SACTD3_SRC_ORDERED on the rollout's stream: stream-ordered behind every update issued before the call. */
int sactd3_rollout_choose(sactd3_rollout* r, int mode);
/* one env step with `actions` (k_env_step_rec: `records` and `obs` are overwritten), then
 * sactd3_rb_extend_records_device(records, num_envs, stream, SACTD3_SRC_ORDERED): the append is ordered behind the step, and the next
 * step's overwrite of `records` behind the append, on the GPU. */
int sactd3_rollout_advance(sactd3_rollout* r);
/* host counters: out = {random choices, policy choices, steps, rows appended} */
int sactd3_rollout_stats(const sactd3_rollout* r, int64_t out[4]);

#ifdef __cplusplus
}
#endif

/* advance, choose and the engine's update as ONE graph launch per env step: declared in a header of its own, which needs the types above */
#include "sactd3_rollout_cycle.h"
/* a whole segment of T env steps, records and append as ONE call: likewise */
#include "sactd3_rollout_collect.h"

#endif /* SACTD3_ROLLOUT_H */
