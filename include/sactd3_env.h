/*
 * sactd3_env.h -- C ABI of the GPU-resident vector environments of libsactd3_hip.so.
 *
 * Two textbook continuous-control tasks whose whole vector step is ONE kernel launch (csrc/env_kernels.h): the host draws
 * nothing, waits for nothing and does no arithmetic between `predict_device`, the env step and `rb_extend_fields_device`.
 * The handle is independent of `sactd3_engine` (include/sactd3.h): an env knows no engine and an engine no env.
 *
 * Conventions (those of sactd3.h)
 *   - every function returns 0 or a negative SACTD3_E* code of sactd3.h and never throws; a NULL handle gives SACTD3_EINVAL;
 *     `sactd3_env_last_error` gives the text of the last failure on that env (NULL env: of the last failed
 *     `sactd3_env_create` on this thread);
 *     a host allocation failure inside a call comes back as SACTD3_EHIP, and then the text may be that of an earlier failure;
 *   - every call enqueues on the CALLER's stream (`stream`: a hipStream_t, NULL = the default stream) and returns at once
 *     unless marked [sync]; a [sync] call waits for that stream.  Ordering against an engine is the engine's own event protocol
 *     of sactd3_predict_device / sactd3_rb_extend_fields_device with that same stream: the env needs none of its own;
 *   - device pointers are float32 / uint8 arrays in the memory of the env's device; `*_ld` is the distance between the rows of
 *     two envs in elements, at least the row's width; one env = one row;
 *   - an env is not thread-safe, different envs are.
 *
 * Randomness: Philox4x32-10 (csrc/philox.h), stream code 0x500, keyed by the seed.  The initial state of episode k of env i is
 * a pure function of (seed, i, k): counter words (k, i, 0x500, 0), the four result words through philox_u01.  So env i sees
 * the same episodes whatever num_envs is.  The j-th random action of env i is word 0 of counter words (j, i, 0x500, 1).
 *
 * Arithmetic: fp32, no contraction, one operation order (csrc/env_kernels.h states it; envs.py: HostVecEnv restates it in
 * numpy float32, where it gives the same bits everywhere except through sinf / cosf).
 *
 * Tasks
 *   SACTD3_ENV_PENDULUM   ob_dim 3, ac_dim 1, bounds +-2, horizon 200, never terminates.  State (theta, omega).
 *       u = clamp(a, +-2); reward = -(angnorm(theta)^2 + 0.1 omega^2 + 0.001 u^2) of the state BEFORE the step;
 *       omega' = clamp(omega + (15 sin theta + 3 u) 0.05, +-8); theta' = angnorm(theta + 0.05 omega');
 *       obs = (cos theta', sin theta', omega').  Reset: theta ~ U(-pi, pi), omega ~ U(-1, 1).
 *   SACTD3_ENV_CARTPOLE   ob_dim 4, ac_dim 1, bounds +-1, horizon 200.  State = obs = (x, x_dot, theta, theta_dot).
 *       force = 10 clamp(a, +-1); g 9.8, cart mass 1.0, pole mass 0.1, half-length 0.5, Euler step 0.02 (Barto, Sutton &
 *       Anderson 1983); terminates when |x'| > 2.4 or |theta'| > 0.20943951 (strictly); reward 1 on every step, the terminating
 *       one included.  Reset: U(-0.05, 0.05)^4.
 *   SACTD3_ENV_POINTGOAL  ob_dim 6, ac_dim 2, bounds +-1, horizon 50, never terminates.  State (x, y, vx, vy): a point mass
 *       that has to reach a goal drawn per episode.  The goal (gx, gy) is not state: for episode k of env i it is
 *       -1 + 2 philox_u01(w) of words 0 and 1 of counter words (k, i, 0x500, 2).  Per dimension c: u_c = clamp(a_c, +-1);
 *       v_c' = 0.8 v_c + 0.2 u_c; p_c' = clamp(p_c + 0.1 v_c', +-1).  obs = (x, y, vx, vy, gx, gy): the achieved goal is
 *       elements 0-1, the desired goal elements 4-5.  reward = 0 if (x'-gx)^2 + (y'-gy)^2 <= 0.1f * 0.1f else -1, of the
 *       ARRIVAL state against the running episode's goal.  Reset: x, y ~ U(-1, 1), at rest.
 *   All: truncated when the episode's step count reaches the horizon and the step did not terminate (termination wins).
 *   A NaN or infinite action component is replaced by 0; a step with any such component is counted once; none reaches the state.
 */
#ifndef SACTD3_ENV_H
#define SACTD3_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SACTD3_ENV_PENDULUM = 0,
  SACTD3_ENV_CARTPOLE = 1,
  SACTD3_ENV_POINTGOAL = 2,
  SACTD3_ENV_NUM_KINDS = 3
};

#define SACTD3_ENV_STATE_DIM 4   /* floats of physical state per env in sactd3_env_state.phys (the pendulum uses two, the rest is 0) */

typedef struct sactd3_env_config {
  int32_t kind;       /* SACTD3_ENV_* */
  int32_t num_envs;   /* >= 1 */
  int32_t horizon;    /* steps to the time limit; 0 = the task's default (200; the point mass: 50) */
  int32_t device_id;  /* HIP device ordinal */
  uint64_t seed;      /* Philox key; sactd3_env_reset replaces it */
} sactd3_env_config;

typedef struct sactd3_env_info {
  int32_t ob_dim, ac_dim, horizon, num_envs;
  float min_ac, max_ac;   /* every action dimension */
} sactd3_env_info;

/* what a step writes: device pointers, any of them except `obs` may be NULL (not wanted) */
typedef struct sactd3_env_out {
  float* obs;          int64_t obs_ld;         /* [n, ob_dim] what the caller acts on next: after any auto-reset */
  float* final_obs;    int64_t final_obs_ld;   /* [n, ob_dim] what the step arrived at, before any reset, for EVERY env */
  float* reward;       int64_t reward_ld;      /* [n] */
  uint8_t* terminated; int64_t terminated_ld;  /* [n] 0 / 1 */
  uint8_t* truncated;  int64_t truncated_ld;   /* [n] 0 / 1; never set together with terminated */
  uint8_t* ended;      int64_t ended_ld;       /* [n] terminated | truncated: the envs that were reset */
} sactd3_env_out;

/* the whole state of the envs, HOST arrays of num_envs rows each; a NULL pointer is skipped */
typedef struct sactd3_env_state {
  float* phys;        /* [n, SACTD3_ENV_STATE_DIM] */
  int32_t* steps;     /* [n] steps taken in the running episode */
  uint32_t* episode;  /* [n] index of the running episode */
  float* returns;     /* [n] running return (fp32 sum of the rewards, in order) */
  uint32_t* draws;    /* [n] random actions drawn so far */
} sactd3_env_state;

/* episode bookkeeping, HOST side; the per-env arrays (num_envs entries each) may be NULL */
typedef struct sactd3_env_stats {
  int64_t episodes;      /* episodes finished since the last reset, over all envs */
  double return_sum;     /* sum of their returns */
  int64_t length_sum;    /* sum of their lengths */
  int64_t bad_actions;   /* NaN / infinite actions replaced by 0 */
  float* last_return;    /* [n] the return of each env's last finished episode (0 before the first) */
  int32_t* last_length;  /* [n] its length (0 before the first) */
  int64_t* env_episodes; /* [n] episodes each env finished */
  float* first_return;   /* [n] the return of the FIRST episode each env finished since the reset (0 before it): one episode per env,
                            whatever their lengths -- what an evaluation over n episodes averages */
  int32_t* first_length; /* [n] its length (0 before it) */
} sactd3_env_stats;

typedef struct sactd3_env sactd3_env;

int sactd3_env_create(const sactd3_env_config* cfg, sactd3_env** out);
void sactd3_env_destroy(sactd3_env* env);
const char* sactd3_env_last_error(const sactd3_env* env);
int sactd3_env_spec(const sactd3_env* env, sactd3_env_info* out);

/* every env starts episode 0 of `seed`; counters, running returns and the episode bookkeeping restart at zero.  obs: [n, ob_dim] */
int sactd3_env_reset(sactd3_env* env, uint64_t seed, float* obs, int64_t obs_ld, void* stream);
/* one vector step = one kernel launch.  actions: [n, ac_dim] device floats */
int sactd3_env_step(sactd3_env* env, const float* actions, int64_t act_ld, const sactd3_env_out* out, void* stream);
/* [n, ac_dim] uniform inside the bounds, drawn on the device; advances each env's draw counter */
int sactd3_env_sample_actions(sactd3_env* env, float* actions, int64_t act_ld, void* stream);

int sactd3_env_episode_stats(sactd3_env* env, sactd3_env_stats* out, void* stream);       /* [sync] */
int sactd3_env_get_state(sactd3_env* env, const sactd3_env_state* out, void* stream);     /* [sync] */
int sactd3_env_set_state(sactd3_env* env, const sactd3_env_state* in, void* stream);      /* [sync] */

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_ENV_H */
