/*
 * sactd3.h -- C ABI of the MI355X-native SAC/TD3 update engine (libsactd3_hip.so).
 *
 * The reference (lionelblonde/sac-td3-cudagraphs-pytorch) has no FFI of its own: its boundary is
 * the duck-typed Python `Agent` object that orchestrator.py drives.  Every
 * entry point below therefore cites the reference *call site / method* it stands in for; the
 * Python mirror of that object lives in sac-td3-cudagraphs-pytorch_amd/agent.py and binds these
 * symbols with ctypes.
 *
 * Conventions
 *   - plain C types only; all host pointers are caller-owned and only read/written during the call;
 *   - every function returns 0 on success, a negative SACTD3_E* code on failure and never throws;
 *     `sactd3_last_error` gives the text of the last failure on that engine (NULL engine: of the
 *     last failed `sactd3_create` on this thread);
 *   - calls are asynchronous on the engine's HIP stream unless marked [sync];
 *   - one engine = one learner = one GPU; an engine is not thread-safe, different engines are.
 *   - all arithmetic is fp32, hidden width is 256 (agents/agent.py:56,101 hard-codes (256,256)).
 *   - the library reads NO environment variable: every behaviour is a field of sactd3_config (tests/test_abi.py checks the
 *     source and the shipped binary).
 */
#ifndef SACTD3_H
#define SACTD3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SACTD3_ABI_VERSION 1

enum {
  SACTD3_OK = 0,
  SACTD3_EINVAL = -1,   /* bad argument / configuration                      */
  SACTD3_EHIP = -2,     /* a HIP runtime call failed (text in last_error)    */
  SACTD3_ESTATE = -3,   /* call not valid in the current state (e.g. empty buffer) */
  SACTD3_ENODEV = -4    /* no usable gfx950 device                            */
};

/* Which parameter set (`which` arguments).  Layout of the float arrays exchanged with the host is the
 * reference's state_dict order (agents/nets.py:66-82, verified key list in SURVEY.md 8-A12):
 *   fc_block_1.fc.weight [256,in] | .bias [256] | (ln.weight [256] | ln.bias [256])   -- LN pair only if layer_norm
 *   fc_block_2.fc.weight [256,256] | .bias | (ln.weight | ln.bias) | head.weight [nh,256] | head.bias [nh]
 * all row-major, unpadded; the twin critics are two such blocks back to back (= the dense-stacked
 * [2, ...] tensors of agents/agent.py:106 viewed net-major). */
enum {
  SACTD3_ACTOR = 0,
  SACTD3_CRITICS = 1,
  SACTD3_ACTOR_TARGET = 2,
  SACTD3_CRITICS_TARGET = 3,
  SACTD3_LOG_ALPHA = 4
};

/* Noise sites (sactd3_set_noise).  Draw order per iteration is the reference's:
 * critic draw -> [actor draw -> alpha draw] x actor_update_delay (agents/agent.py:205,254,298). */
enum {
  SACTD3_SITE_CRITIC = 0,  /* SAC: eps of a'~pi(s') (agent.py:205); TD3: smoothing noise N(0,1) (agent.py:197) */
  SACTD3_SITE_ACTOR0 = 1,  /* eps of a~pi(s), 1st actor update of the iteration (agent.py:254) */
  SACTD3_SITE_ACTOR1 = 2,  /*                 2nd actor update (fused sactd3_step only)       */
  SACTD3_SITE_ALPHA0 = 3,  /* eps of the fresh alpha-loss draw (agent.py:298)                 */
  SACTD3_SITE_ALPHA1 = 4,
  SACTD3_SITE_PREDICT = 5, /* exploration draw in predict (nets.py:156-158,225)               */
  SACTD3_NUM_SITES = 6
};

/* Metrics slots (sactd3_read_metrics): the keys the reference's update methods return
 * (agents/agent.py:238-242,305-311). */
enum {
  SACTD3_M_QF_LOSS = 0,
  SACTD3_M_ACTOR_LOSS = 1,
  SACTD3_M_ALPHA_LOSS = 2,
  SACTD3_M_ALPHA = 3,
  SACTD3_M_BC_LOSS = 4,    /* TD3+BC only (sactd3_set_bc): the unweighted (1 / (B A)) sum (pi - a)^2 of the last actor update */
  SACTD3_M_BC_LAMBDA = 5,  /* TD3+BC only: lambda = bc_alpha / max(mean |Q1(s, pi(s))|, 1e-8) of the last actor update       */
  SACTD3_NUM_METRICS = 8
};

/* Numeric hyper-parameters = the keys of tasks/defaults/{sac,td3}.yml the hot path reads
 * (agents/agent.py:47-58,115-139,194-228,284-331; orchestrator.py:345-348). */
typedef struct sactd3_config {
  int32_t abi_version;          /* must be SACTD3_ABI_VERSION */
  int32_t ob_dim;               /* net_shapes["ob_shape"][-1] */
  int32_t ac_dim;               /* net_shapes["ac_shape"][-1] */
  int32_t batch_size;           /* sac.yml:38 */
  int32_t rb_capacity;          /* sac.yml:40 (rows) */
  int32_t max_envs;             /* largest n accepted by predict / rb_extend in one call (>= num_envs) */
  int32_t prefer_td3_over_sac;  /* sac.yml:42 */
  int32_t layer_norm;           /* sac.yml:29 */
  int32_t autotune;             /* sac.yml:47 */
  int32_t bcq_style_targ_mix;   /* td3.yml:43 */
  int32_t targ_actor_smoothing; /* td3.yml:46 */
  int32_t actor_update_delay;   /* sac.yml:44 */
  int32_t crit_targ_update_freq;/* sac.yml:45 (ignored for TD3, agent.py:323) */
  int32_t use_graphs;           /* 1: hipGraph replay (the reference's cudagraphs: true); 0: eager launches */
  int32_t device_id;            /* HIP device ordinal */
  int32_t reserved0;
  float actor_lr, qnets_lr, log_alpha_lr;   /* sac.yml:32-33,48 */
  float gamma, polyak, alpha_init;          /* sac.yml:39,41,46 */
  float clip_norm;                          /* sac.yml:34; <= 0 disables (agent.py:284) */
  float td3_std, td3_c, actor_noise_std;    /* td3.yml:45-48 */
  float adam_beta1, adam_beta2, adam_eps;   /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 (agent.py:115-139) */
  float bc_alpha;               /* TD3+BC (sactd3_set_bc): > 0 turns the behaviour-cloning actor term on, for good; 0 (the default) = plain TD3 / SAC */
  uint64_t seed;                /* keys the engine's Philox4x32-10 streams (main.py:145-146 seeds torch instead) */
} sactd3_config;

typedef struct sactd3_engine sactd3_engine;

/* Fill `cfg` with tasks/defaults/sac.yml (td3 == 0) or td3.yml (td3 != 0) values; dims/seed left 0. */
void sactd3_default_config(sactd3_config* cfg, int td3);

/* Agent.__init__ (agents/agent.py:24-144).  min_ac/max_ac: [ac_dim] action bounds (agent.py:35-36).
 * Parameters start at zero weights / LN gamma=1: the caller supplies the reference's orthogonal
 * init through sactd3_set_params (the Python mirror does, with torch's own orthogonal_) -- or asks the
 * engine for its own, on the device and without torch: sactd3_init_params (sactd3_init.h). */
int sactd3_create(const sactd3_config* cfg, const float* min_ac, const float* max_ac, sactd3_engine** out);
void sactd3_destroy(sactd3_engine* e);
const char* sactd3_last_error(const sactd3_engine* e);
int sactd3_abi_version(void);
/* the configuration the engine was created with (dims, max_envs, device_id, ...): for code that is handed an engine it did not make */
int sactd3_get_config(const sactd3_engine* e, sactd3_config* out);

/* ---- parameters / optimiser state: Agent.save / load_from_disk (agents/agent.py:333-371) ---- */
int64_t sactd3_param_count(const sactd3_engine* e, int which);            /* floats exchanged for `which` */
int sactd3_get_params(sactd3_engine* e, int which, float* dst);           /* [sync] */
int sactd3_set_params(sactd3_engine* e, int which, const float* src);     /* [sync] */
/* Adam state of the optimiser that owns `which` (ACTOR -> actor_optimizer, CRITICS -> q_optimizer,
 * LOG_ALPHA -> alpha_optimizer): exp_avg / exp_avg_sq in the same layout as the params, step count. */
int sactd3_get_adam_state(sactd3_engine* e, int which, float* exp_avg, float* exp_avg_sq, int64_t* step); /* [sync] */
int sactd3_set_adam_state(sactd3_engine* e, int which, const float* exp_avg, const float* exp_avg_sq, int64_t step); /* [sync] */

/* ---- replay buffer: TensorDictReplayBuffer(LazyTensorStorage(capacity, device)) (main.py:167-171) ---- */
/* rb.extend (orchestrator.py:100-113): n rows, row-major host arrays; `dones` is the reference's
 * `terminations` (== `dones`, orchestrator.py:107-108) as bytes. Rows go to the ring cursor, wrapping. */
int sactd3_rb_extend(sactd3_engine* e, const float* obs, const float* actions, const float* rewards,
                     const float* next_obs, const uint8_t* dones, int n);
int64_t sactd3_rb_len(const sactd3_engine* e);                             /* len(rb) (orchestrator.py:385) */
/* the generation of the batch slot: it strictly increases with every accepted call that changes the rows sactd3_read_batch reports
 * (the sactd3_rb_sample* and sactd3_load_batch* calls, sactd3_step*, the refilling kernels of sactd3_time_kernel / _time_nodes), by no
 * promised amount, and no other call changes it: not an update on the rows already there (sactd3_update_*), not a read-out, not an
 * append, and not a refused call, which changed nothing.  Whoever holds a name for the slot, not a copy of its rows, remembers the
 * value and compares.  Host state: no launch, no wait. */
int64_t sactd3_batch_generation(const sactd3_engine* e);
/* layout of one ring record, in floats: out = {record length, offset of s' (= padded width of [s | a]), padded width of s',
 * rb_capacity}; record = [s (ob_dim) | a (ac_dim) | 0-pad][s' (ob_dim) | 0-pad][r, d (0/1)][0-pad to a 64-byte multiple] */
int sactd3_rb_layout(const sactd3_engine* e, int32_t out[4]);
/* rb.extend (orchestrator.py:100-113) with n records ALREADY PACKED (sactd3_rb_layout) IN DEVICE MEMORY: the shared-replay
 * variant of BASELINE.json's north_star (not in the reference) all-gathers every rank's new rows over RCCL into one device
 * slab and appends it here with one kernel, no host round trip.  `records` must stay valid until sactd3_sync. */
int sactd3_rb_extend_device(sactd3_engine* e, const float* records, int n);
/* ---- the device boundary: the reference's loop hands the agent DEVICE tensors -- rb.extend gets a device TensorDict
 * (orchestrator.py:100-113), update_qnets / update_actor get a device batch (agents/agent.py:183,245) -- and the two calls below take
 * them where they are: five arrays in the memory of the engine's device, each with a row stride in elements and a contiguous inner
 * dimension (rows need not be 16-byte aligned; a [n, 1] or [n] array has width 1).  One kernel launch assembles the records from
 * them; nothing is copied through the host, the host never waits. */
typedef struct sactd3_device_fields {     /* device pointers; *_ld = row stride in elements */
  const float* obs;      int64_t obs_ld;
  const float* actions;  int64_t actions_ld;
  const float* rewards;  int64_t rewards_ld;
  const float* next_obs; int64_t next_obs_ld;
  const uint8_t* dones;  int64_t dones_ld;  /* any non-zero byte = done (torch.bool storage) */
} sactd3_device_fields;
/* flags: order the read against `producer_stream` -- the hipStream_t on which the caller last wrote the arrays and will next overwrite
 * or free them (NULL = the legacy default stream, which is torch's default stream: the flag is the switch, not the pointer) -- on the GPU:
 * the learner stream waits for an event recorded on `producer_stream` now, and `producer_stream` then waits for an event recorded behind
 * the launch, so neither a later write by the caller nor a same-stream reuse of the freed memory overtakes the read.  Without the flag
 * nothing is inserted: the caller has synchronised and leaves the arrays untouched until sactd3_sync (as for sactd3_rb_extend_device). */
#define SACTD3_SRC_ORDERED 1
/* rb.extend (orchestrator.py:100-113) of n >= 0 rows from device fields: same ring state as sactd3_rb_extend of the same rows. */
int sactd3_rb_extend_fields_device(sactd3_engine* e, const sactd3_device_fields* f, int n, void* producer_stream, int flags);
/* sactd3_rb_extend_device for a slab whose PRODUCER is still running: n >= 0 records already packed (sactd3_rb_layout) in the memory of
 * the engine's device, 16-byte aligned -- what a GPU-resident env writes per step (include/sactd3_rollout.h).  The same launches, the
 * same ring-region chunking, the same ring state (pinned prefix, priorities) as sactd3_rb_extend_device of the same records; flags &
 * SACTD3_SRC_ORDERED brackets them with the two events described above, so the caller neither synchronises nor keeps the slab beyond
 * its own stream's order.  n == 0 is a no-op and inserts no events.  SACTD3_EINVAL: a NULL or misaligned pointer, one that is not
 * memory of the engine's device, n < 0, an unknown flag; nothing is launched then. */
int sactd3_rb_extend_records_device(sactd3_engine* e, const float* records, int n, void* producer_stream, int flags /* SACTD3_SRC_ORDERED */);
/* a caller-owned device batch (agents/agent.py:183,245), n == batch_size: same batch slot, bit for bit, as sactd3_load_batch. */
int sactd3_load_batch_device(sactd3_engine* e, const sactd3_device_fields* f, int n, void* producer_stream, int flags);
/* Both: SACTD3_EINVAL for a NULL field, a stride below the field's width, a pointer that is not memory of the engine's device, n out
 * of range.  Like the other sactd3_rb_* calls they neither wait for nor are waited for by an acting call in flight.
 * host counters: out = {device-field extends, rows they appended, device batches staged, calls that inserted event waits} */
int sactd3_boundary_stats(const sactd3_engine* e, int64_t out[4]);
/* ---- the device boundary, outwards: the reference's rb.sample() returns a DEVICE TensorDict (main.py:167-171:
 * LazyTensorStorage(capacity, device); orchestrator.py:338), and whatever is written against it -- an auxiliary loss, a logging hook on
 * batch["rewards"], a sampler of its own that relabels or chains ring rows -- does torch math on device tensors.  The two calls below hand
 * the batch slot and ring records out where they are: six arrays in the memory of the engine's device, each with a row stride in
 * elements (>= its width), a contiguous inner dimension and no alignment beyond its element type's (4 bytes for the floats, 8 for the
 * index, 1 for the flags); a NULL pointer means that field is not wanted.  One kernel launch on the learner stream fills all of them and
 * writes nothing outside the [n, width] windows; no copy command, no wait or synchronisation on the host. */
typedef struct sactd3_device_fields_out {   /* device pointers (NULL = field not wanted); *_ld = row stride in elements */
  float* obs;      int64_t obs_ld;
  float* actions;  int64_t actions_ld;
  float* rewards;  int64_t rewards_ld;
  float* next_obs; int64_t next_obs_ld;
  uint8_t* dones;  int64_t dones_ld;        /* bytes 0 / 1 (torch.bool storage) */
  int64_t* index;  int64_t index_ld;        /* the ring slot of every row */
} sactd3_device_fields_out;
/* flags: order the write against `consumer_stream` -- the hipStream_t on which the caller last used the destinations (and produced `idx`,
 * and on which its allocator hands the blocks out) and will read them next -- with the same bit and the same two events as
 * SACTD3_SRC_ORDERED: the learner stream first waits for what the caller has queued there, and `consumer_stream` then waits for an event
 * recorded behind the launch, so the caller may read the arrays on it at once.  Without the flag nothing is inserted: the caller has
 * synchronised, and calls sactd3_sync before it reads. */
#define SACTD3_DST_ORDERED 1
/* the batch slot sactd3_read_batch reports (the most recent iteration's), n = batch_size rows: the destinations hold, bit for bit, what
 * sactd3_read_batch returns at the same position of the call sequence. */
int sactd3_read_batch_device(sactd3_engine* e, const sactd3_device_fields_out* f, void* consumer_stream, int flags);
/* n >= 1 ring records chosen by a DEVICE int64 array (`idx[i * idx_ld]`: the ring slot, what `index` of a sample and the argument of
 * sactd3_rb_sample_with_indices mean), for a replay sampler the engine does not own.  Indices are checked on the device against the
 * ring length at the call: a row whose index is outside [0, sactd3_rb_len) is handed out as zeros with flag 0 and its index as given,
 * and counted (sactd3_readout_stats); it never becomes an address.  SACTD3_ESTATE on an empty ring. */
int sactd3_rb_read_rows_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, int n, const sactd3_device_fields_out* f,
                               void* consumer_stream, int flags);
/* Both: SACTD3_EINVAL for all six destinations NULL, a stride below the width, a non-NULL pointer (or `idx`) that is not memory of the
 * engine's device, n < 1, an unknown flag; the engine stays usable.  A read-out changes nothing an update depends on: the batch slot, the
 * sample counter and a precomputed opening pair of sactd3_step_period stay as they are.  Like the other sactd3_rb_* calls they neither
 * wait for nor are waited for by an acting call in flight.
 * [sync] out = {batch read-outs, row read-outs, rows requested, rows refused for their index (counted on the device)} */
int sactd3_readout_stats(sactd3_engine* e, int64_t out[4]);
/* ---- training on rows a sampler of the caller's own chose, with loss weights, and the TD errors back: what a prioritised replay
 * iteration needs to stay on the device end to end (index staging, a weighted critic loss, a TD read-out).  Nothing here changes what the
 * calls above and below compute; the fused sactd3_step* paths keep their own uniform sampler and are never weighted (sactd3_step_sampled is
 * the iteration that draws by priority inside its graph).
 * rb.sample() with the caller's indices: one kernel launch on the learner stream fills batch slot 0 (the rows, their ring slots) from the
 * ring -- bit for bit what sactd3_rb_sample_with_indices leaves for the same indices -- and the slot's per-row loss weights from `w`
 * (w[i * w_ld]; NULL: all 1).  `idx` (idx[i * idx_ld], the ring slot of row i) and `w` are DEVICE pointers in the memory of the engine's
 * device, strides in elements (>= 1); n == batch_size.  No host wait, no copy command, no tick of the sample counter.  Indices are checked
 * on the device against the ring length at the call: a row whose index is outside [0, sactd3_rb_len) never becomes an address -- it is
 * stored as a zero record with ring slot -1 and weight 0, contributes nothing to the loss or to any gradient, and is counted
 * (sactd3_priority_stats).  A weight that is negative, NaN or infinite is stored as 0 and counted: a device value cannot poison the
 * parameters.  flags & SACTD3_SRC_ORDERED orders the reads against `caller_stream` as sactd3_load_batch_device does.
 * SACTD3_ESTATE on an empty ring; SACTD3_EINVAL for n != batch_size, a stride below 1, a pointer that is not memory of the engine's
 * device, an unknown flag; the engine stays usable. */
int sactd3_rb_sample_indices_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* w, int64_t w_ld, int n,
                                    void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* Loss weights for whatever batch slot 0 holds -- a caller-owned batch of sactd3_load_batch_device, an index-staged one: one launch, same
 * rules for `w`, n, the flag and the errors as above; rows stored with ring slot -1 stay at weight 0.  w == NULL drops the weights.
 * "The slot carries weights" is host state: the two calls above set it; every other refill of the slot clears it (sactd3_rb_sample,
 * _with_indices, sactd3_load_batch, _device, every sactd3_step*, sactd3_time_nodes, sactd3_time_kernel of a kernel that overwrites the slot).  While it is set,
 * sactd3_update_qnets runs in its weighted form, a captured graph of its own with the same nodes, captured at its first use
 * (sactd3_instantiate_graphs does not make it, the first staging call allocates the weights: an engine that never stages weights holds
 * nothing more than before), with the loss
 *     L = sum_k (1 / B) sum_i w_i (Q_k(s_i, a_i) - y_i)^2        (the divisor is B, not sum w; SACTD3_M_QF_LOSS reports L)
 * sactd3_update_actor is never weighted. */
int sactd3_batch_weights_device(sactd3_engine* e, const float* w, int64_t w_ld, int n, void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* Per-row TD errors of the most recent critic update, whichever entry point issued it (sactd3_update_qnets, sactd3_step,
 * sactd3_step_period, sactd3_step_prefix): td[k * td_ns + i * td_ld] = Q_k(s_i, a_i) - y_i, signed, per critic, the values the update
 * itself computed (its own policy draw included), in the layout of sactd3_qvalues_device's `q`; row i is row i of the batch slot
 * sactd3_read_batch reports.  `td` is a DEVICE pointer, strides in elements (>= 1).  One launch on the learner stream, no host wait;
 * flags & SACTD3_DST_ORDERED orders the write against `caller_stream` as sactd3_read_batch_device does.  Invisible to training in the
 * sense of sactd3_qvalues_device: it reads the stored q and y only, and a precomputed opening pair of sactd3_step_period stays valid.
 * SACTD3_ESTATE when no critic update has run on the rows now in that slot (before the first update, or after a refill of the slot
 * since); SACTD3_EINVAL as above. */
int sactd3_td_errors_device(sactd3_engine* e, float* td, int64_t td_ld, int64_t td_ns, void* caller_stream, int flags /* SACTD3_DST_ORDERED */);
/* [sync] out = {index stagings, weight stagings, td read-outs, rows refused on the device (bad index or bad weight; one per row and call)} */
int sactd3_priority_stats(sactd3_engine* e, int64_t out[4]);
/* ---- prioritised replay the engine owns: proportional prioritisation (Schaul et al. 2016, proportional variant, draws with replacement)
 * with the priorities, their partial sums, the running maximum and the draw counter all in device memory, maintained by kernels on the
 * learner stream.  A prioritised iteration is four calls with no arithmetic of the caller's in between:
 *     sactd3_rb_sample_prioritized -> sactd3_update_qnets (its weighted form) -> sactd3_prio_update_from_td -> [sactd3_update_actor] ->
 *     sactd3_update_targ_nets
 * Nothing above changes: an engine that never calls sactd3_prio_enable allocates nothing more and launches nothing more.
 * State: leaf[rb_capacity] = p_i^alpha per ring slot (0 for a slot the ring has not filled) and one sum per group of 1024 consecutive
 * slots, ALWAYS recomputed from the group's leaves in a fixed order, never adjusted incrementally: two histories that reach the same
 * leaves reach the same sums bit for bit.  The top level is as wide as the ring needs; any rb_capacity works.
 * Allocates and builds the table; rows already in the ring enter at priority 1 (the starting maximum).  alpha >= 0 and eps > 0, both
 * finite, else SACTD3_EINVAL; a second call with the same values does nothing, with other values SACTD3_ESTATE.  From then on every
 * append path (sactd3_rb_extend, _extend_device, _extend_fields_device -- across the wrap too -- and sactd3_rb_fill_synthetic) issues one
 * more launch behind its own, which gives the rows it wrote the current maximum priority and re-sums the groups they touch. [sync] */
int sactd3_prio_enable(sactd3_engine* e, float alpha, float eps);
/* rb.sample(batch_size) by priority.  batch_size uniforms u_b come from the Philox stream SACTD3_STREAM_PRIO (0x300: counter words
 * (draw counter, 0, 0x300, b >> 2), word b & 3, mapped to (0, 1) with 24 bits and kept below 1); the draw counter is a device word of its
 * own, advanced on the device once per call -- the uniform sampler's counter is not consumed.  With T the total of the leaves of rows
 * [0, sactd3_rb_len) and c their inclusive running sum, row b gets the smallest slot i with c[i] > u_b * T (one fp32 multiply) and a
 * positive leaf: a slot of priority 0 or beyond the ring length is never drawn.  (In fp32 the running sums are those of the two-level
 * table: where they are exact -- integer priorities -- the rule above holds to the letter.)  Batch slot 0 receives those rows and
 * their ring slots, bit for bit what sactd3_rb_sample_indices_device leaves for the same indices, and the per-row weights
 *     w_b = (N leaf_i / T)^(-beta) / max_b' (...),   N = sactd3_rb_len   (beta == 0: exactly 1; the batch's largest: exactly 1)
 * and "the slot carries weights" is set: sactd3_update_qnets runs its weighted graph.  Three launches (draw, weights, staging), no copy
 * command, no host wait.  T == 0 (every priority 0): every row is stored as a refused row (ring slot -1, weight 0) and counted in
 * sactd3_priority_stats; never a fault.  SACTD3_ESTATE if priorities are not enabled or the ring is empty; SACTD3_EINVAL for a
 * negative or non-finite beta. */
int sactd3_rb_sample_prioritized(sactd3_engine* e, float beta);
/* Injected uniforms for parity tests, like sactd3_set_noise: host array, n == batch_size, clamped into [0, 1), sticky; the draw counter
 * stands still while they are in use.  u == NULL: back to the native draws. [sync] */
int sactd3_prio_set_uniforms(sactd3_engine* e, const float* u, int n);
/* The write-back for the rows in the batch slot from the critic update that just ran on them (preconditions of
 * sactd3_td_errors_device, SACTD3_ESTATE otherwise): p = max_k |Q_k - y| + eps, leaf[slot] = p^alpha (alpha == 1: p itself, no pow),
 * max priority = max(max priority, p).  Rows with ring slot -1 are skipped; a non-finite TD error leaves its leaf untouched; both are
 * counted (sactd3_prio_stats).  Where a slot occurs several times in the batch the occurrence at the highest batch position wins --
 * decided by position, not by which store lands last.  One launch, one workgroup per batch row; no host wait.  Invisible to the
 * uniform sampler and the fused paths: a precomputed opening pair of sactd3_step_period stays valid.
 * Known and accepted: a row an append overwrote between its draw and this call receives the stale TD error's priority. */
int sactd3_prio_update_from_td(sactd3_engine* e);
/* The same write-back for caller-supplied DEVICE arrays (idx[i * idx_ld] the ring slot, prio[i * prio_ld] the UNSCALED priority), any
 * n >= 1.  A priority >= 0 and finite is taken as given (no eps is added; 0 excludes the row from the draws).  A negative, NaN or
 * infinite priority or an index outside [0, sactd3_rb_len) is refused: it never becomes an address, the leaf stays untouched, the row
 * is counted.  Same duplicate rule.  Each workgroup walks all n rows: meant for batches, not for whole rings.
 * flags & SACTD3_SRC_ORDERED as sactd3_load_batch_device.  SACTD3_EINVAL (NULL or non-device pointers, n < 1, a stride below 1, an
 * unknown flag) leaves the engine usable; SACTD3_ESTATE if priorities are not enabled. */
int sactd3_prio_update_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* prio, int64_t prio_ld, int n,
                              void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* [sync] out = {prioritised samples, write-backs, rows a write-back refused (counted on the device), rows that entered at the maximum
 * priority (sactd3_prio_enable's included)} */
int sactd3_prio_stats(sactd3_engine* e, int64_t out[4]);

/* ---- n-step returns staged in the engine: the batch slot receives, per row, a chain of up to `steps` consecutive ring rows of one env,
 * gathered and summed by ONE launch (k_batch_from_index_nstep), in place of 2n + 1 read-out launches, torch arithmetic and a
 * sactd3_load_batch_device.  No critic kernel changes: every form of the Bellman target is rw + (1 - dn) * gamma * q', so staging
 * rw = sum_j gamma^j r_j and dn = 1 - (1 - d_last) * gamma^(k-1) makes each of them compute the k-step target.
 * Inputs per batch row: a start slot i0; `steps` in [1, 16]; `stride` >= 1 = the rows appended per env step (the env count, or for
 *   shared replay the all-gathered row count); the host's ring state at the call: len, cursor, cap (capacity).
 * Age and chain slots: age(i) = i while len < cap, else (i - cursor) mod cap.  slot_j = (i0 + j * stride) mod cap.  slot_j exists iff
 *   age(i0) + j * stride < len.  This is right for any cap, also when cap % stride != 0, and makes the newest `stride` rows
 *   successor-less without looking at data.
 * Link j -> j+1 holds iff all three are true: slot_{j+1} exists; the flag float of slot_j is 0; the first ob_dim floats of the s' field
 *   of slot_j equal, as 32-bit patterns, the first ob_dim floats of slot_{j+1}'s record (the action columns and zero pad that share the
 *   last chunk are not compared; -0.0 and +0.0 differ; equal NaN patterns are equal).  This is "row t+1 continues row t" without a new
 *   ring field: Rollout / DeviceRollout store the true final observation as next_observations of a truncated row, and the env's
 *   following row starts from the reset observation.
 * Chain length: k = 1 + the number of leading links that hold, 1 <= k <= steps.
 * Staged into batch slot 0: X = the [s|a] chunks of slot_0, as k_batch_from_index writes them; Xn = the s' chunks of slot_{k-1}; the
 *   slot index = i0; rew = R_{k-1} with R_0 = r_0, G_0 = 1, G_j = G_{j-1} * gamma, R_j = R_{j-1} + G_j * r_j -- each operation one
 *   correctly rounded fp32 operation in this order, no fma contraction, so a float32 numpy loop gives the same bits;
 *   done = 1 - (1 - d_{k-1}) * G_{k-1}, which is d_0 exactly when k = 1.  Weights exactly as sactd3_rb_sample_indices_device stages them.
 * Two per-slot int32 arrays, made at the first n-step call (an engine that never makes one holds nothing more than before):
 *   nstep_k[b] = k and nstep_last[b] = slot_{k-1}; read with sactd3_nstep_info_device.
 * Refused rows: a start index outside [0, len) is refused as k_batch_from_index refuses it -- a zero record, slot -1, weight 0, k = 0,
 *   last = -1, counted -- and never becomes an address; nor does a chain slot that does not exist.  A bad weight (negative, NaN,
 *   infinite) is stored as 0 and the row counted as refused, its chain staged all the same, as sactd3_rb_sample_indices_device does.
 *   An accepted row whose chain was cut short (k < steps) is counted too, once per row and call, on the device.
 * For SAC this is the plain n-step target R + gamma^k (min Q' - alpha logp'): the entropy terms of the intermediate steps are NOT added.
 * Read-outs: sactd3_read_batch / _device are unchanged; on an n-step slot they report rewards = the n-step return, next_observations =
 *   the bootstrap state s' of slot_{k-1}, and dones = (mask != 0).  For k > 1 that `dones` is NOT the termination flag (the mask
 *   1 - (1 - d) gamma^(k-1) is non-zero for every chain longer than one row); the mask is exactly 1.0 iff the chain's last row terminated.
 * "Slot 0 is an n-step slot" is host state next to the weighted flag: the three staging calls set it; every other refill of the slot and
 *   every sactd3_step* clears it (the fused paths keep their own 1-step uniform gather inside their graphs; sactd3_step_sampled with
 *   n_step > 1 stages chains inside its graph and sets it).  The three calls break the run-ahead chain and make slot 0 current, exactly as their 1-step counterparts do; a call of
 *   these five that is refused (any SACTD3_EINVAL / SACTD3_ESTATE above) has changed nothing, the run-ahead chain included. */
/* sactd3_rb_sample_indices_device with the chain: same pointer, stride, flag and error rules; in addition SACTD3_EINVAL for `steps`
 * outside [1, 16] or `stride` < 1.  One launch.  With steps == 1 it leaves, bit for bit, what sactd3_rb_sample_indices_device leaves. */
int sactd3_rb_sample_nstep_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* w, int64_t w_ld, int n, int steps,
                                  int stride, void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* The engine's own uniform draw: the start slots are those sactd3_rb_sample would draw at the same sample counter
 * (philox_index(seed, sample_ctr, b, len)); the counter advances once, as it does there.  The slot carries no weights. */
int sactd3_rb_sample_nstep(sactd3_engine* e, int steps, int stride);
/* sactd3_rb_sample_prioritized with the chain: k_prio_draw, k_prio_weights, then the n-step staging kernel in place of
 * k_batch_from_index.  Same preconditions.  sactd3_prio_update_from_td afterwards writes to the START slots, unchanged. */
int sactd3_rb_sample_prioritized_nstep(sactd3_engine* e, float beta, int steps, int stride);
/* k[b * k_ld] = nstep_k[b], last[b * last_ld] = nstep_last[b], DEVICE int32 arrays in the memory of the engine's device; either pointer
 * may be NULL, but not both.  One launch on the learner stream; flags & SACTD3_DST_ORDERED orders the arrays against `caller_stream` as
 * sactd3_td_errors_device does.  SACTD3_ESTATE unless batch slot 0 was filled by an n-step call and not refilled since. */
int sactd3_nstep_info_device(sactd3_engine* e, int32_t* k, int64_t k_ld, int32_t* last, int64_t last_ld, void* caller_stream,
                             int flags /* SACTD3_DST_ORDERED */);
/* [sync] out = {n-step stagings, rows staged, rows cut short (k < steps), rows refused}; the last two are counted on the device */
int sactd3_nstep_stats(sactd3_engine* e, int64_t out[4]);

/* ---- prior data under an online run (RLPD, Ball et al. 2023: a fixed share of every batch from a dataset that is never evicted, LayerNorm
 * critics, several updates per env step).  Not in the reference.  Two pieces: a pinned prefix of the ring, and a draw that takes m batch
 * rows from it and B - m from the rows behind it.  Nothing above changes: an engine that never pins or mixes holds nothing more and
 * launches nothing more than before.
 * sactd3_rb_pin: slots [0, n) become rows no append overwrites.  Allowed while the ring has never overwritten a row (host state),
 * 0 <= n <= sactd3_rb_len and n < rb_capacity; it may be called again under the same conditions, n == 0 unpins.  Refused with nothing
 * changed: SACTD3_EINVAL for n out of range; SACTD3_ESTATE once the ring has wrapped (the live region included), and while priorities
 * are enabled.  With P = the pinned count > 0 every append path (sactd3_rb_extend, _extend_device, _extend_fields_device) goes
 * round-robin over [P, cap): the cursor wraps to P, not to 0; sactd3_rb_len still saturates at cap; an append of more than cap - P rows
 * keeps the last cap - P (as one of cap or more rows keeps the last cap today).  The ingest kernels are the same: they are told the ring
 * advanced by P records, the cursor less P and the capacity cap - P.  The device's ring length and cursor keep their absolute meaning.
 * Unchanged on a pinned ring: sactd3_rb_sample, sactd3_step*, sactd3_rb_sample_with_indices, the read-outs, sactd3_qvalues* -- every
 * slot below sactd3_rb_len holds a row, and they draw over all of them.
 * Out of scope for now, SACTD3_ESTATE while P > 0: sactd3_prio_enable, the three n-step staging calls (sactd3_rb_sample_nstep_device,
 * _nstep, _prioritized_nstep), sactd3_step_sampled with n_step > 1, sactd3_rb_fill_synthetic.  The n-step age formula and the priority
 * refresh assume ONE wrap point, at slot 0; their two-region forms are a later change.
 * Pinning is run-time state: it is not part of a checkpoint. */
int sactd3_rb_pin(sactd3_engine* e, int64_t n);
int64_t sactd3_rb_pinned(const sactd3_engine* e);                          /* the current P */
/* m = `prior_rows`: how many rows of a mixed batch come from the pinned rows.  Host state next to P; the device's copy of both lives in a
 * small struct made at the first mixed draw, and a changed m or P costs one single-thread launch in front of the next graph that reads
 * them (as a changed beta does), never a graph capture.  SACTD3_EINVAL for prior_rows outside [0, batch_size]; whether the ring can
 * serve m is checked where a draw is asked for. */
int sactd3_rb_set_mix(sactd3_engine* e, int prior_rows);
/* rb.sample(batch_size) with a fixed share of prior data.  With w_b the 32-bit Philox word philox_index(seed, sample_ctr, b, .) selects
 * for batch row b (the stream of sactd3_rb_sample: counter words (sample counter, 0, 0x100, b >> 2), word b & 3), len = sactd3_rb_len:
 *     b <  m:  slot = (w_b * P) >> 32                   (a pinned row)
 *     b >= m:  slot = P + ((w_b * (len - P)) >> 32)     (a live row)
 * The sample counter advances once, as in sactd3_rb_sample; with P == 0 and m == 0 the slots ARE those of sactd3_rb_sample, bit for
 * bit.  Batch slot 0 receives the rows and their ring slots, bit for bit what sactd3_rb_sample_indices_device leaves for the same
 * indices; the slot carries no loss weights and sactd3_update_qnets behind it is the unweighted one.  Two launches: the draw (one
 * workgroup; it ticks the counter itself) and k_batch_from_index on an engine-owned int64 index array.  No copy command, no host wait.
 * SACTD3_ESTATE, checked on the host, nothing changed (the run-ahead chain of sactd3_step_period included): an empty ring; m > 0 with
 * P == 0; m < batch_size with no live row (sactd3_rb_len == P).  An accepted call breaks the run-ahead chain and makes slot 0 current. */
int sactd3_rb_sample_mixed(sactd3_engine* e);
/* host counters: out = {mixed draws (sactd3_step_sampled's included), prior rows drawn, live rows drawn, appends that wrapped at the
 * pinned boundary (the cursor came back to P)} */
int sactd3_mix_stats(sactd3_engine* e, int64_t out[4]);

/* ---- hindsight relabelling at staging (hindsight experience replay, Andrychowicz et al. 2017, the "future" strategy): the batch slot
 * receives ring rows whose desired goal was replaced by a goal the same episode achieved at or after the row, with the reward that goal
 * pays -- ONE launch (k_hindsight_stage, csrc/hindsight_kernels.h) in place of a read-out, torch arithmetic and a
 * sactd3_load_batch_device.  The ring needs no episode field: the chain rule of the n-step staging above says where an episode goes on.
 * Config (sactd3_hindsight_configure, host state): the achieved goal is floats [ag_off, ag_off + goal_dim) of an observation, the desired
 *   goal floats [dg_off, dg_off + goal_dim); `window` in [1, 64] rows a goal may lie ahead (the env's horizon); `stride` >= 1 the rows
 *   appended per env step; `threshold` thr; `ratio` in [0, 1] the share of rows relabelled.
 * Rule for batch row b with start slot i0 (age, slot_j, "exists" and "link j -> j+1 holds" exactly as for the n-step staging):
 *   1. accepted iff 0 <= i0 < len; otherwise refused as k_batch_from_index refuses: a zero record, slot index -1, counted, never an address.
 *   2. L = 1 + the number of leading links that hold among links 0 .. window - 2, so 1 <= L <= window.
 *   3. the draw: Philox counter words (hctr, 0, 0x600, b) keyed by the engine's seed -- stream SACTD3_STREAM_HINDSIGHT, hctr = the native
 *      draws made so far (out[0] of sactd3_hindsight_stats).  Relabelled iff philox_u01(v0) < ratio (philox_u01 lies in (0, 1): ratio 0
 *      relabels nothing, ratio 1 every accepted row); j = (v1 * L) >> 32.  With `choice` given: choice[b] < 0 not relabelled, otherwise
 *      relabelled with j = min(choice[b], L - 1); no draw is made and hctr does not move.
 *   4. the goal = floats [ag_off, ag_off + goal_dim) of the s' field of slot_j, as bits (an intermediate goal is a bit copy; j = 0 is
 *      the row's own arrival, whose reward is 0).
 *   5. staged: X = [s|a] of slot_0 with floats [dg_off, dg_off + goal_dim) of s replaced, Xn = s' of slot_0 with the same floats
 *      replaced, done = the stored flag (not recomputed), slot index = i0, rew = (acc <= thr * thr) ? 0 : -1 with acc the sum over c in
 *      index order of (ag'_c - g_c) * (ag'_c - g_c), ag' the achieved goal in slot_0's own s' -- each operation one fp32 rounding, no
 *      contraction.  A row that is not relabelled receives its record's bits: what k_batch_from_index leaves, reward included.  The
 *      slot carries no weights.
 *   6. two per-slot int32 arrays, made at the first staging call: the offset j (-1: not relabelled or refused) and the goal's ring slot
 *      (-1); read with sactd3_hindsight_info_device.
 *   7. three device counters, one atomic per counted row: rows relabelled, rows refused, rows whose relabelled reward is 0.
 * The graph form: sactd3_step_sampled with SACTD3_DRAW_HINDSIGHT holds the native draw and this staging in the iteration's one graph.
 * Out of scope: hindsight inside the fused graphs (sactd3_step, the period graphs), injected choices inside a graph, priorities, n-step
 *   chains or pinned rows beside it, strategies other than "future", recomputing the flag on success, other reward functions, the
 *   config in checkpoints. */
typedef struct sactd3_hindsight_config {
  int32_t ag_off, dg_off, goal_dim, window, stride;
  float threshold, ratio;
} sactd3_hindsight_config;
/* SACTD3_EINVAL: goal_dim outside [1, 8]; a goal range outside [0, ob_dim) or overlapping the other; window outside [1, 64]; stride < 1;
 * threshold negative or not finite; ratio outside [0, 1] or NaN.  Host state only: no launch, the run-ahead chain stays intact.  A
 * changed config drops the graphs sactd3_step_sampled captured for SACTD3_DRAW_HINDSIGHT (they hold the config by value). */
int sactd3_hindsight_configure(sactd3_engine* e, const sactd3_hindsight_config* cfg);
/* The engine's own uniform draw (k_mix_draw with nothing pinned: the slots sactd3_rb_sample would draw; the sample counter advances
 * once), then the staging launch.  SACTD3_ESTATE: hindsight not configured, rows pinned (the age formula assumes one wrap point), ring
 * empty.  Breaks the run-ahead chain and makes slot 0 current; a refused call has changed nothing. */
int sactd3_rb_sample_hindsight(sactd3_engine* e);
/* ... with the caller's start slots (idx[b * idx_ld], DEVICE int64, n == batch_size) and, optionally, the caller's choices
 * (choice[b * choice_ld], DEVICE int32, NULL: the native draw).  Pointer, stride, flag and error rules of sactd3_rb_sample_indices_device. */
int sactd3_rb_sample_hindsight_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const int32_t* choice, int64_t choice_ld, int n,
                                      void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* offset[b * offset_ld] = j or -1, goal_slot[b * goal_slot_ld] = the goal's ring slot or -1: DEVICE int32 arrays, either may be NULL, not
 * both.  One launch on the learner stream, ordered as sactd3_nstep_info_device orders.  SACTD3_ESTATE unless batch slot 0 was filled by a
 * hindsight staging call and not refilled since. */
int sactd3_hindsight_info_device(sactd3_engine* e, int32_t* offset, int64_t offset_ld, int32_t* goal_slot, int64_t goal_slot_ld,
                                 void* caller_stream, int flags /* SACTD3_DST_ORDERED */);
/* [sync] out = {native draws made (staging calls without `choice`), rows relabelled, rows refused, rows whose relabelled reward is 0};
 * the last three are counted on the device */
int sactd3_hindsight_stats(sactd3_engine* e, int64_t out[4]);

/* rb.sample(batch_size) (orchestrator.py:338): uniform-with-replacement indices from the engine's
 * Philox stream + gather into the engine-owned batch slot. */
int sactd3_rb_sample(sactd3_engine* e);
/* same gather with caller-chosen indices (parity tests: the reference's torch RNG stream is not reproduced) */
int sactd3_rb_sample_with_indices(sactd3_engine* e, const int64_t* idx, int n);
/* a caller-owned batch (what update_qnets(batch) receives in the reference), copied into the batch slot */
int sactd3_load_batch(sactd3_engine* e, const float* obs, const float* actions, const float* rewards,
                      const float* next_obs, const uint8_t* dones, int n);
/* read the batch slot back (any pointer may be NULL) [sync] */
int sactd3_read_batch(sactd3_engine* e, float* obs, float* actions, float* rewards, float* next_obs,
                      uint8_t* dones, int64_t* idx);
/* device-side synthetic fill of rows [0,n) for benchmarks: s,s',r ~ N(0,1), a ~ U(min,max), d ~ Bern(0.01) */
int sactd3_rb_fill_synthetic(sactd3_engine* e, int64_t n, uint64_t seed);

/* ---- noise injection (parity): eps [n, ac_dim] standard normals for `site`; sticky until cleared ---- */
int sactd3_set_noise(sactd3_engine* e, int site, const float* eps, int n);
int sactd3_clear_noise(sactd3_engine* e, int site);   /* site < 0: all sites; back to the native Philox draws */
int sactd3_read_noise(sactd3_engine* e, int site, float* eps, int n);      /* last used draws [sync] */

/* ---- the update path ---- */
int sactd3_update_qnets(sactd3_engine* e);    /* Agent.update_qnets  (agents/agent.py:183-242) on the batch slot */
int sactd3_update_actor(sactd3_engine* e);    /* Agent.update_actor  (agents/agent.py:244-318) on the batch slot */
/* Agent.update_targ_nets (agents/agent.py:320-331); the caller passes its already-incremented counter
 * exactly as the reference reads self.qnet_updates_so_far (orchestrator.py:342,352) */
int sactd3_update_targ_nets(sactd3_engine* e, int64_t qnet_updates_so_far);
/* One whole loop iteration of orchestrator.py:337-352 as ONE graph launch: sample+gather, critic
 * update, (if do_actor) actor_update_delay x actor(+alpha) updates on the same batch, Polyak
 * (subject to crit_targ_update_freq and the engine's own update counter). */
int sactd3_step(sactd3_engine* e, int do_actor);
/* The same iteration with a prioritised draw and / or n-step returns, as ONE graph launch: what the call sequence
 *   sactd3_rb_sample_prioritized[_nstep] (or sactd3_rb_sample_nstep) -> sactd3_update_qnets -> sactd3_prio_update_from_td (prioritised
 *   only) -> do_actor: actor_update_delay x sactd3_update_actor -> sactd3_update_targ_nets(the engine's own update counter + 1)
 * computes, bit for bit, and every host counter and slot state that sequence leaves (sactd3_td_errors_device, sactd3_nstep_info_device,
 * sactd3_read_batch, sactd3_prio_stats, sactd3_nstep_stats work behind it as behind the calls); the engine's update counter advances
 * as in sactd3_step.  The graph is linear and holds, in order: the draw, the staging into batch slot 0, the critic update (weighted
 * when the draw is prioritised), the TD write-back (prioritised only), the actor updates, the target update.  Its staging and
 * priority kernels read the ring length, the cursor, `beta` and the injection switch of sactd3_prio_set_uniforms from device memory:
 * a graph is captured once per (do_actor, target update) for the current (draw, n_step, stride) -- a change of those three drops the
 * captured graphs -- and replayed while the ring grows and `beta` anneals; a changed `beta` or switch costs one single-thread launch
 * in front of the graph.  Uniform with n_step == 1 is sactd3_step itself.  With use_graphs == 0 the same launches are issued eagerly.
 * Refused, with nothing changed: NULL struct, unknown `draw`, n_step outside [1, 16], stride < 1 at n_step > 1, beta negative or
 * not finite (SACTD3_EINVAL); a prioritised draw before sactd3_prio_enable, an empty ring (SACTD3_ESTATE).
 * SACTD3_DRAW_MIXED: the mixed draw of sactd3_rb_sample_mixed (below: prior data under an online run) in place of the uniform one, with
 * the current sactd3_rb_set_mix / sactd3_rb_pin values.  The graph holds, in order: the draw (graph form: it reads the ring length, P
 * and m from device memory, and ticks the sample counter), k_batch_from_index_g, the UNWEIGHTED critic update, the actor updates, the
 * target update; no priority write-back.  Bit for bit, host state included, the call sequence sactd3_rb_sample_mixed ->
 * sactd3_update_qnets -> [sactd3_update_actor x actor_update_delay] -> sactd3_update_targ_nets.  Captured under the same
 * (draw, n_step, stride) key and replayed while the ring grows, the live region wraps and m and P change (a changed m or P costs one
 * single-thread launch in front of the graph).  n_step must be 1 (SACTD3_EINVAL); the refusals of sactd3_rb_sample_mixed apply.
 * SACTD3_DRAW_HINDSIGHT: the native draw and the relabelling of sactd3_rb_sample_hindsight (above) with the current
 * sactd3_hindsight_configure values.  The graph holds, in order: k_hindsight_draw_g (the uniform draw; it reads the ring length from
 * device memory, ticks the sample counter and carries the count of native hindsight draws: a device word it advances and whose old
 * value it leaves for the staging), k_hindsight_stage_g (ring length, cursor and that count from device memory, the config by value),
 * the UNWEIGHTED critic update, the actor updates, the target update; no tick launch, no priority write-back: as many nodes as the
 * SACTD3_DRAW_MIXED graph.  Bit for bit, host state included (the slot is a hindsight slot: sactd3_hindsight_info_device and
 * sactd3_hindsight_stats work behind it), the call sequence sactd3_rb_sample_hindsight -> sactd3_update_qnets -> [sactd3_update_actor x
 * actor_update_delay] -> sactd3_update_targ_nets.  Captured under the same (draw, n_step, stride) key and replayed while the ring grows,
 * fills and wraps; sactd3_hindsight_configure with a CHANGED config drops the captured graphs (the same config again drops nothing); a
 * call-form native draw between two graph launches costs one single-thread launch in front of the next graph.  `beta` is checked and
 * otherwise ignored.  n_step must be 1 (SACTD3_EINVAL); SACTD3_ESTATE: hindsight not configured, rows pinned, an empty ring. */
enum { SACTD3_DRAW_UNIFORM = 0, SACTD3_DRAW_PRIORITIZED = 1, SACTD3_DRAW_MIXED = 2, SACTD3_DRAW_HINDSIGHT = 3 };
typedef struct {
  int32_t draw;      /* SACTD3_DRAW_UNIFORM | SACTD3_DRAW_PRIORITIZED | SACTD3_DRAW_MIXED | SACTD3_DRAW_HINDSIGHT */
  int32_t n_step;    /* 1 .. 16 */
  int32_t stride;    /* rows between two steps of one env; ignored at n_step == 1 */
  float beta;        /* exponent of the importance weights; ignored by the uniform draw (but checked) */
} sactd3_sampling;
int sactd3_step_sampled(sactd3_engine* e, int do_actor, const sactd3_sampling* sampling);
/* out = {sactd3_step_sampled calls issued, graphs captured for them, 0, 0} */
int sactd3_step_sampled_stats(sactd3_engine* e, int64_t out[4]);
/* actor_update_delay + 1 consecutive iterations of orchestrator.py:337-352 -- the first with the actor updates, the others
 * critic-only: one period of the schedule of :345-349 -- as ONE graph launch.  Equal to that many sactd3_step calls, bit for
 * bit.  Needs TD3 or crit_targ_update_freq == 1 (else SACTD3_ESTATE: issue the iterations with sactd3_step).
 * Without gradient clipping (clip_norm <= 0) a period -- and sactd3_step_prefix -- does not store what only inspection reads: the
 * gradient arenas and the first layers' dz1.  sactd3_debug_read of "grad_critics" / "c_dz1" and "grad_actor" / "a_dz1" then fails
 * with SACTD3_ESTATE until a call that writes that family again: sactd3_update_qnets or any sactd3_step (critics),
 * sactd3_update_actor or sactd3_step with actor updates (actor). */
int sactd3_step_period(sactd3_engine* e);
/* The first m iterations of a period (1 <= m <= actor_update_delay: the one with the actor updates + m - 1 critic-only ones) as ONE
 * graph launch -- what a run of iterations leaves behind its last whole period (orchestrator.py:337-352 with a number of
 * iterations that is not a multiple of the period).  Equal to sactd3_step(e, 1) followed by m - 1 sactd3_step(e, 0), bit for bit.
 * Same preconditions as sactd3_step_period. */
int sactd3_step_prefix(sactd3_engine* e, int m);
/* k >= 1 whole periods: equal to k sactd3_step_period calls -- k * (actor_update_delay + 1) sactd3_step calls -- bit for bit, host
 * state included.  Where the period graph has its pipelined form, runs of R consecutive periods go out as ONE graph launch (R: an even
 * build constant, 2 as shipped, at most 8; the node sequence of a run is that of R period graphs one behind the other, no kernel and no launch
 * argument differs), so the idle time between two graph replays is paid once per R periods; what is left of k below R goes out as
 * single period graphs.  Elsewhere the k periods go out as k plain period graphs; with use_graphs == 0 the same launches are issued eagerly.
 * It writes the actor parameters (see sactd3_predict_begin), and it acts with the updated ones: a sactd3_predict or a
 * sactd3_predict_begin behind it waits for every launch the call issued, a whole run of R periods at the least -- R times the acting
 * latency behind one sactd3_step_period.  A loop that acts every iteration issues its iterations with sactd3_step, as before.
 * SACTD3_EINVAL: k < 1.  SACTD3_ESTATE as for sactd3_step_period (empty buffer; SAC with crit_targ_update_freq != 1).  A refused
 * call changes nothing. */
int sactd3_step_periods(sactd3_engine* e, int k);
/* out = {sactd3_step_periods calls, run-graph launches, single-period launches made inside those calls, run graphs captured} */
int sactd3_step_periods_stats(sactd3_engine* e, int64_t out[4]);
/* Capture and instantiate the hipGraphs of sactd3_step / sactd3_step_period / sactd3_step_periods now rather than at their first use (the reference's
 * CudaGraphModule captures after a warm-up inside the loop, orchestrator.py:313-315); nothing is launched, no state changes. */
int sactd3_instantiate_graphs(sactd3_engine* e);
/* Agent.predict (agents/agent.py:172-181): obs [n, ob_dim] host -> actions [n, ac_dim] host.  Stream-ordered behind whatever
 * update was issued before it (it acts with the updated parameters, as the reference does) and returns when ITS kernels have
 * finished: [sync] in that sense -- with at most 4 rows (16 for wide heads) the wait is a spin on a pinned host word the last
 * kernel publishes, otherwise a stream synchronisation. */
int sactd3_predict(sactd3_engine* e, const float* obs, int n, int explore, float* actions);
/* Agent.predict in two halves, so that the update issued in between (orchestrator.py:337-352) overlaps with it: the same acting
 * launches as sactd3_predict -- same kernels, same arguments, same (explore, n) graph, or the eager sequence with use_graphs == 0 --
 * on a second, ACTING stream (hipStreamNonBlocking, created with its two events at the first sactd3_predict_begin: an engine that never
 * calls it holds nothing more than before).  `begin` stages `obs`, issues the launches and returns; `end` waits for THOSE kernels
 * only (the pinned-word spin of sactd3_predict for single-block tails, bounded, then a synchronisation of the acting stream) and
 * copies the actions [n, ac_dim] out.  The result is, bit for bit, what sactd3_predict would have returned at the position of
 * `begin` in the call sequence, the native exploration draw included (its counter advances once per call, whichever entry point).
 * Order between the two streams is decided on the host and kept with events, only where the acting kernels (which read the actor
 * parameters, the action bounds, their own scratch and their own control words) meet a learner call:
 *   learner -> acting: if a call that writes the actor parameters was issued on the learner stream since the acting stream last
 *     waited for it (sactd3_update_actor, sactd3_step with actor updates, sactd3_step_period, sactd3_step_periods, sactd3_step_prefix,
 *     sactd3_set_params(ACTOR), sactd3_time_nodes), or a sactd3_predict_device call (its queued kernels use the acting scratch), or if flags has SACTD3_ACT_AFTER_ALL, `begin` makes the acting stream wait for
 *     everything issued on the learner stream so far -- as sactd3_predict does.  Otherwise it waits for nothing: behind a
 *     critic-only iteration the action comes from the same parameters either way.
 *   acting -> learner: while a call is in flight (begun, not ended) the first of the calls above makes the learner stream wait for
 *     the acting kernels, so the actor is not overwritten under a running predict.  After `end` nothing is inserted.
 *   Critic-only sactd3_step, sactd3_update_qnets, sactd3_update_targ_nets, sactd3_rb_* neither wait nor are waited for.
 * A period graph (sactd3_step_period / _prefix) contains actor updates, so a `begin` behind one waits for all of it -- behind
 * sactd3_step_periods for the whole run: the overlap pays with single-iteration sactd3_step loops.
 * One call in flight at most.  While one is, a second `begin`, sactd3_predict, and sactd3_set_noise / _clear_noise / _read_noise on
 * SACTD3_SITE_PREDICT return SACTD3_ESTATE; so does `end` without a `begin`.  sactd3_sync and sactd3_destroy drain the acting
 * stream too (after sactd3_sync the call is still to be collected with `end`). */
#define SACTD3_ACT_AFTER_ALL 1   /* flags: order behind everything issued so far, as sactd3_predict does */
int sactd3_predict_begin(sactd3_engine* e, const float* obs, int n, int explore, int flags);
int sactd3_predict_end(sactd3_engine* e, float* actions);          /* waits for ITS kernels only */
/* host counters of the ordering policy: out = {calls begun, begins that made the acting stream wait for the learner, learner calls
 * that waited for an acting call in flight, calls ended by the pinned-word spin} */
int sactd3_acting_stats(const sactd3_engine* e, int64_t out[4]);

/* ---- acting for an environment that lives on the GPU: Agent.predict (agents/agent.py:172-181) with the observations where a batched
 * simulator, a learned world model or a torch-written env left them, and the actions left where its next step reads them.
 * `obs` [n, ob_dim] and `actions` [n, ac_dim] are DEVICE pointers in the memory of the engine's device, each with a row stride in elements
 * (>= the width), a contiguous inner dimension and no alignment beyond 4 bytes; 1 <= n <= max_envs.  The call launches on the learner
 * stream and returns: no copy command, no wait, spin or synchronisation on the host.  One kernel packs the rows into the zero-padded layout
 * the trunk reads, the acting pair of sactd3_predict runs on engine-owned device buffers (captured once per (explore, n); the eager
 * sequence with use_graphs == 0), one kernel writes the [n, ac_dim] window of `actions` and nothing outside it.
 * Like sactd3_predict it is stream-ordered behind every update issued before it and acts with the updated parameters; its result is,
 * bit for bit, what sactd3_predict returns for the same rows at the same position in the call sequence, the native exploration draw
 * included: host and device calls may be mixed and share one noise stream (one counter tick per call, whichever entry point).  It
 * reads the actor parameters, the action bounds, the acting control words and its own scratch only: a precomputed opening pair of
 * sactd3_step_period stays valid across it, as across sactd3_predict.
 * flags & SACTD3_SRC_ORDERED orders both arrays against `caller_stream` (a hipStream_t; NULL = the legacy default stream) on the GPU, as
 * sactd3_load_batch_device does for its sources: the learner stream waits for what the caller has queued there so far, and
 * `caller_stream` then waits for an event recorded behind the last launch -- the caller may read `actions` on its stream at once, and a
 * later overwrite of `obs` there cannot overtake the read.  Without the flag nothing is inserted: the caller has synchronised, and
 * leaves both arrays alone until sactd3_sync.
 * SACTD3_EINVAL: a NULL pointer, a stride below the width, n out of range, a pointer that is not memory of the engine's device, an
 * unknown flag.  SACTD3_ESTATE while a sactd3_predict_begin call is in flight (it shares the exploration counter, the draw buffer and
 * the acting scratch with that call).  The other way round the engine orders the streams itself: this call returns with its kernels
 * queued, so the next sactd3_predict_begin makes the acting stream wait for the learner stream, as it does behind an actor update. */
int sactd3_predict_device(sactd3_engine* e, const float* obs, int64_t obs_ld, int n, int explore,
                          float* actions, int64_t actions_ld, void* caller_stream, int flags);
/* host counters: out = {calls, rows, calls that inserted event waits, calls that took a multi-block tail} */
int sactd3_predict_device_stats(const sactd3_engine* e, int64_t out[4]);

/* ---- scoring state-action pairs on the device: Agent.batched_qf(params, ob, action) and pi(params, ob) (agents/agent.py:146-163) as a
 * read path -- a forward-only evaluation of the twin critics, online (SACTD3_Q_ONLINE) or target (SACTD3_Q_TARGET), on n >= 1 rows the
 * caller supplies; any n (the engine works through them 1024 rows at a time on its stream).  What a prioritised sampler (|Q(s,a) - y|),
 * an n-step or hindsight relabeller (the value of the state it bootstraps from) or an evaluation (min Q(s, pi(s))) asks of rows it got
 * from sactd3_rb_read_rows_device.
 * `obs` [n, ob_dim], `actions` [n, ac_dim] and `q` are DEVICE pointers in the memory of the engine's device, each with a row stride in
 * elements (>= the width), a contiguous inner dimension and no alignment beyond 4 bytes.  Q_k(obs_i, actions_i) of critic k is stored to
 * q[k * q_ns + i * q_ld] (q_ld, q_ns >= 1; a contiguous [2, n] array: q_ld = 1, q_ns = n) and nothing else of `q` is written.
 * actions == NULL: the pairs are (s, pi(s)), pi(s) = the ONLINE actor's exploit action -- what sactd3_predict(explore = 0) returns --
 * whichever critics `which` names (SAC: tanh(mean); TD3: actor(s)).
 * The launches go on the learner stream, eagerly, stream-ordered behind every update issued before the call (it scores with the updated
 * parameters); no copy command, no wait or synchronisation on the host.  flags & SACTD3_SRC_ORDERED orders all three arrays against
 * `caller_stream` exactly as sactd3_predict_device does.  A row's two values are the same bits whatever n is and whichever rows are
 * scored with it: the hidden layers run in one pinned launch shape (the K split of the B < 1024 update kernels), the head is the
 * forward third of the critic update's tail, so a row is scored with the arithmetic the engine trains with.
 * The call is invisible to training: it writes its own scratch (made at the first call) and its own counters only -- no batch slot, no
 * noise buffer, no acting scratch, no sample / noise / predict counter, and a precomputed opening pair of sactd3_step_period stays
 * valid across it.  It is therefore allowed while a sactd3_predict_begin call is in flight.
 * SACTD3_EINVAL, before anything is launched: a NULL `obs` or `q`, n < 1, a stride below the width, `which` other than the two values,
 * an unknown flag, a pointer that is not memory of the engine's device; the engine stays usable. */
#define SACTD3_Q_ONLINE 0
#define SACTD3_Q_TARGET 1
int sactd3_qvalues_device(sactd3_engine* e, const float* obs, int64_t obs_ld, const float* actions, int64_t actions_ld, int n, int which,
                          float* q, int64_t q_ld, int64_t q_ns, void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* The same for host arrays: obs [n, ob_dim], actions [n, ac_dim] or NULL, q [2 * n] (critic-major), through device staging of the
 * engine's own; bit for bit the values of the device call.  [sync] */
int sactd3_qvalues(sactd3_engine* e, const float* obs, const float* actions, int n, int which, float* q);
/* host counters: out = {calls, rows, calls that inserted event waits, calls in the policy form (actions == NULL)} */
int sactd3_qvalues_stats(const sactd3_engine* e, int64_t out[4]);

/* ---- querying the policy on the device: the actor as a read path, beside ring rows (sactd3_rb_read_rows_device), Q-values
 * (sactd3_qvalues_device) and TD errors (sactd3_td_errors_device).  For n >= 1 rows of observations the caller supplies, any n (worked
 * through 1024 rows at a time on the learner stream: pack, the actor trunk in the pinned launch shape of sactd3_qvalues_device, one head
 * kernel), whichever of these the caller asks for (float32, one rounding per written operation; sc / bi = action scale / bias):
 *   mode         SAC tanh(mean) sc + bi, TD3 actor(s) -- the exploit action, the bits sactd3_predict(explore = 0) computes from the same
 *                trunk output; any n, not only max_envs
 *   mean, log_std   the pre-squash mean and log_std = -5 + 3.5 (tanh(raw) + 1) of the SAC head
 *   sample, sample_logp   y sc + bi with y = tanh(mean + e exp(log_std)) and its log-density, e from `eps`, or -- eps == NULL -- from a
 *                Philox stream of the call's own: counter words (policy_ctr, 0, 0x400, element >> 2), element = row a + j,
 *                philox_normal's construction; policy_ctr is a device word of this feature that advances once per call that draws
 *                natively.  No training or acting counter moves.  eps_out receives the draws used.
 *   action_logp  log pi(actions_i | obs_i) through the inverse squash: v = (g - bi) / sc, c = clamp(v, -M, M), M = float32(1 - 1e-6),
 *                x = 0.5 (logf(1 + c) - logf(1 - c)), sum_j [-(x - mean)^2 / (2 sd^2) - logf(sd) - 0.9189385 - logf(sc (1 - c c) + 1e-6)].
 *                A row with a component outside [-M, M] is clamped and counted; a row with a NaN component gets a quiet NaN and is
 *                counted; neither is an error and neither touches another output or row.
 * Every pointer of sactd3_policy_io is a DEVICE pointer in the memory of the engine's device with a row stride in elements (>= the
 * width), a contiguous inner dimension and 4-byte alignment; NULL = not given / not wanted, and a NULL output costs no store.  Each
 * output is written inside its [n, width] window only.  TD3 knows `mode` alone (every other field NULL), from the online actor or
 * -- SACTD3_PI_TARGET -- the target actor.
 * Launch semantics are those of sactd3_qvalues_device: eager launches on the learner stream, ordered behind every update issued before
 * the call, no copy command and no host wait; flags & SACTD3_SRC_ORDERED orders every given array against `caller_stream` in both
 * directions.  A row's outputs are the same bits whatever n is.  The call is invisible to training and acting: scratch and control
 * words of its own (made at the first call), no batch slot, no noise buffer, no acting scratch, no sample / noise / predict counter;
 * a precomputed opening pair of sactd3_step_period stays valid, and the call is allowed while a sactd3_predict_begin call is in flight.
 * SACTD3_EINVAL, before anything is launched and with the engine left usable: NULL `obs` or `io`, n < 1, no output set, action_logp
 * without actions, eps or eps_out while neither sample nor sample_logp is wanted, a stride below the width, a pointer that is not memory
 * of the engine's device, an unknown flag, `which` outside the two values, SACTD3_PI_TARGET on SAC, a SAC-only field on TD3. */
#define SACTD3_PI_ONLINE 0
#define SACTD3_PI_TARGET 1            /* TD3 only */
typedef struct sactd3_policy_io {     /* device pointers; NULL = not given / not wanted; *_ld = row stride in elements */
  const float* actions; int64_t actions_ld;   /* in : [n, a] actions to score            (SAC)            */
  const float* eps;     int64_t eps_ld;       /* in : [n, a] standard normals for `sample` (SAC; NULL: native) */
  float* mode;        int64_t mode_ld;        /* out: [n, a]                                               */
  float* mean;        int64_t mean_ld;        /* out: [n, a] pre-squash mean               (SAC)           */
  float* log_std;     int64_t log_std_ld;     /* out: [n, a]                               (SAC)           */
  float* sample;      int64_t sample_ld;      /* out: [n, a]                               (SAC)           */
  float* sample_logp; int64_t sample_logp_ld; /* out: [n]                                  (SAC)           */
  float* action_logp; int64_t action_logp_ld; /* out: [n], needs `actions`                 (SAC)           */
  float* eps_out;     int64_t eps_out_ld;     /* out: [n, a] the draws `sample` used       (SAC)           */
} sactd3_policy_io;
int sactd3_policy_device(sactd3_engine* e, const float* obs, int64_t obs_ld, int n, int which,
                         const sactd3_policy_io* io, void* caller_stream, int flags /* SACTD3_SRC_ORDERED */);
/* The same for host arrays, all contiguous ([n, a] / [n]; the *_ld fields are not read), staged a chunk at a time through device
 * buffers of the engine's own; bit for bit the values of the device call.  [sync] */
int sactd3_policy(sactd3_engine* e, const float* obs, int n, int which, const sactd3_policy_io* host_io);
/* out = {calls, rows, rows clamped, rows with a NaN action}; the last two are counted on the device.  [sync] */
int sactd3_policy_stats(sactd3_engine* e, int64_t out[4]);

/* ---- TD3+BC (Fujimoto & Gu 2021): the behaviour-cloning actor term that lets the TD3 engine train on a FIXED dataset -- the workload
 * of the run-ahead modes (sactd3_step_period / sactd3_step_periods), which no ring append interrupts.  An engine created with
 * sactd3_config::bc_alpha > 0 (TD3 only: SACTD3_EINVAL with prefer_td3_over_sac == 0; NaN, infinite or negative: SACTD3_EINVAL) runs
 * sactd3_update_actor, in every entry point that contains it, on the loss
 *     lambda  = bc_alpha / max(mean_b |q_b|, 1e-8)                   q_b = Q1(s_b, pi_b), online critic 1; lambda is a constant of the backward pass
 *     bc      = (1 / (B A)) sum_b sum_j (pi_bj - a_bj)^2             pi = actor(s), a_b = the action stored in the batch slot, A = ac_dim
 *     L_actor = -lambda mean_b q_b + bc_weight bc
 *     dL/dpi_bj = lambda (-1/B) dq_b/da_j + bc_weight 2 (pi_bj - a_bj) / (B A)
 * (bc_weight = 1 and bc_alpha = 2.5 are the paper's form.)  The 1e-8 floor is this engine's own guard, not the paper's: a batch whose
 * q are all 0 must not poison a parameter.  Nothing else of the update changes: critic update, smoothing noise, Polyak, clip_norm, the
 * loss weights (actor updates stay unweighted) and n-step staging are as before, and so is every graph's node count -- the term lives
 * in BC forms of the head-backward launch and of the launch that finalises the actor loss; an engine with bc_alpha == 0 launches
 * exactly the kernels it launched before.  Metrics: SACTD3_M_ACTOR_LOSS = L_actor, SACTD3_M_BC_LOSS = bc (unweighted),
 * SACTD3_M_BC_LAMBDA = lambda; an engine without BC never writes the last two.  Normalising the dataset's states (the paper does) is
 * the caller's business: the engine trains on the rows it is given.
 * sactd3_set_bc: new (bc_alpha > 0, bc_weight >= 0), both finite, else SACTD3_EINVAL with nothing changed; SACTD3_ESTATE on an engine
 * created with bc_alpha == 0 (the kernel forms are chosen at create).  Both values live in device memory beside the other control
 * words and are read there by the kernels: a change costs one single-thread launch on the learner stream, never a graph capture, and
 * does not break the run-ahead chain of sactd3_step_period(s) (nothing that ran ahead depends on them).  bc_weight starts at 1 and is
 * run-time state: not part of sactd3_config. */
int sactd3_set_bc(sactd3_engine* e, float bc_alpha, float bc_weight);
int sactd3_get_bc(sactd3_engine* e, float out[2]);                         /* (bc_alpha, bc_weight) as the device holds them [sync] */

int sactd3_read_metrics(sactd3_engine* e, float out[SACTD3_NUM_METRICS]);  /* [sync] */
/* The engine's HIP stream (hipStream_t) and the DEVICE address of the metrics slots, for callers that want the values the
 * way the reference hands them out -- 0-dim device tensors that are only materialised at evaluation time (agents/agent.py:
 * 238-242,305-311; orchestrator.py:341,348,383): wrap `metrics + SACTD3_M_*` as a tensor and order the consumer's stream
 * after `stream` (the Python mirror does both with torch).  The memory is owned by the engine and overwritten by later updates. */
int sactd3_device_handles(sactd3_engine* e, void** stream, float** metrics);
int sactd3_sync(sactd3_engine* e);                                          /* [sync] */

/* ---- introspection for tests / profiling (not part of the reference surface) ---- */
/* copy a named internal device buffer to the host; returns the number of floats it holds (or < 0).
 * With dst == NULL only the size is returned. Names: see sactd3_debug_names(). [sync]
 * "a_h2", "a_xh2" [B][256], "a_rs2" [B] and "a_tg" [B][4][a4] (a4 = ac_dim rounded up to 4; per row tanh(raw log-std), std and the
 * squashed sample y at offsets 0, a4 and 2 a4; TD3: tanh(mean) at offset 0) are what the last policy pass stored for the head backward.
 * "grad_critics", "c_dz1", "grad_actor", "a_dz1": SACTD3_ESTATE while the family's last writer was a period / cut-short period
 * graph, which leaves them out (see sactd3_step_period) -- stale gradients are not handed out.
 * "prio_leaf" [rb_capacity], "prio_sums" (the level above the leaves: one sum per 1024 slots), "prio_max" [1] and "prio_weights"
 * [batch_size] (the loss weights batch slot 0 carries, whichever call staged them): SACTD3_ESTATE before sactd3_prio_enable.
 * "pi_z2" [m][256]: the actor trunk's output for the last chunk (m <= 1024 rows) of the last sactd3_policy* call, what its head kernel
 * read; SACTD3_ESTATE before the first such call. */
int64_t sactd3_debug_read(sactd3_engine* e, const char* name, float* dst, int64_t max_floats);
const char* sactd3_debug_names(void);
/* number of kernel nodes in the instantiated graph of: 0 update_qnets, 1 update_actor, 2 step(do_actor=0), 3 step(do_actor=1), 4 step_period,
 * 5 the opening graph of a period that cannot use a precomputed opening pair, 6 / 7 step_prefix(1) / step_prefix(2),
 * 8 update_qnets in its weighted form (0 until its first use; the same count as 0),
 * 10 the run graph of sactd3_step_periods (R times the count of 4; 0 until captured; 9 names no graph),
 * 16 + 2 do_actor + (1 with the target update): sactd3_step_sampled's graphs for its current (draw, n_step, stride), 0 until captured */
int sactd3_graph_kernel_count(sactd3_engine* e, int which_graph);
/* average device time in microseconds of `iters` back-to-back launches of one kernel of the path,
 * measured with hipEvents on the engine's stream: "gather" (a fresh index draw per launch), "polyak", "trunk_critics" (the 4-net
 * hidden-layer launch of update_qnets; on wide inputs it is two launches), "batch_from_fields" / "rb_ingest_fields" (the device-boundary
 * pack kernels on batch_size / max_envs rows of the engine's own staging slab; they overwrite the batch slot / append to the ring),
 * "obs_from_field" / "act_to_field" (the pack / unpack kernels of sactd3_predict_device on max_envs rows of engine-owned memory),
 * "batch_to_fields" / "rows_to_fields" (the read-out kernels of sactd3_read_batch_device / sactd3_rb_read_rows_device on batch_size rows,
 * written into the engine's own staging slab; the rows kernel takes its indices from the current slot's, widened to int64),
 * "sa_from_fields" / "q_head" (the pack / head kernels of sactd3_qvalues_device on 1024 rows of the scoring scratch, [s | a] read from
 * the ring's records), "batch_from_index" / "td_to_field" (the staging and TD read-out kernels of sactd3_rb_sample_indices_device /
 * sactd3_td_errors_device on batch_size rows: indices as for "rows_to_fields", no weights, into the batch slot; the TD errors into the
 * engine's own staging slab), "prio_sample" / "prio_update" (SACTD3_ESTATE before sactd3_prio_enable: one whole
 * sactd3_rb_sample_prioritized with beta 0.4 -- its three launches, the batch slot overwritten, the draw counter advanced -- / the
 * write-back kernel on batch_size rows, indices as for "rows_to_fields", every priority 1: those rows' priorities are overwritten),
 * "batch_from_index_nstep" (the staging kernel of sactd3_rb_sample_nstep_device on batch_size rows with steps = 3, stride = 1: indices
 * as for "rows_to_fields", no weights, into the batch slot), "mix_draw" (the draw kernel of sactd3_rb_sample_mixed alone, with the current
 * P and m: the sample counter advances, the batch slot stays; SACTD3_ESTATE where sactd3_rb_sample_mixed is refused), "pi_head" (the head
 * kernel of sactd3_policy_device alone on 1024 rows of that call's scratch, every output wanted and written to the scratch, native
 * draws; its counters are not touched). [sync] */
int sactd3_time_kernel(sactd3_engine* e, const char* kernel, int iters, float* usec);
/* Per-node device time of one fused iteration (sactd3_step with this do_actor; do_actor == 2: of one whole period as
 * sactd3_step_period captures it): every kernel launch of the sequence
 * alone, `iters` times back to back between two HIP events on the engine's stream.  Returns the node count n (<= max_nodes)
 * and fills usec[n], flops[n] (2 x MACs of the GEMMs in the launch), bytes[n] (operands + results, each once),
 * threads[n] (grid x block, rocprofv3's Grid_Size); `names` receives n newline-terminated "kernel-instance:role" strings.  Consumes the learner's state (optimiser steps repeat on
 * stale gradients): call it on a scratch engine.  Stands in for nothing in the reference: SURVEY.md 8d measurement. [sync] */
int sactd3_time_nodes(sactd3_engine* e, int do_actor, int iters, int max_nodes, char* names, int names_cap,
                      float* usec, double* flops, double* bytes, int64_t* threads);
/* run the replay gather at an arbitrary batch size (own scratch outputs, rows of the engine's ring): the bandwidth sweep of SURVEY.md 8d [sync] */
int sactd3_time_gather_sweep(sactd3_engine* e, int batch, int iters, float* usec, double* algo_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_H */
