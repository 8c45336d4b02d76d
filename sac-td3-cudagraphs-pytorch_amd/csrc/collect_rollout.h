// What crosses between engine.hip and env.hip for sactd3_rollout_collect (include/sactd3_rollout_collect.h), split as eval_rollout.h splits
// the evaluation rollout: the kernel, k_collect_rollout<KIND> (collect_kernels.h), needs env_step_body and so is compiled in env.hip, which
// holds the entry point; engine.hip gains host code only -- it opens a call (its own refusals, the feature's counter word at first use, the
// rollout's stream in front of the learner's), hands out where the online actor lives, and closes it (the counter tick of a call that drew,
// the rollout's stream behind the learner's, the host counters).  The append between the two is the public sactd3_rb_extend_records_device.
#pragma once
#include "eval_rollout.h"

// EvalActor with its counter word pointing at collect_ctr (rew / lp unused: NULL), and what TD3's exploring action needs besides
struct CollectActor {
  EvalActor A;
  float noise_std;      // sactd3_config::actor_noise_std
};

// ob / ac / device: the env's; rows = steps * n.  Refuses what the engine's side can see -- rows above the ring slots an append may use, an
// acting call in flight; then (no refusal behind this point) the counter word at first use and the rollout's stream in front.
int engine_collect_open(sactd3_engine* e, int ob, int ac, int device, int64_t rows, void* rollout_stream, CollectActor* out);
// behind the launch and the append: the counter tick of a call that drew, the rollout's stream behind the learner's
int engine_collect_close(sactd3_engine* e, int drew, void* rollout_stream);
// out = {host[0], host[1], host[2], collect_ctr}: the rollout's three host counters and the device word (waits for the engine's stream)
int engine_collect_stats(sactd3_engine* e, const int64_t host[3], int64_t out[4]);
