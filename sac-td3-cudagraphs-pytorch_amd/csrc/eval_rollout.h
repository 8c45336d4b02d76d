// What crosses between engine.hip and env.hip for sactd3_eval_rollout (include/sactd3_eval.h).  The kernel, k_eval_rollout<KIND>
// (eval_kernels.h), needs env_step_body of env_kernels.h, and that header defines a plain kernel: it can be part of one translation unit
// only -- so the kernel is compiled where the env kernels are, in env.hip, which also holds the entry point.  engine.hip gains host code
// only: it opens a call (its own refusals, the feature's state at first use, the caller's stream in front), hands out where the online
// actor lives, and closes the call (the counter tick of a call that drew, the caller's stream behind, the host counters).  The engine never
// sees the env handle and env.hip never sees the engine's fields.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct sactd3_engine;

// the online actor where the engine keeps it: offsets in floats inside the parameter block P (kernels.h: NetLayout; W [out][in], row-major)
struct EvalActor {
  const float* P;
  int ld1, W1, b1, g1, be1, W2, b2, g2, be2, Wh, bh;
  int ln, sac;
  const float* scale; const float* bias;       // [ac_dim] action_scale / action_bias
  const float* log_alpha;                      // [1]; NULL for TD3
  const unsigned long long* seed;              // the key of the engine's Philox streams
  const int* eval_ctr;                         // the feature's counter word
  float* rew; float* lp;                       // scratch [T][n] each: rewards and log-probs wait here for the backward pass
  hipStream_t stream;                          // the learner stream
};

// The engine's half of a refusal: the text goes where sactd3_last_error(engine) finds it -> code
int engine_eval_fail(sactd3_engine* e, int code, const char* what);
// ob / ac / device: the env's; rows = T * n.  Refuses what the engine's side can see; then (no refusal behind this point) the feature's state
// at first use and the caller's stream in front of the learner's.
int engine_eval_open(sactd3_engine* e, int ob, int ac, int device, int sample, int soft, int64_t rows, void* caller_stream, int flags, EvalActor* out);
// behind the launch: the counter tick of a call that drew, the caller's stream behind the learner's, the host counters
int engine_eval_close(sactd3_engine* e, int drew, int64_t rows, void* caller_stream, int flags);
int engine_eval_stats(sactd3_engine* e, int64_t out[4]);
