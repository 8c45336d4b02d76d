// Host side of include/sactd3_env.h: the handle, its one device allocation, and one launch per call (csrc/env_kernels.h).
// A translation unit of its own inside libsactd3_hip.so: it shares philox.h with engine.hip and nothing else.
// Behind it, the host side of include/sactd3_rollout.h: the record-emitting env step and the rollout handle, which reaches the
// engine through its public ABI (include/sactd3.h) only -- and, for sactd3_rollout_cycle alone, through the one entry of rollout_cycle.h.
// Behind that, the host side of include/sactd3_eval.h: the evaluation rollout's kernel steps the envs with env_step_body, so it is compiled
// here (eval_kernels.h); it reaches the engine through eval_rollout.h alone.  The same holds for the collected segment of
// include/sactd3_rollout_collect.h: collect_kernels.h, collect_rollout.h.
// Two things are written once for all of it: guarded(), the C boundary of every entry point, and with_kind(), the way from a handle's
// run-time kind to the task table and the kernel instances of env_kernels.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sactd3.h"
#include "../../include/sactd3_env.h"
#include "../../include/sactd3_rollout.h"
#include "../../include/sactd3_eval.h"
#include "env_kernels.h"
#include "eval_kernels.h"
#include "collect_kernels.h"
#include "rollout_cycle.h"

#define ENV_API extern "C" __attribute__((visibility("default")))

// The C boundary: no exception crosses it (the error texts are std::strings, the getters stage in std::vectors: std::bad_alloc).
// Every entry point that can throw is `return guarded([&]() -> int { ... });`
template <class F>
static int guarded(F&& body) {
  try {
    return body();
  } catch (...) {
    return SACTD3_EHIP;
  }
}

// The run-time kind as a compile-time one: f(std::integral_constant<int, KIND>) -> f's result.  The only switch over the tasks here.
template <class F>
static auto with_kind(int kind, F&& f) {
  switch (kind) {
    case SACTD3_ENV_PENDULUM: return f(std::integral_constant<int, ENV_PENDULUM>{});
    case SACTD3_ENV_CARTPOLE: return f(std::integral_constant<int, ENV_CARTPOLE>{});
    default: return f(std::integral_constant<int, ENV_POINTGOAL>{});
  }
}

static thread_local std::string g_env_create_error;

struct sactd3_env {
  sactd3_env_config cfg{};
  sactd3_env_info info{};
  EnvDev d{};
  void* mem = nullptr;
  std::string err;

  int fail(int code, const char* what, hipError_t he = hipSuccess) {
    err = what;
    if (he != hipSuccess) err += std::string(": ") + hipGetErrorString(he);
    return code;
  }
};

#define ENV_HIP(e, call)                                                \
  do {                                                                  \
    hipError_t he_ = (call);                                            \
    if (he_ != hipSuccess) return (e)->fail(SACTD3_EHIP, #call, he_);   \
  } while (0)

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline dim3 env_grid(const sactd3_env* e) { return dim3((unsigned)((e->d.n + 255) / 256)); }

// The per-env arrays of `d` for n envs, each named once, every one on a 256-byte boundary: -> the bytes they take together; with
// `base` they are placed there, in this order (phys stays component-major: tools/ and the state getters rely on it).
static size_t env_place(EnvDev& d, size_t n, char* base) {
  size_t off = 0;
  auto take = [&](auto*& p, size_t count) {
    if (base) p = (std::remove_reference_t<decltype(p)>)(base + off);
    off += up256(count * sizeof(*p));
  };
  take(d.phys, 4 * n); take(d.steps, n); take(d.episode, n); take(d.ret, n); take(d.draws, n); take(d.done_count, n); take(d.ret_sum, n);
  take(d.len_sum, n); take(d.last_ret, n); take(d.last_len, n); take(d.first_ret, n); take(d.first_len, n); take(d.bad, n);
  return off;
}

static int env_alloc(sactd3_env* e) {
  const size_t n = (size_t)e->cfg.num_envs, bytes = env_place(e->d, n, nullptr);
  ENV_HIP(e, hipMalloc(&e->mem, bytes));
  ENV_HIP(e, hipMemset(e->mem, 0, bytes));
  env_place(e->d, n, (char*)e->mem);
  e->d.n = (int)n;
  return SACTD3_OK;
}

static int env_init(sactd3_env* e, const sactd3_env_config* cfg) {
  e->cfg = *cfg;
  if (cfg->kind < 0 || cfg->kind >= SACTD3_ENV_NUM_KINDS) return e->fail(SACTD3_EINVAL, "kind must be SACTD3_ENV_PENDULUM, SACTD3_ENV_CARTPOLE or SACTD3_ENV_POINTGOAL");
  if (cfg->num_envs < 1 || cfg->num_envs > (1 << 24)) return e->fail(SACTD3_EINVAL, "num_envs must be in [1, 2^24]");
  if (cfg->horizon < 0) return e->fail(SACTD3_EINVAL, "horizon must be >= 0 (0: the task's default)");
  with_kind(cfg->kind, [&](auto K) {
    using T = EnvTask<decltype(K)::value>;
    e->info.ob_dim = T::OB; e->info.ac_dim = T::AC; e->info.max_ac = T::BOUND;
    e->info.horizon = cfg->horizon ? cfg->horizon : T::HORIZON;
  });
  e->info.num_envs = cfg->num_envs;
  e->info.min_ac = -e->info.max_ac;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return e->fail(SACTD3_ENODEV, "no HIP device visible");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return e->fail(SACTD3_EINVAL, "device_id is not a visible device");
  ENV_HIP(e, hipSetDevice(cfg->device_id));
  hipDeviceProp_t prop;
  ENV_HIP(e, hipGetDeviceProperties(&prop, cfg->device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return e->fail(SACTD3_ENODEV, "device is not gfx950 (this library carries gfx950 code objects only)");
  return env_alloc(e);
}

ENV_API int sactd3_env_create(const sactd3_env_config* cfg, sactd3_env** out) {
  return guarded([&]() -> int {
    if (out) *out = nullptr;
    if (!cfg || !out) {
      g_env_create_error = "sactd3_env_create: NULL argument";
      return SACTD3_EINVAL;
    }
    sactd3_env* e = new (std::nothrow) sactd3_env();
    if (!e) {
      g_env_create_error = "sactd3_env_create: out of host memory";
      return SACTD3_EHIP;
    }
    const int rc = guarded([&]() -> int {      // (of its own: nothing is leaked on the way out)
      const int rc = env_init(e, cfg);
      if (rc != SACTD3_OK) g_env_create_error = e->err;
      return rc;
    });
    if (rc != SACTD3_OK) {
      if (e->mem) (void)hipFree(e->mem);
      delete e;
      return rc;
    }
    *out = e;
    return SACTD3_OK;
  });
}

ENV_API void sactd3_env_destroy(sactd3_env* e) {
  if (!e) return;
  if (e->mem) {
    (void)hipSetDevice(e->cfg.device_id);
    (void)hipFree(e->mem);      // (waits for the device: no kernel of this env is in flight behind it)
  }
  delete e;
}

ENV_API const char* sactd3_env_last_error(const sactd3_env* e) { return e ? e->err.c_str() : g_env_create_error.c_str(); }

ENV_API int sactd3_env_spec(const sactd3_env* e, sactd3_env_info* out) {
  if (!e || !out) return SACTD3_EINVAL;
  *out = e->info;
  return SACTD3_OK;
}

ENV_API int sactd3_env_reset(sactd3_env* e, uint64_t seed, float* obs, int64_t obs_ld, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (obs && obs_ld < e->info.ob_dim) return e->fail(SACTD3_EINVAL, "sactd3_env_reset: obs_ld is below ob_dim");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    e->cfg.seed = seed;
    with_kind(e->cfg.kind, [&](auto K) {
      hipLaunchKernelGGL(k_env_reset<decltype(K)::value>, env_grid(e), dim3(256), 0, (hipStream_t)stream, e->d, obs, (long long)obs_ld, seed);
    });
    ENV_HIP(e, hipGetLastError());
    return SACTD3_OK;
  });
}

ENV_API int sactd3_env_step(sactd3_env* e, const float* actions, int64_t act_ld, const sactd3_env_out* out, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!actions || !out || !out->obs) return e->fail(SACTD3_EINVAL, "sactd3_env_step: actions, out and out->obs must not be NULL");
    const int o = e->info.ob_dim;
    if (act_ld < e->info.ac_dim) return e->fail(SACTD3_EINVAL, "sactd3_env_step: act_ld is below ac_dim");
    if (out->obs_ld < o || (out->final_obs && out->final_obs_ld < o)) return e->fail(SACTD3_EINVAL, "sactd3_env_step: an observation stride is below ob_dim");
    if ((out->reward && out->reward_ld < 1) || (out->terminated && out->terminated_ld < 1) || (out->truncated && out->truncated_ld < 1) ||
        (out->ended && out->ended_ld < 1))
      return e->fail(SACTD3_EINVAL, "sactd3_env_step: a per-env output needs a stride of at least 1");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    EnvOut k;
    k.obs = out->obs; k.obs_ld = out->obs_ld;
    k.final_obs = out->final_obs; k.final_obs_ld = out->final_obs_ld;
    k.reward = out->reward; k.reward_ld = out->reward_ld;
    k.terminated = out->terminated; k.terminated_ld = out->terminated_ld;
    k.truncated = out->truncated; k.truncated_ld = out->truncated_ld;
    k.ended = out->ended; k.ended_ld = out->ended_ld;
    with_kind(e->cfg.kind, [&](auto K) {
      hipLaunchKernelGGL(k_env_step<decltype(K)::value>, env_grid(e), dim3(256), 0, (hipStream_t)stream, e->d, actions, (long long)act_ld, k,
                         e->info.horizon, e->cfg.seed);
    });
    ENV_HIP(e, hipGetLastError());
    return SACTD3_OK;
  });
}

ENV_API int sactd3_env_sample_actions(sactd3_env* e, float* actions, int64_t act_ld, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!actions) return e->fail(SACTD3_EINVAL, "sactd3_env_sample_actions: actions must not be NULL");
    if (act_ld < e->info.ac_dim) return e->fail(SACTD3_EINVAL, "sactd3_env_sample_actions: act_ld is below ac_dim");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    hipLaunchKernelGGL(k_env_sample_actions, env_grid(e), dim3(256), 0, (hipStream_t)stream, e->d, actions, (long long)act_ld, e->info.ac_dim,
                       e->info.min_ac, e->info.max_ac - e->info.min_ac, e->cfg.seed);
    ENV_HIP(e, hipGetLastError());
    return SACTD3_OK;
  });
}

// device -> host of one per-env array, behind what the stream has queued
template <class T>
static int env_pull(sactd3_env* e, std::vector<T>& host, const T* dev, size_t count, hipStream_t st) {
  host.resize(count);
  ENV_HIP(e, hipMemcpyAsync(host.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
  return SACTD3_OK;
}

ENV_API int sactd3_env_episode_stats(sactd3_env* e, sactd3_env_stats* out, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!out) return e->fail(SACTD3_EINVAL, "sactd3_env_episode_stats: out must not be NULL");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)e->d.n;
    std::vector<uint32_t> done, bad;
    std::vector<double> rs;
    std::vector<unsigned long long> ls;
    std::vector<float> lr, fr;
    std::vector<int32_t> ll, fl;
    int rc;
    if ((rc = env_pull(e, done, e->d.done_count, n, st)) || (rc = env_pull(e, bad, e->d.bad, n, st)) || (rc = env_pull(e, rs, e->d.ret_sum, n, st)) ||
        (rc = env_pull(e, ls, e->d.len_sum, n, st)) || (rc = env_pull(e, lr, e->d.last_ret, n, st)) || (rc = env_pull(e, ll, e->d.last_len, n, st)) ||
        (rc = env_pull(e, fr, e->d.first_ret, n, st)) || (rc = env_pull(e, fl, e->d.first_len, n, st)))
      return rc;
    ENV_HIP(e, hipStreamSynchronize(st));
    out->episodes = 0; out->return_sum = 0.0; out->length_sum = 0; out->bad_actions = 0;
    for (size_t i = 0; i < n; ++i) {      // the only sums over envs, in env order, on the host
      out->episodes += done[i];
      out->return_sum += rs[i];
      out->length_sum += (int64_t)ls[i];
      out->bad_actions += bad[i];
      if (out->last_return) out->last_return[i] = lr[i];
      if (out->last_length) out->last_length[i] = ll[i];
      if (out->env_episodes) out->env_episodes[i] = done[i];
      if (out->first_return) out->first_return[i] = fr[i];
      if (out->first_length) out->first_length[i] = fl[i];
    }
    return SACTD3_OK;
  });
}

ENV_API int sactd3_env_get_state(sactd3_env* e, const sactd3_env_state* out, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!out) return e->fail(SACTD3_EINVAL, "sactd3_env_get_state: out must not be NULL");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)e->d.n;
    std::vector<float> phys;
    if (out->phys) {
      const int rc = env_pull(e, phys, e->d.phys, 4 * n, st);
      if (rc) return rc;
    }
    if (out->steps) ENV_HIP(e, hipMemcpyAsync(out->steps, e->d.steps, n * 4, hipMemcpyDeviceToHost, st));
    if (out->episode) ENV_HIP(e, hipMemcpyAsync(out->episode, e->d.episode, n * 4, hipMemcpyDeviceToHost, st));
    if (out->returns) ENV_HIP(e, hipMemcpyAsync(out->returns, e->d.ret, n * 4, hipMemcpyDeviceToHost, st));
    if (out->draws) ENV_HIP(e, hipMemcpyAsync(out->draws, e->d.draws, n * 4, hipMemcpyDeviceToHost, st));
    ENV_HIP(e, hipStreamSynchronize(st));
    if (out->phys)
      for (size_t i = 0; i < n; ++i)
        for (int j = 0; j < 4; ++j) out->phys[i * 4 + j] = phys[j * n + i];      // component-major on the device, env-major for the caller
    return SACTD3_OK;
  });
}

ENV_API int sactd3_env_set_state(sactd3_env* e, const sactd3_env_state* in, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!in) return e->fail(SACTD3_EINVAL, "sactd3_env_set_state: in must not be NULL");
    const size_t n = (size_t)e->d.n;
    if (in->phys)
      for (size_t k = 0; k < 4 * n; ++k)
        if (!std::isfinite(in->phys[k])) return e->fail(SACTD3_EINVAL, "sactd3_env_set_state: a physical state is not finite");
    if (in->steps)
      for (size_t i = 0; i < n; ++i)
        if (in->steps[i] < 0) return e->fail(SACTD3_EINVAL, "sactd3_env_set_state: a step count is negative");
    ENV_HIP(e, hipSetDevice(e->cfg.device_id));
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> phys;
    if (in->phys) {
      phys.resize(4 * n);
      for (size_t i = 0; i < n; ++i)
        for (int j = 0; j < 4; ++j) phys[j * n + i] = in->phys[i * 4 + j];
      ENV_HIP(e, hipMemcpyAsync(e->d.phys, phys.data(), 4 * n * 4, hipMemcpyHostToDevice, st));
    }
    if (in->steps) ENV_HIP(e, hipMemcpyAsync(e->d.steps, in->steps, n * 4, hipMemcpyHostToDevice, st));
    if (in->episode) ENV_HIP(e, hipMemcpyAsync(e->d.episode, in->episode, n * 4, hipMemcpyHostToDevice, st));
    if (in->returns) ENV_HIP(e, hipMemcpyAsync(e->d.ret, in->returns, n * 4, hipMemcpyHostToDevice, st));
    if (in->draws) ENV_HIP(e, hipMemcpyAsync(e->d.draws, in->draws, n * 4, hipMemcpyHostToDevice, st));
    ENV_HIP(e, hipStreamSynchronize(st));      // the host arrays (and `phys` above) are free again when the call returns
    return SACTD3_OK;
  });
}

// ---------------------------------------------------------------------------------------------------- include/sactd3_rollout.h
static thread_local std::string g_rollout_create_error;

// device memory of device `dev`?  (the engine's rule for a caller's pointer, csrc/engine.hip: device_ptr_check)
static bool on_device(const void* p, int dev) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != dev) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// the refusals of a record layout for an env of (o, a): NULL = accepted
static const char* layout_refusal(const sactd3_record_layout* L, int o, int a) {
  if (L->record_len % 4 || L->next_off % 4 || L->next_width % 4) return "record_len, next_off and next_width must be multiples of 4";
  if (L->next_off < o + a) return "next_off is below ob_dim + ac_dim";
  if (L->next_width < o) return "next_width is below ob_dim";
  if ((int64_t)L->record_len < (int64_t)L->next_off + L->next_width + 2) return "record_len is below next_off + next_width + 2";
  return nullptr;
}

// the one launch of k_env_step_rec: every argument has been checked.  issue_step_rec: the launch alone, on the current device -- what a
// stream capture may hold (the cycle's graph, below); launch_step_rec: on the env's device, with the error text
static hipError_t issue_step_rec(sactd3_env* e, const float* actions, int64_t act_ld, const sactd3_record_layout* L, float* records, float* obs,
                                 int64_t obs_ld, hipStream_t st) {
  const EnvRec k{L->record_len, L->next_off, L->next_width};
  with_kind(e->cfg.kind, [&](auto K) {
    hipLaunchKernelGGL(k_env_step_rec<decltype(K)::value>, env_grid(e), dim3(256), 0, st, e->d, actions, (long long)act_ld, k, records, obs,
                       (long long)obs_ld, e->info.horizon, e->cfg.seed);
  });
  return hipGetLastError();
}
static int launch_step_rec(sactd3_env* e, const float* actions, int64_t act_ld, const sactd3_record_layout* L, float* records, float* obs,
                           int64_t obs_ld, hipStream_t st) {
  ENV_HIP(e, hipSetDevice(e->cfg.device_id));
  ENV_HIP(e, issue_step_rec(e, actions, act_ld, L, records, obs, obs_ld, st));
  return SACTD3_OK;
}

ENV_API int sactd3_rollout_env_step(sactd3_env* e, const float* actions, int64_t act_ld, const sactd3_record_layout* L, float* records,
                                    float* obs, int64_t obs_ld, void* stream) {
  return guarded([&]() -> int {
    if (!e) return SACTD3_EINVAL;
    if (!actions || !L || !records || !obs) return e->fail(SACTD3_EINVAL, "sactd3_rollout_env_step: actions, layout, records and obs must not be NULL");
    if (act_ld < e->info.ac_dim) return e->fail(SACTD3_EINVAL, "sactd3_rollout_env_step: act_ld is below ac_dim");
    if (obs_ld < e->info.ob_dim) return e->fail(SACTD3_EINVAL, "sactd3_rollout_env_step: obs_ld is below ob_dim");
    if (const char* why = layout_refusal(L, e->info.ob_dim, e->info.ac_dim)) return e->fail(SACTD3_EINVAL, (std::string("sactd3_rollout_env_step: ") + why).c_str());
    if ((uintptr_t)records % 16) return e->fail(SACTD3_EINVAL, "sactd3_rollout_env_step: `records` is not 16-byte aligned");
    if (!on_device(records, e->cfg.device_id)) return e->fail(SACTD3_EINVAL, "sactd3_rollout_env_step: `records` is not device memory of the env's device");
    return launch_step_rec(e, actions, act_ld, L, records, obs, obs_ld, (hipStream_t)stream);
  });
}

// the host counters, in the order sactd3_rollout_stats and sactd3_rollout_cycle_stats give them out
enum { ROLLOUT_RANDOM_CHOICES, ROLLOUT_POLICY_CHOICES, ROLLOUT_STEPS, ROLLOUT_ROWS, ROLLOUT_NUM_STATS };
enum { CYCLE_ISSUED, CYCLE_CAPTURED, CYCLE_GRAPH_NODES, CYCLE_EAGER, CYCLE_NUM_STATS };
static_assert(ROLLOUT_NUM_STATS == 4 && CYCLE_NUM_STATS == 4, "int64_t out[4] of include/sactd3_rollout.h and sactd3_rollout_cycle.h");

struct sactd3_rollout {
  sactd3_engine* eng = nullptr;
  sactd3_env* env = nullptr;
  sactd3_rollout_buffers buf{};
  sactd3_record_layout lay{};
  hipStream_t stream = nullptr;
  int n = 0;
  int64_t stats[ROLLOUT_NUM_STATS] = {};
  int64_t cycle_stats[CYCLE_NUM_STATS] = {};      // (the engine counts in them: CycleBinding::stats)
  int64_t collect_stats[3] = {};        // sactd3_rollout_collect: {calls, env steps, calls that drew}
  bool cycled = false;                  // a cycle reached the engine: it may hold graphs of this binding (sactd3_rollout_destroy)
  std::string err;

  int fail(int code, const std::string& what) {
    err = what;
    return code;
  }
  // a failed call of the env's / the engine's ABI: its code, its text
  int from_env(int rc, const char* call) { return rc ? fail(rc, std::string(call) + ": " + sactd3_env_last_error(env)) : 0; }
  int from_engine(int rc, const char* call) {
    if (!rc) return 0;
    const char* text = sactd3_last_error(eng);
    return fail(rc, std::string(call) + ": " + (text ? text : "?"));
  }
};

ENV_API int sactd3_rollout_create(sactd3_engine* eng, sactd3_env* env, const sactd3_rollout_buffers* b, void* stream, sactd3_rollout** out) {
  return guarded([&]() -> int {
    if (out) *out = nullptr;
    auto refuse = [](const std::string& what) {
      g_rollout_create_error = "sactd3_rollout_create: " + what;
      return (int)SACTD3_EINVAL;
    };
    if (!eng || !env || !b || !out) return refuse("NULL argument");
    if (!b->obs || !b->actions || !b->records) return refuse("a buffer is NULL");
    sactd3_config cfg;
    int32_t lay[4];
    if (sactd3_get_config(eng, &cfg) != SACTD3_OK || sactd3_rb_layout(eng, lay) != SACTD3_OK) return refuse("the engine gave no configuration");
    const sactd3_env_info& info = env->info;
    if (info.ob_dim != cfg.ob_dim || info.ac_dim != cfg.ac_dim)
      return refuse("the env's ob_dim / ac_dim (" + std::to_string(info.ob_dim) + ", " + std::to_string(info.ac_dim) + ") differ from the engine's (" +
                    std::to_string(cfg.ob_dim) + ", " + std::to_string(cfg.ac_dim) + ")");
    if (env->cfg.device_id != cfg.device_id) return refuse("the env and the engine are on different devices");
    if (info.num_envs > cfg.max_envs)
      return refuse("num_envs (" + std::to_string(info.num_envs) + ") is above the engine's max_envs (" + std::to_string(cfg.max_envs) + ")");
    if (b->obs_ld < info.ob_dim || b->actions_ld < info.ac_dim) return refuse("a row stride is below its width");
    const sactd3_record_layout L{lay[0], lay[1], lay[2]};
    if (const char* why = layout_refusal(&L, info.ob_dim, info.ac_dim)) return refuse(why);
    if ((uintptr_t)b->records % 16) return refuse("`records` is not 16-byte aligned");
    if (!on_device(b->obs, cfg.device_id) || !on_device(b->actions, cfg.device_id) || !on_device(b->records, cfg.device_id))
      return refuse("a buffer is not device memory of the handles' device");
    sactd3_rollout* r = new (std::nothrow) sactd3_rollout();
    if (!r) {
      g_rollout_create_error = "sactd3_rollout_create: out of host memory";
      return SACTD3_EHIP;
    }
    r->eng = eng; r->env = env; r->buf = *b; r->lay = L; r->stream = (hipStream_t)stream; r->n = info.num_envs;
    *out = r;
    return SACTD3_OK;
  });
}

// (neither handle nor any buffer is the rollout's; the cycle graphs of its binding, which the engine keeps, go with it)
ENV_API void sactd3_rollout_destroy(sactd3_rollout* r) {
  if (r && r->cycled) engine_rollout_cycle_release(r->eng, r);
  delete r;
}

ENV_API const char* sactd3_rollout_last_error(const sactd3_rollout* r) { return r ? r->err.c_str() : g_rollout_create_error.c_str(); }

ENV_API int sactd3_rollout_reset(sactd3_rollout* r, uint64_t seed) {
  return guarded([&]() -> int {
    if (!r) return SACTD3_EINVAL;
    return r->from_env(sactd3_env_reset(r->env, seed, r->buf.obs, r->buf.obs_ld, r->stream), "sactd3_env_reset");
  });
}

ENV_API int sactd3_rollout_choose(sactd3_rollout* r, int mode) {
  return guarded([&]() -> int {
    if (!r) return SACTD3_EINVAL;
    const sactd3_rollout_buffers& b = r->buf;
    int rc;
    switch (mode) {
      case SACTD3_ROLLOUT_REPEAT:
        return SACTD3_OK;
      case SACTD3_ROLLOUT_RANDOM:
        if ((rc = r->from_env(sactd3_env_sample_actions(r->env, b.actions, b.actions_ld, r->stream), "sactd3_env_sample_actions"))) return rc;
        ++r->stats[ROLLOUT_RANDOM_CHOICES];
        return SACTD3_OK;
      case SACTD3_ROLLOUT_EXPLORE:
      case SACTD3_ROLLOUT_EXPLOIT:
        rc = sactd3_predict_device(r->eng, b.obs, b.obs_ld, r->n, mode == SACTD3_ROLLOUT_EXPLORE ? 1 : 0, b.actions, b.actions_ld, r->stream,
                                   SACTD3_SRC_ORDERED);
        if ((rc = r->from_engine(rc, "sactd3_predict_device"))) return rc;
        ++r->stats[ROLLOUT_POLICY_CHOICES];
        return SACTD3_OK;
      default:
        return r->fail(SACTD3_EINVAL, "sactd3_rollout_choose: mode must be one of SACTD3_ROLLOUT_*");
    }
  });
}

ENV_API int sactd3_rollout_advance(sactd3_rollout* r) {
  return guarded([&]() -> int {
    if (!r) return SACTD3_EINVAL;
    const sactd3_rollout_buffers& b = r->buf;
    int rc = launch_step_rec(r->env, b.actions, b.actions_ld, &r->lay, b.records, b.obs, b.obs_ld, r->stream);
    if ((rc = r->from_env(rc, "k_env_step_rec"))) return rc;
    ++r->stats[ROLLOUT_STEPS];
    rc = sactd3_rb_extend_records_device(r->eng, b.records, r->n, r->stream, SACTD3_SRC_ORDERED);
    if ((rc = r->from_engine(rc, "sactd3_rb_extend_records_device"))) return rc;
    r->stats[ROLLOUT_ROWS] += r->n;
    return SACTD3_OK;
  });
}

ENV_API int sactd3_rollout_stats(const sactd3_rollout* r, int64_t out[4]) {
  if (!r || !out) return SACTD3_EINVAL;
  for (int i = 0; i < ROLLOUT_NUM_STATS; ++i) out[i] = r->stats[i];
  return SACTD3_OK;
}

// ---------------------------------------------------------------------------------------------------- include/sactd3_rollout_cycle.h
// What the engine is handed for the env step: this launcher and the rollout as its context -- no field of either handle.  (The device is
// the engine's, which is the env's: sactd3_rollout_create.  Nothing but the launch, so that the engine's capture may hold it.)
static int cycle_env_step(void* ctx, hipStream_t s) {
  sactd3_rollout* r = (sactd3_rollout*)ctx;
  const sactd3_rollout_buffers& b = r->buf;
  return (int)issue_step_rec(r->env, b.actions, b.actions_ld, &r->lay, b.records, b.obs, b.obs_ld, s);
}

ENV_API int sactd3_rollout_cycle(sactd3_rollout* r, int mode, int do_actor) {
  return guarded([&]() -> int {
    if (!r) return SACTD3_EINVAL;
    if (mode != SACTD3_ROLLOUT_EXPLORE && mode != SACTD3_ROLLOUT_EXPLOIT)
      return r->fail(SACTD3_EINVAL, "sactd3_rollout_cycle: mode must be SACTD3_ROLLOUT_EXPLORE or SACTD3_ROLLOUT_EXPLOIT (a random or repeated choice "
                                    "runs no update: sactd3_rollout_advance / _choose)");
    const sactd3_rollout_buffers& b = r->buf;
    const CycleBinding bind{r, cycle_env_step, r, b.obs, b.obs_ld, b.actions, b.actions_ld, b.records, r->n, r->stream, r->cycle_stats};
    const int64_t had = r->cycle_stats[CYCLE_ISSUED] + r->cycle_stats[CYCLE_CAPTURED];
    int rc = engine_rollout_cycle(r->eng, bind, mode == SACTD3_ROLLOUT_EXPLORE ? 1 : 0, do_actor);
    if (r->cycle_stats[CYCLE_ISSUED] + r->cycle_stats[CYCLE_CAPTURED] != had) r->cycled = true;      // (a capture counts: the engine holds a graph of ours)
    if ((rc = r->from_engine(rc, "sactd3_rollout_cycle"))) return rc;
    ++r->stats[ROLLOUT_POLICY_CHOICES]; ++r->stats[ROLLOUT_STEPS]; r->stats[ROLLOUT_ROWS] += r->n;
    return SACTD3_OK;
  });
}

ENV_API int sactd3_rollout_cycle_stats(const sactd3_rollout* r, int64_t out[4]) {
  if (!r || !out) return SACTD3_EINVAL;
  for (int i = 0; i < CYCLE_NUM_STATS; ++i) out[i] = r->cycle_stats[i];
  return SACTD3_OK;
}

ENV_API int sactd3_rollout_cycle_clamped(sactd3_rollout* r, int64_t* out) {
  return guarded([&]() -> int {
    if (!r || !out) return SACTD3_EINVAL;
    return r->from_engine(engine_rollout_cycle_clamped(r->eng, out), "sactd3_rollout_cycle_clamped");
  });
}

// ---------------------------------------------------------------------------------------------------- include/sactd3_rollout_collect.h
// Every refusal stands in front of the first side effect.  The launches, all on the engine's learner stream between ONE pair of events
// against the rollout's: k_collect_rollout, the append of its slab (flags 0: the slab was written on the stream that reads it), the
// counter tick of a call that drew.
ENV_API int sactd3_rollout_collect(sactd3_rollout* r, int mode, int steps, float* records, float* eps) {
  return guarded([&]() -> int {
    if (!r) return SACTD3_EINVAL;
    sactd3_env* e = r->env;
    const int dev = e->cfg.device_id;
    if (!records) return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: `records` must not be NULL");
    if ((uintptr_t)records % 16) return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: `records` is not 16-byte aligned");
    if (mode != SACTD3_ROLLOUT_RANDOM && mode != SACTD3_ROLLOUT_EXPLORE && mode != SACTD3_ROLLOUT_EXPLOIT)
      return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: mode must be SACTD3_ROLLOUT_RANDOM, SACTD3_ROLLOUT_EXPLORE or SACTD3_ROLLOUT_EXPLOIT");
    if (steps < 1 || steps > SACTD3_COLLECT_MAX_STEPS) return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: steps must be in [1, 4096]");
    if (!on_device(records, dev)) return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: `records` is not device memory of the handles' device");
    if (eps && !on_device(eps, dev)) return r->fail(SACTD3_EINVAL, "sactd3_rollout_collect: `eps` is not device memory of the handles' device");
    const int64_t rows = (int64_t)steps * r->n;
    CollectActor ca{};
    int rc = engine_collect_open(r->eng, e->info.ob_dim, e->info.ac_dim, dev, rows, r->stream, &ca);
    if ((rc = r->from_engine(rc, "sactd3_rollout_collect"))) return rc;
    // ---- no refusal behind this point
    const sactd3_rollout_buffers& b = r->buf;
    CollectLaunch p{};
    p.A = ca.A; p.T = steps; p.horizon = e->info.horizon; p.mode = mode; p.noise_std = ca.noise_std;
    p.lo = e->info.min_ac; p.span = e->info.max_ac - e->info.min_ac; p.env_seed = e->cfg.seed;
    p.L = EnvRec{r->lay.record_len, r->lay.next_off, r->lay.next_width};
    p.records = records; p.eps = eps; p.obs = b.obs; p.obs_ld = (long long)b.obs_ld; p.actions = b.actions; p.actions_ld = (long long)b.actions_ld;
    const dim3 grid((unsigned)((e->d.n + EV_TILE - 1) / EV_TILE));
    with_kind(e->cfg.kind, [&](auto K) { hipLaunchKernelGGL(k_collect_rollout<decltype(K)::value>, grid, dim3(256), 0, ca.A.stream, e->d, p); });
    // a HIP error behind the opening half of the event pair: the pair is closed (no tick), so that the rollout's stream still stands
    // behind whatever the learner stream was given, and the call's own error is what is reported
    auto broken = [&](int code) {
      (void)engine_collect_close(r->eng, 0, r->stream);
      return code;
    };
    if (const hipError_t he = hipGetLastError())
      return broken(r->fail(SACTD3_EHIP, std::string("sactd3_rollout_collect: k_collect_rollout: ") + hipGetErrorString(he)));
    rc = sactd3_rb_extend_records_device(r->eng, records, (int)rows, nullptr, 0);
    if ((rc = r->from_engine(rc, "sactd3_rb_extend_records_device"))) return broken(rc);
    const bool drew = mode == SACTD3_ROLLOUT_EXPLORE;
    rc = engine_collect_close(r->eng, drew ? 1 : 0, r->stream);
    if ((rc = r->from_engine(rc, "sactd3_rollout_collect"))) return rc;
    // the counters of `steps` choose + advance calls, and the feature's own
    r->stats[mode == SACTD3_ROLLOUT_RANDOM ? ROLLOUT_RANDOM_CHOICES : ROLLOUT_POLICY_CHOICES] += steps;
    r->stats[ROLLOUT_STEPS] += steps;
    r->stats[ROLLOUT_ROWS] += rows;
    ++r->collect_stats[0]; r->collect_stats[1] += steps;
    if (drew) ++r->collect_stats[2];
    return SACTD3_OK;
  });
}

ENV_API int sactd3_rollout_collect_stats(sactd3_rollout* r, int64_t out[4]) {
  return guarded([&]() -> int {
    if (!r || !out) return SACTD3_EINVAL;
    return r->from_engine(engine_collect_stats(r->eng, r->collect_stats, out), "sactd3_rollout_collect_stats");
  });
}

// ---------------------------------------------------------------------------------------------------- include/sactd3_eval.h
// Every refusal stands in front of the first side effect: the env's words, the engine's state and both streams are untouched by a refused call.
ENV_API int sactd3_eval_rollout(sactd3_engine* eng, sactd3_env* e, const sactd3_eval_config* cfg, const sactd3_eval_out* out, void* caller_stream,
                                int flags) {
  return guarded([&]() -> int {
    if (!eng) return SACTD3_EINVAL;
    auto refuse = [&](const std::string& what) { return engine_eval_fail(eng, SACTD3_EINVAL, ("eval_rollout: " + what).c_str()); };
    if (!e || !cfg || !out) return refuse("NULL argument");
    sactd3_config ec;
    if (sactd3_get_config(eng, &ec) != SACTD3_OK) return refuse("the engine gave no configuration");
    const sactd3_env_info& info = e->info;
    if (info.ob_dim != ec.ob_dim || info.ac_dim != ec.ac_dim)
      return refuse("the env's ob_dim / ac_dim (" + std::to_string(info.ob_dim) + ", " + std::to_string(info.ac_dim) + ") differ from the engine's (" +
                    std::to_string(ec.ob_dim) + ", " + std::to_string(ec.ac_dim) + ")");
    if (e->cfg.device_id != ec.device_id) return refuse("the env and the engine are on different devices");
    if (flags & ~(SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED)) return refuse("unknown flag");
    if (cfg->steps < 0 || cfg->steps > SACTD3_EVAL_MAX_STEPS) return refuse("steps must be in [1, 4096] (0: the env's horizon)");
    const int T = cfg->steps ? cfg->steps : info.horizon;
    if (T < 1 || T > SACTD3_EVAL_MAX_STEPS) return refuse("the env's horizon is above 4096 steps: name `steps`");
    if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return refuse("gamma must be in [0, 1]");
    if (cfg->mode != SACTD3_EVAL_GREEDY && cfg->mode != SACTD3_EVAL_SAMPLE) return refuse("mode must be SACTD3_EVAL_GREEDY or SACTD3_EVAL_SAMPLE");
    if (cfg->reset != 0 && cfg->reset != 1) return refuse("reset must be 0 or 1");
    if (cfg->soft != 0 && cfg->soft != 1) return refuse("soft must be 0 or 1");
    const bool sample = cfg->mode == SACTD3_EVAL_SAMPLE;
    if (ec.prefer_td3_over_sac && (sample || cfg->soft)) return refuse("SACTD3_EVAL_SAMPLE and soft are SAC only");
    if (cfg->soft && !sample) return refuse("soft needs SACTD3_EVAL_SAMPLE (a greedy action has no log-probability)");
    const void* outs[12] = {out->obs, out->actions, out->eps, out->reward, out->logp, out->rtg, out->live, out->ep_return, out->ep_length,
                            out->ep_terminated, out->g0, out->alpha};
    static const char* const names[12] = {"obs", "actions", "eps", "reward", "logp", "rtg", "live", "ep_return", "ep_length", "ep_terminated", "g0", "alpha"};
    for (int k = 0; k < 12; ++k)
      if (outs[k] && !on_device(outs[k], ec.device_id)) return refuse(std::string("`") + names[k] + "` is not device memory of the handles' device");
    const int64_t rows = (int64_t)T * info.num_envs;
    EvalActor A{};
    int rc = engine_eval_open(eng, info.ob_dim, info.ac_dim, e->cfg.device_id, sample ? 1 : 0, cfg->soft, rows, caller_stream, flags, &A);
    if (rc) return rc;
    // ---- no refusal behind this point
    if (cfg->reset) {
      e->cfg.seed = cfg->seed;
      with_kind(e->cfg.kind, [&](auto K) {
        hipLaunchKernelGGL(k_env_reset<decltype(K)::value>, env_grid(e), dim3(256), 0, A.stream, e->d, (float*)nullptr, 0ll, cfg->seed);
      });
      if (const hipError_t he = hipGetLastError()) return engine_eval_fail(eng, SACTD3_EHIP, (std::string("eval_rollout: k_env_reset: ") + hipGetErrorString(he)).c_str());
    }
    EvalLaunch p{};
    p.A = A; p.T = T; p.horizon = info.horizon; p.sample = sample ? 1 : 0; p.soft = cfg->soft; p.gamma = cfg->gamma; p.env_seed = e->cfg.seed;
    p.obs = out->obs; p.actions = out->actions; p.eps = out->eps; p.reward = out->reward; p.logp = out->logp; p.rtg = out->rtg; p.live = out->live;
    p.ep_return = out->ep_return; p.ep_length = out->ep_length; p.ep_terminated = out->ep_terminated; p.g0 = out->g0; p.alpha = out->alpha;
    const dim3 grid((unsigned)((e->d.n + EV_TILE - 1) / EV_TILE));
    with_kind(e->cfg.kind, [&](auto K) { hipLaunchKernelGGL(k_eval_rollout<decltype(K)::value>, grid, dim3(256), 0, A.stream, e->d, p); });
    if (const hipError_t he = hipGetLastError()) return engine_eval_fail(eng, SACTD3_EHIP, (std::string("eval_rollout: k_eval_rollout: ") + hipGetErrorString(he)).c_str());
    return engine_eval_close(eng, sample ? 1 : 0, rows, caller_stream, flags);
  });
}

ENV_API int sactd3_eval_stats(sactd3_engine* eng, int64_t out[4]) {
  return guarded([&]() -> int { return engine_eval_stats(eng, out); });
}
