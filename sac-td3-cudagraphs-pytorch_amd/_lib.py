"""ctypes binding of include/sactd3.h.  Fails loudly when the HIP library is missing: there is no
CPU fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ABI_VERSION = 1
ACTOR, CRITICS, ACTOR_TARGET, CRITICS_TARGET, LOG_ALPHA = range(5)
SITE_CRITIC, SITE_ACTOR0, SITE_ACTOR1, SITE_ALPHA0, SITE_ALPHA1, SITE_PREDICT = range(6)
NUM_METRICS = 8
M_QF_LOSS, M_ACTOR_LOSS, M_ALPHA_LOSS, M_ALPHA, M_BC_LOSS, M_BC_LAMBDA = range(6)   # metrics slots (SACTD3_M_*); the last two: TD3+BC only
ACT_AFTER_ALL = 1   # sactd3_predict_begin flags
SRC_ORDERED = 1     # sactd3_rb_extend_fields_device / sactd3_rb_extend_records_device / sactd3_load_batch_device / sactd3_predict_device / sactd3_qvalues_device / sactd3_rb_sample_indices_device / sactd3_batch_weights_device flags
DST_ORDERED = 1     # sactd3_read_batch_device / sactd3_rb_read_rows_device / sactd3_td_errors_device flags (the same bit, the same two events)
Q_ONLINE, Q_TARGET = 0, 1   # sactd3_qvalues / sactd3_qvalues_device `which`
PI_ONLINE, PI_TARGET = 0, 1   # sactd3_policy / sactd3_policy_device `which` (the target actor: TD3 only)
ESTATE, EINVAL = -3, -1
DRAW_UNIFORM, DRAW_PRIORITIZED = 0, 1   # sactd3_sampling.draw
DRAW_MIXED = 2                          # ... the mixed draw over pinned and live rows (sactd3_rb_pin / sactd3_rb_set_mix)
DRAW_HINDSIGHT = 3                      # ... the uniform draw with goals relabelled while the rows are staged (sactd3_hindsight_configure)

# every symbol include/sactd3.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = [
    "sactd3_abi_version", "sactd3_default_config", "sactd3_create", "sactd3_destroy", "sactd3_last_error",
    "sactd3_param_count", "sactd3_get_params", "sactd3_set_params", "sactd3_get_adam_state", "sactd3_set_adam_state",
    "sactd3_rb_extend", "sactd3_rb_len", "sactd3_rb_sample", "sactd3_rb_sample_with_indices", "sactd3_load_batch",
    "sactd3_read_batch", "sactd3_rb_fill_synthetic", "sactd3_set_noise", "sactd3_clear_noise", "sactd3_read_noise",
    "sactd3_update_qnets", "sactd3_update_actor", "sactd3_update_targ_nets", "sactd3_step", "sactd3_predict",
    "sactd3_read_metrics", "sactd3_sync", "sactd3_debug_read", "sactd3_debug_names", "sactd3_graph_kernel_count",
    "sactd3_time_kernel", "sactd3_time_gather_sweep", "sactd3_time_nodes", "sactd3_rb_layout", "sactd3_rb_extend_device", "sactd3_step_period", "sactd3_step_prefix", "sactd3_instantiate_graphs", "sactd3_device_handles",
    "sactd3_predict_begin", "sactd3_predict_end", "sactd3_acting_stats",
    "sactd3_rb_extend_fields_device", "sactd3_load_batch_device", "sactd3_boundary_stats",
    "sactd3_predict_device", "sactd3_predict_device_stats",
    "sactd3_read_batch_device", "sactd3_rb_read_rows_device", "sactd3_readout_stats",
    "sactd3_qvalues_device", "sactd3_qvalues", "sactd3_qvalues_stats",
    "sactd3_rb_sample_indices_device", "sactd3_batch_weights_device", "sactd3_td_errors_device", "sactd3_priority_stats",
    "sactd3_prio_enable", "sactd3_rb_sample_prioritized", "sactd3_prio_set_uniforms", "sactd3_prio_update_from_td", "sactd3_prio_update_device",
    "sactd3_prio_stats",
    "sactd3_rb_sample_nstep_device", "sactd3_rb_sample_nstep", "sactd3_rb_sample_prioritized_nstep", "sactd3_nstep_info_device",
    "sactd3_nstep_stats",
    "sactd3_step_sampled", "sactd3_step_sampled_stats",
    "sactd3_step_periods", "sactd3_step_periods_stats",
    "sactd3_set_bc", "sactd3_get_bc",
    "sactd3_rb_pin", "sactd3_rb_pinned", "sactd3_rb_set_mix", "sactd3_rb_sample_mixed", "sactd3_mix_stats",
    "sactd3_policy_device", "sactd3_policy", "sactd3_policy_stats",
    "sactd3_get_config", "sactd3_rb_extend_records_device", "sactd3_batch_generation",
    "sactd3_hindsight_configure", "sactd3_rb_sample_hindsight", "sactd3_rb_sample_hindsight_device", "sactd3_hindsight_info_device",
    "sactd3_hindsight_stats",
]

# every symbol include/sactd3_env.h declares (tests/test_env_host.py checks the header against this list)
ENV_SYMBOLS = [
    "sactd3_env_create", "sactd3_env_destroy", "sactd3_env_last_error", "sactd3_env_spec", "sactd3_env_reset", "sactd3_env_step",
    "sactd3_env_sample_actions", "sactd3_env_episode_stats", "sactd3_env_get_state", "sactd3_env_set_state",
]
ENV_PENDULUM, ENV_CARTPOLE, ENV_POINTGOAL = 0, 1, 2   # sactd3_env_config.kind
ENV_STATE_DIM = 4                   # SACTD3_ENV_STATE_DIM

# every symbol include/sactd3_rollout.h declares (tests/test_native_rollout_host.py checks the header against this list)
ROLLOUT_SYMBOLS = [
    "sactd3_rollout_env_step", "sactd3_rollout_create", "sactd3_rollout_destroy", "sactd3_rollout_last_error", "sactd3_rollout_reset",
    "sactd3_rollout_choose", "sactd3_rollout_advance", "sactd3_rollout_stats",
]
ROLLOUT_RANDOM, ROLLOUT_EXPLORE, ROLLOUT_EXPLOIT, ROLLOUT_REPEAT = range(4)   # sactd3_rollout_choose `mode` (SACTD3_ROLLOUT_*)
# every symbol include/sactd3_rollout_cycle.h declares -- the header sactd3_rollout.h ends with (tests/test_rollout_cycle_host.py checks it
# against this list)
ROLLOUT_CYCLE_SYMBOLS = ["sactd3_rollout_cycle", "sactd3_rollout_cycle_stats", "sactd3_rollout_cycle_clamped"]
# every symbol include/sactd3_rollout_collect.h declares -- the header behind it (tests/test_collect_host.py checks it against this list)
ROLLOUT_COLLECT_SYMBOLS = ["sactd3_rollout_collect", "sactd3_rollout_collect_stats"]
COLLECT_MAX_STEPS = 4096            # SACTD3_COLLECT_MAX_STEPS
STREAM_COLLECT = 0x900              # csrc/collect_kernels.h: SACTD3_STREAM_COLLECT
# every symbol include/sactd3_init.h declares (tests/test_param_init_host.py checks the header against this list)
INIT_SYMBOLS = ["sactd3_init_params", "sactd3_init_stats"]
INIT_ACTOR, INIT_CRITICS, INIT_ALPHA = 1, 2, 4   # sactd3_init_params `what` (SACTD3_INIT_*)
INIT_ALL = INIT_ACTOR | INIT_CRITICS | INIT_ALPHA
# every symbol include/sactd3_eval.h declares (tests/test_eval_rollout_host.py checks the header against this list)
EVAL_SYMBOLS = ["sactd3_eval_rollout", "sactd3_eval_stats"]
EVAL_GREEDY, EVAL_SAMPLE = 0, 1     # sactd3_eval_config.mode (SACTD3_EVAL_*)
EVAL_MAX_STEPS = 4096               # SACTD3_EVAL_MAX_STEPS
STREAM_EVAL = 0x800                 # csrc/eval_kernels.h: SACTD3_STREAM_EVAL
# the outputs of sactd3_eval_out, in the header's order: (name, width: "o" = ob_dim, "a" = ac_dim; rows: "T" = [T][n], "n" = [n], 1 = one word; dtype)
EVAL_OUT_FIELDS = (("obs", "o", "T", "float32"), ("actions", "a", "T", "float32"), ("eps", "a", "T", "float32"), ("reward", 1, "T", "float32"),
                   ("logp", 1, "T", "float32"), ("rtg", 1, "T", "float32"), ("live", 1, "T", "uint8"), ("ep_return", 1, "n", "float32"),
                   ("ep_length", 1, "n", "int32"), ("ep_terminated", 1, "n", "uint8"), ("g0", 1, "n", "float32"), ("alpha", 1, 1, "float32"))


class EngineError(RuntimeError):
    pass


class CConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "ob_dim", "ac_dim", "batch_size", "rb_capacity", "max_envs", "prefer_td3_over_sac",
        "layer_norm", "autotune", "bcq_style_targ_mix", "targ_actor_smoothing", "actor_update_delay",
        "crit_targ_update_freq", "use_graphs", "device_id", "reserved0")] + [(n, C.c_float) for n in (
        "actor_lr", "qnets_lr", "log_alpha_lr", "gamma", "polyak", "alpha_init", "clip_norm", "td3_std", "td3_c",
        "actor_noise_std", "adam_beta1", "adam_beta2", "adam_eps", "bc_alpha")] + [("seed", C.c_uint64)]


class CDeviceFields(C.Structure):
    """sactd3_device_fields: five device pointers, each with its row stride in elements"""
    _fields_ = [(n, t) for f in ("obs", "actions", "rewards", "next_obs", "dones") for n, t in ((f, C.c_void_p), (f + "_ld", C.c_int64))]


class CDeviceFieldsOut(C.Structure):
    """sactd3_device_fields_out: six device pointers (None = field not wanted), each with its row stride in elements"""
    _fields_ = [(n, t) for f in ("obs", "actions", "rewards", "next_obs", "dones", "index") for n, t in ((f, C.c_void_p), (f + "_ld", C.c_int64))]


class CSampling(C.Structure):
    """sactd3_sampling: how sactd3_step_sampled draws and stages its batch"""
    _fields_ = [("draw", C.c_int32), ("n_step", C.c_int32), ("stride", C.c_int32), ("beta", C.c_float)]


# the fields of sactd3_policy_io, in the header's order: two inputs, seven outputs; (name, width: "a" = ac_dim)
POLICY_IO_FIELDS = (("actions", "a"), ("eps", "a"), ("mode", "a"), ("mean", "a"), ("log_std", "a"), ("sample", "a"),
                    ("sample_logp", 1), ("action_logp", 1), ("eps_out", "a"))


class CPolicyIO(C.Structure):
    """sactd3_policy_io: nine pointers (None = not given / not wanted), each with its row stride in elements"""
    _fields_ = [(n, t) for f, _ in POLICY_IO_FIELDS for n, t in ((f, C.c_void_p), (f + "_ld", C.c_int64))]


class CHindsightConfig(C.Structure):
    """sactd3_hindsight_config"""
    _fields_ = [(n, C.c_int32) for n in ("ag_off", "dg_off", "goal_dim", "window", "stride")] + [("threshold", C.c_float), ("ratio", C.c_float)]


class CEnvConfig(C.Structure):
    """sactd3_env_config"""
    _fields_ = [("kind", C.c_int32), ("num_envs", C.c_int32), ("horizon", C.c_int32), ("device_id", C.c_int32), ("seed", C.c_uint64)]


class CEnvInfo(C.Structure):
    """sactd3_env_info"""
    _fields_ = [("ob_dim", C.c_int32), ("ac_dim", C.c_int32), ("horizon", C.c_int32), ("num_envs", C.c_int32), ("min_ac", C.c_float), ("max_ac", C.c_float)]


class CEnvOut(C.Structure):
    """sactd3_env_out: six device pointers (None = not wanted; obs is required), each with its row stride in elements"""
    _fields_ = [(n, t) for f in ("obs", "final_obs", "reward", "terminated", "truncated", "ended") for n, t in ((f, C.c_void_p), (f + "_ld", C.c_int64))]


class CEnvState(C.Structure):
    """sactd3_env_state: five host arrays (None = skipped)"""
    _fields_ = [(n, C.c_void_p) for n in ("phys", "steps", "episode", "returns", "draws")]


class CEnvStats(C.Structure):
    """sactd3_env_stats: four totals, five per-env host arrays (None = not wanted)"""
    _fields_ = [("episodes", C.c_int64), ("return_sum", C.c_double), ("length_sum", C.c_int64), ("bad_actions", C.c_int64),
                ("last_return", C.c_void_p), ("last_length", C.c_void_p), ("env_episodes", C.c_void_p),
                ("first_return", C.c_void_p), ("first_length", C.c_void_p)]


class CRecordLayout(C.Structure):
    """sactd3_record_layout: the first three values of sactd3_rb_layout"""
    _fields_ = [("record_len", C.c_int32), ("next_off", C.c_int32), ("next_width", C.c_int32)]


class CRolloutBuffers(C.Structure):
    """sactd3_rollout_buffers: obs and actions with their row strides in elements, the contiguous record slab"""
    _fields_ = [("obs", C.c_void_p), ("obs_ld", C.c_int64), ("actions", C.c_void_p), ("actions_ld", C.c_int64), ("records", C.c_void_p)]


class CEvalConfig(C.Structure):
    """sactd3_eval_config"""
    _fields_ = [("steps", C.c_int32), ("mode", C.c_int32), ("reset", C.c_int32), ("soft", C.c_int32), ("gamma", C.c_float), ("seed", C.c_uint64)]


class CEvalOut(C.Structure):
    """sactd3_eval_out: twelve device pointers (None = not wanted)"""
    _fields_ = [(f[0], C.c_void_p) for f in EVAL_OUT_FIELDS]


def library_path() -> str:
    """In-tree build product; SACTD3_LIBRARY overrides it (A/B-testing kernel variants)."""
    return os.environ.get("SACTD3_LIBRARY") or os.path.join(_HERE, "libsactd3_hip.so")


def build_library(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> libsactd3_hip.so in-tree (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")] + (["-B"] if force else [])
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return library_path()


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise EngineError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C sac-td3-cudagraphs-pytorch_amd/csrc`). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.  If our library (linked against
    # /opt/rocm's) were loaded first, a later `import torch` would bring a second runtime that finds no GPU.  Importing
    # torch first makes the dynamic linker resolve our dependency to the copy already loaded.  (No torch: nothing to do.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    fp, u8p, i64p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.c_void_p
    sig = {
        "sactd3_abi_version": (C.c_int, []),
        "sactd3_default_config": (None, [C.POINTER(CConfig), C.c_int]),
        "sactd3_create": (C.c_int, [C.POINTER(CConfig), fp, fp, C.POINTER(vp)]),
        "sactd3_destroy": (None, [vp]),
        "sactd3_last_error": (C.c_char_p, [vp]),
        "sactd3_param_count": (C.c_int64, [vp, C.c_int]),
        "sactd3_get_params": (C.c_int, [vp, C.c_int, fp]),
        "sactd3_set_params": (C.c_int, [vp, C.c_int, fp]),
        "sactd3_get_adam_state": (C.c_int, [vp, C.c_int, fp, fp, i64p]),
        "sactd3_set_adam_state": (C.c_int, [vp, C.c_int, fp, fp, C.c_int64]),
        "sactd3_rb_extend": (C.c_int, [vp, fp, fp, fp, fp, u8p, C.c_int]),
        "sactd3_rb_len": (C.c_int64, [vp]),
        "sactd3_batch_generation": (C.c_int64, [vp]),
        "sactd3_rb_layout": (C.c_int, [vp, C.POINTER(C.c_int32)]),
        "sactd3_rb_extend_device": (C.c_int, [vp, C.c_void_p, C.c_int]),
        "sactd3_rb_sample": (C.c_int, [vp]),
        "sactd3_rb_sample_with_indices": (C.c_int, [vp, i64p, C.c_int]),
        "sactd3_load_batch": (C.c_int, [vp, fp, fp, fp, fp, u8p, C.c_int]),
        "sactd3_read_batch": (C.c_int, [vp, fp, fp, fp, fp, u8p, i64p]),
        "sactd3_rb_fill_synthetic": (C.c_int, [vp, C.c_int64, C.c_uint64]),
        "sactd3_set_noise": (C.c_int, [vp, C.c_int, fp, C.c_int]),
        "sactd3_clear_noise": (C.c_int, [vp, C.c_int]),
        "sactd3_read_noise": (C.c_int, [vp, C.c_int, fp, C.c_int]),
        "sactd3_update_qnets": (C.c_int, [vp]),
        "sactd3_update_actor": (C.c_int, [vp]),
        "sactd3_update_targ_nets": (C.c_int, [vp, C.c_int64]),
        "sactd3_step": (C.c_int, [vp, C.c_int]),
        "sactd3_step_period": (C.c_int, [vp]),
        "sactd3_step_prefix": (C.c_int, [vp, C.c_int]),
        "sactd3_instantiate_graphs": (C.c_int, [vp]),
        "sactd3_predict": (C.c_int, [vp, fp, C.c_int, C.c_int, fp]),
        "sactd3_predict_begin": (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_int]),
        "sactd3_predict_end": (C.c_int, [vp, fp]),
        "sactd3_acting_stats": (C.c_int, [vp, i64p]),
        "sactd3_rb_extend_fields_device": (C.c_int, [vp, C.POINTER(CDeviceFields), C.c_int, vp, C.c_int]),
        "sactd3_load_batch_device": (C.c_int, [vp, C.POINTER(CDeviceFields), C.c_int, vp, C.c_int]),
        "sactd3_boundary_stats": (C.c_int, [vp, i64p]),
        "sactd3_predict_device": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int]),
        "sactd3_predict_device_stats": (C.c_int, [vp, i64p]),
        "sactd3_read_batch_device": (C.c_int, [vp, C.POINTER(CDeviceFieldsOut), vp, C.c_int]),
        "sactd3_rb_read_rows_device": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.POINTER(CDeviceFieldsOut), vp, C.c_int]),
        "sactd3_readout_stats": (C.c_int, [vp, i64p]),
        "sactd3_qvalues_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp, C.c_int]),
        "sactd3_qvalues": (C.c_int, [vp, fp, fp, C.c_int, C.c_int, fp]),
        "sactd3_qvalues_stats": (C.c_int, [vp, i64p]),
        "sactd3_rb_sample_indices_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int]),
        "sactd3_batch_weights_device": (C.c_int, [vp, vp, C.c_int64, C.c_int, vp, C.c_int]),
        "sactd3_td_errors_device": (C.c_int, [vp, vp, C.c_int64, C.c_int64, vp, C.c_int]),
        "sactd3_priority_stats": (C.c_int, [vp, i64p]),
        "sactd3_prio_enable": (C.c_int, [vp, C.c_float, C.c_float]),
        "sactd3_rb_sample_prioritized": (C.c_int, [vp, C.c_float]),
        "sactd3_prio_set_uniforms": (C.c_int, [vp, fp, C.c_int]),
        "sactd3_prio_update_from_td": (C.c_int, [vp]),
        "sactd3_prio_update_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int]),
        "sactd3_prio_stats": (C.c_int, [vp, i64p]),
        "sactd3_rb_sample_nstep_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, C.c_int]),
        "sactd3_rb_sample_nstep": (C.c_int, [vp, C.c_int, C.c_int]),
        "sactd3_rb_sample_prioritized_nstep": (C.c_int, [vp, C.c_float, C.c_int, C.c_int]),
        "sactd3_nstep_info_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int]),
        "sactd3_nstep_stats": (C.c_int, [vp, i64p]),
        "sactd3_step_sampled": (C.c_int, [vp, C.c_int, C.POINTER(CSampling)]),
        "sactd3_step_sampled_stats": (C.c_int, [vp, i64p]),
        "sactd3_step_periods": (C.c_int, [vp, C.c_int]),
        "sactd3_step_periods_stats": (C.c_int, [vp, i64p]),
        "sactd3_set_bc": (C.c_int, [vp, C.c_float, C.c_float]),
        "sactd3_get_bc": (C.c_int, [vp, fp]),
        "sactd3_rb_pin": (C.c_int, [vp, C.c_int64]),
        "sactd3_rb_pinned": (C.c_int64, [vp]),
        "sactd3_rb_set_mix": (C.c_int, [vp, C.c_int]),
        "sactd3_rb_sample_mixed": (C.c_int, [vp]),
        "sactd3_mix_stats": (C.c_int, [vp, i64p]),
        "sactd3_policy_device": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, C.POINTER(CPolicyIO), vp, C.c_int]),
        "sactd3_policy": (C.c_int, [vp, fp, C.c_int, C.c_int, C.POINTER(CPolicyIO)]),
        "sactd3_policy_stats": (C.c_int, [vp, i64p]),
        "sactd3_get_config": (C.c_int, [vp, C.POINTER(CConfig)]),
        "sactd3_rb_extend_records_device": (C.c_int, [vp, vp, C.c_int, vp, C.c_int]),
        "sactd3_hindsight_configure": (C.c_int, [vp, C.POINTER(CHindsightConfig)]),
        "sactd3_rb_sample_hindsight": (C.c_int, [vp]),
        "sactd3_rb_sample_hindsight_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int]),
        "sactd3_hindsight_info_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int]),
        "sactd3_hindsight_stats": (C.c_int, [vp, i64p]),
        "sactd3_read_metrics": (C.c_int, [vp, fp]),
        "sactd3_sync": (C.c_int, [vp]),
        "sactd3_device_handles": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
        "sactd3_debug_read": (C.c_int64, [vp, C.c_char_p, fp, C.c_int64]),
        "sactd3_debug_names": (C.c_char_p, []),
        "sactd3_graph_kernel_count": (C.c_int, [vp, C.c_int]),
        "sactd3_time_kernel": (C.c_int, [vp, C.c_char_p, C.c_int, fp]),
        "sactd3_time_gather_sweep": (C.c_int, [vp, C.c_int, C.c_int, fp, C.POINTER(C.c_double)]),
        "sactd3_time_nodes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, fp, C.POINTER(C.c_double), C.POINTER(C.c_double), i64p]),
    }
    assert sorted(sig) == sorted(SYMBOLS)
    env_sig = {
        "sactd3_env_create": (C.c_int, [C.POINTER(CEnvConfig), C.POINTER(vp)]),
        "sactd3_env_destroy": (None, [vp]),
        "sactd3_env_last_error": (C.c_char_p, [vp]),
        "sactd3_env_spec": (C.c_int, [vp, C.POINTER(CEnvInfo)]),
        "sactd3_env_reset": (C.c_int, [vp, C.c_uint64, vp, C.c_int64, vp]),
        "sactd3_env_step": (C.c_int, [vp, vp, C.c_int64, C.POINTER(CEnvOut), vp]),
        "sactd3_env_sample_actions": (C.c_int, [vp, vp, C.c_int64, vp]),
        "sactd3_env_episode_stats": (C.c_int, [vp, C.POINTER(CEnvStats), vp]),
        "sactd3_env_get_state": (C.c_int, [vp, C.POINTER(CEnvState), vp]),
        "sactd3_env_set_state": (C.c_int, [vp, C.POINTER(CEnvState), vp]),
    }
    assert sorted(env_sig) == sorted(ENV_SYMBOLS)
    sig.update(env_sig)
    rollout_sig = {
        "sactd3_rollout_env_step": (C.c_int, [vp, vp, C.c_int64, C.POINTER(CRecordLayout), vp, vp, C.c_int64, vp]),
        "sactd3_rollout_create": (C.c_int, [vp, vp, C.POINTER(CRolloutBuffers), vp, C.POINTER(vp)]),
        "sactd3_rollout_destroy": (None, [vp]),
        "sactd3_rollout_last_error": (C.c_char_p, [vp]),
        "sactd3_rollout_reset": (C.c_int, [vp, C.c_uint64]),
        "sactd3_rollout_choose": (C.c_int, [vp, C.c_int]),
        "sactd3_rollout_advance": (C.c_int, [vp]),
        "sactd3_rollout_stats": (C.c_int, [vp, i64p]),
    }
    assert sorted(rollout_sig) == sorted(ROLLOUT_SYMBOLS)
    sig.update(rollout_sig)
    cycle_sig = {
        "sactd3_rollout_cycle": (C.c_int, [vp, C.c_int, C.c_int]),
        "sactd3_rollout_cycle_stats": (C.c_int, [vp, i64p]),
        "sactd3_rollout_cycle_clamped": (C.c_int, [vp, i64p]),
    }
    assert sorted(cycle_sig) == sorted(ROLLOUT_CYCLE_SYMBOLS)
    sig.update(cycle_sig)
    collect_sig = {
        "sactd3_rollout_collect": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
        "sactd3_rollout_collect_stats": (C.c_int, [vp, i64p]),
    }
    assert sorted(collect_sig) == sorted(ROLLOUT_COLLECT_SYMBOLS)
    sig.update(collect_sig)
    init_sig = {
        "sactd3_init_params": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_uint32]),
        "sactd3_init_stats": (C.c_int, [vp, i64p]),
    }
    assert sorted(init_sig) == sorted(INIT_SYMBOLS)
    sig.update(init_sig)
    eval_sig = {
        "sactd3_eval_rollout": (C.c_int, [vp, vp, C.POINTER(CEvalConfig), C.POINTER(CEvalOut), vp, C.c_int]),
        "sactd3_eval_stats": (C.c_int, [vp, i64p]),
    }
    assert sorted(eval_sig) == sorted(EVAL_SYMBOLS)
    sig.update(eval_sig)
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError here = the .so does not export what the header declares
        fn.restype, fn.argtypes = res, args
    if lib.sactd3_abi_version() != ABI_VERSION:
        raise EngineError("libsactd3_hip.so ABI version mismatch; rebuild it")
    _LIB = lib
    return lib
