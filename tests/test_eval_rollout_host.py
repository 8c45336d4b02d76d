"""The one-launch evaluation rollout without a GPU: include/sactd3_eval.h, the binding and the library agree; the compiler's resource
remarks for the translation unit that holds the kernel show no scratch; and the default paths of greedy_returns / device_episodes are
what they were, with the new keyword refused on the host twin."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

P = pytest.importorskip("sac_td3_cudagraphs_pytorch_amd")
from sac_td3_cudagraphs_pytorch_amd import _lib, envs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the header, the binding, the library
def test_header_binding_and_library_cover_each_other():
    header = text("include", "sactd3_eval.h")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_eval_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.EVAL_SYMBOLS) and len(_lib.EVAL_SYMBOLS) == 2
    others = set(_lib.SYMBOLS) | set(_lib.ENV_SYMBOLS) | set(_lib.ROLLOUT_SYMBOLS) | set(_lib.ROLLOUT_CYCLE_SYMBOLS) | set(_lib.INIT_SYMBOLS)
    assert not set(_lib.EVAL_SYMBOLS) & others
    assert _lib.ABI_VERSION == 1 and re.search(r"#define\s+SACTD3_ABI_VERSION\s+1\b", text("include", "sactd3.h"))
    defines = dict(re.findall(r"#define\s+(SACTD3_EVAL_[A-Z_]+)\s+(\d+)", header))
    assert {k: int(v) for k, v in defines.items()} == {"SACTD3_EVAL_GREEDY": _lib.EVAL_GREEDY, "SACTD3_EVAL_SAMPLE": _lib.EVAL_SAMPLE,
                                                       "SACTD3_EVAL_MAX_STEPS": _lib.EVAL_MAX_STEPS}
    assert "0x800" in header and "SACTD3_STREAM_EVAL 0x800u" in text(CSRC, "eval_kernels.h") and _lib.STREAM_EVAL == 0x800
    for phrase in ("learner stream", "No host wait", "invisible to training and acting", "Refused with nothing changed"):
        assert phrase in header, phrase
    # the structs: the C compiler's layout is the binding's, field by field
    fields_c = [f for f, _ in _lib.CEvalConfig._fields_]
    fields_o = [f for f, _ in _lib.CEvalOut._fields_]
    assert fields_o == [f[0] for f in _lib.EVAL_OUT_FIELDS] == re.findall(r"\*\s*(\w+)\s*[,;]", re.search(r"typedef struct sactd3_eval_out \{(.*?)\}", code, re.S).group(1))
    P.build_library()                                                                         # hipcc --offload-arch=gfx950 (a no-op when current)
    assert C.sizeof(_lib.CEvalConfig) == 32 and _lib.CEvalConfig.seed.offset == 24 and _lib.CEvalConfig.gamma.offset == 16
    assert C.sizeof(_lib.CEvalOut) == 12 * C.sizeof(C.c_void_p)
    raw = C.CDLL(P.library_path())
    for name in _lib.EVAL_SYMBOLS:
        assert hasattr(raw, name), f"{name} is declared but not exported"
    lib = P.load_library()
    assert lib.sactd3_eval_rollout.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(_lib.CEvalConfig), C.POINTER(_lib.CEvalOut), C.c_void_p, C.c_int]
    # NULL handles are refused without a device
    out = (C.c_int64 * 4)()
    assert lib.sactd3_eval_rollout(None, None, None, None, None, 0) == _lib.EINVAL and lib.sactd3_eval_stats(None, out) == _lib.EINVAL


def test_the_c_layout_of_the_structs_is_the_bindings():
    fields_c = [f for f, _ in _lib.CEvalConfig._fields_]
    fields_o = [f for f, _ in _lib.CEvalOut._fields_]
    checks = [f"_Static_assert(sizeof(sactd3_eval_config) == {C.sizeof(_lib.CEvalConfig)}, \"config size\");",
              f"_Static_assert(sizeof(sactd3_eval_out) == {C.sizeof(_lib.CEvalOut)}, \"out size\");"]
    checks += [f"_Static_assert(offsetof(sactd3_eval_config, {f}) == {getattr(_lib.CEvalConfig, f).offset}, \"{f}\");" for f in fields_c]
    checks += [f"_Static_assert(offsetof(sactd3_eval_out, {f}) == {getattr(_lib.CEvalOut, f).offset}, \"{f}\");" for f in fields_o]
    probe = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], capture_output=True, text=True,
                           input='#include <stddef.h>\n#include "sactd3_eval.h"\n' + "\n".join(checks) + "\n")
    assert probe.returncode == 0, probe.stderr


# ------------------------------------------------------------------------------------------ the kernel's resources
def test_the_eval_kernels_use_no_scratch(tmp_path):
    """hipcc's resource remarks for env.hip, the translation unit the kernel is compiled in: every k_eval_rollout instance has ScratchSize 0,
    and engine.hip, which gains host code only, names no kernel of the feature"""
    flags = re.search(r"^PRELOAD\s*:=\s*(.*)$", text(CSRC, "Makefile"), re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          "-DSACTD3_BUILD", *flags, "env.hip", "-o", str(tmp_path / "env.s")], cwd=CSRC, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    remarks = run.stderr
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if b.split()[0].startswith("_Z14k_eval_rollout")]
    assert len(mine) == 3, [b.split()[0] for b in blocks]                      # one instance per task
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 160 * 1024
    for b in blocks:                                                           # ... and the env kernels beside it keep theirs
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:200]
    assert "mfma_f32_16x16x4" in (tmp_path / "env.s").read_text()              # layer 2 runs on the matrix cores
    engine = text(CSRC, "engine.hip")
    assert "k_eval_rollout" not in re.sub(r"//.*", "", engine) and "eval_kernels.h" not in re.sub(r"//.*", "", engine)
    deps = re.search(r"^ENV_DEPS\s*:=\s*(.*)$", text(CSRC, "Makefile"), re.M).group(1).split()
    assert {"eval_kernels.h", "eval_rollout.h", "../../include/sactd3_eval.h"} <= set(deps)


# ------------------------------------------------------------------------------------------ the default paths
class LoopAgent:
    """an agent that is no engine: a fixed linear policy on the host"""

    def __init__(self, o, a):
        self.W = np.linspace(-0.5, 0.5, o * a, dtype=np.float32).reshape(o, a)
        self.calls = 0

    def predict(self, in_td, *, explore):
        assert explore is False
        self.calls += 1
        return np.tanh(np.asarray(in_td["observations"], np.float32) @ self.W)


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "pointgoal"])
def test_the_default_paths_are_unchanged_and_the_host_twin_refuses_the_keyword(name):
    assert inspect.signature(envs.greedy_returns).parameters["one_launch"].default is False
    assert inspect.signature(envs.device_episodes).parameters["one_launch"].default is False
    n, seed = 5, 3
    env = envs.HostVecEnv(name, n, seed=seed, horizon=9)
    agent = LoopAgent(env.o, env.a)
    got = envs.greedy_returns(env, agent, n)
    assert agent.calls == env.horizon
    # the loop, restated: reset, one horizon of greedy steps, the first episodes' books
    twin = envs.HostVecEnv(name, n, seed=seed, horizon=9)
    obs, _ = twin.reset(seed=seed)
    for _ in range(twin.horizon):
        obs = twin.step(agent.predict({"observations": obs}, explore=False))[0]
    st = twin.episode_stats()
    assert got["returns"].tobytes() == st["first_return"].tobytes() and got["lengths"].tobytes() == st["first_length"].tobytes()
    assert sorted(got) == ["bad_actions", "episodes", "length", "lengths", "return", "returns"]
    again = envs.greedy_returns(env, agent, n, one_launch=False)
    assert again["returns"].tobytes() == got["returns"].tobytes()
    first = next(envs.device_episodes(env, agent, seed))
    assert set(first) == {"length", "return"}
    for call in (lambda: envs.greedy_returns(env, agent, n, one_launch=True), lambda: next(envs.device_episodes(env, agent, seed, one_launch=True)),
                 lambda: envs.policy_rollout(env, agent), lambda: envs.q_bias(env, agent, seed=1)):
        with pytest.raises(TypeError, match="NativeVecEnv.*physics runs inside the kernel"):
            call()
    assert "one_launch" in envs.greedy_returns.__doc__ and "policy_rollout" in envs.__doc__


# ------------------------------------------------------------------------------------------ the loop's and the launcher's keywords
def test_the_loop_and_the_launcher_check_their_keywords_before_anything_runs(capsys):
    from types import SimpleNamespace
    from sac_td3_cudagraphs_pytorch_amd import launcher, loop
    assert inspect.signature(loop.train).parameters["q_bias"].default is None
    assert inspect.signature(loop.train_offline).parameters["q_bias"].default is None
    assert loop.QBias.KEYS == ("vitals/q_bias_mean", "vitals/q_bias_std", "vitals/q_bias_rows")
    host_env, agent = envs.HostVecEnv("pendulum", 4), SimpleNamespace(engine=None)
    for spec in (4, {}, {"env": host_env}, {"seed": 1}):
        with pytest.raises(ValueError, match="q_bias must be a dict"):
            loop.QBias(agent, spec)
    with pytest.raises(ValueError, match="unknown keys"):
        loop.QBias(agent, {"env": host_env, "seed": 1, "horizon": 3})
    with pytest.raises(TypeError, match="NativeVecEnv"):
        loop.QBias(agent, {"env": host_env, "seed": 1})
    assert loop._vitals(agent, 0, None, 0) is None                          # neither asked for: no object, no call
    # the launcher: both flags need --device_env and a native bundle, and say so in the parent
    ns = lambda **kw: SimpleNamespace(**dict(dict(eval_one_launch=False, q_bias=0, device_env=False, offline_dataset=None), **kw))
    native, foreign = launcher.ENV_BUNDLES["native"], launcher.ENV_BUNDLES["debug"]
    assert launcher.eval_plan(ns(), foreign, False) == {}
    assert launcher.eval_plan(ns(eval_one_launch=True, q_bias=8, device_env=True), native, False) == {"eval_one_launch": True, "q_bias": 8}
    assert launcher.eval_plan(ns(q_bias=8, device_env=True), native, False) == {"q_bias": 8}
    for bad, bundle, factory in ((ns(q_bias=8), native, False), (ns(eval_one_launch=True), native, False),
                                 (ns(q_bias=8, device_env=True), foreign, False), (ns(q_bias=8, device_env=True), native, True),
                                 (ns(q_bias=-1, device_env=True), native, False)):
        with pytest.raises(ValueError, match="--q_bias|--eval_one_launch"):
            launcher.eval_plan(bad, bundle, factory)
    with pytest.raises(SystemExit):
        launcher.main(["--env_bundle", "native", "--q_bias", "4"])
    assert "--device_env" in capsys.readouterr().err
    with pytest.raises(ValueError, match="native env id"):
        launcher.run_job("sac", "Hopper-v4", 0, 0, "unused", q_bias=4, device_env=True)
