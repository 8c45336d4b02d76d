"""CPU: the host side of the rollout cycle (include/sactd3_rollout_cycle.h) -- the header, the binding and the built library cover each
other, a NULL handle is refused, the new kernel lives outside engine.hip behind its small internal header, and the keyword rules of
`fused_rollout` in loop.rollout_for / loop.update_plan / loop.train and in the launcher, each asked before an agent is touched."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, envs, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def declared(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src)))


def test_header_binding_and_library_cover_each_other():
    cycle, rollout = text("include", "sactd3_rollout_cycle.h"), text("include", "sactd3_rollout.h")
    assert declared(cycle) == sorted(_lib.ROLLOUT_CYCLE_SYMBOLS) and len(_lib.ROLLOUT_CYCLE_SYMBOLS) == 3
    assert '#include "sactd3_rollout_cycle.h"' in rollout                                     # whoever includes the rollout's header has them
    assert rollout.index("typedef struct sactd3_rollout sactd3_rollout;") < rollout.index('#include "sactd3_rollout_cycle.h"')
    assert not set(_lib.ROLLOUT_CYCLE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ENV_SYMBOLS) | set(_lib.ROLLOUT_SYMBOLS))
    assert "boundary_stats" in cycle and _lib.ABI_VERSION == 1                                # the one counter that may differ is named
    assert re.search(r"#define\s+SACTD3_ABI_VERSION\s+1\b", text("include", "sactd3.h"))
    P.build_library()                                                                         # hipcc --offload-arch=gfx950 (a no-op when current)
    raw = C.CDLL(P.library_path())
    for name in _lib.ROLLOUT_CYCLE_SYMBOLS:
        assert hasattr(raw, name), f"{name} is declared but not exported"
    lib = P.load_library()
    assert lib.sactd3_rollout_cycle.argtypes == [C.c_void_p, C.c_int, C.c_int]
    # a C compiler takes the header through the rollout's
    probe = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], capture_output=True, text=True,
                           input='#include "sactd3_rollout.h"\nint f(sactd3_rollout* r) { int64_t o[4]; return sactd3_rollout_cycle(r, SACTD3_ROLLOUT_EXPLORE, 1) + sactd3_rollout_cycle_stats(r, o); }\n')
    assert probe.returncode == 0, probe.stderr[-2000:]


def test_a_null_handle_is_refused():
    lib = P.load_library()
    for mode in range(5):
        assert lib.sactd3_rollout_cycle(None, mode, 1) == _lib.EINVAL
    assert lib.sactd3_rollout_cycle_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL
    assert lib.sactd3_rollout_cycle_clamped(None, C.byref(C.c_int64())) == _lib.EINVAL


def test_the_new_kernel_is_a_translation_unit_of_its_own():
    """engine.hip gains host code only: k_rb_ingest_g stands in rollout_cycle.hip, engine.hip and env.hip reach it and each other through
    rollout_cycle.h, and the library's build lists the new unit"""
    unit, header, engine, env = (text(CSRC, n) for n in ("rollout_cycle.hip", "rollout_cycle.h", "engine.hip", "env.hip"))
    assert re.findall(r"__global__[^\n]*\bvoid\s+(\w+)", unit) == ["k_rb_ingest_g", "k_rb_publish_g"]
    assert re.findall(r'#include "([^"]+)"', unit) == ["rollout_cycle.h"] and "DevCtl" not in unit
    assert "__global__" not in header and "rb_ingest_g_launch" in header and "engine_rollout_cycle" in header
    assert '#include "rollout_cycle.h"' in engine and '#include "rollout_cycle.h"' in env
    assert "k_rb_ingest_g<<<" not in engine and not re.search(r"__global__[^\n]*k_rb_ingest_g", engine)
    assert "rollout_cycle.hip" in text(CSRC, "Makefile")


CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:
    """an agent (an env) that fails on any attribute access: a refusal must come before either is touched"""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


PLAN = dict(fused=True, sampler=None, prioritized=None, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1)
# keyword changes -> a word of the refusal; every one WITH fused_rollout=True
EXCLUDED = [
    (dict(fused=False), "fused=True"),
    (dict(fused=False, n_step=3, one_launch=True), "fused=True"),                             # ... whatever else the call says
    (dict(sampler=object()), "sampler"),
    (dict(prioritized=dict(alpha=0.6)), "prioritized"),
    (dict(n_step=3), "n_step"),
    (dict(prior_fraction=0.25), "prior_fraction"),
    (dict(hindsight=dict(achieved=0, desired=2, dim=2, threshold=0.05)), "hindsight"),
    (dict(one_launch=True), "one_launch"),
]


@pytest.mark.parametrize("change,word", EXCLUDED, ids=[f"{'-'.join(c)}" for c, _ in EXCLUDED])
def test_update_plan_refuses_what_fused_rollout_excludes(change, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match="fused_rollout=True") as ex:
        loop.update_plan(cfg, **dict(PLAN, **change), fused_rollout=True)
    assert word in str(ex.value)
    with pytest.raises(ValueError, match="fused_rollout=True"):                              # ... and train() before it touches anything
        loop.train(cfg, Untouchable(), Untouchable(), device_env=True, native_rollout=True, fused_rollout=True,
                   **{k: v for k, v in dict(PLAN, **change).items() if k != "updates_per_step"})


@pytest.mark.parametrize("field", ["segment_len", "action_repeat"])
def test_update_plan_refuses_a_segment_or_a_repeat_other_than_one(field):
    cfg = SimpleNamespace(**dict(CFG, **{field: 2}))
    with pytest.raises(ValueError, match=field):
        loop.update_plan(cfg, **PLAN, fused_rollout=True)
    with pytest.raises(ValueError, match=field):
        loop.train(cfg, Untouchable(), Untouchable(), device_env=True, native_rollout=True, fused_rollout=True)
    loop.update_plan(cfg, **PLAN)                                                             # without the keyword: the plan it was
    assert loop.update_plan(SimpleNamespace(**CFG), **PLAN, fused_rollout=True).updates_per_step == 1
    assert loop.update_plan(SimpleNamespace(**CFG), **dict(PLAN, updates_per_step=2), fused_rollout=True).updates_per_step == 2
    assert loop.update_plan(SimpleNamespace(batch_size=4), **PLAN).updates_per_step == 1      # off: cfg needs neither field


def test_rollout_for_refuses_before_it_looks_at_the_env():
    with pytest.raises(ValueError, match="native_rollout=True"):
        loop.rollout_for(Untouchable(), overlap=False, device_env=True, native_rollout=False, fused_rollout=True)
    with pytest.raises(ValueError, match="native_rollout=True"):
        loop.rollout_for(Untouchable(), overlap=False, device_env=False, native_rollout=False, fused_rollout=True)
    with pytest.raises(ValueError, match="overlap"):
        loop.rollout_for(Untouchable(), overlap=True, device_env=True, native_rollout=True, fused_rollout=True)
    with pytest.raises(TypeError, match="step_records"):                                      # the native rollout's own rules behind them
        loop.rollout_for(envs.HostVecEnv("pendulum", 2), overlap=False, device_env=True, native_rollout=True, fused_rollout=True)
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match="native_rollout=True"):
        loop.train(cfg, Untouchable(), Untouchable(), device_env=True, fused_rollout=True)
    with pytest.raises(ValueError, match="overlap"):
        loop.train(cfg, Untouchable(), Untouchable(), device_env=True, native_rollout=True, overlap=True, fused_rollout=True)
    assert loop.rollout_for(None, overlap=False, device_env=True, native_rollout=False) is loop.DeviceRollout      # off: what it was
    assert callable(loop.NativeRollout.cycle) and callable(loop.NativeRollout.cycle_stats)


def test_the_launcher_maps_and_refuses_the_flag():
    cfg = launcher.job_config("sac", "Pendulum-native", 0)
    facts = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False,
                 device_env=True, native_rollout=True, policy_stats=0)
    kw = launcher.train_keywords(cfg, **facts, fused_rollout=True)
    assert kw["fused_rollout"] is True and kw["fused"] is True and kw["native_rollout"] is True
    assert "fused_rollout" not in launcher.train_keywords(cfg, **facts)                       # a key only when the flag was given
    for change, word in ((dict(native_rollout=False), "native_rollout"), (dict(prioritized=True), "fused=True"), (dict(n_step=3), "fused=True"),
                         (dict(prior_fraction=0.5), "fused=True")):
        with pytest.raises(ValueError, match="fused_rollout=True") as ex:
            launcher.train_keywords(cfg, **dict(facts, **change), fused_rollout=True)
        assert word in str(ex.value)
    with pytest.raises(ValueError, match="action_repeat"):
        launcher.train_keywords(launcher.job_config("sac", "Pendulum-native", 0, action_repeat=2), **facts, fused_rollout=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run", "--env_bundle", "native"]

    def run(*more):
        return subprocess.run(base + list(more), capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    out = run("--device_env", "--native_rollout", "--fused_rollout")
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert len(jobs) == 2 and all(j["rollout"] == "NativeRollout" and j["fused_rollout"] is True and j["dry_run"] for j in jobs)
    out = run("--device_env", "--native_rollout")
    assert out.returncode == 0 and all("fused_rollout" not in json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB "))
    for more, word in ((("--device_env", "--fused_rollout"), "native_rollout"), (("--fused_rollout",), "native_rollout"),
                       (("--device_env", "--native_rollout", "--fused_rollout", "--prioritized"), "fused_rollout"),
                       (("--device_env", "--native_rollout", "--fused_rollout", "--n_step", "3"), "fused_rollout"),
                       (("--device_env", "--native_rollout", "--fused_rollout", "--overlap_acting"), "overlap")):
        out = run(*more)
        assert out.returncode == 2 and word in out.stderr and "JOB " not in out.stdout, (more, out.stderr[-500:])
