"""CPU: the host side of the collected rollout segment (include/sactd3_rollout_collect.h) -- the header, the binding and the built library
cover each other, a NULL handle is refused, the kernel lives in env.hip and uses no scratch, the keyword rules of `collected_rollout`
in loop.rollout_for / loop.train and in the launcher, each asked before an agent or an env is touched, and the loop bodies with and
without the keyword, shown with a stub rollout."""
import ctypes as C
import inspect
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


def code(src):
    return re.sub(r"//.*", "", src)


def test_header_binding_and_library_cover_each_other():
    collect, rollout = text("include", "sactd3_rollout_collect.h"), text("include", "sactd3_rollout.h")
    assert declared(collect) == sorted(_lib.ROLLOUT_COLLECT_SYMBOLS) and len(_lib.ROLLOUT_COLLECT_SYMBOLS) == 2
    assert '#include "sactd3_rollout_collect.h"' in rollout                                   # whoever includes the rollout's header has them
    assert rollout.index("typedef struct sactd3_rollout sactd3_rollout;") < rollout.index('#include "sactd3_rollout_collect.h"')
    others = set(_lib.SYMBOLS) | set(_lib.ENV_SYMBOLS) | set(_lib.ROLLOUT_SYMBOLS) | set(_lib.ROLLOUT_CYCLE_SYMBOLS) | set(_lib.EVAL_SYMBOLS)
    assert not set(_lib.ROLLOUT_COLLECT_SYMBOLS) & others
    assert _lib.ABI_VERSION == 1 and re.search(r"#define\s+SACTD3_ABI_VERSION\s+1\b", text("include", "sactd3.h"))
    assert re.search(r"#define\s+SACTD3_COLLECT_MAX_STEPS\s+4096\b", collect) and _lib.COLLECT_MAX_STEPS == 4096
    assert re.search(r"#define\s+SACTD3_STREAM_COLLECT\s+0x900u\b", text(CSRC, "collect_kernels.h")) and _lib.STREAM_COLLECT == 0x900
    assert "0x900" in collect
    P.build_library()                                                                         # hipcc --offload-arch=gfx950 (a no-op when current)
    raw = C.CDLL(P.library_path())
    for name in _lib.ROLLOUT_COLLECT_SYMBOLS:
        assert hasattr(raw, name), f"{name} is declared but not exported"
    lib = P.load_library()
    assert lib.sactd3_abi_version() == 1
    assert lib.sactd3_rollout_collect.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # a C compiler takes the header through the rollout's, and not on its own
    probe = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], capture_output=True, text=True,
                           input='#include "sactd3_rollout.h"\nint f(sactd3_rollout* r, float* rec) { int64_t o[4]; return '
                                 'sactd3_rollout_collect(r, SACTD3_ROLLOUT_EXPLORE, SACTD3_COLLECT_MAX_STEPS, rec, 0) + sactd3_rollout_collect_stats(r, o); }\n')
    assert probe.returncode == 0, probe.stderr[-2000:]
    alone = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], capture_output=True, text=True,
                           input='#include "sactd3_rollout_collect.h"\n')
    assert alone.returncode != 0 and "sactd3_rollout.h" in alone.stderr


def test_a_null_handle_is_refused():
    lib = P.load_library()
    for mode in range(5):
        assert lib.sactd3_rollout_collect(None, mode, 1, None, None) == _lib.EINVAL
    assert lib.sactd3_rollout_collect_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL


def test_the_kernel_lives_beside_the_env_kernels_and_uses_no_scratch(tmp_path):
    """engine.hip gains host code only; env.hip compiles k_collect_rollout, which calls the one actor pass, the one step body and the one
    record writer; hipcc's resource remarks give every instance ScratchSize 0"""
    engine, env, kernels, evalk, envk = (text(CSRC, n) for n in ("engine.hip", "env.hip", "collect_kernels.h", "eval_kernels.h", "env_kernels.h"))
    assert "k_collect_rollout" not in code(engine) and "collect_kernels.h" not in code(engine) and '#include "collect_rollout.h"' in engine
    assert '#include "collect_kernels.h"' in env and "__global__" not in text(CSRC, "collect_rollout.h")
    assert re.findall(r"__global__[^\n]*\bvoid\s+(\w+)", kernels) == ["k_collect_rollout"]
    for name, home in (("ev_actor_pass", evalk), ("env_write_record", envk), ("env_step_body", envk)):
        assert len(re.findall(rf"__forceinline__[^\n]*\b{name}\(", home)) == 1, name         # stated once ...
        assert re.search(rf"\b{name}<", code(kernels)), name                                  # ... and used here
    assert len(re.findall(r"\bev_actor_pass<", code(evalk))) == 1 and len(re.findall(r"\benv_write_record<", code(envk))) == 1
    assert "mfma" not in code(kernels)                                                        # the pass is not restated
    deps = re.search(r"^ENV_DEPS\s*:=\s*(.*)$", text(CSRC, "Makefile"), re.M).group(1).split()
    assert {"collect_kernels.h", "collect_rollout.h", "../../include/sactd3_rollout_collect.h"} <= set(deps)
    flags = re.search(r"^PRELOAD\s*:=\s*(.*)$", text(CSRC, "Makefile"), re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          "-DSACTD3_BUILD", *flags, "env.hip", "-o", str(tmp_path / "env.s")], cwd=CSRC, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", run.stderr)[1:]
    mine = [b for b in blocks if b.split()[0].startswith("_Z17k_collect_rollout")]
    assert len(mine) == 3, [b.split()[0] for b in blocks]                                     # one instance per task
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 160 * 1024


# ------------------------------------------------------------------------------------------ the keyword's rules
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=3, num_envs=2, num_timesteps=40, eval_every=10 ** 9, batch_size=4,
           actor_update_delay=2)


class Untouchable:
    """an agent (an env) that fails on any attribute access: a refusal must come before either is touched"""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_rollout_for_states_the_rules_and_refuses_before_it_looks_at_the_env():
    ok = dict(overlap=False, device_env=True, native_rollout=True, collected_rollout=True)
    with pytest.raises(ValueError, match="native_rollout=True"):
        loop.rollout_for(Untouchable(), **dict(ok, native_rollout=False))
    with pytest.raises(ValueError, match="fused_rollout"):
        loop.rollout_for(Untouchable(), **ok, fused_rollout=True)
    with pytest.raises(ValueError, match="overlap"):
        loop.rollout_for(Untouchable(), **dict(ok, overlap=True))
    with pytest.raises(ValueError, match="action_repeat"):
        loop.rollout_for(Untouchable(), **ok, action_repeat=2)
    with pytest.raises(ValueError, match="segment_len"):
        loop.rollout_for(Untouchable(), **ok, segment_len=0)
    with pytest.raises(ValueError, match="device_env"):                                       # the native rollout's own rules behind them
        loop.rollout_for(Untouchable(), **dict(ok, device_env=False))
    with pytest.raises(TypeError, match="step_records"):
        loop.rollout_for(envs.HostVecEnv("pendulum", 2), **ok)
    env = SimpleNamespace(step_records=lambda *a: None)
    for seg in (1, 8, 64):                                                                    # any segment_len >= 1
        assert loop.rollout_for(env, **ok, segment_len=seg) is loop.NativeRollout
    assert loop.rollout_for(None, overlap=False, device_env=True, native_rollout=False) is loop.DeviceRollout      # off: what it was
    assert inspect.signature(loop.rollout_for).parameters["collected_rollout"].default is False
    assert inspect.signature(loop.train).parameters["collected_rollout"].default is False
    assert callable(loop.NativeRollout.collect) and callable(loop.NativeRollout.collect_stats)


def test_train_refuses_before_it_touches_anything():
    cfg = SimpleNamespace(**CFG)
    for more, word in ((dict(), "native_rollout=True"), (dict(native_rollout=True, fused_rollout=True, device_env=True), "fused_rollout"),
                       (dict(native_rollout=True, overlap=True, device_env=True), "overlap"), (dict(native_rollout=True), "device_env")):
        with pytest.raises(ValueError, match=word):
            loop.train(SimpleNamespace(**dict(CFG, segment_len=1)) if "fused_rollout" in more else cfg, Untouchable(), Untouchable(),
                       collected_rollout=True, **more)
    with pytest.raises(ValueError, match="action_repeat"):
        loop.train(SimpleNamespace(**dict(CFG, action_repeat=2)), Untouchable(), Untouchable(), device_env=True, native_rollout=True,
                   collected_rollout=True)


def test_the_launcher_maps_and_refuses_the_flag():
    cfg = launcher.job_config("sac", "Pendulum-native", 0)
    facts = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=4, overlap_acting=False,
                 device_env=True, native_rollout=True, policy_stats=0)
    kw = launcher.train_keywords(cfg, **facts, collected_rollout=True)
    assert kw["collected_rollout"] is True and kw["native_rollout"] is True and kw["updates_per_step"] == 4
    assert "collected_rollout" not in launcher.train_keywords(cfg, **facts)                   # a key only when the flag was given
    assert launcher.train_keywords(cfg, **dict(facts, prioritized=True), collected_rollout=True)["prioritized"]      # the other draws go with it
    for change, word in ((dict(native_rollout=False), "native_rollout"), (dict(overlap_acting=True), "overlap")):
        with pytest.raises(ValueError, match="collected_rollout=True") as ex:
            launcher.train_keywords(cfg, **dict(facts, **change), collected_rollout=True)
        assert word in str(ex.value)
    with pytest.raises(ValueError, match="fused_rollout"):
        launcher.train_keywords(cfg, **dict(facts, updates_per_step=1), collected_rollout=True, fused_rollout=True)
    with pytest.raises(ValueError, match="action_repeat"):
        launcher.train_keywords(launcher.job_config("sac", "Pendulum-native", 0, action_repeat=2), **facts, collected_rollout=True)
    launcher.train_keywords(launcher.job_config("sac", "Pendulum-native", 0, segment_len=8), **facts, collected_rollout=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run", "--env_bundle", "native"]

    def run(*more):
        return subprocess.run(base + list(more), capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    out = run("--device_env", "--native_rollout", "--collected_rollout")
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert len(jobs) == 2 and all(j["rollout"] == "NativeRollout" and j["collected_rollout"] is True and j["dry_run"] for j in jobs)
    out = run("--device_env", "--native_rollout")
    assert out.returncode == 0 and all("collected_rollout" not in json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB "))
    # refused in the parent process: exit status 2 from the argument parser, no job line, no worker started
    for more, word in ((("--device_env", "--collected_rollout"), "native_rollout"), (("--collected_rollout",), "native_rollout"),
                       (("--device_env", "--native_rollout", "--collected_rollout", "--fused_rollout"), "fused_rollout"),
                       (("--device_env", "--native_rollout", "--collected_rollout", "--overlap_acting"), "overlap")):
        out = run(*more)
        assert out.returncode == 2 and word in out.stderr and "JOB " not in out.stdout, (more, out.stderr[-500:])


# ------------------------------------------------------------------------------------------ the loop bodies, with a stub rollout
class StubRollout:
    def __init__(self, env, agent, seed, learning_starts, action_repeat):
        self.log, self.agent, self.steps = env.log, agent, 0
        self.log.append(("reset", seed, learning_starts, action_repeat))

    def choose(self):
        self.log.append(("choose", self.agent.timesteps_so_far))

    def advance(self):
        self.log.append(("advance", self.agent.timesteps_so_far))
        self.steps += 1

    def collect(self, steps):
        self.log.append(("collect", steps, self.agent.timesteps_so_far))
        self.steps += steps

    def resolve(self):
        pass


def stub_run(monkeypatch, **more):
    log = []
    env = SimpleNamespace(log=log, step_records=lambda *a: None)
    agent = SimpleNamespace(rb=object(), timesteps_so_far=0, qnet_updates_so_far=0, engine=SimpleNamespace(read_metrics=lambda: {"m": 1.0}),
                            iteration=lambda i: log.append(("iteration", i)))
    seen = {}

    def fake_rollout_for(env, **kw):
        real(env, **kw)                                                                       # the rules are still asked
        seen.update(kw)
        return StubRollout
    real = loop.rollout_for
    monkeypatch.setattr(loop, "rollout_for", fake_rollout_for)
    out = loop.train(SimpleNamespace(**CFG), env, agent, device_env=True, native_rollout=True, updates_per_step=2, **more)
    assert out == {"m": 1.0}
    return log, seen


def test_the_default_loop_is_the_loop_it_was_and_the_collected_one_differs_by_one_call(monkeypatch):
    """segment_len 3, 2 envs, learning_starts 10, updates_per_step 2, bodies until 40 timesteps are passed.  Default: segment() chooses,
    then yields -- the action that opens a segment is chosen BEFORE the updates in front of it.  Collected: one collect(3) per body, its
    choices made after them.  Everything else -- the counts, the update indices, where the updates start -- is the same."""
    plain, seen = stub_run(monkeypatch)
    assert "collected_rollout" not in seen                                                    # off: rollout_for is asked what it was asked
    want = [("reset", 0, 10, 1)]
    ts, i = 0, 0
    for body in range(7):                                                                     # 0, 6, ..., 36 <= 40: seven bodies
        if body == 0:
            want.append(("choose", 0))
        want += [("advance", ts), ("choose", ts), ("advance", ts), ("choose", ts), ("advance", ts), ("choose", ts)]
        ts += 6
        if ts <= 10:
            i += 1
            continue
        want += [("iteration", i), ("iteration", i + 1)]
        i += 2
    assert plain == want
    collected, seen = stub_run(monkeypatch, collected_rollout=True)
    assert seen["collected_rollout"] is True and seen["action_repeat"] == 1 and seen["segment_len"] == 3
    assert [e for e in collected if e[0] == "iteration"] == [e for e in plain if e[0] == "iteration"]
    assert [e for e in collected if e[0] == "collect"] == [("collect", 3, 6 * k) for k in range(7)]
    assert not [e for e in collected if e[0] in ("choose", "advance")]
    # the one difference: a segment's choices stand behind the updates in front of it
    k = collected.index(("collect", 3, 12))
    assert collected[k - 2:k] == [("iteration", 1), ("iteration", 2)] and collected[k + 1] == ("iteration", 3)
    k = plain.index(("iteration", 1))                                                         # ... where the default loop chose before them
    assert plain[k - 1] == ("choose", 6) and plain[k + 2] == ("advance", 12)
