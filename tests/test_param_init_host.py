"""CPU: the host side of the parameter initialiser (include/sactd3_init.h) -- the header, the binding and the built library cover each
other; the new kernels live in a translation unit of their own; the keyword rules of `reset_every` in loop.update_plan / loop.train /
loop.train_offline and in the launcher, each asked before an agent is touched; and what Agent(init=...) asks of its engine."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def declared(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src)))


# ------------------------------------------------------------------------------------------ the header, the binding, the library
def test_header_binding_and_library_cover_each_other():
    header = text("include", "sactd3_init.h")
    assert declared(header) == sorted(_lib.INIT_SYMBOLS) and len(_lib.INIT_SYMBOLS) == 2
    assert not set(_lib.INIT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ENV_SYMBOLS) | set(_lib.ROLLOUT_SYMBOLS) | set(_lib.ROLLOUT_CYCLE_SYMBOLS))
    enum = dict(re.findall(r"(SACTD3_INIT_[A-Z]+)\s*=\s*(\d+)", header))
    assert {k: int(v) for k, v in enum.items()} == {"SACTD3_INIT_ACTOR": _lib.INIT_ACTOR, "SACTD3_INIT_CRITICS": _lib.INIT_CRITICS,
                                                    "SACTD3_INIT_ALPHA": _lib.INIT_ALPHA}
    assert (_lib.INIT_ACTOR, _lib.INIT_CRITICS, _lib.INIT_ALPHA) == (1, 2, 4) and _lib.INIT_ALL == 7
    assert agent_mod.RESET_NAMES == {"actor": 1, "critics": 2, "alpha": 4} and tuple(agent_mod.RESET_NAMES) == loop.RESET_ALL
    assert _lib.ABI_VERSION == 1 and re.search(r"#define\s+SACTD3_ABI_VERSION\s+1\b", text("include", "sactd3.h"))
    assert "0x700" in header and "SACTD3_STREAM_INIT 0x700u" in text(CSRC, "param_init_kernels.h")      # the counter words stand in the header
    P.build_library()                                                                         # hipcc --offload-arch=gfx950 (a no-op when current)
    raw = C.CDLL(P.library_path())
    for name in _lib.INIT_SYMBOLS:
        assert hasattr(raw, name), f"{name} is declared but not exported"
    lib = P.load_library()
    assert lib.sactd3_init_params.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32]
    probe = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], capture_output=True, text=True,
                           input='#include "sactd3_init.h"\nint f(sactd3_engine* e) { int64_t o[4]; return sactd3_init_params(e, SACTD3_INIT_ACTOR | '
                                 'SACTD3_INIT_CRITICS | SACTD3_INIT_ALPHA, 1u, 0u) + sactd3_init_stats(e, o); }\n')
    assert probe.returncode == 0, probe.stderr[-2000:]


def test_a_null_handle_is_refused():
    lib = P.load_library()
    for what in (0, 1, 7, 8):
        assert lib.sactd3_init_params(None, what, 0, 0) == _lib.EINVAL
    assert lib.sactd3_init_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL


def test_the_new_kernels_are_a_translation_unit_of_their_own():
    """engine.hip gains host code only: the two kernels stand in param_init_kernels.h, which param_init.hip alone includes; engine.hip
    reaches them through param_init.h; the library's build lists the new unit and `make asm` stays engine.hip alone"""
    unit, kernels, header, engine, make = (text(CSRC, n) for n in ("param_init.hip", "param_init_kernels.h", "param_init.h", "engine.hip", "Makefile"))
    new = re.findall(r"__global__[^\n]*\bvoid\s+(\w+)", kernels)
    assert new == ["k_init_orth", "k_init_fanout"]
    assert "__global__" not in unit and "__global__" not in header and '#include "param_init_kernels.h"' in unit
    assert re.findall(r'#include "([^"]+)"', kernels) == ["param_init.h", "philox.h"] and "DevCtl" not in kernels + unit
    assert '#include "param_init.h"' in engine and '#include "param_init_kernels.h"' not in engine
    for name in new:      # (engine.hip names them in its error texts only)
        assert not re.search(r"__global__[^\n]*\b%s\b|hipLaunchKernelGGL\(\s*%s\b|\b%s\s*<<<|LAUNCH\w*\([^\n]*\b%s\b" % ((name,) * 4), engine)
    # no other file of csrc/ defines a kernel of these names, and every other unit's kernels are the ones it had
    for f in sorted(os.listdir(CSRC)):
        if f not in ("param_init_kernels.h",):
            assert not re.search(r"__global__[^\n]*\b(k_init_orth|k_init_fanout)\b", text(CSRC, f)), f
    assert "param_init.hip" in make
    asm = re.search(r"^asm:.*\n\t(.*)$", make, re.M).group(1)
    assert "param_init.hip" not in asm and "$(PI_SRC)" not in asm and "$(SRC)" in asm
    # the draws go through the one Box-Muller of the engine's noise
    assert "philox_box_muller4" in text(CSRC, "philox.h") and "philox_box_muller4" in kernels and "philox_box_muller4" in text(CSRC, "kernels.h")


# ------------------------------------------------------------------------------------------ loop.update_plan / train / train_offline
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)
PLAN = dict(fused=True, sampler=None, prioritized=None, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1)


class Untouchable:
    """an agent (an env) that fails on any attribute access: a refusal must come before either is touched"""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


BAD = [(dict(reset_every=0), "reset_every"), (dict(reset_every=-3), "reset_every"), (dict(reset_every=5, reset_what=("actor", "ring")), "ring"),
       (dict(reset_every=5, reset_what=()), "reset_what"), (dict(reset_every=5, reset_what="actor,,alpha"), "reset_what")]


@pytest.mark.parametrize("change,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_reset_keywords_are_refused_before_an_agent_is_touched(change, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.update_plan(cfg, **PLAN, **change)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), **change)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), device_env=True, native_rollout=True, fused_rollout=True, **change)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, **change)


def test_an_offline_plan_that_never_reaches_the_reset_is_refused():
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match="never reached"):
        loop.update_plan(cfg, **PLAN, reset_every=101, num_updates=100)
    with pytest.raises(ValueError, match="never reached"):
        loop.train_offline(cfg, Untouchable(), num_updates=100, reset_every=101)
    assert loop.update_plan(cfg, **PLAN, reset_every=100, num_updates=100).reset is not None


def test_the_reset_rule_fires_once_per_multiple_reached():
    """plan.reset between two bodies: one reset_networks per multiple of reset_every the count has reached since the last look, with
    the names as given; without the keyword the plan has no rule, in every branch of the table"""
    for change in (dict(), dict(fused=False), dict(fused=False, n_step=3), dict(fused=False, prioritized=dict(alpha=0.6), one_launch=True),
                   dict(fused_rollout=True), dict(updates_per_step=20)):
        assert loop.update_plan(SimpleNamespace(**CFG), **dict(PLAN, **change)).reset is None
        assert loop.update_plan(SimpleNamespace(**CFG), **dict(PLAN, **change), reset_every=7).reset is not None
    calls, order = [], []
    agent = SimpleNamespace(qnet_updates_so_far=0, reset_networks=lambda what: calls.append((agent.qnet_updates_so_far, what)))
    plan = loop.update_plan(SimpleNamespace(**CFG), **PLAN, reset_every=50, reset_what="actor,critics")
    seen = 0
    for count in (1, 49, 50, 51, 99, 103, 104, 150, 150):
        agent.qnet_updates_so_far = count
        seen = plan.reset(agent, seen, lambda: order.append(count))
    assert calls == [(50, ("actor", "critics")), (103, ("actor", "critics")), (150, ("actor", "critics"))] and order == [50, 103, 150]
    assert loop.update_plan(SimpleNamespace(**CFG), **PLAN, reset_every=5).reset.__defaults__ == (None,)


def test_train_offline_ends_its_runs_where_a_reset_is_due():
    """a stub agent: the runs of train_offline end at every multiple of reset_every (and at the evaluation points), one reset each,
    none behind the last update unless the count reached a multiple; without the keyword the runs are what they were"""
    def offline(num_updates, **kw):
        runs, resets, evals = [], [], []
        engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {},
                                 run_iterations=lambda i, n: runs.append((i, n)))
        agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, resets_so_far=0)
        agent.reset_networks = lambda what: (resets.append((agent.qnet_updates_so_far, tuple(what))), setattr(agent, "resets_so_far", agent.resets_so_far + 1))
        out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=num_updates, on_eval=lambda ag, n: evals.append(n), **kw)
        return runs, resets, evals, out, agent
    runs, resets, evals, out, agent = offline(25, eval_every_updates=10)
    assert runs == [(0, 10), (10, 10), (20, 5)] and resets == [] and evals == [10, 20, 25] and "vitals/resets" not in out
    runs, resets, evals, out, agent = offline(25, eval_every_updates=10, reset_every=8, reset_what=("critics",))
    assert runs == [(0, 8), (8, 2), (10, 6), (16, 4), (20, 4), (24, 1)] and resets == [(8, ("critics",)), (16, ("critics",)), (24, ("critics",))]
    assert evals == [10, 20, 25] and out["vitals/resets"] == 3 and agent.qnet_updates_so_far == 25 and agent.actor_updates_so_far == 2 * 9


# ------------------------------------------------------------------------------------------ the launcher
def test_the_launcher_maps_the_flags_and_refuses_bad_ones_in_the_parent():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    assert "reset_every" not in plain and "reset_what" not in plain and "init" not in plain              # absent: the keywords they were
    kw = launcher.train_keywords(cfg, **base, reset_every=500, reset_what=("actor", "critics"), init="engine")
    assert kw["reset_every"] == 500 and kw["reset_what"] == ("actor", "critics") and "init" not in kw
    assert {k: v for k, v in kw.items() if k not in ("reset_every", "reset_what")} == plain
    assert launcher.train_keywords(cfg, **base, reset_every=500)["reset_what"] == loop.RESET_ALL
    with pytest.raises(ValueError, match="reset_every"):
        launcher.train_keywords(cfg, **base, reset_every=0)
    with pytest.raises(ValueError, match="never reached"):
        launcher.train_keywords(cfg, **base, reset_every=500, num_updates=499)
    with pytest.raises(ValueError, match="init"):
        launcher.train_keywords(cfg, **base, init="lapack")
    with pytest.raises(ValueError):
        launcher.run_job("sac", "Hopper-v4", 0, 0, "unused", reset_every=0, device_env=True, native_rollout=True)      # before anything is built
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run"]

    def run(*more):
        return subprocess.run(cmd + list(more), capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    out = run("--init", "engine", "--reset_every", "2000", "--reset_what", "actor,critics", "--updates_per_step", "8")
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert jobs and all(j["init"] == "engine" and j["reset_every"] == 2000 and j["reset_what"] == ["actor", "critics"] and j["dry_run"] for j in jobs)
    out = run("--reset_every", "2000", "--env_bundle", "native", "--device_env", "--native_rollout", "--fused_rollout")
    assert out.returncode == 0 and all(json.loads(ln[4:])["reset_what"] == list(loop.RESET_ALL) for ln in out.stdout.splitlines() if ln.startswith("JOB "))
    out = run()
    assert out.returncode == 0 and not any(k in ln for ln in out.stdout.splitlines() if ln.startswith("JOB ") for k in ("init", "reset_"))
    for bad, word in ((("--reset_every", "0"), "reset_every"), (("--reset_what", "actor"), "--reset_every"), (("--init", "lapack"), "--init"),
                      (("--reset_every", "10", "--reset_what", "actor,ring"), "ring")):
        out = run(*bad)
        assert out.returncode == 2 and word in out.stderr and "JOB " not in out.stdout, (bad, out.stderr[-500:])


# ------------------------------------------------------------------------------------------ what Agent(init=...) asks of its engine
class StubEngine:
    """records the calls an Agent makes on its engine"""
    log = []

    def __init__(self, cfg, min_ac, max_ac):
        self.cfg = cfg
        StubEngine.log.append(("create", cfg.seed))

    def __getattr__(self, name):
        def call(*args, **kw):
            StubEngine.log.append((name,) + tuple(a if isinstance(a, (int, str, type(None))) else type(a).__name__ for a in args) + tuple(sorted(kw.items())))
        return call


def make_agent(monkeypatch, algo="sac", **kw):
    monkeypatch.setattr(agent_mod, "Engine", StubEngine)
    StubEngine.log = []
    cfg = launcher.job_config(algo, None, 0)
    a = agent_mod.Agent({"ob_shape": (3,), "ac_shape": (1,)}, np.full(1, -1, np.float32), np.full(1, 1, np.float32), SimpleNamespace(index=0), cfg,
                        seed=5, metrics="lazy", **kw)
    return a, list(StubEngine.log)


def test_agent_init_torch_issues_the_calls_it_always_issued(monkeypatch):
    want = [("create", 5)] + [("set_params", w, "ndarray") for w in (_lib.ACTOR, _lib.CRITICS, _lib.ACTOR_TARGET, _lib.CRITICS_TARGET)]
    _, default = make_agent(monkeypatch)
    _, named = make_agent(monkeypatch, init="torch")
    assert default == want and named == want
    assert make_agent(monkeypatch, init_params=False)[1] == [("create", 5)]
    with pytest.raises(ValueError, match="init"):
        make_agent(monkeypatch, init="lapack")


def test_agent_init_engine_is_one_call_and_resets_count_epochs(monkeypatch):
    a, log = make_agent(monkeypatch, init="engine")
    assert log == [("create", 5), ("init_params", _lib.INIT_ALL, ("epoch", 0))] and a.resets_so_far == 0
    assert a.reset_networks() == 1 and a.reset_networks(("critics",)) == 2 and a.reset_networks("actor,alpha") == 3
    assert StubEngine.log[2:] == [("init_params", 7, ("epoch", 1)), ("init_params", 2, ("epoch", 2)), ("init_params", 5, ("epoch", 3))]
    with pytest.raises(ValueError):
        a.reset_networks(("actor", "ring"))
    assert a.resets_so_far == 3 and len(StubEngine.log) == 5                                  # a refused reset counted and called nothing
    t, log = make_agent(monkeypatch, algo="td3", init="engine")
    assert log[1] == ("init_params", _lib.INIT_ACTOR | _lib.INIT_CRITICS, ("epoch", 0))      # TD3 drops "alpha" silently
    assert t.reset_networks() == 1 and StubEngine.log[-1] == ("init_params", 3, ("epoch", 1))
    with pytest.raises(ValueError, match="temperature"):
        t.reset_networks(("alpha",))
    assert "NOT saved" in agent_mod.Agent.reset_networks.__doc__
