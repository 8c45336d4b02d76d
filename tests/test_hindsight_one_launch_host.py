"""CPU: the hindsight iteration as one graph launch (include/sactd3.h: sactd3_step_sampled with SACTD3_DRAW_HINDSIGHT), checked without a
GPU -- the plan and the bindings that lead to it, and, with the numpy restatements alone (tests/hindsight_ref.py, tests/mix_ref.py), that
the ring schedule of tests/test_gpu_hindsight_one_launch.py meets every situation the staging kernel has a rule for: the GPU test cannot
pass on an easy draw."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, envs, launcher, loop
from tests import hindsight_ref as hr
from tests import mix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GOAL = dict(achieved=0, desired=4, dim=2, threshold=0.1)
BASE = dict(fused=False, sampler=None, prioritized=None, n_step=1, one_launch=True, prior_fraction=None, updates_per_step=1)
CFG = SimpleNamespace(batch_size=64, num_envs=4, actor_update_delay=2)


# ------------------------------------------------------------------------------------------ the plan
def stub_agent(calls):
    return SimpleNamespace(iteration=lambda i, **kw: calls.append((i, kw)))


def test_update_plan_issues_the_hindsight_iteration_as_one_launch():
    plan = loop.update_plan(CFG, **BASE, hindsight=dict(GOAL))
    assert plan.hindsight == dict(GOAL, stride=4) and plan.priorities is None and plan.updates_per_step == 1
    calls = []
    for i in (0, 1, 5):
        plan.update(stub_agent(calls), i, {})
    assert calls == [(0, dict(hindsight=True)), (1, dict(hindsight=True)), (5, dict(hindsight=True))]
    # the update-to-data ratio as in every other branch; the config's own keys go through
    plan = loop.update_plan(CFG, **dict(BASE, updates_per_step=3), hindsight=dict(GOAL, ratio=0.5, window=9, stride=7))
    assert plan.updates_per_step == 3 and plan.hindsight == dict(GOAL, ratio=0.5, window=9, stride=7)
    # call by call is still what one_launch=False gives
    seen = []
    rb = SimpleNamespace(sample_hindsight=lambda n: seen.append("sample_hindsight") or "batch")
    agent = SimpleNamespace(rb=rb, update_qnets=lambda b: seen.append("q") or {}, update_actor=lambda b: seen.append("pi") or {},
                            update_targ_nets=lambda: seen.append("targ"), qnet_updates_so_far=0, actor_updates_so_far=0)
    loop.update_plan(CFG, **dict(BASE, one_launch=False), hindsight=dict(GOAL)).update(agent, 1, {})
    assert seen == ["sample_hindsight", "q", "targ"]


def test_the_other_refusals_stand_with_their_texts():
    for over, msg in ((dict(fused=True), "one_launch=True needs fused=False: fused=True is the uniform 1-step iteration, already one launch"),
                      (dict(sampler=object()), "one_launch=True excludes sampler=...: a sampler outside the engine cannot be part of its graph"),
                      (dict(prioritized=dict(alpha=0.6)),
                       "hindsight=... and prioritized=... exclude each other: a relabelled row's TD error is not its record's priority"),
                      (dict(n_step=3), "hindsight=... excludes n_step > 1: a relabelled reward is a single step's, the chain's return is not"),
                      (dict(prior_fraction=0.5), "hindsight=... and prior_fraction=... exclude each other: a pinned ring has no episode chains yet")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            loop.update_plan(CFG, **dict(BASE, **over), hindsight=dict(GOAL))
    for over, msg in ((dict(fused=True), "hindsight=... needs fused=False: the fused iteration samples uniformly inside its graph and relabels nothing"),
                      (dict(sampler=object()), "hindsight=... and sampler=... exclude each other: the engine relabels the rows of its own draw")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            loop.update_plan(CFG, **dict(BASE, one_launch=False, **over), hindsight=dict(GOAL))
    # without a reason for it one_launch is refused as before, in the same words
    with pytest.raises(ValueError, match=re.escape("one_launch=True needs prioritized=... and / or n_step > 1: the uniform 1-step iteration is fused=True")):
        loop.update_plan(CFG, **BASE)
    with pytest.raises(ValueError, match="unknown keys"):
        loop.update_plan(CFG, **BASE, hindsight=dict(GOAL, horizon=50))
    with pytest.raises(ValueError, match="missing keys"):
        loop.update_plan(CFG, **BASE, hindsight=dict(achieved=0, desired=4))


# ------------------------------------------------------------------------------------------ the bindings
class NoLibrary:
    """stands where the loaded library would: any use of it is a failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def test_step_sampled_and_iteration_refuse_the_excluded_keywords_before_the_library():
    eng = object.__new__(P.Engine)
    eng.lib, eng._h = NoLibrary(), None
    for kw in (dict(beta=0.4), dict(n_step=2, stride=4), dict(prior_rows=8), dict(beta=0.4, prior_rows=8)):
        with pytest.raises(ValueError, match="hindsight"):
            eng.step_sampled(True, hindsight=True, **kw)
    agent = object.__new__(P.Agent)
    agent.engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2), step_sampled=NoLibrary().__getattr__)
    agent.qnet_updates_so_far = agent.actor_updates_so_far = 0
    for kw in (dict(beta=0.4), dict(n_step=2), dict(prior_rows=8)):
        with pytest.raises(ValueError, match="hindsight"):
            agent.iteration(0, hindsight=True, **kw)
    assert agent.qnet_updates_so_far == 0
    # ... and what it passes on when nothing is excluded
    seen = []
    agent.engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2), step_sampled=lambda do_actor, **kw: seen.append((do_actor, kw)))
    for i in range(4):
        agent.iteration(i, hindsight=True)
    assert seen == [(True, dict(hindsight=True)), (False, dict(hindsight=True)), (False, dict(hindsight=True)), (True, dict(hindsight=True))]
    assert agent.qnet_updates_so_far == 4 and agent.actor_updates_so_far == 4


def test_the_draw_kind_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sactd3.h")).read(), flags=re.S)
    enum = dict(re.findall(r"(SACTD3_DRAW_\w+)\s*=\s*(-?\d+)", src))
    assert enum == dict(SACTD3_DRAW_UNIFORM="0", SACTD3_DRAW_PRIORITIZED="1", SACTD3_DRAW_MIXED="2", SACTD3_DRAW_HINDSIGHT="3")
    assert (_lib.DRAW_UNIFORM, _lib.DRAW_PRIORITIZED, _lib.DRAW_MIXED, _lib.DRAW_HINDSIGHT) == (0, 1, 2, 3)
    assert _lib.ABI_VERSION == 1 and C.sizeof(_lib.CSampling) == 16
    # the new kernels live in the hindsight translation unit: engine.hip names their launchers and defines no kernel for them
    csrc = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
    eng = open(os.path.join(csrc, "engine.hip")).read()
    assert "hindsight_draw_g_launch" in eng and "hindsight_stage_g_launch" in eng and not re.search(r"__global__[^;{]*hindsight", eng)
    own = open(os.path.join(csrc, "hindsight_kernels.h")).read() + open(os.path.join(csrc, "hindsight.hip")).read()
    for kernel in ("k_hindsight_stage", "k_hindsight_draw_g", "k_hindsight_stage_g"):
        assert re.search(rf"__global__[^;{{]*\b{kernel}\(", own), kernel


def test_launcher_dry_run_accepts_hindsight_with_one_launch():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run", "--env_bundle", "native_goal",
                          "--hindsight", "--one_launch"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert len(jobs) == 1 and jobs[0]["env_id"] == "PointGoal-native" and jobs[0]["dry_run"] is True
    assert jobs[0]["hindsight"] == dict(achieved=0, desired=4, dim=2, threshold=0.1, window=50, stride=4) and jobs[0]["one_launch"] is True
    kw = launcher.train_keywords(SimpleNamespace(batch_size=8, num_envs=4), prioritized=False, n_step=1, one_launch=True, prior_fraction=None,
                                 updates_per_step=1, overlap_acting=False, device_env=False, native_rollout=False, policy_stats=0,
                                 hindsight=launcher.hindsight_keywords("PointGoal-native", 4))
    assert kw["one_launch"] is True and kw["fused"] is False and kw["hindsight"]["window"] == 50


# ------------------------------------------------------------------------------------------ the GPU test's schedule covers its cases
# (restated in tests/test_gpu_hindsight_one_launch.py: no test module imports another)
STRIDE, SEED, HELD_STEPS, ITERS = 4, 3, 20, 7
# name -> (o, a, B, achieved, desired, dim, horizon of its episodes, window)
CASES = {"goal-8": (6, 2, 8, 0, 4, 2, 9, 9), "goal-260": (6, 2, 260, 0, 4, 2, 9, 9), "long-16": (376, 17, 16, 1, 200, 3, 5, 5)}
RUNS = [("goal-8", 96, "sac"), ("goal-260", 101, "td3"), ("long-16", 96, "sac"), ("goal-260", 96, "sac")]
RATIO = 0.8
ROW_SEED = 9                                                              # of the synthetic episodes: every second one ends by termination


@functools.lru_cache(maxsize=None)
def rows_of(case):
    """HELD_STEPS + ITERS vector steps in append order: computed once, never written"""
    o, a, B, ag, dg, G, horizon, _ = CASES[case]
    return hr.synthetic_ring(o, a, STRIDE, HELD_STEPS + ITERS, horizon, seed=ROW_SEED, term_every=2, achieved=ag, dim=G)


def config(case, ratio=RATIO, window=None):
    o, a, B, ag, dg, G, _, w = CASES[case]
    return dict(achieved=ag, desired=dg, dim=G, threshold=0.1, ratio=ratio, window=window or w, stride=STRIDE)


@functools.lru_cache(maxsize=None)
def expected(case, cap, i):
    """the slot iteration i must leave: the ring after HELD_STEPS + i + 1 vector steps, the uniform draw at sample counter i, the
    relabelling draw at hindsight counter i"""
    rows, _ = rows_of(case)
    n = (HELD_STEPS + i + 1) * STRIDE
    fields, geom, held = hr.place({k: v[:n] for k, v in rows.items()}, cap)
    idx = mix_ref.mixed_indices(SEED, i, CASES[case][2], 0, 0, geom["length"])
    return dict(hr.stage(fields, geom, idx, config(case), seed=SEED, hctr=i), geom=geom, held=held, idx=idx, n=n)


def test_the_schedule_grows_fills_and_wraps():
    for case, cap, _ in RUNS:
        lens = [expected(case, cap, i)["geom"]["length"] for i in range(ITERS)]
        curs = [expected(case, cap, i)["geom"]["cursor"] for i in range(ITERS)]
        assert lens[0] < cap and lens[-1] == cap and lens == sorted(lens) and len(set(lens)) > 2, (case, cap, lens)
        assert any(n == cap and c == 0 for n, c in zip(lens, curs)) == (cap % STRIDE == 0)      # exactly full, the cursor back at 0
        assert sum(1 for n, c in zip(lens, curs) if n == cap and c > 0) >= 2, (case, cap, curs)  # ... and wrapped, the cursor moving on


@pytest.mark.parametrize("case,cap,algo", RUNS)
def test_the_seven_iterations_meet_every_rule(case, cap, algo):
    rows, _ = rows_of(case)
    window = CASES[case][7]
    seen = dict(wrap=0, newest=0, termination=0, rew0=0, rewm1=0, kept=0, later=0)
    for i in range(ITERS):
        w = expected(case, cap, i)
        rel, L, idx, held = w["offset"] >= 0, w["L"], w["idx"], w["held"]
        assert (w["slot_idx"] == idx).all() and (L >= 1).all()              # the uniform draw refuses nothing
        seen["wrap"] += int((rel & (w["goal_slot"] < w["slot_idx"])).sum())  # the goal lies behind the wrap point
        seen["later"] += int((rel & (w["offset"] > 0)).sum())
        seen["rew0"] += int((rel & (w["rew"] == 0)).sum())
        seen["rewm1"] += int((rel & (w["rew"] == -1)).sum())
        seen["kept"] += int((~rel).sum())
        for b in np.flatnonzero(L < window):
            last = int(held[idx[b]]) + (L[b] - 1) * STRIDE
            if last + STRIDE >= w["n"]:
                seen["newest"] += 1                                           # cut by the ring's newest rows
            elif rows["done"][last] != 0:
                seen["termination"] += 1                                      # cut by a termination flag
    print(case, cap, seen)
    assert all(v > 0 for v in seen.values()), (case, cap, seen)
