"""CPU: hindsight relabelling at staging, checked without a GPU -- the numpy restatement (tests/hindsight_ref.py) against true episode
bookkeeping on rollouts of the host goal env, the properties a relabelled batch must have, the restatement's power to tell a planted
defect from the rule, and the plans and bindings around the engine's calls."""
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
from sac_td3_cudagraphs_pytorch_amd import _lib, envs, launcher, loop
from tests import hindsight_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_ENVS, HORIZON = 4, 9
GOAL = dict(achieved=0, desired=4, dim=2, threshold=0.1)
# (capacity, vector steps): unwrapped and wrapped rings, cap % stride == 0 and != 0
RINGS = [(96, 20), (96, 24), (96, 61), (101, 25), (101, 77)]


def goal_ring(cap, steps, seed=3):
    env = envs.HostVecEnv("pointgoal", N_ENVS, seed=seed, horizon=HORIZON)
    rows, episode = hr.host_rollout(env, steps)
    fields, geom, held = hr.place(rows, cap)
    return rows, episode, fields, geom, held


def cfg_of(window, ratio=1.0, **over):
    return dict(GOAL, ratio=ratio, window=window, stride=N_ENVS, **over)


@pytest.mark.parametrize("cap,steps", RINGS)
def test_chain_lengths_are_the_episodes_own(cap, steps):
    rows, episode, fields, geom, held = goal_ring(cap, steps)
    assert geom["length"] == min(cap, steps * N_ENVS) and geom["cursor"] == (steps * N_ENVS) % cap
    idx = np.arange(geom["length"])
    for window in (1, 5, 64):
        got = hr.stage(fields, geom, idx, cfg_of(window), choice=np.zeros(len(idx), np.int32))
        want = hr.true_lengths(episode, rows["done"], held, geom, idx, window, N_ENVS)
        assert np.array_equal(got["L"], want), (window, np.flatnonzero(got["L"] != want)[:8])
        assert got["L"].min() == 1 and got["L"].max() == min(window, HORIZON)
    if steps * N_ENVS > cap:                                              # a chain crosses the wrap; the newest rows have no successor
        first_slots = (np.arange(N_ENVS) + geom["cursor"] - N_ENVS) % cap
        assert (hr.stage(fields, geom, first_slots, cfg_of(64), choice=np.zeros(N_ENVS, np.int32))["L"] == 1).all()
        L = hr.stage(fields, geom, idx, cfg_of(64), choice=np.zeros(len(idx), np.int32))["L"]
        assert any(i + (L[i] - 1) * N_ENVS >= cap for i in idx)


@pytest.mark.parametrize("cap,steps", RINGS[1:])
def test_every_relabelled_goal_was_achieved_later_in_the_same_episode(cap, steps):
    rows, episode, fields, geom, held = goal_ring(cap, steps)
    B = 256
    idx = np.random.default_rng(cap).integers(0, geom["length"], B)
    for hctr, ratio in ((0, 1.0), (1, 0.5), (2, 0.0)):
        got = hr.stage(fields, geom, idx, cfg_of(HORIZON, ratio), seed=11, hctr=hctr)
        rel = got["offset"] >= 0
        assert (rel.sum() == B) if ratio == 1.0 else (rel.sum() == 0) if ratio == 0.0 else (0.3 * B < rel.sum() < 0.7 * B)
        for b in np.flatnonzero(rel):
            r0, rg = held[idx[b]], held[got["goal_slot"][b]]
            assert episode[rg] == episode[r0] and rg == r0 + got["offset"][b] * N_ENVS and 0 <= got["offset"][b] < got["L"][b]
            g = rows["nobs"][rg][0:2]
            assert hr.bits(got["obs"][b, 4:6]).tolist() == hr.bits(g).tolist() == hr.bits(got["nobs"][b, 4:6]).tolist()
            assert hr.bits(got["obs"][b, :4]).tolist() == hr.bits(rows["obs"][r0][:4]).tolist()          # nothing else moved
            if got["offset"][b] == 0:
                assert got["rew"][b] == 0.0                                   # the row's own arrival is on its goal
        keep = ~rel
        for k, src in (("obs", "obs"), ("nobs", "nobs"), ("act", "act"), ("rew", "rew"), ("done", "done")):
            assert hr.bits(got[k][keep]).tolist() == hr.bits(fields[src][idx[keep]]).tolist(), k
        assert np.array_equal(got["done"], fields["done"][idx])               # the flag is never recomputed
    u, v1 = hr.draws(11, 0, B)
    assert 0.0 < u.min() and u.max() < 1.0 and not np.array_equal(hr.draws(11, 1, B)[1], v1) and not np.array_equal(hr.draws(12, 0, B)[1], v1)


def test_relabelling_a_row_with_its_own_goal_gives_the_stored_reward():
    rows, _, _, _, _ = goal_ring(4096, 400, seed=8)
    own = np.array([hr.goal_reward(rows["nobs"][r][0:2], rows["obs"][r][4:6], GOAL["threshold"]) for r in range(len(rows["rew"]))], F)
    assert hr.bits(own).tolist() == hr.bits(rows["rew"]).tolist() and (own == 0).sum() > 0 and (own == -1).sum() > 0


# ------------------------------------------------------------------------------------------ the restatement tells defects apart
def synthetic_case(o, a, ag, dg, G, cap=101, steps=40, window=8):
    rows, episode = hr.synthetic_ring(o, a, N_ENVS, steps, horizon=5, seed=o, term_every=3, achieved=ag, dim=G)
    fields, geom, held = hr.place(rows, cap)
    newest = (geom["cursor"] - N_ENVS + np.arange(N_ENVS)) % cap
    for s in newest:                                                      # the oldest rows continue the newest ones, bit for bit:
        fields["obs"][(s + N_ENVS) % cap] = fields["nobs"][s]             # only the age rule cuts there
        fields["done"][s] = 0.0
    cfg = dict(achieved=ag, desired=dg, dim=G, threshold=0.1, ratio=1.0, window=window, stride=N_ENVS)
    return fields, geom, cfg, newest


@pytest.mark.parametrize("defect", hr.DEFECTS)
def test_a_planted_defect_is_told_apart(defect):
    fields, geom, cfg, newest = synthetic_case(13, 3, 0, 10, 3)
    # a row whose relabelled acc is exactly thr^2: one goal dimension 0.1f away, the others on the spot
    s = int((geom["cursor"] + 3 * N_ENVS) % geom["cap"])
    nxt = (s + N_ENVS) % geom["cap"]
    fields["done"][s] = 0.0
    fields["nobs"][s][0:3] = [F(0.1), F(0.25), F(-0.5)]
    fields["obs"][nxt] = fields["nobs"][s]
    fields["nobs"][nxt][0:3] = [F(0.0), F(0.25), F(-0.5)]
    B = 64
    idx = np.concatenate([[s], newest, np.random.default_rng(5).integers(0, geom["length"], B - 1 - N_ENVS)])
    choice = np.concatenate([[1], np.full(N_ENVS, 63), np.random.default_rng(6).integers(-1, 9, B - 1 - N_ENVS)]).astype(np.int32)
    keys = hr.KEYS + ("X", "Xn")
    for ch, hctr in ((choice, 0), (None, 4)):                             # injected choices, and the native draw
        want = hr.stage(fields, geom, idx, cfg, seed=2, hctr=hctr, choice=ch)
        hr.check(want, hr.stage(fields, geom, idx, cfg, seed=2, hctr=hctr, choice=ch), keys)      # the rule equals itself
        if ch is not None:
            acc = F(F(0.1) - F(0.0)) ** 2
            assert want["rew"][0] == 0.0 and F(acc) == F(F(0.1) * F(0.1)) and (want["L"][1:1 + N_ENVS] == 1).all()
    told = 0
    for ch, hctr in ((choice, 0), (None, 4)):
        want = hr.stage(fields, geom, idx, cfg, seed=2, hctr=hctr, choice=ch)
        try:
            hr.check(want, hr.stage(fields, geom, idx, cfg, seed=2, hctr=hctr, choice=ch, defect=defect), keys)
        except hr.Mismatch:
            told += 1
    assert told >= 1, defect
    assert len(hr.DEFECTS) >= 8


# ------------------------------------------------------------------------------------------ plans and bindings
def test_update_plan_refusals_for_hindsight():
    cfg = SimpleNamespace(batch_size=64, num_envs=4, actor_update_delay=2)
    base = dict(fused=False, sampler=None, prioritized=None, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1)
    plan = loop.update_plan(cfg, **base, hindsight=dict(GOAL))
    assert plan.hindsight == dict(GOAL, stride=4) and callable(plan.update) and plan.priorities is None
    assert loop.update_plan(cfg, **base, hindsight=dict(GOAL, stride=7, ratio=0.5, window=9)).hindsight == dict(GOAL, stride=7, ratio=0.5, window=9)
    assert loop.update_plan(cfg, **base).hindsight is None and loop.update_plan(cfg, **dict(base, fused=True)).hindsight is None
    for over, msg in ((dict(fused=True), "hindsight=... needs fused=False"), (dict(sampler=object()), "hindsight=... and sampler"),
                      (dict(prioritized=dict(alpha=0.6)), "hindsight=... and prioritized"), (dict(n_step=3), "hindsight=... excludes n_step"),
                      (dict(prior_fraction=0.5), "hindsight=... and prior_fraction"),
                      (dict(n_step=3, one_launch=True), "hindsight=... excludes n_step")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            loop.update_plan(cfg, **dict(base, **over), hindsight=dict(GOAL))
    with pytest.raises(ValueError, match="unknown keys"):
        loop.update_plan(cfg, **base, hindsight=dict(GOAL, horizon=50))
    with pytest.raises(ValueError, match="missing keys"):
        loop.update_plan(cfg, **base, hindsight=dict(achieved=0, desired=4))
    # the draw of the call-by-call iteration is rb.sample_hindsight
    calls = []
    rb = SimpleNamespace(sample_hindsight=lambda n: calls.append(("sample_hindsight", n)) or "batch")
    agent = SimpleNamespace(rb=rb, update_qnets=lambda b: calls.append(("q", b)) or {}, update_actor=lambda b: calls.append(("pi", b)) or {},
                            update_targ_nets=lambda: calls.append(("targ",)), qnet_updates_so_far=0, actor_updates_so_far=0)
    plan.update(agent, 3, {})
    assert calls == [("sample_hindsight", 64), ("q", "batch"), ("pi", "batch"), ("pi", "batch"), ("targ",)]


def test_the_launcher_maps_the_flag_only_when_given():
    facts = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                 native_rollout=False, policy_stats=0)
    cfg = SimpleNamespace(batch_size=8, num_envs=4)
    assert "hindsight" not in launcher.train_keywords(cfg, **facts)
    kw = launcher.hindsight_keywords("PointGoal-native", 4)
    assert kw == dict(achieved=0, desired=4, dim=2, threshold=0.1, window=50, stride=4)
    got = launcher.train_keywords(cfg, **facts, hindsight=kw)
    assert got["hindsight"] == kw and got["fused"] is False
    args = SimpleNamespace(algo="sac", updates_per_step=None, **{k: v for k, v in facts.items() if k not in ("prior_fraction", "updates_per_step")})
    assert "hindsight" not in launcher.mode_flags(args, {})
    assert launcher.mode_flags(SimpleNamespace(hindsight=True, **vars(args)), {})["hindsight"] is True
    assert launcher.goal_layout_of("Hopper-v4") is None and launcher.goal_layout_of("CartPole-native") is None
    with pytest.raises(ValueError, match="goal layout"):
        launcher.hindsight_plan(["PointGoal-native", "Pendulum-native"], False, False)
    with pytest.raises(ValueError, match="prioritized"):
        launcher.train_keywords(cfg, **dict(facts, prioritized=True), hindsight=kw)


def run_launcher(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run"] + list(argv),
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)


@pytest.mark.parametrize("extra", [[], ["--device_env", "--native_rollout"]])
def test_launcher_dry_run_of_the_goal_bundle_with_hindsight(extra):
    out = run_launcher("--env_bundle", "native_goal", "--hindsight", *extra)
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert len(jobs) == 1 and jobs[0]["env_id"] == "PointGoal-native" and jobs[0]["rollout"] == ("NativeRollout" if extra else "Rollout")
    assert jobs[0]["hindsight"] == dict(achieved=0, desired=4, dim=2, threshold=0.1, window=50, stride=4)
    plain = run_launcher("--env_bundle", "native_goal")
    assert plain.returncode == 0 and "hindsight" not in [json.loads(ln[4:]) for ln in plain.stdout.splitlines() if ln.startswith("JOB ")][0]


def test_hindsight_on_an_env_without_a_goal_is_refused_at_the_command_line():
    out = run_launcher("--env_bundle", "debug", "--hindsight")             # Hopper-v4
    assert out.returncode == 2 and "goal layout" in out.stderr and "Hopper-v4" in out.stderr and "JOB" not in out.stdout
    out = run_launcher("--env_bundle", "native", "--hindsight")
    assert out.returncode == 2 and "Pendulum-native" in out.stderr
    out = run_launcher("--env_bundle", "native_goal", "--hindsight", "--prioritized")
    assert out.returncode == 2 and "hindsight=... and prioritized" in out.stderr


def test_header_and_binding_cover_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sactd3.h")).read(), flags=re.S)
    new = ["sactd3_hindsight_configure", "sactd3_rb_sample_hindsight", "sactd3_rb_sample_hindsight_device", "sactd3_hindsight_info_device",
           "sactd3_hindsight_stats"]
    for name in new:
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 1 and C.sizeof(_lib.CHindsightConfig) == 28 and _lib.CHindsightConfig.threshold.offset == 20
    P.build_library()
    raw = C.CDLL(P.library_path())
    assert all(hasattr(raw, name) for name in new)
    lib = P.load_library()
    assert all(getattr(lib, name).argtypes is not None for name in new)
    cfg = _lib.CHindsightConfig(0, 4, 2, 50, 4, 0.1, 0.8)
    assert lib.sactd3_hindsight_configure(None, C.byref(cfg)) == _lib.EINVAL and lib.sactd3_rb_sample_hindsight(None) == _lib.EINVAL
    assert lib.sactd3_rb_sample_hindsight_device(None, None, 1, None, 1, 0, None, 0) == _lib.EINVAL
    assert lib.sactd3_hindsight_info_device(None, None, 1, None, 1, None, 0) == _lib.EINVAL
    assert lib.sactd3_hindsight_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL
    # the kernel lives in a translation unit of its own: engine.hip names its launcher and defines no kernel for it
    csrc = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
    eng = open(os.path.join(csrc, "engine.hip")).read()
    assert "hindsight_stage_launch" in eng and not re.search(r"__global__[^;{]*hindsight", eng) and '#include "hindsight_kernels.h"' not in eng
    own = open(os.path.join(csrc, "hindsight_kernels.h")).read()
    assert re.findall(r'#include "([^"]+)"', own) == ["hindsight.h", "philox.h"] and "DevCtl" not in own
