"""GPU: the collected rollout segment (include/sactd3_rollout_collect.h, csrc/collect_kernels.h, loop.NativeRollout.collect) -- the random
mode against the call sequence bit for bit; the policy modes against the float64 actor and Philox models with their a-priori bounds
(tests/collect_model.py) and a twin env stepped with the recorded actions; the greedy mode against the evaluation kernel, which shares
its actor pass; the counters; training engines beside it; pinned rows and priorities; the refusals; and a learning run end to end."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import collect_model as M, eval_model
from tests.gpu_support import (DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, loop, same_bits, track)  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
envs = P.envs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["pendulum", "cartpole", "pointgoal"]
HORIZON, T12 = 5, 12                 # every env crosses two resets in twelve steps
RANDOM, EXPLORE, EXPLOIT, REPEAT = _lib.ROLLOUT_RANDOM, _lib.ROLLOUT_EXPLORE, _lib.ROLLOUT_EXPLOIT, _lib.ROLLOUT_REPEAT


def host(x):
    return x.cpu().numpy()


def dims_of(name):
    return envs.SPECS[envs.kind_of(name)][:3]


def new_env(name, n, seed=0, horizon=HORIZON):
    return track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=horizon))


def bound_pair(name, n, cap, algo="sac", ln=True, seed=4, B=64, count=2):
    """`count` engines at the env's dims with the same (perturbed) parameters, each behind a ReplayBuffer and the agent a rollout takes"""
    _, engs, _ = build_engines(algo, dims_of(name), B, ln=ln, count=count, seed=seed, cap=cap, max_envs=max(n, 8))
    out = []
    for e in engs:
        rb = P.ReplayBuffer(cap)
        rb._bind(e)
        out.append(SimpleNamespace(engine=e, rb=rb, timesteps_so_far=0))
    return out


def new_rollout(env, agent, seed):
    ro = loop.NativeRollout(env, agent, seed, 10 ** 9, 1)
    track(ro)
    return ro


def env_books(env):
    st, books = env.state(), env.episode_stats()
    return {**{"state." + k: v for k, v in st.items()}, **{"books." + k: np.asarray(v) for k, v in books.items()}}


def assert_same_books(x, y, what=""):
    a, b = env_books(x), env_books(y)
    assert list(a) == list(b), what
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


def ring_of(rb):
    return {k: host(v) for k, v in rb.rows(torch.arange(len(rb), device=DEV)).items()} if len(rb) else {}


def assert_same_ring(x, y, what=""):
    a, b = ring_of(x), ring_of(y)
    assert len(x) == len(y) and list(a) == list(b), what
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


def call_sequence(ro, mode, steps):
    for _ in range(steps):
        ro._ck(ro._lib.sactd3_rollout_choose(ro._h, mode))
        ro._ck(ro._lib.sactd3_rollout_advance(ro._h))


# ------------------------------------------------------------------------------------------ 1. RANDOM is the call sequence
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("name", KINDS)
def test_one_random_call_of_twelve_steps_is_the_call_sequence(name, n):
    """what the 64-row ring of the test below cannot hold: T = 12 as ONE call at a full tile and at two tiles, two resets of every env inside
    it, on a 256-row ring; a second call makes the append wrap"""
    cap, seed = 256, 9
    A, B = bound_pair(name, n, cap)
    envA, envB = new_env(name, n, seed=seed), new_env(name, n, seed=seed)
    roA, roB = new_rollout(envA, A, seed), new_rollout(envB, B, seed)
    for k in range(2):
        call_sequence(roA, RANDOM, T12)
        slab = roB.collect(T12, RANDOM)
        assert same_bits(host(roA.obs), host(roB.obs)) and same_bits(host(roA.actions), host(roB.actions)), k
        assert same_bits(host(roA.records), host(slab[(T12 - 1) * n:])), k
        assert_same_books(envA, envB, k)
        assert_same_ring(A.rb, B.rb, k)
        assert (envB.state()["episode"] >= 2 * (k + 1)).all()
    assert 2 * T12 * n > cap and len(B.rb) == cap and roA.stats() == roB.stats()
    assert_same_state(A.engine, B.engine, "ring")


@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("name", KINDS)
def test_random_collects_are_the_call_sequence_bit_for_bit(name, n):
    """A 64-row ring, horizon 5, twelve steps: every env crosses two resets and the append wraps.  A call may not hold more rows than the
    ring has slots (its own refusal), so the twelve steps are one call where they fit (n = 1, then repeated until the ring wraps) and
    the largest calls that fit otherwise; T = 1 is among them everywhere."""
    cap, seed = 64, 7
    per = min(T12, cap // n)
    calls = [1] + ([T12] * 6 if n == 1 else [per] * ((T12 - 1) // per) + ([(T12 - 1) % per] if (T12 - 1) % per else []))
    assert sum(calls) >= T12 and sum(calls) * n > cap and max(calls) * n <= cap
    A, B = bound_pair(name, n, cap)
    envA, envB = new_env(name, n, seed=seed), new_env(name, n, seed=seed)
    roA, roB = new_rollout(envA, A, seed), new_rollout(envB, B, seed)
    for k, steps in enumerate(calls):
        call_sequence(roA, RANDOM, steps)
        slab = roB.collect(steps, RANDOM)
        assert slab.shape == (steps * n, A.engine.rb_layout()["record_floats"])
        assert same_bits(host(roA.obs), host(roB.obs)) and same_bits(host(roA.actions), host(roB.actions)), k
        assert same_bits(host(roA.records), host(slab[(steps - 1) * n:])), k      # the last step's records are the sequence's slab
        assert_same_books(envA, envB, k)
        assert_same_ring(A.rb, B.rb, k)
    total = sum(calls)
    assert roA.stats() == roB.stats() == dict(random_choices=total, policy_choices=0, steps=total, rows_appended=total * n)
    assert roB.steps == total and (envB.state()["draws"] == total).all() and (envB.state()["episode"] >= 2).all()
    assert roB.collect_stats() == dict(calls=len(calls), env_steps=total, calls_that_drew=0, collect_ctr=0)
    assert roA.collect_stats() == dict(calls=0, env_steps=0, calls_that_drew=0, collect_ctr=0)
    assert len(B.rb) == cap
    assert_same_state(A.engine, B.engine, "ring")


# ------------------------------------------------------------------------------------------ 2. the policy modes
def collect_and_check(name, algo, ln, mode, n, T, agents, seed):
    """one call on agents[0]'s engine; the twin env stepped with the recorded actions; agents[1]'s engine given the slab by extend_records"""
    sac = algo == "sac"
    o, a, bound = dims_of(name)
    A, B = agents
    eng = A.engine
    env, twin = new_env(name, n, seed=seed), new_env(name, n, seed=seed)
    ro = new_rollout(env, A, seed)
    twin.reset(seed=seed)
    before = env.state()
    assert_same_books(env, twin, "before")
    ctr = ro.collect_stats()["collect_ctr"]
    slab, eps = ro.collect(T, mode, eps=True)
    layout = eng.rb_layout()
    L = (layout["record_floats"], layout["next_obs_offset"], layout["next_obs_width"])
    assert L == M.layout_for(o, a)
    got_slab = host(slab)
    acts = M.fields(got_slab, L, o, a)["a"].reshape(T, n, a)
    rec, obs = torch.zeros((n, L[0]), device=DEV), torch.zeros((n, o), device=DEV)
    rebuilt = []
    for t in range(T):
        twin.step_records(torch.as_tensor(np.ascontiguousarray(acts[t]), device=DEV), layout, rec, obs)
        rebuilt.append(host(rec))
    p = eval_model.actor_params(eng.get_params(_lib.ACTOR), o, (2 if sac else 1) * a, ln)
    worst = M.check_collect({"slab": got_slab, "eps": host(eps), "state": env.state()}, p, kind=name, n=n, T=T, mode=mode, sac=sac, ln=ln,
                            scale=np.full(a, bound, np.float32), bias=np.zeros(a, np.float32), noise_std=eng.cfg.actor_noise_std,
                            seed=eng.cfg.seed, ctr=ctr, env_seed=seed, draws0=before["draws"], layout=L, rebuilt=np.concatenate(rebuilt, 0),
                            twin_state=twin.state())
    assert_same_books(env, twin, "after")
    assert same_bits(host(ro.obs), host(obs)) and same_bits(host(ro.actions), acts[T - 1])
    B.rb.extend_records(slab)
    assert_same_ring(A.rb, B.rb)
    assert ro.stats() == dict(random_choices=0, policy_choices=T, steps=T, rows_appended=T * n)
    ro.close()
    return worst


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("name", KINDS)
def test_policy_collects_sit_inside_the_models_and_replay_on_a_twin(name, algo, ln):
    n, T = 17, HORIZON + 3                       # two tiles with a ragged second; a reset inside the call
    agents = bound_pair(name, n, 512, algo=algo, ln=ln)
    worst = {}
    for k, mode in enumerate((EXPLOIT, EXPLORE, EXPLORE)):
        worst[k] = collect_and_check(name, algo, ln, mode, n, T, agents, seed=3 + k)
    print(f"{name} {algo} ln={ln}: worst |err| / bound {worst}")
    assert all(0.0 < w <= 1.0 for w in worst.values())
    assert_same_state(agents[0].engine, agents[1].engine, "ring")


def test_one_env_and_one_step_pass():
    agents = bound_pair("pointgoal", 1, 64)
    assert collect_and_check("pointgoal", "sac", True, EXPLORE, 1, 1, agents, seed=1) <= 1.0
    agents = bound_pair("pendulum", 16, 64, algo="td3")
    assert collect_and_check("pendulum", "td3", True, EXPLORE, 16, 1, agents, seed=1) <= 1.0


# ------------------------------------------------------------------------------------------ 3. EXPLOIT against the evaluation kernel
@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("name", KINDS)
def test_exploit_is_the_evaluation_kernels_greedy_rollout(name, algo):
    """the same env state, the same parameters: sactd3_eval_rollout(GREEDY, reset = 0) gives the same actions, observations and rewards
    bit for bit -- both kernels call the one actor pass"""
    n, T, seed = 17, HORIZON + 3, 5
    o, a, _ = dims_of(name)
    (A,) = bound_pair(name, n, 512, algo=algo, count=1)
    env, other = new_env(name, n, seed=seed), new_env(name, n, seed=seed)
    ro = new_rollout(env, A, seed)
    other.reset(seed=seed)
    slab = host(ro.collect(T, EXPLOIT))
    rec = envs.policy_rollout(other, A, steps=T, mode="greedy", reset=False, trajectories=True)
    layout = A.engine.rb_layout()
    f = M.fields(slab, (layout["record_floats"], layout["next_obs_offset"], layout["next_obs_width"]), o, a)
    assert same_bits(f["a"].reshape(T, n, a), host(rec["actions"]))
    assert same_bits(f["s"].reshape(T, n, o), host(rec["obs"]))
    assert same_bits(f["r"].reshape(T, n), host(rec["reward"]))
    assert_same_books(env, other)


# ------------------------------------------------------------------------------------------ 4. counters, and what training sees
def test_only_exploring_calls_move_the_counter_and_training_sees_rows_alone():
    name, n, T, seed = "pendulum", 17, 4, 2
    o, a, bound = dims_of(name)
    A, B = bound_pair(name, n, 2048)
    data = synth_transitions(1024, o, a, bound, seed=6)
    for ag in (A, B):
        ag.engine.rb_extend(*[t.numpy() for t in data])
    env = new_env(name, n, seed=seed)
    ro = new_rollout(env, B, seed)
    stats0 = {k: getattr(B.engine, k)() for k in ("predict_device_stats", "policy_stats", "eval_stats") if hasattr(B.engine, k)}
    seen, ctrs = [], []
    for mode in (EXPLORE, RANDOM, EXPLORE, EXPLOIT):
        slab, eps = ro.collect(T, mode, eps=True)
        seen.append(host(eps).copy())
        ctrs.append(ro.collect_stats()["collect_ctr"])
        A.rb.extend_records(slab.clone())
        for i in range(3):
            A.engine.step(i % 2 == 0)
            B.engine.step(i % 2 == 0)
    torch.cuda.synchronize()
    assert ctrs == [1, 1, 2, 2]
    assert np.abs(seen[0]).min() > 0 and np.abs(seen[2]).min() > 0 and not same_bits(seen[0], seen[2])
    assert not seen[1].any() and not seen[3].any()
    assert ro.collect_stats() == dict(calls=4, env_steps=4 * T, calls_that_drew=2, collect_ctr=2)
    assert stats0 == {k: getattr(B.engine, k)() for k in stats0}                # no acting, policy or evaluation counter moved
    assert_same_state(A.engine, B.engine, "slot", "noise", "ring")


# ------------------------------------------------------------------------------------------ 5. pinned rows, priorities
@pytest.mark.parametrize("case", ["pinned", "priorities"])
def test_the_append_is_extend_records_behind_a_pinned_prefix_and_with_priorities(case):
    name, n, T, cap, seed = "cartpole", 4, 9, 150, 3
    o, a, bound = dims_of(name)
    A, B = bound_pair(name, n, cap)
    if case == "pinned":
        pre = [t.numpy() for t in synth_transitions(37, o, a, bound, seed=2)]
        for ag in (A, B):
            ag.engine.rb_extend(*pre)
            ag.rb.pin()
    else:
        for ag in (A, B):
            ag.rb.enable_priorities()
    env = new_env(name, n, seed=seed)
    ro = new_rollout(env, B, seed)
    for k in range(5):                                                         # 180 rows: the region behind the prefix wraps
        slab = ro.collect(T, (RANDOM, EXPLORE)[k % 2])
        A.rb.extend_records(slab.clone())
    torch.cuda.synchronize()
    assert len(A.rb) == len(B.rb) == cap
    if case == "pinned":
        assert A.engine.rb_pinned() == B.engine.rb_pinned() == 37
        assert_same_state(A.engine, B.engine, "ring")
    else:
        assert_same_state(A.engine, B.engine, "prio", "ring")


# ------------------------------------------------------------------------------------------ 6. refusals
def test_every_refusal_leaves_engine_env_ring_and_counters_untouched():
    name, n, cap, seed = "pendulum", 4, 64, 2
    o, a, bound = dims_of(name)
    (A,) = bound_pair(name, n, cap, count=1)
    A.engine.rb_extend(*[t.numpy() for t in synth_transitions(10, o, a, bound, seed=2)])
    A.rb.pin()
    env = new_env(name, n, seed=seed)
    ro = new_rollout(env, A, seed)
    ro.collect(2, RANDOM)                                                       # an accepted call in front: first-use state exists
    torch.cuda.synchronize()
    A.engine.sync()
    lib, h = ro._lib, ro._h
    L = A.engine.rb_layout()["record_floats"]
    slab = torch.full((16 * n + 1, L), -7.0, device=DEV)
    eps = torch.full((16, n, a), -7.0, device=DEV)
    room = np.zeros(4 * n * L + 4, np.float32)
    on_host = room[(-room.ctypes.data % 16) // 4:]

    def snapshot():
        return (env_books(env), ring_of(A.rb), ro.stats(), ro.collect_stats(), host(ro.obs), host(ro.actions), host(slab), host(eps),
                engine_state(A.engine))
    before = snapshot()
    boundary = A.engine.boundary_stats()

    def call(mode=EXPLORE, steps=2, rec=slab.data_ptr(), e=eps.data_ptr(), handle=h):
        rc = lib.sactd3_rollout_collect(handle, mode, steps, C.c_void_p(rec), C.c_void_p(e))
        return rc, lib.sactd3_rollout_last_error(handle).decode()
    assert lib.sactd3_rollout_collect(None, EXPLORE, 2, C.c_void_p(slab.data_ptr()), None) == _lib.EINVAL
    assert lib.sactd3_rollout_collect_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL
    cases = {"no slab": (dict(rec=None), "NULL"), "misaligned": (dict(rec=slab.data_ptr() + 4), "aligned"),
             "host slab": (dict(rec=on_host.ctypes.data), "device memory"), "host eps": (dict(e=on_host.ctypes.data), "device memory"),
             "repeat": (dict(mode=REPEAT), "mode"), "unknown mode": (dict(mode=9), "mode"), "negative mode": (dict(mode=-1), "mode"),
             "no steps": (dict(steps=0), "steps"), "negative steps": (dict(steps=-3), "steps"), "too many steps": (dict(steps=4097), "steps"),
             "more rows than slots": (dict(steps=14), "ring slots")}         # 14 * 4 = 56 > 64 - 10 pinned; 13 * 4 = 52 fits
    for what, (kw, word) in cases.items():
        rc, text = call(**kw)
        assert rc == _lib.EINVAL and word in text and "collect" in text, (what, rc, text)
    A.engine.predict_begin(np.zeros((n, o), np.float32), True)
    rc, text = call()
    assert rc == _lib.ESTATE and "in flight" in text
    A.engine.predict_end()
    torch.cuda.synchronize()
    A.engine.sync()
    assert A.engine.boundary_stats() == boundary                                # no refused call recorded an event
    after = snapshot()
    for x, y in zip(before[:2], after[:2]):
        assert list(x) == list(y) and all(same_bits(x[k], y[k]) for k in x)
    assert before[2] == after[2] and before[3] == after[3]
    assert all(same_bits(x, y) for x, y in zip(before[4:8], after[4:8]))
    assert_same_state(before[8], after[8])
    # and the largest call that fits, right behind them
    rc, text = call(steps=13)
    assert rc == 0, text
    torch.cuda.synchronize()
    got = host(slab)
    assert (got[13 * n:] == np.float32(-7.0)).all() and not (got[:13 * n] == np.float32(-7.0)).any()
    assert (host(eps)[:13] != np.float32(-7.0)).all() and (host(eps)[13:] == np.float32(-7.0)).all()
    assert ro.collect_stats() == dict(calls=2, env_steps=15, calls_that_drew=1, collect_ctr=1) and len(A.rb) == cap
    for bad in (0, -1, 4097):                                                  # the mirror refuses these itself, and allocates nothing for them
        with pytest.raises(ValueError, match="steps"):
            ro.collect(bad)
    assert sorted(ro._slabs) == [2]
    with pytest.raises(P.EngineError, match="ring slots"):                      # the engine's own refusal comes through the call
        ro.collect(14)


# ------------------------------------------------------------------------------------------ 7. learning end to end
def test_sac_learns_the_pendulum_through_collected_segments():
    """loop.train(collected_rollout=True): 4 envs, segment_len 4, updates_per_step 4, the 3 500 updates of the pendulum test.  The bar is the
    oracle agent's under the same collect-then-update schedule on the host twin: worst of three seeds minus their spread
    (tools/collect_probe.py --oracle -> profiles/collect.json)."""
    with open(os.path.join(ROOT, "profiles", "collect.json")) as f:
        rec = json.load(f)["learning"]
    b = rec["budget"]
    name, seed, episodes = b["kind"], 0, rec["episodes"]
    assert (b["num_envs"], b["segment_len"], b["updates_per_step"], b["updates"]) == (4, 4, 4, 3500)

    def sac_cfg(max_envs=None):
        steps = b["learning_starts"] + (b["updates"] // b["updates_per_step"]) * b["segment_len"] * b["num_envs"]
        return P.launcher.job_config("sac", name, seed, num_envs=max_envs or b["num_envs"], learning_starts=b["learning_starts"],
                                     batch_size=b["batch_size"], num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15,
                                     segment_len=b["segment_len"])
    cfg = sac_cfg()
    o, a, bound = dims_of(name)
    torch.manual_seed(seed)
    acfg = sac_cfg(max_envs=episodes)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), acfg,
                    P.ReplayBuffer(acfg.rb_capacity), seed=seed)
    track(agent.engine)
    eval_env = new_env(name, episodes, seed=seed + rec["eval_seed_offset"], horizon=None)
    before = envs.greedy_returns(eval_env, agent, episodes, one_launch=True)
    env = new_env(name, cfg.num_envs, seed=seed, horizon=None)
    loop.train(cfg, env, agent, device_env=True, native_rollout=True, collected_rollout=True, updates_per_step=b["updates_per_step"])
    after = envs.greedy_returns(eval_env, agent, episodes, one_launch=True)
    print(f"{name}: greedy return {before['return']:.1f} -> {after['return']:.1f}; bar {rec['bar']:.1f}; updates {agent.qnet_updates_so_far}")
    assert agent.qnet_updates_so_far >= b["updates"] and agent.engine.predict_device_stats()["calls"] == 0      # every action came from a collect
    assert after["bad_actions"] == 0 and len(agent.rb) == agent.timesteps_so_far
    assert before["return"] < rec["bar"] < after["return"], (before["return"], after["return"], rec["bar"])
