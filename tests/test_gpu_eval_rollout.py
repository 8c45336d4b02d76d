"""GPU: the one-launch evaluation rollout (include/sactd3_eval.h, csrc/eval_kernels.h, envs.policy_rollout / q_bias) against a twin env
stepped with the recorded actions (bit for bit), the float64 actor and Philox models with their a-priori bounds and the float32 return
recurrences (tests/eval_model.py), beside training engines, through its refusals, and end to end: a learned pendulum evaluated in one
launch against the bar tests/test_gpu_native_env.py applies, and the Q-bias of critics set to a constant."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bounds, eval_model as M
from tests.gpu_support import (DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, loop, same_bits, schema, track)  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
envs = P.envs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["pendulum", "cartpole", "pointgoal"]
HORIZON = 4                         # an auto-reset and the end of the call's episode fall inside a handful of steps
NS = (1, 5, 16, 17, 33)             # a partial tile, exactly one, one plus a row, two plus a row
TS = (1, 3, HORIZON + 3)
GAMMA = 0.9


def new_env(name, n, seed=0, horizon=HORIZON):
    return track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=horizon))


def dims_of(name):
    return envs.SPECS[envs.kind_of(name)][:3]


def engine_for(name, algo, ln, count=1, seed=7, **kw):
    _, engs, _ = build_engines(algo, dims_of(name), 64, ln=ln, count=count, seed=seed, cap=2048, **kw)
    return engs if count > 1 else engs[0]


def host(rec):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()}


def roll(eng, env, **kw):
    return host(envs.policy_rollout(env, SimpleNamespace(engine=eng), trajectories=True, gamma=GAMMA, **kw))


def replay_on_twin(twin, rec, obs0):
    """(a): the twin stepped with the recorded actions gives the recorded observations and rewards -> the flags of every step"""
    T = rec["steps"]
    ended, terminated = [], []
    obs = obs0
    for t in range(T):
        assert same_bits(obs.cpu().numpy(), rec["obs"][t]), ("obs", t)
        obs, rew, term, trunc, infos = twin.step(torch.as_tensor(rec["actions"][t], device=DEV))
        assert same_bits(rew.cpu().numpy(), rec["reward"][t]), ("reward", t)
        terminated.append(term.cpu().numpy().astype(bool))
        ended.append(infos["_final_observation"].cpu().numpy().astype(bool))
        assert np.array_equal(ended[-1], terminated[-1] | trunc.cpu().numpy().astype(bool))
    return np.stack(ended), np.stack(terminated)


def same_env(env, twin):
    a, b = env.state(), twin.state()
    for k in a:
        assert same_bits(a[k], b[k]), ("state", k)
    a, b = env.episode_stats(), twin.episode_stats()
    for k in a:
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), ("books", k)


def check(eng, rec, ended, terminated, *, ln, sac, sample, ctr):
    """(b), (c): every recorded element against tests/eval_model.py; rec["_bound"]: the env's action bound (scale; the bias is 0)"""
    a = eng.cfg.ac_dim
    p = M.actor_params(eng.get_params(_lib.ACTOR), eng.cfg.ob_dim, (2 if sac else 1) * a, ln)
    scale = np.full(a, rec["_bound"], np.float32)
    rec = dict(rec, ended=ended, terminated=terminated, ep_terminated=rec["ep_terminated"].astype(np.uint8))      # (policy_rollout hands out bools)
    return M.check_rollout(rec, p, ln=ln, sac=sac, sample=sample, soft=sample, gamma=GAMMA, scale=scale, bias=np.zeros(a, np.float32),
                           log_alpha=float(eng.get_params(_lib.LOG_ALPHA)[0]) if sac else 0.0, seed=eng.cfg.seed, ctr=ctr)


# ------------------------------------------------------------------------------------------ (a) (b) (c): every shape, every config
@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("name", KINDS)
def test_rollouts_replay_on_a_twin_and_sit_inside_the_models(name, algo, ln):
    sac = algo == "sac"
    eng = engine_for(name, algo, ln)
    bound = dims_of(name)[2]
    worst, calls, drew = 0.0, 0, 0
    for n in NS:
        env, twin = new_env(name, n, seed=1), new_env(name, n, seed=2)
        for T in TS:
            sample = sac and (T != 3 or n == 5)            # SAC: sampled and soft, and greedy at T = 3
            seed = 100 * n + T
            ctr = eng.eval_stats()["eval_ctr"]
            rec = roll(eng, env, steps=T, mode="sample" if sample else "greedy", soft=sample, seed=seed)
            obs0 = twin.reset(seed=seed)[0]
            ended, terminated = replay_on_twin(twin, rec, obs0)
            same_env(env, twin)
            rec["_bound"] = bound
            worst = max(worst, check(eng, rec, ended, terminated, ln=ln, sac=sac, sample=sample, ctr=ctr))
            calls, drew = calls + 1, drew + int(sample)
            if T > HORIZON:                                 # the time limit ended every call's episode; the steps behind it are not its own
                assert (rec["ep_length"] == HORIZON).all() and not rec["live"][HORIZON:].any() and rec["live"][:HORIZON].all()
                st = env.episode_stats()
                assert same_bits(rec["ep_return"], st["first_return"]) and same_bits(rec["ep_length"], st["first_length"])
            else:
                assert (rec["ep_length"] == 0).all() and rec["live"].all() and not rec["rtg"].any()
            if sample:
                assert np.abs(rec["eps"]).max() > 0 and np.isfinite(rec["logp"]).all()
    st = eng.eval_stats()
    assert st["calls"] == calls and st["calls_that_drew"] == drew == st["eval_ctr"] and st["env_steps"] == sum(NS) * sum(TS)
    print(f"{name} {algo} ln={ln}: worst |err| / bound {worst:.3g} over {calls} rollouts")
    assert 0.0 < worst <= 1.0


def test_saturated_heads_stay_inside_the_model():
    """the head weights x 50: tanh saturates, the log-prob's correction term is at its worst"""
    name, n, T = "pointgoal", 17, HORIZON + 3
    eng = engine_for(name, "sac", True)
    o, a, bound = dims_of(name)
    p = M.actor_params(eng.get_params(_lib.ACTOR), o, 2 * a, True)
    p["Wh"] = (p["Wh"] * np.float32(50.0)).astype(np.float32)
    eng.set_params(_lib.ACTOR, M.flat_of(p, o, 2 * a, True))
    env, twin = new_env(name, n, seed=1), new_env(name, n, seed=2)
    rec = roll(eng, env, steps=T, mode="sample", soft=True, seed=9)
    ended, terminated = replay_on_twin(twin, rec, twin.reset(seed=9)[0])
    same_env(env, twin)
    rec["_bound"] = bound
    assert check(eng, rec, ended, terminated, ln=True, sac=True, sample=True, ctr=0) <= 1.0
    assert (np.abs(rec["actions"]) > 0.999 * bound).mean() > 0.25      # the case is what it says


def test_termination_beats_truncation_from_a_set_state():
    """the cart-pole one step from its angle limit, two steps into a four-step horizon, reset == 0: the call's episode is one step long"""
    name, n, T = "cartpole", 17, 3
    eng = engine_for(name, "td3", True)
    env, twin = new_env(name, n, seed=3), new_env(name, n, seed=3)
    state = {"phys": np.tile(np.array([0.0, 0.0, 0.2094, 2.0], np.float32), (n, 1)), "steps": np.full(n, 2, np.int32),
             "returns": np.full(n, 2.0, np.float32)}
    for e in (env, twin):
        e.reset(seed=3)
        e.set_state(state)
    rec = roll(eng, env, steps=T, reset=False)
    obs0 = torch.as_tensor(np.ascontiguousarray(state["phys"]), device=DEV)      # (the cart-pole observes its state)
    ended, terminated = replay_on_twin(twin, rec, obs0)
    same_env(env, twin)
    rec["_bound"] = 1.0
    assert check(eng, rec, ended, terminated, ln=True, sac=False, sample=False, ctr=0) <= 1.0
    assert terminated[0].all() and (rec["ep_length"] == 1).all() and rec["ep_terminated"].all() and (rec["live"].sum(0) == 1).all()
    assert same_bits(rec["ep_return"], np.ones(n, np.float32)) and same_bits(rec["g0"], np.ones(n, np.float32))      # inside the call only
    assert same_bits(env.episode_stats()["first_return"], np.full(n, 3.0, np.float32))                                 # the env's books count all of it


# ------------------------------------------------------------------------------------------ (d) invisible to training and acting
def test_training_does_not_see_the_rollouts():
    name = "pendulum"
    o, a, bound = dims_of(name)
    A, B = engine_for(name, "sac", True, count=2, seed=4)
    data = synth_transitions(1024, o, a, bound, seed=6)
    for e in (A, B):
        e.rb_extend(*[t.numpy() for t in data])
    env = new_env(name, 17, seed=1)
    agent = SimpleNamespace(engine=B)

    def evaluate(k):
        envs.policy_rollout(env, agent, steps=5, mode="sample" if k % 2 else "greedy", soft=bool(k % 2), seed=k, trajectories=bool(k % 3))
    for i in range(6):
        for e in (A, B):
            e.step(i % 2 == 0)
        evaluate(i)
    for i in range(4):                                       # the pipelined period: its precomputed opening pair stays valid
        for e in (A, B):
            e.step_period()
        evaluate(i + 1)
    for e in (A, B):                                         # the API sequence
        e.rb_sample()
        e.update_qnets()
        if e is B:
            evaluate(1)
        e.update_actor()
        e.update_actor()
        e.update_targ_nets(1)
    torch.cuda.synchronize()
    assert_same_state(A, B, "slot", "noise")
    for stats in ("predict_device_stats", "policy_stats", "acting_stats", "qvalues_stats"):
        if hasattr(A, stats):
            assert getattr(A, stats)() == getattr(B, stats)(), stats
    assert A.eval_stats() == {"calls": 0, "env_steps": 0, "calls_that_drew": 0, "eval_ctr": 0}
    got = B.eval_stats()
    assert got["calls"] == 11 and got["env_steps"] == 11 * 5 * 17 and got["calls_that_drew"] == got["eval_ctr"] == 6


# ------------------------------------------------------------------------------------------ (e) a NaN parameter
def test_a_nan_parameter_yields_counted_bad_actions():
    """a NaN behind the last ReLU (the head's bias: fmaxf(NaN, 0) = 0 swallows one in a hidden layer, here as in the engine's own acting
    kernels) makes every action NaN: the env replaces and counts it, nothing faults"""
    name, n, T = "pendulum", 17, 5
    eng = engine_for(name, "sac", True)
    o, a, _ = dims_of(name)
    p = M.actor_params(eng.get_params(_lib.ACTOR), o, 2 * a, True)
    p["bh"][0] = np.nan
    eng.set_params(_lib.ACTOR, M.flat_of(p, o, 2 * a, True))
    env, twin = new_env(name, n, seed=1), new_env(name, n, seed=2)
    rec = roll(eng, env, steps=T, seed=4)
    assert np.isnan(rec["actions"]).all()
    replay_on_twin(twin, rec, twin.reset(seed=4)[0])          # the NaN never reaches the state: the twin replaces it the same way
    same_env(env, twin)
    assert env.episode_stats()["bad_actions"] == n * T and np.isfinite(env.state()["phys"]).all() and np.isfinite(rec["reward"]).all()


# ------------------------------------------------------------------------------------------ (f) refusals
def raw_call(eng, env_handle, cfg, out, flags=_lib.SRC_ORDERED):
    return eng.lib.sactd3_eval_rollout(eng._h, env_handle, C.byref(cfg) if cfg is not None else None, C.byref(out) if out is not None else None,
                                       None, flags)


def test_every_refusal_leaves_engine_and_env_untouched():
    sac, td3 = engine_for("pendulum", "sac", True), engine_for("pendulum", "td3", True)
    env, other = new_env("pendulum", 5, seed=1), new_env("cartpole", 5, seed=1)
    env.reset(seed=1)
    env.step(env.action_space.sample())
    before_env, before_books = env.state(), env.episode_stats()
    before = {id(e): engine_state(e) for e in (sac, td3)}
    dev = torch.zeros(64, device=DEV)
    on_host = np.zeros(64, np.float32)

    def cfg(steps=3, mode=0, reset=1, soft=0, gamma=0.9, seed=1):
        return _lib.CEvalConfig(steps, mode, reset, soft, gamma, seed)

    def out(**kw):
        o = _lib.CEvalOut()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    ok = out(reward=dev.data_ptr())
    cases = {
        "steps below": (sac, env._h, cfg(steps=-1), ok, 1), "steps above": (sac, env._h, cfg(steps=4097), ok, 1),
        "gamma below": (sac, env._h, cfg(gamma=-0.1), ok, 1), "gamma above": (sac, env._h, cfg(gamma=1.5), ok, 1),
        "gamma nan": (sac, env._h, cfg(gamma=float("nan")), ok, 1), "mode": (sac, env._h, cfg(mode=2), ok, 1),
        "reset": (sac, env._h, cfg(reset=2), ok, 1), "sample on td3": (td3, env._h, cfg(mode=1), ok, 1),
        "soft on td3": (td3, env._h, cfg(soft=1), ok, 1), "soft without sample": (sac, env._h, cfg(soft=1), ok, 1),
        "host output": (sac, env._h, cfg(), out(reward=on_host.ctypes.data), 1), "host summary": (sac, env._h, cfg(), out(g0=on_host.ctypes.data), 1),
        "unknown flag": (sac, env._h, cfg(), ok, 2), "dims": (sac, other._h, cfg(), ok, 1), "no env": (sac, None, cfg(), ok, 1),
        "no config": (sac, env._h, None, ok, 1), "no outputs": (sac, env._h, cfg(), None, 1),
    }
    for what, (eng, handle, c, o, flags) in cases.items():
        assert raw_call(eng, handle, c, o, flags) == _lib.EINVAL, what
        assert b"eval_rollout" in eng.lib.sactd3_last_error(eng._h), what
    assert sac.lib.sactd3_eval_rollout(None, env._h, C.byref(cfg()), C.byref(ok), None, 1) == _lib.EINVAL
    torch.cuda.synchronize()
    for e in (sac, td3):
        assert e.eval_stats() == {"calls": 0, "env_steps": 0, "calls_that_drew": 0, "eval_ctr": 0}
        assert_same_state(before[id(e)], engine_state(e))
    for k, v in env.state().items():
        assert same_bits(v, before_env[k]), k
    for k, v in env.episode_stats().items():
        assert same_bits(np.asarray(v), np.asarray(before_books[k])), k
    assert not dev.any()
    with pytest.raises(P.EngineError, match="SAC only"):
        envs.policy_rollout(env, SimpleNamespace(engine=td3), mode="sample")
    with pytest.raises(TypeError, match="NativeVecEnv"):
        envs.policy_rollout(envs.HostVecEnv("pendulum", 5), SimpleNamespace(engine=sac))
    # and an accepted call right behind them, with every output left out but one
    assert raw_call(sac, env._h, cfg(), ok) == 0
    torch.cuda.synchronize()
    assert dev[:15].abs().min() > 0 and not dev[15:].any() and sac.eval_stats()["calls"] == 1


# ------------------------------------------------------------------------------------------ (g) learned end to end, evaluated in one launch
def test_sac_learns_the_pendulum_and_one_launch_evaluation_says_so():
    """the recipe and the bar of tests/test_gpu_native_env.py::test_sac_learns_the_task_on_the_device (profiles/native_env.json), the greedy
    return read through greedy_returns(one_launch=True); the default loop, on the same trained policy, is float32-close to it"""
    name = "pendulum"
    with open(os.path.join(ROOT, "profiles", "native_env.json")) as f:
        rec = json.load(f)["learning"]
    task = rec["tasks"][name]
    assert task["test_kept"]
    seed, episodes, budget = 0, rec["episodes"], task["budget"]

    def sac_cfg(max_envs=None):
        steps = budget["learning_starts"] + budget["updates"] * budget["num_envs"]
        return P.launcher.job_config("sac", name, seed, num_envs=max_envs or budget["num_envs"], learning_starts=budget["learning_starts"],
                                     batch_size=budget["batch_size"], num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)
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
    loop.train(cfg, env, agent, device_env=True)
    after = envs.greedy_returns(eval_env, agent, episodes, one_launch=True)
    looped = envs.greedy_returns(eval_env, agent, episodes)
    print(f"{name}: one-launch greedy return {before['return']:.1f} -> {after['return']:.1f} (the loop: {looped['return']:.1f}); bar {task['bar']:.1f}")
    assert set(after) == set(looped) and after["episodes"] == episodes and (after["lengths"] == eval_env.horizon).all()
    assert after["bad_actions"] == 0 and agent.engine.eval_stats()["calls"] == 2
    assert before["return"] < task["bar"] < after["return"], (before["return"], after["return"], task["bar"])
    gen = envs.device_episodes(eval_env, agent, seed, one_launch=True)
    first = next(gen)
    assert set(first) == {"length", "return"} and float(first["length"]) == eval_env.horizon


# ------------------------------------------------------------------------------------------ (h) the Q-bias of constant critics
def test_q_bias_of_constant_critics_is_exact():
    name, n, c, seed = "cartpole", 16, 7.5, 3
    o, a, bound = dims_of(name)
    cfg = P.launcher.job_config("td3", name, seed, num_envs=4, learning_starts=10 ** 6, batch_size=64, num_timesteps=10, eval_every=10 ** 9,
                                rb_capacity=1 << 12)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    eng = track(agent.engine)
    ln = bool(eng.cfg.layer_norm)
    one = schema.flat_to_dict(np.zeros_like(eng.get_params(_lib.CRITICS).reshape(2, -1)[0]), o + a, 1, ln)
    one["head.bias"] = np.full(1, c, np.float32)
    flat = schema.dict_to_flat(one, o + a, 1, ln)
    eng.set_params(_lib.CRITICS, np.concatenate([flat, flat]))
    env = new_env(name, n, seed=seed, horizon=None)
    got = envs.q_bias(env, agent, seed=seed)
    rec = host(envs.policy_rollout(env, agent, seed=seed, trajectories=True))          # greedy TD3: the same episodes again
    g = float(np.float32(eng.cfg.gamma))
    T = rec["steps"]
    L, term = rec["ep_length"].astype(np.int64), rec["ep_terminated"]
    left = np.maximum(L[None, :] - np.arange(T)[:, None], 0).astype(np.float64)
    counted = (rec["live"] != 0) & (L[None, :] > 0) & (term[None, :] | (g ** left <= 0.05))
    G = rec["rtg"].astype(np.float64)[counted]
    bias = c - G
    assert term.any() and got["rows"] == int(counted.sum()) > 0                       # the untrained policy drops the pole
    assert got["bias_mean"] == pytest.approx(bias.mean(), rel=1e-9) and got["bias_std"] == pytest.approx(bias.std(), rel=1e-7)
    assert got["return_mean"] == pytest.approx(G.mean(), rel=1e-9)
    assert got["mean"] == pytest.approx(bias.mean() / abs(G.mean()), rel=1e-9) and got["std"] == pytest.approx(bias.std() / abs(G.mean()), rel=1e-7)
    short = new_env("pendulum", 5, seed=1)                                             # four steps, nothing terminates, 0.99^4 > 0.05
    o2, a2, b2 = dims_of("pendulum")
    cfg2 = P.launcher.job_config("td3", "pendulum", seed, num_envs=4, learning_starts=10 ** 6, batch_size=64, num_timesteps=10, eval_every=10 ** 9,
                                 rb_capacity=1 << 12)
    agent2 = P.Agent({"ob_shape": (o2,), "ac_shape": (a2,)}, np.full(a2, -b2, np.float32), np.full(a2, b2, np.float32), torch.device(DEV), cfg2,
                     P.ReplayBuffer(cfg2.rb_capacity), seed=seed)
    track(agent2.engine)
    with pytest.raises(ValueError, match="longer horizon"):
        envs.q_bias(short, agent2, seed=1)


# ------------------------------------------------------------------------------------------ the loop's keyword
def test_a_run_with_q_bias_logs_it_and_keeps_its_bits():
    """loop.train(q_bias=dict(env=, seed=)) on the cart-pole: the three vitals at every evaluation point, and the run's engine ends bit for
    bit where the run without the keyword ends"""
    name, seed = "cartpole", 5
    o, a, bound = dims_of(name)

    def run(with_bias):
        cfg = P.launcher.job_config("sac", name, seed, num_envs=4, learning_starts=200, batch_size=64, num_timesteps=999, eval_every=400,
                                    rb_capacity=1 << 12)
        torch.manual_seed(seed)
        agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), cfg,
                        P.ReplayBuffer(cfg.rb_capacity), seed=seed)
        track(agent.engine)
        env = new_env(name, cfg.num_envs, seed=seed, horizon=None)
        seen = []
        kw = dict(q_bias=dict(env=new_env(name, 16, seed=seed + 1, horizon=None), seed=seed + 1)) if with_bias else {}
        metrics = loop.train(cfg, env, agent, device_env=True, evaluator=None, on_eval=lambda ag, t: seen.append(("eval", t)), **kw)
        return agent, metrics, seen
    plain, m0, seen0 = run(False)
    biased, m1, seen1 = run(True)
    torch.cuda.synchronize()
    assert_same_state(plain.engine, biased.engine, "slot", "noise")
    assert seen0 == seen1 == [("eval", 400), ("eval", 800)]
    assert set(m1) - set(m0) == set(loop.QBias.KEYS) and m1["vitals/q_bias_rows"] > 0 and np.isfinite(m1["vitals/q_bias_mean"])
    assert m1["vitals/q_bias_std"] >= 0 and biased.engine.eval_stats()["calls"] == 2 and plain.engine.eval_stats()["calls"] == 0
    assert {k: v for k, v in m1.items() if k in m0} == m0
