"""GPU: the GPU-resident vector environments (include/sactd3_env.h, csrc/env_kernels.h, envs.py) against the float64 model and its
a-priori bound (tests/env_model.py), the numpy Philox model bit for bit, through the loop into the replay ring, beside a training
engine, and -- what they are for -- learned by the engine end to end, against a bar measured on the oracle
(profiles/native_env.json, tools/native_env_probe.py --oracle)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import bounds, env_model as em
from tests.gpu_support import (DEV, SENTINEL, P, _lib, assert_same_state, build_engines, close_engines, loop, same_bits, track)  # noqa: F401
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu
envs = P.envs
KINDS = ["pendulum", "cartpole"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def new_env(name, n, seed=0, horizon=None):
    return track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=horizon))


def host(x):
    return x.cpu().numpy()


def got_of(res):
    """what NativeVecEnv.step returned, on the host, as em.check_step takes it"""
    obs, rew, term, trunc, infos = res
    return {"obs": host(obs), "final_obs": host(infos["final_observation"]), "reward": host(rew), "terminated": host(term),
            "truncated": host(trunc), "ended": host(infos["_final_observation"])}


def step_wide(env, actions):
    """sactd3_env_step through the raw ABI with every stride wider than its row, sentinels in between -> got; the sentinels survive"""
    n, o = env.n, env.o
    act = torch.full((n, 3), SENTINEL, device=DEV)
    act[:, 0] = torch.as_tensor(np.asarray(actions, np.float32).reshape(-1), device=DEV)
    obs, final = torch.full((n, o + 3), SENTINEL, device=DEV), torch.full((n, o + 2), SENTINEL, device=DEV)
    rew = torch.full((n, 2), SENTINEL, device=DEV)
    flags = torch.full((3, n, 5), 77, dtype=torch.uint8, device=DEV)
    out = _lib.CEnvOut(obs.data_ptr(), o + 3, final.data_ptr(), o + 2, rew.data_ptr(), 2, flags[0].data_ptr(), 5, flags[1].data_ptr(), 5,
                       flags[2].data_ptr(), 5)
    env._call("sactd3_env_step", act.data_ptr(), 3, C.byref(out), env._stream())
    obs, final, rew, flags = host(obs), host(final), host(rew), host(flags)
    assert (obs[:, o:] == np.float32(SENTINEL)).all() and (final[:, o:] == np.float32(SENTINEL)).all() and (rew[:, 1:] == np.float32(SENTINEL)).all()
    assert (flags[:, :, 1:] == 77).all() and set(np.unique(flags[:, :, 0])) <= {0, 1}
    return {"obs": obs[:, :o], "final_obs": final[:, :o], "reward": rew[:, 0], "terminated": flags[0, :, 0], "truncated": flags[1, :, 0],
            "ended": flags[2, :, 0]}


# ------------------------------------------------------------------------------------------ 1. one step from planted states
@pytest.mark.parametrize("n", [1, 4, 257])
@pytest.mark.parametrize("name", KINDS)
def test_one_step_from_planted_states_against_the_float64_model(name, n):
    kind, seed = em.KINDS[name], 21
    env = new_env(name, n, seed=seed)
    env.reset(seed=seed)
    m = len(em.planted(kind)[1])
    rng = np.random.default_rng(n)
    worst, flags = 0.0, np.zeros(3, int)
    for offset in range(0, m if n < m else 1, n):                     # (1 and 4 envs: in rounds, until every planted state had its step)
        phys, steps, act = em.batch(kind, n, offset, rng)
        before = {"phys": phys, "steps": steps, "episode": (np.arange(n) % 3).astype(np.uint32), "returns": rng.standard_normal(n).astype(np.float32)}
        assert em.conditioned(kind, before, act).all()                  # no input within its bound of a threshold: the model alone says so
        env.set_state(before)
        assert all(same_bits(env.state()[k], before[k]) for k in before)
        got = step_wide(env, act)
        worst = max(worst, em.check_step(kind, seed, env.horizon, before, act, got, env.state()))
        flags += [int(got["terminated"].sum()), int(got["truncated"].sum()), int(got["ended"].sum())]
    print(f"{name} n={n}: worst |err| / bound {worst:.3f}; terminated, truncated, ended {flags}")
    assert 0.0 < worst <= 1.0
    assert flags[1] >= 1 and flags[2] == flags[0] + flags[1] and (flags[0] >= 4) == (name == "cartpole")


# ------------------------------------------------------------------------------------------ 2. resets and auto-resets
@pytest.mark.parametrize("name", KINDS)
def test_resets_and_auto_resets_are_the_philox_model_bit_for_bit(name):
    kind, seed, n = em.KINDS[name], 2 ** 35 + 17, 257
    big, small = new_env(name, n, seed=seed, horizon=3), new_env(name, 5, seed=seed, horizon=3)
    obs_b, obs_s = big.reset(seed=seed)[0], small.reset(seed=seed)[0]
    first = em.first_states(kind, seed, np.arange(n), np.zeros(n))
    assert same_bits(big.state()["phys"], first) and same_bits(small.state()["phys"], first[:5])
    want, wb = em.observe64(kind, first)
    assert (np.abs(host(obs_b) - want) <= wb).all() and same_bits(host(obs_b)[:5], host(obs_s))
    ended_seen = 0
    for t in range(7):                                                 # horizon 3: every env is cut twice
        before_b = big.state()
        act = big.action_space.sample()
        assert same_bits(host(act), em.random_actions(kind, seed, np.arange(n), before_b["draws"]))
        res_b, res_s = got_of(big.step(act)), got_of(small.step(act[:5].clone()))
        after = big.state()
        em.check_step(kind, seed, 3, before_b, host(act), res_b, after)      # obs = the reset state, final_obs = the one before it
        for k in res_b:
            assert same_bits(res_b[k][:5], res_s[k]), k                      # env i is the same whatever num_envs is
        ended = res_b["ended"].astype(bool)
        assert same_bits(after["phys"][ended], em.first_states(kind, seed, np.flatnonzero(ended), after["episode"][ended]))
        if ended.any():
            assert not np.array_equal(res_b["obs"][ended], res_b["final_obs"][ended])
        ended_seen += int(ended.sum())
    assert ended_seen >= 2 * n and (big.state()["episode"] >= 2).all()
    # another seed, other episodes; reset restarts the books
    big.reset(seed=seed + 1)
    assert not same_bits(big.state()["phys"], first)
    st = big.episode_stats()
    assert st["episodes"] == 0 and st["length_sum"] == 0 and not big.state()["draws"].any()


# ------------------------------------------------------------------------------------------ 3. 450 steps, each one checked singly
@pytest.mark.parametrize("name", KINDS)
def test_450_steps_each_from_the_devices_own_state(name):
    kind, seed, n, T = em.KINDS[name], 5, 5, 450
    env = new_env(name, n, seed=seed)
    env.reset(seed=seed)
    run, lens = np.zeros(n, np.float32), np.zeros(n, np.int32)
    returns, lengths = [[] for _ in range(n)], [[] for _ in range(n)]
    worst, log = 0.0, []
    for t in range(T):
        before = env.state()                                          # the device's own state: no drift accumulates
        act = env.action_space.sample()
        res = env.step(act)
        got, a = got_of(res), host(act)
        assert em.conditioned(kind, before, a).all(), t
        worst = max(worst, em.check_step(kind, seed, env.horizon, before, a, got, env.state()))
        log.append(got)
        run, lens = (run + got["reward"]).astype(np.float32), lens + 1          # fp32 accumulation of the device's own rewards
        for k in np.flatnonzero(got["ended"]):
            returns[k].append(run[k])
            lengths[k].append(lens[k])
            run[k], lens[k] = 0.0, 0
    st = env.episode_stats()
    print(f"{name}: worst |err| / bound over {T} steps {worst:.3f}; {st['episodes']} episodes")
    assert 0.0 < worst <= 1.0
    assert list(st["env_episodes"]) == [len(r) for r in returns] and min(len(r) for r in returns) >= 2
    assert same_bits(st["last_return"], np.array([r[-1] for r in returns], np.float32))              # bit for bit
    assert same_bits(st["last_length"], np.array([x[-1] for x in lengths], np.int32))
    assert same_bits(st["first_return"], np.array([r[0] for r in returns], np.float32))             # ... and each env's first episode
    assert same_bits(st["first_length"], np.array([x[0] for x in lengths], np.int32))
    assert st["length_sum"] == sum(int(x) for xs in lengths for x in xs) and st["bad_actions"] == 0
    assert st["return_sum"] == pytest.approx(sum(float(np.sum(np.float64(r))) for r in returns), rel=1e-12)
    assert same_bits(env.state()["returns"], run) and same_bits(env.state()["steps"], lens)
    if name == "pendulum":
        assert all(int(x) == 200 for xs in lengths for x in xs)
    else:
        assert max(int(x) for xs in lengths for x in xs) < 200                     # random pushes never balance it
    # a second env with the same seed, driven on another torch stream without a look at it in between: the same bits
    twin = new_env(name, n, seed=seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        twin.reset(seed=seed)
        outs = [twin.step(twin.action_space.sample()) for _ in range(T)]
        stacked = {"obs": torch.stack([r[0] for r in outs]), "reward": torch.stack([r[1] for r in outs]),
                   "terminated": torch.stack([r[2] for r in outs]), "truncated": torch.stack([r[3] for r in outs]),
                   "final_obs": torch.stack([r[4]["final_observation"] for r in outs])}
    side.synchronize()
    for k, v in stacked.items():
        assert same_bits(host(v), np.stack([g[k] for g in log])), k
    assert all(same_bits(twin.state()[k], env.state()[k]) for k in ("phys", "steps", "episode", "returns", "draws"))


# ------------------------------------------------------------------------------------------ 4. actions that are not numbers
@pytest.mark.parametrize("name", KINDS)
def test_nan_and_infinite_actions_are_counted_and_never_reach_the_state(name):
    kind, seed, n = em.KINDS[name], 3, 6
    env = new_env(name, n, seed=seed)
    env.reset(seed=seed)
    bad = np.array([[np.nan], [np.inf], [-np.inf], [0.25], [-np.nan], [3.4028235e38]], np.float32)      # (the last: FLT_MAX, finite)
    for t in range(3):
        before = env.state()
        got = got_of(env.step(torch.as_tensor(bad, device=DEV)))
        em.check_step(kind, seed, env.horizon, before, bad, got, env.state())        # the model steps them with 0 (FLT_MAX: clamped)
        assert np.isfinite(got["obs"]).all() and np.isfinite(got["reward"]).all() and np.isfinite(env.state()["phys"]).all()
    assert env.episode_stats()["bad_actions"] == 3 * 4                                # every finite float is an action: not counted
    twin = envs.HostVecEnv(name, n, seed=seed)                                        # the host twin counts the same ones
    twin.reset(seed=seed)
    for t in range(3):
        twin.step(bad)
    assert twin.episode_stats()["bad_actions"] == 3 * 4 and same_bits(twin.state()["steps"], env.state()["steps"])
    # and the errors of the calls themselves
    with pytest.raises(P.EngineError, match="act_ld"):
        env._call("sactd3_env_sample_actions", torch.zeros(n, device=DEV).data_ptr(), 0, env._stream())
    with pytest.raises(ValueError):
        env.set_state({"phys": np.full((n, 4), np.inf, np.float32)})
    with pytest.raises(P.EngineError, match="obs"):
        env._call("sactd3_env_step", torch.zeros(n, 1, device=DEV).data_ptr(), 1, C.byref(_lib.CEnvOut()), env._stream())


# ------------------------------------------------------------------------------------------ 5. through the loop into the ring
def sac_cfg(name, seed, budget, max_envs=None):
    """launcher.DEFAULTS["sac"] sized by a budget of profiles/native_env.json (tools/native_env_probe.py: learning_cfg)"""
    steps = budget["learning_starts"] + budget["updates"] * budget["num_envs"]
    return P.launcher.job_config("sac", name, seed, num_envs=max_envs or budget["num_envs"], learning_starts=budget["learning_starts"],
                                 batch_size=budget["batch_size"], num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)


def new_agent(name, cfg, seed):
    o, a, bound = envs.SPECS[envs.kind_of(name)][:3]
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    return agent


@pytest.mark.parametrize("name", KINDS)
def test_the_ring_holds_what_the_env_emitted(name):
    n, seed, T = 4, 8, 60
    horizon = 7 if name == "pendulum" else 30
    cfg = sac_cfg(name, seed, dict(num_envs=n, learning_starts=10 ** 6, updates=0, batch_size=64))
    agent, env = new_agent(name, cfg, seed), new_env(name, n, seed=seed, horizon=horizon)
    emitted, step = [], env.step

    def spy(actions):
        res = step(actions)
        emitted.append((actions, res))
        return res
    env.step = spy
    ro = loop.DeviceRollout(env, agent, seed, cfg.learning_starts, 1)
    held = [ro.obs]
    for _ in range(T):
        ro.choose()
        ro.advance()
        held.append(ro.obs)
    rows = agent.rb.rows(np.arange(T * n))
    rows = {k: host(v) for k, v in rows.items()}
    term = np.concatenate([host(r[2]) for _, r in emitted])
    trunc = np.concatenate([host(r[3]) for _, r in emitted])
    obs = np.concatenate([host(x) for x in held[:-1]])
    arrived = np.concatenate([host(r[0]) for _, r in emitted])
    final = np.concatenate([host(r[4]["final_observation"]) for _, r in emitted])
    assert term.sum() >= (1 if name == "cartpole" else 0) and trunc.sum() >= (n if name == "pendulum" else 0) and (term | trunc).sum() >= n
    assert same_bits(rows["observations"], obs)
    assert same_bits(rows["actions"], np.concatenate([host(a) for a, _ in emitted]))
    assert same_bits(rows["rewards"].reshape(-1), np.concatenate([host(r[1]) for _, r in emitted]))
    assert same_bits(rows["next_observations"], np.where(trunc[:, None], final, arrived))      # the true last observation where time ran out
    assert same_bits(rows["next_observations"][trunc], final[trunc]) and same_bits(rows["next_observations"][term], arrived[term])
    assert np.array_equal(rows["dones"].reshape(-1).astype(bool), term)                        # the terminations only
    assert len({x.data_ptr() for x in held}) == len(held)                                      # no buffer was handed out twice while held


# ------------------------------------------------------------------------------------------ 6. beside a training engine
def test_an_engine_trains_the_same_bits_with_an_env_stepping_beside_it():
    N = 12
    _, (A, B), (o, a, bound) = build_engines("sac", DIMS["hopper"], 64, count=2, seed=4, cap=2048)
    data = synth_transitions(1024, o, a, bound, seed=6)
    for e in (A, B):
        e.rb_extend(*[t.numpy() for t in data])
    env = new_env("cartpole", 257, seed=1)
    env.reset(seed=1)
    for i in range(N):
        A.step(i % 3 == 0)
        B.step(i % 3 == 0)
        for _ in range(3):
            env.step(env.action_space.sample())                       # on torch's stream, while B's iteration runs on the engine's
    torch.cuda.synchronize()
    assert_same_state(A, B, "slot", "noise")
    assert env.episode_stats()["length_sum"] + int(env.state()["steps"].sum()) == 3 * N * 257


# ------------------------------------------------------------------------------------------ 7. learned end to end
def learning_record():
    with open(os.path.join(ROOT, "profiles", "native_env.json")) as f:
        return json.load(f)["learning"]


@pytest.mark.parametrize("name", KINDS)
def test_sac_learns_the_task_on_the_device(name):
    """SAC, default hyper-parameters, loop.train(device_env=True) on 4 envs for the recorded budget, then the greedy return over 16
    envs for one horizon.  The bar is not this engine's: the oracle agent on the host twin, 3 seeds at the same budget
    (profiles/native_env.json: per-seed untrained and trained returns), bar = the midpoint between its worst trained and its best
    untrained seed, and the test is kept only because every oracle seed clears that bar by a quarter of the gap."""
    rec = learning_record()
    task = rec["tasks"][name]
    assert task["test_kept"] and all(r["trained"] - task["bar"] >= task["margin_needed"] for r in task["seeds"])
    seed, episodes = 0, rec["episodes"]
    cfg = sac_cfg(name, seed, task["budget"])
    agent = new_agent(name, sac_cfg(name, seed, task["budget"], max_envs=episodes), seed)      # (max_envs: the evaluation's 16 rows in one call)
    eval_env = new_env(name, episodes, seed=seed + rec["eval_seed_offset"])
    before = envs.greedy_returns(eval_env, agent, episodes)
    env = new_env(name, cfg.num_envs, seed=seed)
    loop.train(cfg, env, agent, device_env=True)
    after = envs.greedy_returns(eval_env, agent, episodes)
    print(f"{name}: greedy return {before['return']:.1f} -> {after['return']:.1f} after {agent.qnet_updates_so_far} updates; bar {task['bar']:.1f}")
    assert agent.qnet_updates_so_far == task["budget"]["updates"] and agent.engine.predict_device_stats()["calls"] > 0
    assert env.episode_stats()["bad_actions"] == 0 and after["bad_actions"] == 0
    assert before["return"] < task["bar"] < after["return"], (before["return"], after["return"], task["bar"])


# ------------------------------------------------------------------------------------------ 8. evaluation on the device, and the launcher's job
@pytest.mark.parametrize("name", KINDS)
def test_greedy_returns_in_chunks_of_max_envs_equal_one_call(name):
    """10 evaluation envs on an engine whose max_envs is 4 (the launcher's defaults): three predict_device calls per step into slices
    of one tensor -- the same bits as one call on an engine with room for all ten, and one episode per env: its first"""
    seed, n = 2, 10
    budget = dict(num_envs=4, learning_starts=10 ** 6, updates=0, batch_size=64)
    small, wide = new_agent(name, sac_cfg(name, seed, budget), seed), new_agent(name, sac_cfg(name, seed, budget, max_envs=n), seed)
    assert small.engine.cfg.max_envs == 4 and wide.engine.cfg.max_envs == n
    env = new_env(name, n, seed=seed)
    a, calls = envs.greedy_returns(env, small, n), small.engine.predict_device_stats()["calls"]
    books = env.episode_stats()
    b = envs.greedy_returns(env, wide, n)
    assert calls == 3 * env.horizon and wide.engine.predict_device_stats()["calls"] == env.horizon
    assert same_bits(a["returns"], b["returns"]) and same_bits(a["lengths"], b["lengths"]) and a["return"] == b["return"]
    assert same_bits(a["returns"], books["first_return"]) and a["episodes"] == n and (a["lengths"] >= 1).all()
    if name == "cartpole":                                           # the untrained policy drops the pole: further episodes are not counted
        assert books["episodes"] > n and not same_bits(books["first_return"], books["last_return"])
        assert a["return"] == float(books["first_length"].astype(np.float64).mean())
    gen = envs.device_episodes(env, small, seed)
    eps = [next(gen) for _ in range(n + 1)]                          # one window and the first episode of the next
    assert all(set(e) == {"length", "return"} and 1 <= float(e["length"]) <= env.horizon for e in eps)


def test_the_launchers_job_on_a_native_id_stays_on_the_device(tmp_path, monkeypatch):
    """launcher.run_job("CartPole-native", device_env=True): training through DeviceRollout on NativeVecEnv and every evaluation through
    envs.device_episodes -- no host env is built or stepped"""
    def no_host_env(*a, **k):
        raise AssertionError("a host env was built in a job that stays on the device")
    monkeypatch.setattr(envs, "HostVecEnv", no_host_env)
    out = P.launcher.run_job("sac", "CartPole-native", 0, 0, tmp_path, device_env=True, num_timesteps=1600, learning_starts=400, eval_every=800,
                             eval_steps=10, batch_size=64, rb_capacity=4096)
    rows = [json.loads(ln) for ln in open(os.path.join(out["dir"], "progress.json"))]
    assert out["gradient_steps"] == 301 and [r["timestep"] for r in rows] == [800, 1600]
    assert all(1.0 <= r["length"] <= 200.0 and r["return"] == r["length"] for r in rows)      # the cart-pole pays 1 per step
    assert np.isfinite(out["best_eval_return"]) and all(np.isfinite(v) for v in out["final_metrics"].values())
