"""GPU: the rollout cycle (include/sactd3_rollout_cycle.h, csrc/rollout_cycle.hip: k_rb_ingest_g, loop.NativeRollout.cycle,
loop.train(fused_rollout=True)) against the three calls it stands for -- sactd3_rollout_advance, sactd3_rollout_choose, sactd3_step --
on twins: the same bits in every buffer after every cycle, and in the engines, the rings, the envs' books and the counters at the end;
across the ring's wrap point, with a slab of several blocks, replayed without a recapture, interleaved with other calls, without graphs,
through its refusals, and through the training loop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.gpu_support import (DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, loop, same_bits, track)  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
envs = P.envs
EXPLORE, EXPLOIT = _lib.ROLLOUT_EXPLORE, _lib.ROLLOUT_EXPLOIT
STATE = ("slot", "noise")                                                 # engine_state parts compared wherever twins are compared


def host(x):
    return x.cpu().numpy()


def dims_of(name):
    return envs.SPECS[envs.kind_of(name)][:3]


def twins(algo, name, n, cap, B=64, use_graphs=(True, True), horizon=None, seed=4, **hp):
    """two engines with the same parameters, each with a ring, an env and a NativeRollout bound to both (closed before them); the
    rollouts open with the same random action"""
    _, engs, _ = build_engines(algo, dims_of(name), B, seed=seed, cap=cap, max_envs=n, use_graphs=use_graphs, **hp)
    out = []
    for e in engs:
        rb = P.ReplayBuffer(cap)
        rb._bind(e)
        agent = SimpleNamespace(engine=e, rb=rb, timesteps_so_far=0, qnet_updates_so_far=0, actor_updates_so_far=0)
        env = track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=horizon))
        ro = track(loop.NativeRollout(env, agent, seed, 0, 1))            # (tracked last: closed first)
        assert e.lib.sactd3_rollout_choose(ro._h, _lib.ROLLOUT_RANDOM) == 0
        out.append(SimpleNamespace(eng=e, rb=rb, agent=agent, env=env, ro=ro, lib=e.lib))
    return out


def period_of(t):
    return t.eng.cfg.actor_update_delay + 1


def three_calls(t, i, mode=EXPLORE):
    """what a cycle stands for, with the counters Agent.iteration keeps"""
    do_actor = i % period_of(t) == 0
    t.ro.advance()
    t.ro._ck(t.lib.sactd3_rollout_choose(t.ro._h, mode))
    t.eng.step(do_actor)
    t.agent.qnet_updates_so_far += 1
    t.agent.actor_updates_so_far += t.eng.cfg.actor_update_delay if do_actor else 0


def cycle(t, i, mode=EXPLORE):
    if mode == EXPLORE:
        t.ro.cycle(i)
        return
    do_actor = i % period_of(t) == 0
    t.ro._ck(t.lib.sactd3_rollout_cycle(t.ro._h, mode, int(do_actor)))
    t.ro.steps += 1
    t.agent.qnet_updates_so_far += 1
    t.agent.actor_updates_so_far += t.eng.cfg.actor_update_delay if do_actor else 0


def buffers(t):
    return {"obs": host(t.ro.obs), "actions": host(t.ro.actions), "records": host(t.ro.records)}


def same_buffers(a, b):
    x, y = buffers(a), buffers(b)
    return all(same_bits(x[k], y[k]) for k in x)


def env_books(env):
    st, books = env.state(), env.episode_stats()
    return {**{"state." + k: v for k, v in st.items()}, **{"books." + k: np.asarray(v) for k, v in books.items()}}


def ring_of(rb):
    return {k: host(v) for k, v in rb.rows(np.arange(len(rb))).items()} if len(rb) else {}


def same_maps(x, y):
    return list(x) == list(y) and all(same_bits(x[k], y[k]) for k in x)


def outside_of(t):
    """what the ring, the env and the rollout hold, beside the engine's own state"""
    return {"ring": ring_of(t.rb), "len": len(t.rb), "books": env_books(t.env), "rollout": t.ro.stats(), "buffers": buffers(t)}


def assert_twins_equal(a, b, what=""):
    """everything the header's equivalence names: buffers, engines (parameters, Adam state, metrics, the batch slot, the critic site's
    draws), every ring row, the envs' state and books, the rollouts' stats, the acting route's counters and draws, the host counters"""
    assert same_buffers(a, b), what
    assert_same_state(a.eng, b.eng, *STATE, what=what)
    assert len(a.rb) == len(b.rb) and same_maps(ring_of(a.rb), ring_of(b.rb)), what
    assert same_maps(env_books(a.env), env_books(b.env)), what
    assert a.ro.stats() == b.ro.stats() and a.ro.steps == b.ro.steps, what
    assert a.eng.predict_device_stats() == b.eng.predict_device_stats(), what
    assert same_bits(a.eng.read_noise(_lib.SITE_PREDICT), b.eng.read_noise(_lib.SITE_PREDICT)), what
    assert a.eng.batch_generation() == b.eng.batch_generation(), what
    assert (a.agent.qnet_updates_so_far, a.agent.actor_updates_so_far) == (b.agent.qnet_updates_so_far, b.agent.actor_updates_so_far), what
    assert b.ro.cycle_stats()["clamped"] == 0, what


def assert_counters_equal(a, b, i):
    """the sample, predict and noise counters live on the device: one more body in the CALL form on both twins draws from all three
    streams -- a counter that differed would give another sample, another exploring action, other critic noise -- and engine_state's
    "ring" part reads every ring row through the batch slot"""
    three_calls(a, i)
    three_calls(b, i)
    assert_twins_equal(a, b, "the body behind the run")
    assert_same_state(a.eng, b.eng, "ring", what="every ring row")


def run_pair(a, b, cycles, first=0, every_cycle=True):
    for i in range(first, first + cycles):
        three_calls(a, i)
        cycle(b, i)
        if every_cycle:
            assert same_buffers(a, b), i


def schedules(t, first, count):
    """the distinct (actor updates run, targets updated) of iterations first .. first + count - 1, the critics' update count starting at `first`"""
    cfg = t.eng.cfg
    td3 = bool(cfg.prefer_td3_over_sac)
    return {(i % period_of(t) == 0 and cfg.actor_update_delay > 0, td3 or (i + 1) % cfg.crit_targ_update_freq == 0) for i in range(first, first + count)}


# ------------------------------------------------------------------------------------------ 1. + 3. the cycle is the three calls; replayed
@pytest.mark.parametrize("name", ["pendulum", "pointgoal"])
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_cycle_equals_the_three_calls(algo, name):
    """4 envs into a ring of 42 rows: the slab of cycle 11 goes to the slots 40, 41, 0, 1.  actor_update_delay 2 and, for SAC,
    crit_targ_update_freq 2: all four schedules occur.  60 cycles: every env's episode ends (the pendulum's horizon is set to 25, the
    goal task's is its own 50) and is reset inside the graph."""
    n, cap, cycles = 4, 42, 60
    hp = dict(actor_update_delay=2, **(dict(crit_targ_update_freq=2) if algo == "sac" else {}))
    a, b = twins(algo, name, n, cap, horizon=25 if name == "pendulum" else None, **hp)
    assert cap % n == 2 and tuple(dims_of(name)[:2]) == ((3, 1) if name == "pendulum" else (6, 2))
    run_pair(a, b, cycles)
    books = b.env.episode_stats()
    assert books["episodes"] >= n and (np.asarray(books["env_episodes"]) >= 1).all()      # every env ended an episode and went on
    assert len(b.rb) == cap and b.ro.stats() == dict(random_choices=1, policy_choices=cycles, steps=cycles, rows_appended=cycles * n)
    assert_twins_equal(a, b)
    # 3. replayed, not recaptured
    kinds = schedules(b, 0, cycles)
    assert len(kinds) == (4 if algo == "sac" else 2)
    st = b.ro.cycle_stats()
    assert st["cycles"] == cycles and st["graphs_captured"] == len(kinds) and st["eager_cycles"] == 0 and st["graph_nodes"] > 6
    assert a.ro.cycle_stats() == dict(cycles=0, graphs_captured=0, graph_nodes=0, eager_cycles=0, clamped=0)
    run_pair(a, b, 30, first=cycles, every_cycle=False)
    st = b.ro.cycle_stats()
    assert st["cycles"] == cycles + 30 and st["graphs_captured"] == len(kinds)
    assert_twins_equal(a, b, "second pass")
    assert_counters_equal(a, b, cycles + 30)
    # fewer events, and nothing else: the sequence orders the rollout's stream twice per body, the cycle once
    assert a.eng.boundary_stats()["ordered_calls"] - b.eng.boundary_stats()["ordered_calls"] == cycles + 30


# ------------------------------------------------------------------------------------------ 2. several blocks
def test_a_slab_of_several_blocks_and_a_multi_block_acting_tail():
    """512 envs: the acting tail is several blocks (its counter launch is a node of the graph), and the slab is 512 x 4 float4 chunks,
    8 blocks of the append -- which then publishes through the launch behind it.  The ring holds 2.5 slabs and 2 rows: the third
    slab goes across the wrap point."""
    n = 512
    cap = 2 * n + n // 2 + 2
    a, b = twins("sac", "pendulum", n, cap, horizon=4, actor_update_delay=2)
    assert b.eng.rb_layout()["record_floats"] // 4 * n > 256                                 # more chunks than one block of the append holds
    run_pair(a, b, 6)
    assert b.eng.predict_device_stats()["multi_block_tails"] == 6 and len(b.rb) == cap
    assert b.env.episode_stats()["episodes"] >= n
    assert_twins_equal(a, b)
    assert b.ro.cycle_stats()["graphs_captured"] == len(schedules(b, 0, 6))
    assert_counters_equal(a, b, 6)


# ------------------------------------------------------------------------------------------ 4. interleaving
def test_cycles_between_other_calls():
    n, cap = 4, 150
    a, b = twins("sac", "pendulum", n, cap, horizon=9, actor_update_delay=2)
    o, ac, bound = dims_of("pendulum")
    outside = [t.numpy() for t in synth_transitions(10, o, ac, bound, seed=8)]
    perturbed = a.eng.get_params(_lib.ACTOR) * np.float32(1.03125)
    obs = np.linspace(-1.0, 1.0, 3 * o, dtype=np.float32).reshape(3, o)
    i = 0
    seen, kinds = [], set()      # kinds: (mode, actor updates run) of every cycle -- the targets are updated in every iteration here

    def both(fn):
        got = [fn(t) for t in (a, b)]
        if got[0] is not None:
            assert same_bits(got[0], got[1])

    def run_period(t, i0):
        t.eng.run_iterations(i0, period_of(t))
        t.agent.qnet_updates_so_far += period_of(t)
        t.agent.actor_updates_so_far += t.eng.cfg.actor_update_delay

    between = [lambda t: three_calls(t, i), lambda t: t.eng.rb_extend(*outside), lambda t: t.eng.set_params(_lib.ACTOR, perturbed),
               lambda t: t.eng.predict(obs, True), lambda t: run_period(t, i), None]
    for lap in range(3):
        for k, other in enumerate(between):
            for _ in range(2):                                            # two cycles, then something else
                three_calls(a, i)
                cycle(b, i)
                kinds.add((EXPLORE, i % period_of(b) == 0))
                i += 1
                assert same_buffers(a, b), (lap, k)
            if other is None:                                             # the cycle with the greedy action
                three_calls(a, i, EXPLOIT)
                cycle(b, i, EXPLOIT)
                seen.append((EXPLOIT, i))
                kinds.add((EXPLOIT, i % period_of(b) == 0))
                i += 1
            else:
                both(other)
                i += {0: 1, 4: period_of(a)}.get(k, 0)
            assert same_buffers(a, b), (lap, k)
    assert_twins_equal(a, b)
    st = b.ro.cycle_stats()
    assert st["cycles"] == 3 * (2 * len(between) + 1) and len(seen) == 3
    assert st["graphs_captured"] == len(kinds) and (EXPLORE, True) in kinds and (EXPLORE, False) in kinds and len(b.rb) == cap
    captured = st["graphs_captured"]                                      # no capture beyond the first of each kind
    for _ in range(2 * period_of(b)):                                     # every schedule of the exploring cycle has been used: nothing new
        three_calls(a, i)
        cycle(b, i)
        i += 1
    assert b.ro.cycle_stats()["graphs_captured"] == captured
    assert_counters_equal(a, b, i)


# ------------------------------------------------------------------------------------------ 5. without graphs
def test_the_eager_cycle_is_the_graph_cycle():
    a, b = twins("td3", "pointgoal", 4, 42, use_graphs=(True, False), actor_update_delay=2)
    for i in range(12):
        cycle(a, i)
        cycle(b, i)
        assert same_buffers(a, b), i
    assert_twins_equal(a, b)
    sa, sb = a.ro.cycle_stats(), b.ro.cycle_stats()
    assert (sa["cycles"], sa["eager_cycles"], sa["graphs_captured"]) == (12, 0, 2) and sa["graph_nodes"] > 6
    assert (sb["cycles"], sb["eager_cycles"], sb["graphs_captured"], sb["graph_nodes"]) == (12, 12, 0, 0)
    assert_counters_equal(a, b, 12)


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing():
    n = 4
    (t, big) = twins("sac", "pendulum", n, 64, actor_update_delay=2)
    _, (small,), _ = build_engines("sac", dims_of("pendulum"), 64, seed=4, cap=2, max_envs=n)      # a ring that does not hold one slab
    small_rb = P.ReplayBuffer(2)
    small_rb._bind(small)
    narrow = track(loop.NativeRollout(track(envs.NativeVecEnv("pendulum", n, seed=4, device=DEV)),
                                      SimpleNamespace(engine=small, rb=small_rb, timesteps_so_far=0), 4, 0, 1))
    for i in range(5):
        cycle(t, i)
    lib = t.lib

    def snapshot(x):
        """(a read-out orders streams and counts in boundary_stats: those counters are taken in front of the reads and behind them)"""
        torch.cuda.synchronize()
        x.eng.sync()
        first = x.eng.boundary_stats()
        return engine_state(x.eng, *STATE), outside_of(x), x.ro.cycle_stats(), x.eng.predict_device_stats(), first, x.eng.boundary_stats()

    def refused(x, call, code, word):
        before = snapshot(x)
        assert call() == code
        assert word in lib.sactd3_rollout_last_error(x.ro._h).decode()
        after = snapshot(x)
        assert_same_state(before[0], after[0], what=word)
        for k in before[1]:
            u, v = before[1][k], after[1][k]
            assert (same_maps(u, v) if isinstance(u, dict) and k != "rollout" else u == v), (word, k)
        assert before[2:4] == after[2:4], word
        assert before[5] == after[4], word                               # no event was recorded, no call counted

    assert lib.sactd3_rollout_cycle(None, EXPLORE, 1) == _lib.EINVAL
    for mode in (_lib.ROLLOUT_RANDOM, _lib.ROLLOUT_REPEAT, 4, -1):
        refused(t, lambda: lib.sactd3_rollout_cycle(t.ro._h, mode, 1), _lib.EINVAL, "mode")
    before, state = len(small_rb), engine_state(small, *STATE)
    assert lib.sactd3_rollout_cycle(narrow._h, EXPLORE, 1) == _lib.EINVAL and b"rb_capacity" in lib.sactd3_rollout_last_error(narrow._h)
    assert len(small_rb) == before == 0 and narrow.stats()["steps"] == 0 and narrow.cycle_stats()["cycles"] == 0
    assert_same_state(state, engine_state(small, *STATE), what="rb_capacity")
    # an acting call in flight
    t.eng.predict_begin(np.zeros((1, 3), np.float32), True)
    refused(t, lambda: lib.sactd3_rollout_cycle(t.ro._h, EXPLORE, 0), _lib.ESTATE, "in flight")
    t.eng.predict_end()
    cycle(t, 5)                                                           # a normal cycle succeeds behind them
    assert t.ro.cycle_stats()["cycles"] == 6 and t.ro.stats()["steps"] == 6
    # engine-owned priorities, then pinned rows, on the other twin (neither can be taken back)
    for i in range(3):
        cycle(big, i)
    big.rb.enable_priorities()
    refused(big, lambda: lib.sactd3_rollout_cycle(big.ro._h, EXPLORE, 1), _lib.ESTATE, "priorities")
    three_calls(big, 3)                                                   # the call sequence serves them
    assert big.ro.stats()["steps"] == 4
    pinned, _ = twins("sac", "pendulum", n, 64, actor_update_delay=2)[:2]
    for i in range(2):
        cycle(pinned, i)
    pinned.rb.pin()
    refused(pinned, lambda: lib.sactd3_rollout_cycle(pinned.ro._h, EXPLORE, 1), _lib.ESTATE, "pinned")
    three_calls(pinned, 2)
    assert len(pinned.rb) == 3 * n


def test_a_second_rollout_takes_the_graphs_over():
    """the graphs hold the binding's buffers: a cycle of another rollout of the same engine drops them and captures its own"""
    a, b = twins("sac", "pendulum", 4, 42, actor_update_delay=2)
    env2 = track(envs.NativeVecEnv("pendulum", 4, seed=4, device=DEV))
    second = track(loop.NativeRollout(env2, b.agent, 4, 0, 1))
    for i in range(3):
        three_calls(a, i)
        cycle(b, i)
    first = b.ro
    b.ro = second                                                         # the same engine, ring and agent; other buffers, another env
    held = buffers(SimpleNamespace(ro=first))
    a2 = SimpleNamespace(**{**vars(a), "ro": track(loop.NativeRollout(track(envs.NativeVecEnv("pendulum", 4, seed=4, device=DEV)), a.agent, 4, 0, 1))})
    for i in range(3, 7):
        three_calls(a2, i)
        cycle(b, i)
        assert same_buffers(a2, b), i
    assert same_maps(held, buffers(SimpleNamespace(ro=first)))            # the first binding's buffers were not written again
    assert second.cycle_stats()["graphs_captured"] >= 1 and first.cycle_stats()["cycles"] == 3
    assert_same_state(a.eng, b.eng, *STATE)
    assert len(a.rb) == len(b.rb) and same_maps(ring_of(a.rb), ring_of(b.rb))


# ------------------------------------------------------------------------------------------ 7. the loop
def new_agent(name, cfg, seed):
    o, a, bound = dims_of(name)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    return agent


@pytest.mark.parametrize("updates_per_step", [1, 2])
def test_training_with_the_fused_rollout_is_training_with_the_native_rollout(updates_per_step, monkeypatch):
    n, seed = 4, 3
    cfg = P.launcher.job_config("sac", "Pendulum-native", seed, num_envs=n, learning_starts=40, batch_size=64, num_timesteps=400, eval_every=100,
                                rb_capacity=300)
    runs, cycles = [], []
    plain_close = loop.NativeRollout.close

    def recording_close(self):                                            # train() closes the rollout it made: its counters are read here
        if getattr(self, "_h", None):
            cycles.append(self.cycle_stats())
        plain_close(self)
    monkeypatch.setattr(loop.NativeRollout, "close", recording_close)
    for fused_rollout in (True, False):
        agent, env = new_agent("pendulum", cfg, seed), track(envs.NativeVecEnv("pendulum", n, seed=seed, device=DEV, horizon=25))
        seen = []
        on_eval = lambda ag, count: seen.append((count, ag.qnet_updates_so_far, dict(ag.engine.read_metrics())))
        out = loop.train(cfg, env, agent, device_env=True, native_rollout=True, fused_rollout=fused_rollout, on_eval=on_eval,
                         updates_per_step=updates_per_step)
        runs.append(SimpleNamespace(agent=agent, env=env, out=out, seen=seen))
    f, p = runs
    assert cycles and cycles[0]["cycles"] == (400 - 40) // n + 1 and cycles[0]["clamped"] == 0      # every body from step count 40 on
    assert f.out == p.out and f.seen == p.seen and [c for c, _, _ in f.seen] == [100, 200, 300, 400]
    for name in ("timesteps_so_far", "qnet_updates_so_far", "actor_updates_so_far"):
        assert getattr(f.agent, name) == getattr(p.agent, name), name
    assert f.agent.qnet_updates_so_far == updates_per_step * ((404 - 40) // n)
    assert f.agent.engine.predict_device_stats() == p.agent.engine.predict_device_stats()
    assert len(f.agent.rb) == len(p.agent.rb) == 300 and same_maps(ring_of(f.agent.rb), ring_of(p.agent.rb))
    assert same_maps(env_books(f.env), env_books(p.env))
    assert_same_state(f.agent.engine, p.agent.engine, "slot", "noise", "ring")
