"""GPU: the hindsight iteration as one graph launch (include/sactd3.h: sactd3_step_sampled with SACTD3_DRAW_HINDSIGHT; device code:
k_hindsight_draw_g, k_hindsight_stage_g of the hindsight translation unit) against the call sequence
sactd3_rb_sample_hindsight -> sactd3_update_qnets -> [sactd3_update_actor x delay] -> sactd3_update_targ_nets, bit for bit, and, on its
own, against the numpy restatements (tests/hindsight_ref.py on the slots of tests/mix_ref.py).

Shapes (o, a, B) from tests/test_gpu_hindsight.py: (6, 2, 8) one partial block; (6, 2, 260) rows straddle blocks; (376, 17, 16) the
per-block span is cut to fit the LDS tables.  Rings of 96 and 101 slots at stride 4 that hold 20 vector steps and receive one more in
front of each of 7 iterations: the ring grows, fills and wraps under the captured graphs.  tests/test_hindsight_one_launch_host.py
asserts, without a GPU, that this schedule meets every rule of the staging kernel."""
import functools

import numpy as np
import pytest
import torch

from tests import hindsight_ref as hr
from tests import mix_ref
from tests.gpu_support import (DEV, P, _lib, assert_same_bits, assert_same_state, build_engines, call_sequence, close_engines,  # noqa: F401
                               engine_state, iteration_state, loop, raw_step, same_bits, stream, track)

pytestmark = pytest.mark.gpu
envs = P.envs
F = np.float32
SENT = -77
# (restated in tests/test_hindsight_one_launch_host.py: no test module imports another)
STRIDE, SEED, HELD_STEPS, ITERS = 4, 3, 20, 7
# name -> (o, a, B, achieved, desired, dim, horizon of its episodes, window)
CASES = {"goal-8": (6, 2, 8, 0, 4, 2, 9, 9), "goal-260": (6, 2, 260, 0, 4, 2, 9, 9), "long-16": (376, 17, 16, 1, 200, 3, 5, 5)}
RUNS = [("goal-8", 96, "sac"), ("goal-260", 101, "td3"), ("long-16", 96, "sac"), ("goal-260", 96, "sac")]
RATIO = 0.8
ROW_SEED = 9                                                              # of the synthetic episodes: every second one ends by termination
E, S, H = _lib.EINVAL, _lib.ESTATE, _lib.DRAW_HINDSIGHT


def last_error(eng):
    return eng.lib.sactd3_last_error(eng._h).decode()


@functools.lru_cache(maxsize=None)
def rows_of(case):
    """HELD_STEPS + ITERS vector steps in append order: computed once, never written"""
    o, a, B, ag, dg, G, horizon, _ = CASES[case]
    return hr.synthetic_ring(o, a, STRIDE, HELD_STEPS + ITERS, horizon, seed=ROW_SEED, term_every=2, achieved=ag, dim=G)


def config(case, ratio=RATIO, window=None):
    o, a, B, ag, dg, G, _, w = CASES[case]
    return dict(achieved=ag, desired=dg, dim=G, threshold=0.1, ratio=ratio, window=window or w, stride=STRIDE)


@functools.lru_cache(maxsize=None)
def expected(case, cap, i, ratio=RATIO, window=None):
    """the slot iteration i must leave: the ring after HELD_STEPS + i + 1 vector steps, the uniform draw at sample counter i, the
    relabelling draw at hindsight counter i"""
    rows, _ = rows_of(case)
    n = (HELD_STEPS + i + 1) * STRIDE
    fields, geom, held = hr.place({k: v[:n] for k, v in rows.items()}, cap)
    idx = mix_ref.mixed_indices(SEED, i, CASES[case][2], 0, 0, geom["length"])
    return hr.stage(fields, geom, idx, config(case, ratio, window), seed=SEED, hctr=i)


def append(eng, case, lo, hi):
    """vector steps [lo, hi) of the case's rows"""
    rows, _ = rows_of(case)
    five = [rows[k] for k in ("obs", "act", "rew", "nobs")] + [rows["done"] != 0]
    eng.rb_extend(*[f[lo * STRIDE:hi * STRIDE] for f in five])


def engines(case, cap, algo, count=2, use_graphs=True, fill=True, configure=True):
    o, a, B = CASES[case][:3]
    _, engs, _ = build_engines(algo, (o, a, 1.0), B, count=count, seed=SEED, cap=cap, max_envs=STRIDE, use_graphs=use_graphs)
    for e in engs:
        if fill:
            append(e, case, 0, HELD_STEPS)
        if configure:
            e.hindsight_configure(**config(case))
    return engs


def read_slot(eng, o, a):
    """batch slot 0 as hr.stage states it, the padded rows included; a sentinel on either side of the info arrays must survive"""
    B = eng.cfg.batch_size
    cx4, cn4 = -(-(o + a) // 4) * 4, -(-o // 4) * 4
    X = eng.debug_read("X").reshape(B, -1)[:, :cx4]
    Xn = eng.debug_read("Xn").reshape(B, -1)[:, :cn4]
    off = torch.full((B + 2,), SENT, dtype=torch.int32, device=DEV)
    gs = torch.full((B + 2,), SENT, dtype=torch.int32, device=DEV)
    eng.hindsight_info_device(off[1:].data_ptr(), 1, gs[1:].data_ptr(), 1, stream())
    off, gs = off.cpu().numpy(), gs.cpu().numpy()
    assert off[0] == off[-1] == gs[0] == gs[-1] == SENT
    return dict(X=X, Xn=Xn, obs=X[:, :o], act=X[:, o:o + a], nobs=Xn[:, :o], rew=eng.debug_read("rew")[:B], done=eng.debug_read("done")[:B],
                slot_idx=eng.read_batch()["index"].astype(np.int32), offset=off[1:-1], goal_slot=gs[1:-1])


# behind a critic update Xn's columns from o on hold the next action, no longer the record's pad: the staged s' is "nobs"
ALL_KEYS = hr.KEYS + ("X",)
sample_hindsight = lambda e: e.rb_sample_hindsight()


def iteration_pair(A, Bt, u, what):
    """iteration u (0-based) on both: A call by call, Bt as one launch; the slot, the TD errors and the metrics agree afterwards"""
    call_sequence(A, u % 3 == 0, sample_hindsight, u + 1)
    Bt.step_sampled(u % 3 == 0, hindsight=True)
    assert_same_bits(iteration_state(A), iteration_state(Bt), what=what)


# ------------------------------------------------------------------------------------------ 1. one launch equals the call sequence
@pytest.mark.parametrize("case,cap,algo", RUNS)
def test_one_launch_equals_the_call_sequence(case, cap, algo):
    """7 iterations, one vector step appended in front of each: after every iteration the slot with its ring indices, the TD errors, the
    metrics and the per-row offsets and goal slots, against twin A and against the restatement; at the end every parameter set, the Adam
    state, the noise, the ring, the counters and one further uniform sample.  Two graph captures, whatever moved."""
    o, a, B = CASES[case][:3]
    A, Bt, M = engines(case, cap, algo, count=3)
    for i in range(ITERS):
        for eng in (A, Bt):
            append(eng, case, HELD_STEPS + i, HELD_STEPS + i + 1)
        iteration_pair(A, Bt, i, f"iteration {i}")
        got_a, got_b = read_slot(A, o, a), read_slot(Bt, o, a)
        assert_same_bits(got_a, got_b, what=f"slot and info of iteration {i}")
        hr.check(expected(case, cap, i), got_b, ALL_KEYS)
    assert A.rb_len() == Bt.rb_len() == cap
    assert A.hindsight_stats() == Bt.hindsight_stats() and Bt.hindsight_stats()["native_draws"] == ITERS
    assert Bt.hindsight_stats()["rows_refused"] == 0 and 0 < Bt.hindsight_stats()["rows_reward_zero"] < Bt.hindsight_stats()["rows_relabelled"]
    assert Bt.step_sampled_stats() == dict(launches=ITERS, graph_captures=2) and A.step_sampled_stats()["launches"] == 0
    # as many nodes as the mixed draw's graphs of an engine of the same shape
    M.rb_pin(8)
    for u in range(2):
        M.step_sampled(u % 3 == 0, prior_rows=B // 2)
    nodes = [Bt.graph_kernel_count(16 + k) for k in range(4)]
    assert nodes == [M.graph_kernel_count(16 + k) for k in range(4)] and nodes[0] == nodes[2] == 0 and nodes[3] > nodes[1] > 4, nodes
    assert_same_state(A, Bt, "slot", "noise", "ring")
    for eng in (A, Bt):
        eng.rb_sample()
    assert_same_bits(A.read_batch(), Bt.read_batch(), what="a further uniform sample")


# ------------------------------------------------------------------------------------------ 2. one counter, whichever form draws
def test_the_draw_counters_stay_joined_across_forms():
    """graph, graph, the native call, the call with injected choices (it ticks nothing), graph -- on A all five as calls"""
    case, cap, algo = "goal-260", 101, "sac"
    o, a, B = CASES[case][:3]
    A, Bt = engines(case, cap, algo)
    idx = torch.as_tensor((np.arange(B) * 7) % (HELD_STEPS * STRIDE), device=DEV)
    choice = torch.as_tensor(np.array([(-1, 0, 2, 70)[b % 4] for b in range(B)], np.int32), device=DEV)

    def same_slot(what):
        got = read_slot(Bt, o, a)
        assert_same_bits(read_slot(A, o, a), got, what=what)
        return got
    for u in range(2):
        iteration_pair(A, Bt, u, f"graph {u}")
        same_slot(f"graph {u}")
    assert Bt.step_sampled_stats() == dict(launches=2, graph_captures=2)
    for eng in (A, Bt):
        eng.rb_sample_hindsight()
    got = same_slot("the native call")
    fields, geom, _ = hr.place({k: v[:HELD_STEPS * STRIDE] for k, v in rows_of(case)[0].items()}, cap)
    hr.check(hr.stage(fields, geom, mix_ref.mixed_indices(SEED, 2, B, 0, 0, geom["length"]), config(case), seed=SEED, hctr=2), got, ALL_KEYS)
    for eng in (A, Bt):
        eng.rb_sample_hindsight_device(idx.data_ptr(), 1, choice.data_ptr(), 1, B, stream())
    same_slot("the call with injected choices")
    assert A.hindsight_stats()["native_draws"] == Bt.hindsight_stats()["native_draws"] == 3
    iteration_pair(A, Bt, 2, "the graph behind the calls")
    got = same_slot("the graph behind the calls")
    hr.check(hr.stage(fields, geom, mix_ref.mixed_indices(SEED, 3, B, 0, 0, geom["length"]), config(case), seed=SEED, hctr=3), got, ALL_KEYS)
    assert A.hindsight_stats() == Bt.hindsight_stats() and Bt.hindsight_stats()["native_draws"] == 4
    assert Bt.step_sampled_stats() == dict(launches=3, graph_captures=2)      # the calls in between cost a launch, never a capture
    assert_same_state(A, Bt, "slot", "noise")


# ------------------------------------------------------------------------------------------ 3. the config travels by value
def test_a_changed_config_drops_the_graphs_and_the_same_config_does_not():
    case, cap, algo = "goal-260", 96, "sac"
    o, a, B = CASES[case][:3]
    A, Bt = engines(case, cap, algo)
    other = dict(ratio=0.5, window=3)
    captures = []
    for u in range(7):
        if u == 2:                                                        # between two launches of the same graph
            for eng in (A, Bt):
                eng.hindsight_configure(**config(case, **other))
        if u in (3, 4):                                                   # the identical config, issued again
            Bt.hindsight_configure(**config(case, **other))
        for eng in (A, Bt):
            append(eng, case, HELD_STEPS + u, HELD_STEPS + u + 1)
        iteration_pair(A, Bt, u, f"iteration {u}")
        hr.check(expected(case, cap, u, **(other if u >= 2 else {})), read_slot(Bt, o, a), ALL_KEYS)
        captures.append(Bt.step_sampled_stats()["graph_captures"])
    # u: 0 actor, 1 critic only, [changed] 2 critic only again: captured anew, 3 actor: anew, 4 5 6: replayed
    assert captures == [1, 2, 3, 4, 4, 4, 4], captures
    assert_same_state(A, Bt, "slot", "noise", "ring")
    assert A.hindsight_stats() == Bt.hindsight_stats()


# ------------------------------------------------------------------------------------------ 4. the eager form
def test_eager_form_equals_the_graph():
    """use_graphs = 0: the same launches issued one by one"""
    case, cap, algo = "goal-260", 96, "td3"
    o, a, B = CASES[case][:3]
    G, Eg = engines(case, cap, algo, use_graphs=(True, False))
    for i in range(6):
        for eng in (G, Eg):
            append(eng, case, HELD_STEPS + i, HELD_STEPS + i + 1)
            eng.step_sampled(i % 3 == 0, hindsight=True)
        assert_same_bits(iteration_state(G), iteration_state(Eg), what=f"iteration {i}")
        assert_same_bits(read_slot(G, o, a), read_slot(Eg, o, a), what=f"slot and info of iteration {i}")
    assert Eg.step_sampled_stats() == dict(launches=6, graph_captures=0) and G.step_sampled_stats() == dict(launches=6, graph_captures=2)
    assert G.hindsight_stats() == Eg.hindsight_stats()
    assert_same_state(G, Eg, "slot", "noise", "ring")


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing_and_leave_the_engine_usable():
    case, cap, algo = "goal-8", 96, "sac"
    B = CASES[case][2]
    eng, twin = engines(case, cap, algo, configure=False)
    (empty,) = engines(case, cap, algo, count=1, fill=False)
    eng.rb_sample()
    before = engine_state(eng, "slot")
    gen = eng.batch_generation()
    assert raw_step(eng, 1, H, 1, 1, 0.0) == S and "not configured" in last_error(eng)      # hindsight not configured
    assert raw_step(eng, 1, H, 2, 4, 0.0) == E and raw_step(eng, 0, H, 16, 1, 0.0) == E     # n_step must be 1
    eng.hindsight_configure(**config(case))
    assert raw_step(eng, 1, H, 2, 4, 0.0) == E and "n_step" in last_error(eng)
    for beta in (-1.0, float("nan"), float("inf")):                       # beta is checked as for the other draws
        assert raw_step(eng, 1, H, 1, 1, beta) == E, beta
    eng.rb_pin(10)
    assert raw_step(eng, 1, H, 1, 1, 0.0) == S and "pinned" in last_error(eng)             # pinned rows
    eng.rb_pin(0)
    assert raw_step(empty, 1, H, 1, 1, 0.0) == S and "empty" in last_error(empty)          # an empty ring
    assert raw_step(eng, 1, 7, 1, 1, 0.0) == E and raw_step(eng, 1, -1, 1, 1, 0.0) == E      # still no such draw
    assert eng.batch_generation() == gen
    assert_same_state(before, engine_state(eng, "slot"), what="refused calls")
    assert eng.step_sampled_stats() == dict(launches=0, graph_captures=0)
    assert eng.hindsight_stats() == dict(native_draws=0, rows_relabelled=0, rows_refused=0, rows_reward_zero=0)
    # the run-ahead chain: periods on both, refused one-launch calls on one of them in between -- the same bits afterwards
    twin.rb_sample()
    for k in range(3):
        eng.step_period()
        twin.step_period()
        assert raw_step(eng, 1, H, 2, 4, 0.0) == E and raw_step(eng, 1, H, 1, 1, -1.0) == E
    eng.hindsight_configure(**config(case))                               # (host state only)
    assert_same_state(eng, twin, "slot", "noise")
    # ... and the engine serves a plain iteration, and then the one it refused
    params = eng.get_params(_lib.CRITICS)
    eng.step(True)
    assert not same_bits(eng.get_params(_lib.CRITICS), params)
    eng.step_sampled(True, hindsight=True)
    assert eng.step_sampled_stats() == dict(launches=1, graph_captures=1) and eng.hindsight_stats()["native_draws"] == 1


# ------------------------------------------------------------------------------------------ 6. the loop
def run_20(one_launch):
    seed = 1
    cfg = P.launcher.job_config("sac", "PointGoal-native", seed, num_envs=STRIDE, learning_starts=240, batch_size=64, num_timesteps=240 + 20 * STRIDE - 1,
                                eval_every=10 ** 9, rb_capacity=4096)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, F), np.full(2, 1.0, F), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    env = track(envs.NativeVecEnv("pointgoal", STRIDE, seed=seed, device=DEV))
    metrics = loop.train(cfg, env, agent, device_env=True, fused=False, hindsight=dict(env.goal_layout, window=env.horizon), one_launch=one_launch)
    assert agent.qnet_updates_so_far == 20 and all(np.isfinite(v) for v in metrics.values())
    return agent


def test_train_as_one_launch_equals_train_call_by_call():
    A, Bt = run_20(False), run_20(True)
    assert A.engine.step_sampled_stats()["launches"] == 0
    assert Bt.engine.step_sampled_stats()["launches"] == 20 and Bt.engine.step_sampled_stats()["graph_captures"] <= 2
    st = Bt.engine.hindsight_stats()
    assert A.engine.hindsight_stats() == st and st["native_draws"] == 20 and st["rows_refused"] == 0 and st["rows_relabelled"] > 0
    assert A.actor_updates_so_far == Bt.actor_updates_so_far
    assert_same_state(A.engine, Bt.engine, "slot", "noise", "ring")
