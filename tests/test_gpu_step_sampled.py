"""GPU: the prioritised / n-step iteration as one graph launch (include/sactd3.h: sactd3_step_sampled, sactd3_step_sampled_stats) against
the call sequence it replaces, for equal bits throughout -- that sequence is pinned against the numpy restatements and the oracle by
tests/test_gpu_native_priorities.py and tests/test_gpu_nstep.py.

Engines are the twin small ones of tests/test_gpu_native_priorities.py (tests/gpu_support.py: PRIO_CASES, shape_engines; the oracle's
perturbed parameters, the critic site's noise injected): a 5000-slot ring that holds 2500 rows, or a 2504-slot one that the appends of
the test wrap.  The chained cases hold gpu_support.trajectories, the rows of tests/test_gpu_nstep.py (4 envs, so stride 4) -- on
independent rows every chain would be cut at its first link."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import priorities_ref as pref
from tests.gpu_support import (CAP, DEV, HELD, NSTEP_STRIDE as STRIDE, PRIO_CASES as CASES, SEED, SHAPES, P, _lib, assert_same_bits,  # noqa: F401
                               assert_same_state, boundary_uniforms, call_sequence, close_engines, engine_state, info, integer_priorities,
                               iteration_state, loop, raw_step, ring_rows, same_bits, sampled_draw, shape_engines, td_of, track, trajectories,
                               upload_priorities)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def chained_rows(shape, n, seed):
    """n rows of 4 envs' trajectories in append order (numpy, no NaN): computed once, never written"""
    _, (o, a, _), _ = SHAPES[shape]
    return trajectories(o, a, n, seed)


def held_rows(shape, chained):
    return chained_rows(shape, HELD, 21) if chained else [t.numpy() for t in ring_rows(shape)]


def fresh_rows(shape, chained, i):
    """the 4 rows appended in front of iteration i: one env step of the 4 envs"""
    if chained:
        return [f[4 * i:4 * i + 4] for f in chained_rows(shape, 64, 33)]
    return [t.numpy()[4 * i:4 * i + 4] for t in ring_rows(shape, 64, 34)]


def twins(case, count, chained=False, cap=CAP, enable=(0.6, 1e-6), held=True):
    shape, B = CASES[case]
    _, engs, (o, a, bound) = shape_engines(shape, count, B=B, cap=cap)
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for eng in engs:
        if held:
            eng.rb_extend(*held_rows(shape, chained))
        eng.set_noise(_lib.SITE_CRITIC, eps)
        if enable is not None:
            eng.prio_enable(*enable)
    return engs, shape, B


def betas(n):
    return [float(b) for b in np.linspace(0.4, 1.0, n)]


# ------------------------------------------------------------------------------------------ 1. one launch equals the call sequence
#        (case, prioritised, n_step, ring capacity)
EQUAL = [("sac-hopper-64", True, 1, CAP), ("sac-hopper-40", True, 1, CAP), ("td3-halfcheetah-64", True, 1, CAP), ("sac-hopper-1024", True, 1, CAP),
         ("sac-hopper-64", True, 3, CAP), ("td3-halfcheetah-64", True, 3, CAP), ("sac-hopper-40", False, 3, CAP),
         ("sac-hopper-64", True, 3, HELD + 4)]      # ... the appends wrap the ring: the length stops growing, the cursor passes 0


@pytest.mark.parametrize("case,prio,n_step,cap", EQUAL, ids=[f"{c}-{'prio' if p else 'uniform'}-n{n}-cap{k}" for c, p, n, k in EQUAL])
def test_one_launch_equals_the_call_sequence(case, prio, n_step, cap):
    """7 iterations, 4 rows appended in front of each, beta rising from 0.4 to 1.0, native draws: after every iteration the slot (with its
    ring indices), the slot weights, the priority table, the TD errors and the metrics; at the end every parameter set, Adam state, the
    counters, and one further prioritised and one uniform sample (the Philox counters ended equal)"""
    chained = n_step > 1
    (A, Bt), shape, B = twins(case, 2, chained=chained, cap=cap, enable=(0.6, 1e-6) if prio else None)
    for i, beta in enumerate(betas(7)):
        for eng in (A, Bt):
            eng.rb_extend(*fresh_rows(shape, chained, i))
        call_sequence(A, i % 3 == 0, sampled_draw(beta if prio else None, n_step, STRIDE), i + 1, write_back=prio)
        Bt.step_sampled(i % 3 == 0, beta=beta if prio else None, n_step=n_step, stride=STRIDE)
        assert_same_bits(iteration_state(A, prio), iteration_state(Bt, prio), what=f"iteration {i}")
        if chained:
            (ka, la), (kb, lb) = info(A), info(Bt)
            assert np.array_equal(ka, kb) and np.array_equal(la, lb), f"chains of iteration {i}"
    assert A.rb_len() == Bt.rb_len() == min(HELD + 28, cap)
    assert_same_state(A, Bt)
    assert A.nstep_stats() == Bt.nstep_stats() and A.priority_stats() == Bt.priority_stats()
    if chained:
        st = Bt.nstep_stats()
        assert st["stagings"] == 7 and st["rows_staged"] == 7 * B and st["rows_cut_short"] > 0 and st["rows_refused"] == 0
        assert 0 < st["rows_cut_short"] < 7 * B                    # some chains ran their whole length
    if prio:
        assert A.prio_stats() == Bt.prio_stats() == dict(samples=7, write_backs=7, rows_refused=0, rows_entered_at_max=HELD + 28)
        for eng in (A, Bt):
            eng.rb_sample_prioritized(0.5)
        assert_same_bits(A.read_batch(), Bt.read_batch(), what="a further prioritised sample")
        assert same_bits(A.debug_read("prio_weights"), Bt.debug_read("prio_weights"))
    for eng in (A, Bt):
        eng.rb_sample()
    assert_same_bits(A.read_batch(), Bt.read_batch(), what="a further uniform sample")
    assert Bt.step_sampled_stats()["launches"] == 7


def test_eager_form_equals_the_graph():
    """use_graphs = 0: the same launches issued one by one"""
    shape, B = CASES["sac-hopper-64"]
    _, (G, E), (o, a, bound) = shape_engines(shape, B=B, cap=CAP, use_graphs=(True, False))
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for eng in (G, E):
        eng.rb_extend(*held_rows(shape, True))
        eng.set_noise(_lib.SITE_CRITIC, eps)
        eng.prio_enable(0.6, 1e-6)
    for i, beta in enumerate(betas(4)):
        for eng in (G, E):
            eng.step_sampled(i % 3 == 0, beta=beta, n_step=3, stride=STRIDE)
        assert_same_bits(iteration_state(G, True), iteration_state(E, True), what=f"iteration {i}")
    assert_same_state(G, E)
    assert E.step_sampled_stats() == dict(launches=4, graph_captures=0) and G.step_sampled_stats()["graph_captures"] == 2


# ------------------------------------------------------------------------------------------ 2. replayed, not re-captured
def test_graphs_are_replayed_while_beta_moves_and_the_ring_grows():
    (eng,), shape, B = twins("sac-hopper-64", 1, chained=True, enable=(1.0, 1e-6))
    for i, beta in enumerate(betas(12)):
        eng.rb_extend(*fresh_rows(shape, True, i))
        eng.step_sampled(i % 3 == 0, beta=beta)
    st = eng.step_sampled_stats()
    assert st == dict(launches=12, graph_captures=2)               # (do_actor, target update) in {(1, 1), (0, 1)}: SAC, crit_targ_update_freq 1
    nodes = [eng.graph_kernel_count(16 + k) for k in range(4)]
    assert nodes[0] == nodes[2] == 0 and nodes[3] > nodes[1] > 4 and eng.graph_kernel_count(8) == 0      # (the graph holds the weighted update itself)
    # injected uniforms select the restatement's slots through the graph, without a capture; the draw counter stands still
    length = eng.rb_len()
    assert length == HELD + 48
    prio = np.ones(length, np.float32)
    prio[:HELD] = integer_priorities()
    keep = upload_priorities(eng, np.arange(length), prio)
    leaf = eng.debug_read("prio_leaf")
    assert np.array_equal(leaf[:length], prio) and float(leaf.sum()) < 4096
    u = boundary_uniforms(B)
    eng.prio_set_uniforms(u)
    eng.step_sampled(False, beta=0.4)
    got, want = eng.read_batch()["index"], pref.select(leaf, length, u)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    eng.prio_set_uniforms(None)
    keep2 = upload_priorities(eng, np.arange(length), prio)                     # (the write-back moved the drawn rows' leaves)
    eng.step_sampled(False, beta=0.4)                               # native again: draw 12 of the Philox stream
    want = pref.select(leaf, length, pref.native_uniforms(SEED, 12, B))
    assert np.array_equal(eng.read_batch()["index"], want)
    assert eng.step_sampled_stats() == dict(launches=14, graph_captures=2)
    eng.step_sampled(False, beta=0.4, n_step=3, stride=STRIDE)      # another (draw, n_step, stride): the cached graphs are dropped
    assert eng.step_sampled_stats() == dict(launches=15, graph_captures=3)
    assert eng.graph_kernel_count(16 + 3) == 0 and eng.graph_kernel_count(16 + 1) > 0
    del keep, keep2


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_change_nothing_and_leave_the_engine_usable():
    (eng, N), shape, B = twins("sac-hopper-64", 2, chained=True)
    (empty,), _, _ = twins("sac-hopper-64", 1, held=False)
    before = engine_state(eng, "prio")
    U, PR, E, S = _lib.DRAW_UNIFORM, _lib.DRAW_PRIORITIZED, _lib.EINVAL, _lib.ESTATE
    assert eng.lib.sactd3_step_sampled(eng._h, 1, None) == E
    assert eng.lib.sactd3_step_sampled(None, 1, None) == E and eng.lib.sactd3_step_sampled_stats(None, None) == E
    for args, code in (((7, 1, 1, 0.4), E), ((-1, 1, 1, 0.4), E),                                 # unknown draw
                       ((PR, 0, 1, 0.4), E), ((PR, 17, 4, 0.4), E), ((U, 0, 1, 0.0), E),          # n_step outside [1, 16]
                       ((PR, 3, 0, 0.4), E), ((U, 3, -2, 0.0), E),                                # stride < 1 at n_step > 1
                       ((PR, 1, 1, -0.5), E), ((PR, 1, 1, float("nan")), E), ((PR, 3, 4, float("inf")), E)):
        assert raw_step(eng, 1, *args) == code, args
    N2 = twins("sac-hopper-64", 1, chained=True, enable=None)[0][0]
    assert raw_step(N2, 1, PR, 1, 1, 0.4) == S                     # priorities not enabled
    assert raw_step(empty, 1, PR, 1, 1, 0.4) == S and raw_step(empty, 0, U, 3, 4, 0.0) == S      # empty ring
    assert_same_state(before, engine_state(eng, "prio"), what="refused calls")
    assert eng.step_sampled_stats() == dict(launches=0, graph_captures=0)
    # nothing to draw from: zero-weight rows, refused counts, unchanged parameters (a fresh Adam state: a zero gradient moves nothing)
    keep = upload_priorities(N, np.arange(HELD), np.zeros(HELD, np.float32))
    pa, pc = N.get_params(_lib.ACTOR), N.get_params(_lib.CRITICS)
    N.step_sampled(False, beta=0.4, n_step=3, stride=STRIDE)
    assert not N.debug_read("prio_weights").any() and (N.read_batch()["index"] == -1).all()
    assert same_bits(N.get_params(_lib.ACTOR), pa) and same_bits(N.get_params(_lib.CRITICS), pc)
    assert N.nstep_stats()["rows_refused"] == B and N.prio_stats()["rows_refused"] == B and not N.debug_read("prio_leaf").any()
    # ... and the refused engine runs a normal iteration
    eng.step_sampled(True, beta=0.4, n_step=3, stride=STRIDE)
    assert eng.step_sampled_stats() == dict(launches=1, graph_captures=1)
    assert not same_bits(eng.get_params(_lib.CRITICS), before["params.critics"])
    assert eng.prio_stats() == dict(samples=1, write_backs=1, rows_refused=0, rows_entered_at_max=HELD)
    del keep


# ------------------------------------------------------------------------------------------ 4. nothing else moved
def test_the_other_entry_points_agree_behind_it():
    (A, Bt), shape, B = twins("sac-hopper-64", 2, chained=True)
    for i, beta in enumerate(betas(4)):
        call_sequence(A, i % 3 == 0, sampled_draw(beta, 3, STRIDE), i + 1, write_back=True)
        Bt.step_sampled(i % 3 == 0, beta=beta, n_step=3, stride=STRIDE)
    # the slot behind the one-launch iteration serves the read-outs and the caller's write-back
    assert same_bits(td_of(A), td_of(Bt))
    (ka, la), (kb, lb) = info(A), info(Bt)
    assert np.array_equal(ka, kb) and np.array_equal(la, lb) and (kb >= 1).all()
    idx = Bt.read_batch()["index"]
    keep = [upload_priorities(e, idx, np.linspace(0.5, 2.0, B)) for e in (A, Bt)]
    assert same_bits(A.debug_read("prio_leaf"), Bt.debug_read("prio_leaf")) and same_bits(A.debug_read("prio_sums"), Bt.debug_read("prio_sums"))
    for eng in (A, Bt):
        for i in range(3):
            eng.step(i % 3 == 0)
        eng.step_period()
    assert_same_state(A, Bt)
    assert_same_bits(A.read_batch(), Bt.read_batch(), what="the slot behind step and step_period")
    del keep


# ------------------------------------------------------------------------------------------ 5. acting overlap
def test_acting_overlaps_with_the_one_launch_iteration():
    (S, O), shape, B = twins("sac-hopper-64", 2, chained=True)
    _, (o, a, _), _ = SHAPES[shape]
    g = torch.Generator().manual_seed(17)
    for i, beta in enumerate(betas(6)):
        obs = torch.randn(4, o, generator=g).numpy()
        want = S.predict(obs, True)
        S.step_sampled(i % 3 == 0, beta=beta, n_step=3, stride=STRIDE)
        O.predict_begin(obs, True)
        O.step_sampled(i % 3 == 0, beta=beta, n_step=3, stride=STRIDE)
        got = O.predict_end()
        assert same_bits(want, got), f"actions of iteration {i}"
    assert_same_state(S, O)
    assert O.acting_stats()["learner_waited_for_acting"] + O.acting_stats()["begin_waited_for_learner"] > 0


# ------------------------------------------------------------------------------------------ 6. the loop
def test_train_one_launch_equals_the_call_by_call_loop():
    o, a, n, iters = 11, 3, 4, 60
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 200 + iters * n - 1, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 1000})
    res = []
    for one_launch in (False, True):
        env = loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5)
        env.action_space.seed(0)
        torch.manual_seed(0)
        np.random.seed(0)
        agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                        torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
        loop.train(cfg, env, agent, fused=False, prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6), n_step=3, one_launch=one_launch)
        eng = track(agent.engine)
        res.append(engine_state(eng, "prio", extra=dict(
            nstep=np.float32(list(eng.nstep_stats().values())),
            counters=np.float32([agent.qnet_updates_so_far, agent.actor_updates_so_far, agent.timesteps_so_far, len(agent.rb)]))))
        launches = eng.step_sampled_stats()
        assert launches["launches"] == (agent.qnet_updates_so_far if one_launch else 0) and launches["graph_captures"] <= 2
        assert agent.qnet_updates_so_far >= iters
        eng.close()
    assert_same_state(res[0], res[1], what="one_launch against the call sequence")
