"""GPU: runs of whole periods as one graph launch (include/sactd3.h: sactd3_step_periods, sactd3_step_periods_stats) against the calls they
replace -- sactd3_step_period, and the single iterations of sactd3_step -- for equal bits throughout.  What those compute is pinned
against the oracle by tests/test_gpu_engine.py; here only the sequences are compared with each other.

The smallest shapes that reach every form: the narrow pipelined period with the temperature pair (SAC Hopper, B = 64), the TD3 run-ahead
through the target actors of the next Polyak updates (HalfCheetah, B = 64), the smallest wide-observation pipelined batch (SAC Humanoid,
B = 1024) and a configuration without the pipelined form, where the call loops over single periods (SAC Humanoid, B = 64).  Rings hold
3000 synthetic rows."""
import functools

import numpy as np
import pytest

from oracle.sac_td3_ref import Hps
from tests.gpu_support import (P, _lib, assert_same_state, build_engines, close_engines, engine_state, flat_actor, flat_critics,  # noqa: F401
                               new_engine)
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu

# (algo, env, B, the period graph is pipelined)
CASES = {"sac-hopper-64": ("sac", "hopper", 64, True), "td3-halfcheetah-64": ("td3", "halfcheetah", 64, True),
         "sac-humanoid-1024": ("sac", "humanoid", 1024, True), "sac-humanoid-64": ("sac", "humanoid", 64, False)}
PERIOD = 3      # actor_update_delay 2 (the default of both algorithms)
ROWS = 3000
PARTS = ("index", "noise", "td")      # what a sequence of iterations leaves behind, beside parameters, optimisers and metrics


@functools.lru_cache(maxsize=None)
def material(case):
    """(hps, dims, the oracle's perturbed initial parameters, the ring's rows): computed once per case, never written"""
    algo, env, B, _ = CASES[case]
    ref, _, (o, a, bound) = build_engines(algo, DIMS[env], B, count=0, seed=5)
    params = {_lib.ACTOR: flat_actor(ref, ref.actor), _lib.ACTOR_TARGET: flat_actor(ref, ref.actor_target),
              _lib.CRITICS: flat_critics(ref, ref.qnets), _lib.CRITICS_TARGET: flat_critics(ref, ref.qnets_target)}
    rows = [t.numpy() for t in synth_transitions(ROWS + 400, o, a, bound, seed=31)]
    return ref.hps, (o, a, bound), params, rows


def engine(hps, dims, **cfg):
    return new_engine(hps, dims, max_envs=8, seed=5, **cfg)


def build(case, use_graphs=True, cap=4096):
    hps, dims, params, rows = material(case)
    eng = engine(hps, dims, rb_capacity=cap, use_graphs=use_graphs)
    for which, flat in params.items():
        eng.set_params(which, flat)
    eng.rb_extend(*[r[:ROWS] for r in rows])
    return eng


@functools.lru_cache(maxsize=None)
def run_len():
    """R, the periods of one run graph: a constant of the build, read off the node counts"""
    eng = build("sac-hopper-64")
    eng.instantiate_graphs()
    run, one = eng.graph_kernel_count(10), eng.graph_kernel_count(4)
    eng.close()
    assert one > 0 and run % one == 0
    R = run // one
    assert R in (2, 4, 6, 8)
    return R


def singles(eng, it, n):
    for i in range(it, it + n):
        eng.step(i % PERIOD == 0)
    return it + n


# ------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("started", [False, True], ids=["fresh", "behind-a-period"])
@pytest.mark.parametrize("case", list(CASES))
def test_step_periods_equals_periods_and_single_iterations(case, started):
    """step_periods(k) == k x step_period == 3k x step, for k below, at, just above R and across two runs; from a fresh engine (opening
    graph, variant 0) and behind one period (precomputed pair, variant 1)."""
    R = run_len()
    for k in (1, R, R + 1, 2 * R + 1):
        engs = [build(case) for _ in range(3)]
        if started:
            for e in engs[:2]:
                e.step_period()
            singles(engs[2], 0, PERIOD)
        engs[0].step_periods(k)
        for _ in range(k):
            engs[1].step_period()
        singles(engs[2], 0, PERIOD * k)
        assert_same_state(engs[0], engs[1], *PARTS, what=f"k={k}: runs vs periods")
        assert_same_state(engs[0], engs[2], *PARTS, what=f"k={k}: runs vs single iterations")
        assert engs[0].get_adam_state(_lib.CRITICS)[2] == PERIOD * (k + started)
        st = engs[0].step_periods_stats()
        if CASES[case][3]:
            assert (st["calls"], st["run_launches"], st["single_period_launches"]) == (1, k // R, k % R)
        else:
            assert (st["calls"], st["run_launches"], st["single_period_launches"]) == (1, 0, k)
        for e in engs:
            e.close()


# ------------------------------------------------------------------------------------------ 2. state changes between runs
@pytest.mark.parametrize("case", list(CASES))
def test_state_changes_between_runs_equal_single_iterations(case):
    """Between two runs: new rows that wrap a small ring under the captured graphs, acting, a write of perturbed actor and actor-target
    parameters, a single iteration -- each has to drop the precomputed opening pair (or keep it, where it may) exactly as between periods."""
    R = run_len()
    _, _, _, rows = material(case)
    res = []
    for mode in ("runs", "single"):
        eng = build(case, cap=ROWS + 100)

        def run(k):
            if mode == "runs":
                eng.step_periods(k)
            else:
                singles(eng, 0, PERIOD * k)                        # (a run starts a period wherever the caller stands)
        run(R)
        eng.rb_extend(*[r[ROWS:ROWS + 300] for r in rows])        # 3000 + 300 rows into 3100 slots: the ring wraps
        assert eng.rb_len() == ROWS + 100
        run(R)
        acted = eng.predict(rows[0][:4], True)
        run(R + 1)
        eng.set_params(_lib.ACTOR, eng.get_params(_lib.ACTOR) * np.float32(1.01))
        eng.set_params(_lib.ACTOR_TARGET, eng.get_params(_lib.ACTOR_TARGET) * np.float32(0.99))
        run(R)
        eng.step(False)                                            # a single critic-only iteration
        run(R)
        res.append(engine_state(eng, *PARTS, extra={"acted": acted}))
        eng.close()
    assert_same_state(*res, what="runs vs single iterations")


# ------------------------------------------------------------------------------------------ 3. node counts and counters
def test_run_graph_node_count_and_counters():
    R = run_len()
    plain, eng = build("sac-hopper-64"), build("sac-hopper-64")
    assert eng.graph_kernel_count(10) == 0 and eng.step_periods_stats()["run_graphs_captured"] == 0
    for e in (plain, eng):
        e.instantiate_graphs()
    eng.step_periods(2 * R + 1)
    for _ in range(2 * R + 1):
        plain.step_period()
    assert eng.graph_kernel_count(4) == 21 and eng.graph_kernel_count(10) == R * 21
    assert [eng.graph_kernel_count(i) for i in range(9)] == [plain.graph_kernel_count(i) for i in range(9)]
    with pytest.raises(P.EngineError):
        eng.graph_kernel_count(9)
    st = eng.step_periods_stats()
    assert st == {"calls": 1, "run_launches": 2, "single_period_launches": 1, "run_graphs_captured": 2}
    # the refusals: nothing changes
    before = engine_state(eng, *PARTS)
    with pytest.raises(P.EngineError, match="-1"):
        eng.step_periods(0)
    assert eng.step_periods_stats() == st
    assert_same_state(before, engine_state(eng, *PARTS), what="a refused step_periods")
    hps, dims, _, _ = material("sac-hopper-64")
    empty = engine(hps, dims, rb_capacity=256)
    with pytest.raises(P.EngineError, match="-3"):
        empty.step_periods(2)
    gated = engine(Hps.sac(batch_size=64, crit_targ_update_freq=2), dims, rb_capacity=256)
    gated.rb_fill_synthetic(200)
    with pytest.raises(P.EngineError, match="-3"):
        gated.step_periods(2)
    assert gated.get_adam_state(_lib.CRITICS)[2] == 0
    # without the pipelined form there is no run graph
    flat = build("sac-humanoid-64")
    flat.instantiate_graphs()
    flat.step_periods(R)
    assert flat.graph_kernel_count(10) == 0 and flat.step_periods_stats()["run_graphs_captured"] == 0


# ------------------------------------------------------------------------------------------ 4. eager launches
@pytest.mark.parametrize("case", list(CASES))
def test_eager_launches_equal_the_run_graphs(case):
    R = run_len()
    engs = [build(case, use_graphs=g) for g in (True, False)]
    for e in engs:
        e.step_periods(R + 1)
        e.step_periods(R)
    assert_same_state(*engs, *PARTS)
    assert engs[1].graph_kernel_count(10) == 0 and engs[1].step_periods_stats()["run_graphs_captured"] == 0


# ------------------------------------------------------------------------------------------ 5. reads behind a run
@pytest.mark.parametrize("case", ["sac-hopper-64", "td3-halfcheetah-64"])
def test_reads_behind_a_run_report_its_last_iteration(case):
    R = run_len()
    A, B = build(case), build(case)
    A.step_periods(R)
    singles(B, 0, PERIOD * R)
    assert_same_state(A, B, "slot", "noise", "td", what="reads behind a run")
    for name in ("grad_critics", "c_dz1", "grad_actor", "a_dz1"):
        with pytest.raises(P.EngineError, match="-3"):
            A.debug_read(name)
        assert B.debug_read(name).size > 0


# ------------------------------------------------------------------------------------------ 6. acting in flight
@pytest.mark.parametrize("case", ["sac-hopper-64", "td3-halfcheetah-64"])
def test_a_run_behind_predict_begin_leaves_the_action_of_the_serial_order(case):
    R = run_len()
    _, _, _, rows = material(case)
    A, B = build(case), build(case)
    for e in (A, B):
        e.step_periods(R)
    A.predict_begin(rows[0][:4], True)
    A.step_periods(R)
    got = A.predict_end()
    want = B.predict(rows[0][:4], True)
    B.step_periods(R)
    assert np.array_equal(got, want)
    assert_same_state(A, B, *PARTS)
    assert np.array_equal(A.predict(rows[0][4:8], True), B.predict(rows[0][4:8], True))      # the exploration stream stands where it should
    assert A.acting_stats()["learner_waited_for_acting"] == 1


# ------------------------------------------------------------------------------------------ 8. run_iterations end to end
@pytest.mark.parametrize("case", list(CASES))
def test_run_iterations_through_runs_equals_single_iterations(case):
    """single iterations 1, 2, then 2R + 1 periods in one step_periods call (two runs and a single period), a cut-short period of two
    iterations, one more iteration, and one period on its own"""
    R = run_len()
    A, B = build(case), build(case)
    n = 2 + PERIOD * (2 * R + 1) + 2
    it = A.run_iterations(1, n)
    it = A.run_iterations(it, 1 + PERIOD)
    assert it == singles(B, 1, n + 1 + PERIOD)
    assert_same_state(A, B, *PARTS)
    st = A.step_periods_stats()
    want = (2, 1) if CASES[case][3] else (0, 2 * R + 1)
    assert (st["calls"], st["run_launches"], st["single_period_launches"]) == (1,) + want
