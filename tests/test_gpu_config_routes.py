"""GPU: every configuration corner through every route of an iteration.  csrc/engine.hip builds its sequences from the configuration, not
only from the shapes: enqueue_update_actor (can_merge, defer_alpha, the clipped k_tn + k_gradnorm + k_adam form that moves TD3's
actor-target lerp and noise tick into k_adam, the actor targets written ahead), period_is_pipelined (SAC without autotune, TD3 with
clip_norm, a delay outside 1..2 fall to single iterations back to back), enqueue_period's lean stores, iteration_schedule's four step
graphs, actor_update_delay = 0.  Three parts:

 1. Routes agree, bit for bit, per configuration: the call sequence, sactd3_step, Engine.run_iterations (periods, prefixes, run graphs)
    and the same with use_graphs = 0 leave one engine_state -- every parameter set, m / v / t of the three optimisers, every metric, the
    slot's ring indices, the critic site's draws, the TD errors; with clip_norm the stored gradients too (lean stores are off there).
    One non-default field at a time and three interacting pairs at the narrow pipelined shapes (B = 64); the fields that change the
    graph's structure also at the smallest shape of every other builder form.  A Python restatement of period_is_pipelined names the
    form each case must take and the counters of sactd3_step_periods_stats confirm it, so a configuration that falls into the other
    form cannot keep passing while testing nothing new.  Beside the equalities: crit_targ_update_freq = 2 moves the critic targets on
    even update counts only; actor_update_delay = 0 never moves the actor; step_sampled at three corners equals its call sequence.
 2. The anchor: route equality proves nothing unless the call sequence itself is right at these corners, so five of them run
    gpu_stage_checks.run_one_iteration stage by stage against float64 with the a-priori bounds of tests/bounds.py (no tolerance of
    this module's own).
 3. State changes between chained periods: two periods, one state-changing call, two more periods equal the same sequence as single
    iterations -- for every call that has to drop the precomputed opening pair (csrc/engine.hip: CHAIN_BREAK) and that the other
    modules never place between two periods -- and the call did reach the result.

Iteration numbering: iteration i runs the actor updates when i % (delay + 1) == 0; the span of part 1 is iterations 1 .. 3 (delay + 1) + 1,
which starts off a period boundary and crosses two whole chained periods (delay 2 and 3: then two iterations of a cut-short one; delay
1: a third whole period; delay 0 has no periods).  The target-update count handed to update_targ_nets is the number of critic updates
the engine has done, which is what sactd3_step counts itself -- not i + 1, since the span does not start at 0."""
import functools

import numpy as np
import pytest
import torch

from tests.gpu_stage_checks import run_one_iteration
from tests.gpu_support import (DEV, NSTEP_STRIDE, P, SHAPES, _lib, assert_same_bits, assert_same_state, build_engines, call_sequence,  # noqa: F401
                               close_engines, cuda, engine_state, extend_device, iteration_state, rows, same_bits, sampled_draw, shape_engines,
                               stream, trajectories)
from tests.helpers import DIMS

pytestmark = pytest.mark.gpu

ROWS = 600                            # the ring of every engine here: synthetic rows
PARTS = ("index", "noise", "td")
SEED = 5
HID, BIG_BATCH = 256, 1024            # csrc/kernels.h, csrc/engine.hip


# ------------------------------------------------------------------------------------------ the form model
def _cdiv(a, b):
    return -(-a // b)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def period_is_pipelined(algo, o, a, B, num_cus, autotune=True, clip_norm=0.0, actor_update_delay=2, **_):
    """csrc/engine.hip: period_is_pipelined with opening_trunk_carries_alpha, opening_trunk_gathers and actor_dw_is_tiled64, restated"""
    big = B >= BIG_BATCH
    opening_tiled = big and _cdiv(B, 64) * (HID // 64) * 2 >= (3 * num_cus) // 4      # the k_nt64 pair: no riding temperature step, no ring rows
    gathers = (o <= 64 and not big) or (o > 64 and big and not opening_tiled)
    if actor_update_delay not in (1, 2) or not gathers:
        return False
    if algo == "td3":
        # the actor's weight-gradient launch on the split-M route (64 x 32 tiles of head, layer 2 and layer 1 over at least half the CUs)
        # has no epilogue that writes the next Polyak updates' actor targets ahead; nor has the clipped k_adam
        tiles64 = _cdiv(a, 64) * _cdiv(HID, 32) + _cdiv(HID, 64) * _cdiv(HID, 32) + _cdiv(HID, 64) * _cdiv((o + 3) // 4 * 4, 32)
        return clip_norm <= 0 and not (big and tiles64 >= num_cus // 2)
    return bool(autotune)


# ------------------------------------------------------------------------------------------ 1. the routes
# fields, one non-default value at a time, then the pairs whose branches interact
FIELDS = {"sac": [dict(autotune=False), dict(bcq_style_targ_mix=True), dict(clip_norm=0.05), dict(ln=False), dict(crit_targ_update_freq=2),
                  dict(actor_update_delay=0), dict(actor_update_delay=1), dict(actor_update_delay=3),
                  dict(autotune=False, clip_norm=0.05), dict(autotune=False, actor_update_delay=1)],
          "td3": [dict(targ_actor_smoothing=False), dict(bcq_style_targ_mix=False), dict(clip_norm=0.05), dict(ln=False),
                  dict(actor_update_delay=0), dict(actor_update_delay=1), dict(actor_update_delay=3),
                  dict(clip_norm=0.05, targ_actor_smoothing=False)]}
# the sets that change the graph's structure (crit_targ_update_freq and autotune exist under SAC only)
STRUCTURAL = {"sac": [dict(autotune=False), dict(clip_norm=0.05), dict(crit_targ_update_freq=2), dict(actor_update_delay=1), dict(actor_update_delay=3)],
              "td3": [dict(clip_norm=0.05), dict(actor_update_delay=1), dict(actor_update_delay=3)]}
NARROW = {"sac": ("hopper", 64), "td3": ("halfcheetah", 64)}          # the narrow pipelined shapes
# the smallest shape of every other builder form: wide observations below the large-batch threshold (k_gather, never pipelined); wide
# ones pipelined at large batch; narrow ones at large batch; the first batch where opening_trunk_carries_alpha is false on 256 CUs
OTHER_FORMS = [("humanoid", 64), ("humanoid", 1024), ("hopper", 1024), ("humanoid", 1473)]
ROUTE_CASES = [(algo, *NARROW[algo], f) for algo in ("sac", "td3") for f in FIELDS[algo]]
ROUTE_CASES += [(algo, env, B, f) for env, B in OTHER_FORMS for algo in ("sac", "td3") for f in STRUCTURAL[algo]]


def _fields_id(fields):
    return "+".join(f"{k}={v}" for k, v in fields.items())


def _case_id(case):
    algo, env, B, fields = case
    return f"{algo}-{env}-{B}-{_fields_id(fields)}"


def _calls(eng, i0, n, delay):
    for done, i in enumerate(range(i0, i0 + n)):
        eng.rb_sample()
        eng.update_qnets()
        if i % (delay + 1) == 0:
            for _ in range(delay):
                eng.update_actor()
        eng.update_targ_nets(done + 1)


def _steps(eng, i0, n, delay, after=None):
    for done, i in enumerate(range(i0, i0 + n)):
        before = eng.get_params(_lib.CRITICS_TARGET) if after else None
        eng.step(i % (delay + 1) == 0)
        if after:
            after(done + 1, before, eng.get_params(_lib.CRITICS_TARGET))


def _state(eng, clip):
    extra = {"grad_actor": eng.debug_read("grad_actor"), "grad_critics": eng.debug_read("grad_critics")} if clip else None
    return engine_state(eng, *PARTS, extra=extra)


@pytest.mark.parametrize("case", ROUTE_CASES, ids=[_case_id(c) for c in ROUTE_CASES])
def test_routes_agree_bit_for_bit(case):
    algo, env, B, fields = case
    hp = dict(fields)
    ln = hp.pop("ln", True)
    delay, freq, clip = hp.get("actor_update_delay", 2), hp.get("crit_targ_update_freq", 1), hp.get("clip_norm", 0.0) > 0
    o, a, _ = DIMS[env]
    i0, n = 1, 3 * (delay + 1) + 1
    _, engs, _ = build_engines(algo, DIMS[env], B, ln=ln, seed=SEED, use_graphs=(True, True, True, False), **hp)
    for eng in engs:
        eng.rb_fill_synthetic(ROWS, seed=7)
    calls, step, periods, eager = engs
    first = engine_state(step)

    # crit_targ_update_freq: sactd3_step counts the critic updates itself; the targets move when that count reaches a multiple
    moved = {}

    def after(count, t0, t1):
        moved[count] = not same_bits(t0, t1)
    _calls(calls, i0, n, delay)
    _steps(step, i0, n, delay, after if algo == "sac" else None)
    assert periods.run_iterations(i0, n) == i0 + n
    assert eager.run_iterations(i0, n) == i0 + n
    want = _state(calls, clip)
    for name, eng in (("step", step), ("periods", periods), ("eager", eager)):
        assert_same_state(want, _state(eng, clip), what=f"{_case_id(case)}: calls vs {name}")
    n_act = delay * len([i for i in range(i0, i0 + n) if i % (delay + 1) == 0])
    assert int(want["adam_t.critics"][0]) == n and int(want["adam_t.actor"][0]) == n_act
    assert not same_bits(want["params.critics"], first["params.critics"])
    if algo == "sac":
        assert moved == {c: c % freq == 0 for c in range(1, n + 1)}, moved
    if delay == 0:
        # step(True) is the critic-only sequence (equal to the calls above, TD3's actor target through the API path's k_polyak
        # included): nothing of the actor's moves
        for k in ("params.actor", "adam_m.actor", "adam_v.actor", "adam_t.actor") + (("params.log_alpha",) if algo == "sac" else ()):
            assert same_bits(want[k], first[k]), k
        if algo == "td3":
            assert not same_bits(want["params.actor_target"], first["params.actor_target"])
    elif algo == "td3" or hp.get("autotune", True):
        assert not same_bits(want["params.actor"], first["params.actor"])
    if algo == "sac" and not hp.get("autotune", True):      # a fixed temperature, and Adam words nobody touched
        for k in ("params.log_alpha", "adam_m.log_alpha", "adam_v.log_alpha", "adam_t.log_alpha"):
            assert same_bits(want[k], first[k]), k

    # the form the period graph took: the model against the counters of step_periods
    pipelined = period_is_pipelined(algo, o, a, B, _cus(), **hp)
    st = periods.step_periods_stats()
    print(f"FORM {_case_id(case)}: model pipelined={pipelined} counters={st}")
    if freq != 1:
        assert st["calls"] == 0, st                           # run_iterations fell back to single iterations
        for refused in (periods.step_period, lambda: periods.step_periods(2), lambda: periods.step_prefix(1)):
            with pytest.raises(P.EngineError, match="-3"):
                refused()
        assert periods.step_periods_stats() == st and periods.get_adam_state(_lib.CRITICS)[2] == n
        return
    whole = (i0 + n) // (delay + 1) - 1 if delay else 0      # whole periods of the span, one step_periods call
    assert st["calls"] == (1 if whole else 0), st
    if whole and not pipelined:
        assert (st["run_launches"], st["single_period_launches"], st["run_graphs_captured"]) == (0, whole, 0), st
    # ... and behind 8 more periods (a run graph holds at most 8)
    periods.step_periods(8)
    st8 = periods.step_periods_stats()
    if pipelined:
        assert st8["run_launches"] > st["run_launches"] and st8["run_graphs_captured"] >= 1, (st, st8)
    else:
        assert (st8["run_launches"], st8["single_period_launches"], st8["run_graphs_captured"]) == (0, st["single_period_launches"] + 8, 0), (st, st8)
    assert periods.get_adam_state(_lib.CRITICS)[2] == n + 8 * (delay + 1)


def test_route_cases_reach_both_forms_of_every_rule():
    """over ROUTE_CASES on 256 CUs, by the model the test above holds against the counters: each rule of period_is_pipelined turns a
    pipelined shape into the other form at least once, and each builder form appears"""
    forms = {}
    for algo, env, B, fields in ROUTE_CASES:
        o, a, _ = DIMS[env]
        hp = {k: v for k, v in fields.items() if k != "ln"}
        forms[(algo, env, B, _fields_id(fields))] = (period_is_pipelined(algo, o, a, B, 256, **hp), period_is_pipelined(algo, o, a, B, 256))
    for key in (("sac", "hopper", 64, "autotune=False"), ("td3", "halfcheetah", 64, "clip_norm=0.05"), ("sac", "hopper", 64, "actor_update_delay=3"),
                ("sac", "hopper", 64, "actor_update_delay=0"), ("sac", "humanoid", 1024, "autotune=False"), ("td3", "humanoid", 1024, "clip_norm=0.05"),
                ("td3", "humanoid", 1024, "actor_update_delay=3")):
        assert forms[key] == (False, True), (key, forms[key])
    for key in (("sac", "hopper", 64, "clip_norm=0.05"), ("sac", "hopper", 64, "actor_update_delay=1"), ("td3", "halfcheetah", 64, "actor_update_delay=1"),
                ("sac", "humanoid", 1024, "clip_norm=0.05"), ("td3", "humanoid", 1024, "actor_update_delay=1"), ("sac", "hopper", 64, "ln=False")):
        assert forms[key] == (True, True), (key, forms[key])
    for env, B in (("humanoid", 64), ("hopper", 1024), ("humanoid", 1473)):
        assert not any(f[1] for k, f in forms.items() if k[1:3] == (env, B)), (env, B)
    # the split-M rule of the actor's weight gradients needs observations wider than any shape here: the model alone covers it
    assert not period_is_pipelined("td3", 700, 17, 1024, 256) and period_is_pipelined("sac", 700, 17, 1024, 256)


# ---- step_sampled at the corners that change its graphs
SAMPLED_CASES = [("sac-hopper", dict(autotune=False)), ("sac-hopper", dict(clip_norm=0.05)), ("sac-hopper", dict(crit_targ_update_freq=2)),
                 ("td3-halfcheetah", dict(clip_norm=0.05))]


@functools.lru_cache(maxsize=None)
def _chained_rows(shape):
    _, (o, a, _), _ = SHAPES[shape]
    return trajectories(o, a, ROWS, 21)


@pytest.mark.parametrize("prio", [False, True], ids=["uniform-n2", "prioritised"])
@pytest.mark.parametrize("shape,fields", SAMPLED_CASES, ids=[f"{s}-{_fields_id(f)}" for s, f in SAMPLED_CASES])
def test_step_sampled_equals_the_call_sequence(shape, fields, prio):
    """7 iterations with the uniform draw at n_step = 2, and with the prioritised draw: after every iteration the slot with its ring
    indices, the TD errors, the metrics (prioritised: the slot weights and the priority table); at the end the whole state"""
    _, (A, Bt), _ = shape_engines(shape, 2, B=64, **fields)
    beta, n_step = (0.7, 1) if prio else (None, 2)
    for eng in (A, Bt):
        eng.rb_extend(*_chained_rows(shape))
        if prio:
            eng.prio_enable(0.6, 1e-6)
    for i in range(7):
        call_sequence(A, i % 3 == 0, sampled_draw(beta, n_step, NSTEP_STRIDE), i + 1, write_back=prio)
        Bt.step_sampled(i % 3 == 0, beta=beta, n_step=n_step, stride=NSTEP_STRIDE)
        assert_same_bits(iteration_state(A, prio), iteration_state(Bt, prio), what=f"iteration {i}")
    assert_same_state(A, Bt, *PARTS)
    assert Bt.step_sampled_stats()["launches"] == 7 and A.get_adam_state(_lib.CRITICS)[2] == 7 and A.get_adam_state(_lib.ACTOR)[2] == 6


# ------------------------------------------------------------------------------------------ 2. the anchor
ANCHORS = [("sac", "humanoid", 1024, True, dict(autotune=False)),
           ("td3", "humanoid", 1024, True, dict(clip_norm=0.05)),         # k_gradnorm + k_adam behind the large-batch weight-gradient route
           ("sac", "hopper", 1473, True, dict(clip_norm=0.05)),
           ("td3", "halfcheetah", 64, False, dict()),
           ("sac", "hopper", 1024, False, dict())]


@pytest.mark.parametrize("algo,env,B,ln,hp", ANCHORS, ids=[f"{a}-{e}-{b}-{'ln' if ln else 'noln'}{'-' + _fields_id(hp) if hp else ''}" for a, e, b, ln, hp in ANCHORS])
def test_call_sequence_of_the_corners_against_float64(algo, env, B, ln, hp):
    run_one_iteration(algo, env, B, ln, f"config_routes_anchor[{algo}-{env}-{B}-{ln}-{_fields_id(hp)}]", stages=True, **hp)


# ------------------------------------------------------------------------------------------ 3. state changes between chained periods
# a mutation: f(eng, dims, period) -- `period` issues one period in the route under test (only the noise mutation holds one)
def _scaled(x, f):
    return np.asarray(x, np.float32) * np.float32(f)


def _set_params(which, add=0.0):
    def go(eng, dims, period):
        eng.set_params(which, _scaled(eng.get_params(which), 1.01) + np.float32(add))
    return go


def _set_adam(which):
    def go(eng, dims, period):
        m, v, t = eng.get_adam_state(which)
        eng.set_adam_state(which, _scaled(m, 0.5) + np.float32(1e-4), _scaled(v, 2.0) + np.float32(1e-8), t + 3)
    return go


def _noise_period(eng, dims, period):
    eng.set_noise(_lib.SITE_CRITIC, torch.randn(eng.cfg.batch_size, dims[1], generator=torch.Generator().manual_seed(4)))
    period()
    eng.clear_noise(_lib.SITE_CRITIC)


def _extend_fields(eng, dims, period):
    five = cuda(rows(100, *dims, seed=9))
    extend_device(eng, five)
    eng.sync()                                  # (the arrays stay alive until the engine has read them)


def _extend_records(eng, dims, period):
    rec = torch.as_tensor(eng.pack_records(*[t.numpy() for t in rows(100, *dims, seed=9)])).to(DEV)
    eng.rb_extend_records_device(rec.data_ptr(), 100, stream())
    eng.sync()


def _load_and_update(eng, dims, period):
    eng.load_batch(*[t.numpy() for t in rows(eng.cfg.batch_size, *dims, seed=10)])
    eng.update_qnets()


INJECTED = np.random.default_rng(14).integers(0, ROWS, 64)
MUTATIONS = {"set_params-actor": _set_params(_lib.ACTOR), "set_params-critics": _set_params(_lib.CRITICS),
             "set_params-actor_target": _set_params(_lib.ACTOR_TARGET), "set_params-critics_target": _set_params(_lib.CRITICS_TARGET),
             "set_params-log_alpha": _set_params(_lib.LOG_ALPHA, 0.1),
             "set_adam_state-actor": _set_adam(_lib.ACTOR), "set_adam_state-critics": _set_adam(_lib.CRITICS), "set_adam_state-log_alpha": _set_adam(_lib.LOG_ALPHA),
             "set_noise-critic+period+clear_noise": _noise_period, "rb_extend_fields_device": _extend_fields, "rb_extend_records_device": _extend_records,
             "load_batch+update_qnets": _load_and_update, "rb_sample_with_indices": lambda eng, dims, period: eng.rb_sample_with_indices(INJECTED),
             "set_bc": lambda eng, dims, period: eng.set_bc(1.5, 0.25)}
SAC_ONLY, TD3_ONLY = ("set_params-log_alpha", "set_adam_state-log_alpha"), ("set_bc",)
BETWEEN = [(algo, m) for algo in ("sac", "td3") for m in MUTATIONS if m not in (TD3_ONLY if algo == "sac" else SAC_ONLY)]


def _between_engine(algo, bc):
    env, B = NARROW[algo]
    _, (eng,), dims = build_engines(algo, DIMS[env], B, seed=SEED, cap=1024, **({"bc_alpha": 2.5} if bc else {}))
    eng.rb_fill_synthetic(ROWS, seed=7)
    return eng, dims


@functools.lru_cache(maxsize=None)
def _periods_alone(algo, bc, periods):
    """the state behind `periods` chained periods with nothing in between: computed once, never written"""
    eng, _ = _between_engine(algo, bc)
    eng.step_period()
    eng.step_period()
    eng.step_periods(periods - 2)
    state = engine_state(eng, *PARTS)
    eng.close()
    return state


@pytest.mark.parametrize("algo,mutation", BETWEEN, ids=[f"{a}-{m}" for a, m in BETWEEN])
def test_state_changes_between_chained_periods_equal_single_iterations(algo, mutation):
    """Two periods (the second on the opening pair the first left, leaving one itself in batch slot 0), the call, two more periods in
    one step_periods call == the same as single iterations; and the result differs from that of the periods alone -- a call that
    reached nothing proves nothing.  rb_sample_with_indices is the exception to the second half: it replaces the rows of batch slot 0
    and nothing else, the next period's opening graph replaces them again, so a correct engine ends where the periods alone end;
    what the call reached is the slot, read right behind it."""
    bc = mutation == "set_bc"
    res = {}
    for mode in ("periods", "single"):
        eng, dims = _between_engine(algo, bc)
        it = [0]

        def run(k):
            if mode == "single":
                for _ in range(3 * k):
                    eng.step(it[0] % 3 == 0)
                    it[0] += 1
            elif k == 1:
                eng.step_period()
            else:
                eng.step_periods(k)
        run(1)
        run(1)
        if mode == "periods":
            assert eng.graph_kernel_count(5) > 0      # the opening graph exists: the chained form is in use
        MUTATIONS[mutation](eng, dims, lambda: run(1))
        if mutation == "rb_sample_with_indices":
            assert np.array_equal(eng.read_batch()["index"], INJECTED)
        run(2)
        res[mode] = engine_state(eng, *PARTS)
        eng.close()
    assert_same_state(res["periods"], res["single"], what=f"{algo} {mutation}: periods vs single iterations")
    alone = _periods_alone(algo, bc, 5 if mutation.startswith("set_noise") else 4)
    differs = [k for k in alone if not same_bits(alone[k], res["periods"][k])]
    if mutation == "rb_sample_with_indices":
        assert not differs, differs
    else:      # (nothing reads SAC's actor target: a write of it reaches that set alone)
        reached = "params.actor_target" if (algo, mutation) == ("sac", "set_params-actor_target") else "params.critics"
        assert reached in differs, (mutation, differs)


