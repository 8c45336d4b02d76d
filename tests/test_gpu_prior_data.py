"""GPU: learning online from prior data (include/sactd3.h: sactd3_rb_pin, sactd3_rb_set_mix, sactd3_rb_sample_mixed, sactd3_mix_stats,
SACTD3_DRAW_MIXED) -- the pinned ring against the numpy cursor model and the mixed draw against the numpy slot formula of
tests/mix_ref.py, bit for bit; the one-launch iteration against the call sequence it replaces; the refusals; the paths that must not
notice a pinned ring; the loop.

Shapes: SAC Hopper dims at B = 64 and B = 40 (a ragged last block in the staging) and TD3 HalfCheetah dims at B = 64; rings of 38 to
64 slots with 37 pinned rows."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.replay_ref import sample_indices
from oracle.sac_td3_ref import Hps
from tests import mix_ref
from tests.gpu_support import (DEV, MAXN, SEED, SHAPES, P, _lib, agent_mod, assert_same_bits, assert_same_state, call_sequence,  # noqa: F401
                               close_engines, engine_state, fields_of, iteration_state, loop, new_engine, raw_step, rows, same_bits,
                               shape_engines, stream, track)

pytestmark = pytest.mark.gpu

PIN = 37
CASES = {"sac-hopper-64": ("sac-hopper", 64), "sac-hopper-40": ("sac-hopper", 40), "td3-halfcheetah-64": ("td3-halfcheetah", 64)}
E, S = _lib.EINVAL, _lib.ESTATE


def bare_engine(shape, B, cap, **cfg):
    """an engine whose parameters nobody reads: rings and draws only"""
    algo, dims, ln = SHAPES[shape]
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=ln, batch_size=B)
    return new_engine(hps, dims, rb_capacity=cap, max_envs=MAXN, seed=SEED, **cfg)


@functools.lru_cache(maxsize=None)
def some_rows(shape, n, seed, first=0):
    """n transitions on the host (torch, never written): every 7th flag done"""
    _, (o, a, bound), _ = SHAPES[shape]
    return rows(n, o, a, bound, seed, first)


def flat(five):
    """[n, o + a + 1 + o + 1] float32: one row per transition, for the cursor model"""
    obs, act, rew, nobs, done = [np.asarray(t) for t in five]
    n = obs.shape[0]
    return np.concatenate([obs, act, rew.reshape(n, 1), nobs, done.reshape(n, 1).astype(np.float32)], axis=1).astype(np.float32)


def ring_flat(eng, n):
    """slots [0, n) of the engine's ring through ReplayBuffer.rows, in flat()'s layout"""
    rb = agent_mod.ReplayBuffer(eng.cfg.rb_capacity)
    rb._bind(eng)
    d = rb.rows(np.arange(n))
    torch.cuda.synchronize()
    return np.concatenate([d[k].reshape(n, -1).float().cpu().numpy() for k in ("observations", "actions", "rewards", "next_observations", "dones")], axis=1)


def append(eng, path, five, keep):
    if path == "host":
        eng.rb_extend(*five)
    elif path == "records":                       # packed records in device memory (sactd3_rb_extend_device)
        rec = torch.from_numpy(eng.pack_records(*[np.asarray(t) for t in five])).to(DEV)
        torch.cuda.synchronize()
        eng.rb_extend_device(rec.data_ptr(), rec.shape[0])
        keep.append(rec)
    else:                                         # five device fields (sactd3_rb_extend_fields_device)
        dev = tuple(t.to(DEV) for t in five)
        fields, n, hold = fields_of(eng, dev)
        eng.rb_extend_fields_device(fields, n, stream())
        keep.append((dev, hold))


def pinned_engine(shape, B, cap, live, **cfg):
    """PIN prior rows, pinned, and `live` rows behind them"""
    eng = bare_engine(shape, B, cap, **cfg)
    eng.rb_extend(*some_rows(shape, PIN, 1))
    eng.rb_pin(PIN)
    if live:
        eng.rb_extend(*some_rows(shape, live, 2))
    return eng


# ------------------------------------------------------------------------------------------ 1. pinned appends
@pytest.mark.parametrize("cap", [64, PIN + 1], ids=["cap64", "live1"])
@pytest.mark.parametrize("path", ["host", "records", "fields"])
def test_pinned_appends_follow_the_cursor_model(path, cap):
    """20 appends of 4 rows, then one of 40 (more than the live region holds), through each append path: the ring equals the numpy
    cursor model bit for bit, slots [0, P) are untouched, len == cap, the cursor has passed P more than once"""
    shape = "sac-hopper"
    eng = bare_engine(shape, 64, cap)
    prior = some_rows(shape, PIN, 1)
    width = flat(prior).shape[1]
    model = mix_ref.PinnedRing(cap, width)
    eng.rb_extend(*prior)
    model.extend(flat(prior))
    assert eng.rb_pinned() == 0
    eng.rb_pin(PIN)
    model.pin(PIN)
    assert eng.rb_pinned() == PIN and eng.rb_len() == PIN
    keep = []
    for k in range(20):
        five = some_rows(shape, 4, 100 + k, 4 * k)
        append(eng, path, five, keep)
        model.extend(flat(five))
        assert eng.rb_len() == model.len
    big = some_rows(shape, 40, 77)
    append(eng, path, big, keep)
    model.extend(flat(big))
    got = ring_flat(eng, cap)
    assert same_bits(got, model.rows), np.flatnonzero((got.view(np.uint32) != model.rows.view(np.uint32)).any(axis=1))
    assert same_bits(got[:PIN], flat(prior))
    assert eng.rb_len() == cap == model.len and eng.rb_pinned() == PIN
    st = eng.mix_stats()
    assert st["pinned_wraps"] == model.wraps > 1 and st["mixed_draws"] == 0
    eng.sync()
    del keep


def test_pin_on_an_exactly_full_ring_and_unpin():
    shape = "sac-hopper"
    eng = bare_engine(shape, 64, 48)
    first = some_rows(shape, 48, 5)
    model = mix_ref.PinnedRing(48, flat(first).shape[1])
    eng.rb_extend(*first)                         # exactly full, nothing overwritten: the cursor stands at 0
    model.extend(flat(first))
    eng.rb_pin(PIN)
    model.pin(PIN)
    eng.rb_pin(20)                                # again, under the same conditions
    model.pin(20)
    five = some_rows(shape, 4, 6)
    eng.rb_extend(*five)
    model.extend(flat(five))
    assert same_bits(ring_flat(eng, 48), model.rows) and same_bits(ring_flat(eng, 48)[20:24], flat(five))
    assert eng.lib.sactd3_rb_pin(eng._h, 10) == S and eng.rb_pinned() == 20      # rows have been overwritten: no re-pin, no unpin
    eng.close()
    eng = bare_engine(shape, 64, 48)
    eng.rb_extend(*some_rows(shape, PIN, 1))
    eng.rb_pin(PIN)
    eng.rb_pin(0)                                 # unpin before anything wrapped: the plain ring again
    eng.rb_extend(*some_rows(shape, 11, 2))
    assert eng.rb_len() == 48 and eng.mix_stats()["pinned_wraps"] == 0
    eng.rb_extend(*five)
    assert same_bits(ring_flat(eng, 48)[:4], flat(five))


# ------------------------------------------------------------------------------------------ 2. the exact draw
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("live", [13, 1])
def test_mixed_draw_is_the_slot_formula_and_ticks_the_counter_once(case, live):
    shape, B = CASES[case]
    A, T = (pinned_engine(shape, B, 64, live) for _ in range(2))
    length = PIN + live
    ring = ring_flat(A, length)
    for ctr, m in enumerate((0, 1, B // 2, B - 1, B)):
        A.rb_set_mix(m)
        A.rb_sample_mixed()
        T.rb_sample()                             # the twin draws uniformly in the mixed draw's place
        b = A.read_batch()
        want = mix_ref.mixed_indices(SEED, ctr, B, m, PIN, length)
        assert np.array_equal(b["index"], want), (m, np.flatnonzero(b["index"] != want))
        assert same_bits(flat([b[k] for k in ("observations", "actions", "rewards", "next_observations", "dones")]), ring[want]), m
    assert A.mix_stats() == dict(mixed_draws=5, prior_rows_drawn=5 * B // 2, live_rows_drawn=5 * B // 2, pinned_wraps=0)
    for eng in (A, T):
        eng.rb_sample()
    assert_same_bits(A.read_batch(), T.read_batch(), what="the uniform sample behind five draws")      # the counter moved once per draw
    assert np.array_equal(A.read_batch()["index"], sample_indices(SEED, 5, B, length))


@pytest.mark.parametrize("case", sorted(CASES))
def test_mixed_draw_without_pinned_rows_is_rb_sample(case):
    shape, B = CASES[case]
    A, T = (bare_engine(shape, B, 64) for _ in range(2))
    for eng in (A, T):
        eng.rb_extend(*some_rows(shape, 50, 2))
    for _ in range(3):
        A.rb_sample_mixed()                       # P = 0, m = 0
        T.rb_sample()
        assert_same_bits(A.read_batch(), T.read_batch(), what="P = 0, m = 0")


def test_every_row_pinned_and_every_batch_row_prior():
    shape, B = CASES["sac-hopper-40"]
    eng = pinned_engine(shape, B, 64, 0)          # len == P
    eng.rb_set_mix(B)
    eng.rb_sample_mixed()
    assert np.array_equal(eng.read_batch()["index"], mix_ref.mixed_indices(SEED, 0, B, B, PIN, PIN))


# ------------------------------------------------------------------------------------------ 3. one launch equals the call sequence
def mixed_draw(m):
    """the mixed draw with m prior rows, as call_sequence takes it (the mix is set only when it changes)"""
    def draw(eng):
        if eng.mix_rows != m:
            eng.rb_set_mix(m)
            eng.mix_rows = m
        eng.rb_sample_mixed()
    return draw


def twins(case, cap, use_graphs=(True, True)):
    shape, B = CASES[case]
    _, engs, _ = shape_engines(shape, B=B, cap=cap, use_graphs=use_graphs)
    for eng in engs:
        eng.rb_extend(*some_rows(shape, PIN, 1))
        eng.rb_pin(PIN)
    return engs, shape, B


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_launch_equals_the_call_sequence(case):
    """7 iterations, 4 rows appended in front of each into a live region of 20 slots (the fifth fills it, the sixth overwrites), m from B/2 to B/4 half-way:
    the slot with its indices, the TD errors and the metrics after every iteration; at the end every parameter set, the Adam state,
    the counters, and one further uniform sample.  Two graph captures, whatever moved."""
    (A, Bt), shape, B = twins(case, PIN + 20)
    A.mix_rows = None
    for i in range(7):
        for eng in (A, Bt):
            eng.rb_extend(*some_rows(shape, 4, 200 + i, 4 * i))
        m = B // 2 if i < 3 else B // 4
        call_sequence(A, i % 3 == 0, mixed_draw(m), i + 1)
        Bt.step_sampled(i % 3 == 0, prior_rows=m)
        assert_same_bits(iteration_state(A), iteration_state(Bt), what=f"iteration {i}")
        idx = Bt.read_batch()["index"]
        assert np.array_equal(idx, mix_ref.mixed_indices(SEED, i, B, m, PIN, min(PIN + 4 * (i + 1), PIN + 20)))
    assert A.rb_len() == Bt.rb_len() == PIN + 20
    assert_same_state(A, Bt)
    want = dict(mixed_draws=7, prior_rows_drawn=3 * (B // 2) + 4 * (B // 4), live_rows_drawn=7 * B - 3 * (B // 2) - 4 * (B // 4), pinned_wraps=1)
    assert A.mix_stats() == Bt.mix_stats() == want
    for eng in (A, Bt):
        eng.rb_sample()
    assert_same_bits(A.read_batch(), Bt.read_batch(), what="a further uniform sample")
    assert Bt.step_sampled_stats() == dict(launches=7, graph_captures=2) and A.step_sampled_stats()["launches"] == 0
    nodes = [Bt.graph_kernel_count(16 + k) for k in range(4)]
    assert nodes[0] == nodes[2] == 0 and nodes[3] > nodes[1] > 4


# ------------------------------------------------------------------------------------------ 4. the eager form
def test_eager_form_equals_the_graph():
    """use_graphs = 0: the same launches issued one by one"""
    (G, Eg), shape, B = twins("sac-hopper-64", PIN + 20, use_graphs=(True, False))
    for i in range(6):
        for eng in (G, Eg):
            eng.rb_extend(*some_rows(shape, 4, 200 + i, 4 * i))
            eng.step_sampled(i % 3 == 0, prior_rows=B // 2 if i < 3 else B // 4)
        assert_same_bits(iteration_state(G), iteration_state(Eg), what=f"iteration {i}")
    assert_same_state(G, Eg)
    assert Eg.step_sampled_stats() == dict(launches=6, graph_captures=0) and G.step_sampled_stats()["graph_captures"] == 2
    assert G.mix_stats() == Eg.mix_stats()


# ------------------------------------------------------------------------------------------ 5. refusals
def ring_and_counters(eng):
    """what a pinned ring adds to an engine's state: every held row, the mix counters, the length and the pinned rows"""
    return dict(ring_flat=ring_flat(eng, eng.rb_len()) if eng.rb_len() else np.zeros(1, np.float32),
                mix_stats=np.float32(list(eng.mix_stats().values()) + [eng.rb_len(), eng.rb_pinned()]))


def test_refusals_change_nothing_and_leave_the_engine_usable():
    (eng,), shape, B = twins("sac-hopper-64", PIN + 20, use_graphs=(True,))
    eng.rb_extend(*some_rows(shape, 8, 2))        # 37 pinned + 8 live
    lib, h = eng.lib, eng._h
    M, U = _lib.DRAW_MIXED, _lib.DRAW_UNIFORM
    before = engine_state(eng, extra=ring_and_counters(eng))
    # sactd3_rb_pin: n out of range
    for n in (-1, PIN + 9, PIN + 20, 10 ** 12):
        assert lib.sactd3_rb_pin(h, n) == E, n
    # sactd3_rb_set_mix: outside [0, B]
    for m in (-1, B + 1):
        assert lib.sactd3_rb_set_mix(h, m) == E, m
    # out of scope while rows are pinned
    assert lib.sactd3_prio_enable(h, 0.6, 1e-6) == S
    assert lib.sactd3_rb_sample_nstep(h, 3, 4) == S and lib.sactd3_rb_sample_prioritized_nstep(h, 0.4, 3, 4) == S
    idx = torch.zeros(B, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert lib.sactd3_rb_sample_nstep_device(h, idx.data_ptr(), 1, None, 1, B, 3, 4, None, 0) == S
    assert raw_step(eng, 1, U, 3, 4, 0.0) == S and lib.sactd3_rb_fill_synthetic(h, 16, 0) == S
    # the mixed draw inside the one launch: n_step must be 1; beta is still checked
    assert raw_step(eng, 1, M, 2, 4, 0.0) == E and raw_step(eng, 1, M, 16, 1, 0.0) == E and raw_step(eng, 1, M, 1, 1, -1.0) == E
    assert_same_state(before, engine_state(eng, extra=ring_and_counters(eng)), what="refused calls on a pinned ring")
    # no live row: m < B is refused, by the call and by the one launch
    full = pinned_engine(shape, B, 64, 0)
    full.rb_set_mix(B - 1)
    assert full.lib.sactd3_rb_sample_mixed(full._h) == S and raw_step(full, 0, M, 1, 1, 0.0) == S
    # no pinned row: m > 0 is refused; an empty ring: everything is
    plain, empty = bare_engine(shape, B, 64), bare_engine(shape, B, 64)
    plain.rb_extend(*some_rows(shape, 8, 2))
    plain.rb_set_mix(1)
    assert plain.lib.sactd3_rb_sample_mixed(plain._h) == S and raw_step(plain, 0, M, 1, 1, 0.0) == S
    assert empty.lib.sactd3_rb_sample_mixed(empty._h) == S and raw_step(empty, 0, M, 1, 1, 0.0) == S
    assert empty.lib.sactd3_rb_pin(empty._h, 1) == E and empty.lib.sactd3_rb_pin(empty._h, 0) == 0
    # a ring that has wrapped, and one with priorities: no pin
    wrapped, prio = bare_engine(shape, B, 40), bare_engine(shape, B, 64)
    wrapped.rb_extend(*some_rows(shape, 48, 5))
    prio.rb_extend(*some_rows(shape, 8, 2))
    prio.prio_enable(0.6, 1e-6)
    assert wrapped.lib.sactd3_rb_pin(wrapped._h, 8) == S and prio.lib.sactd3_rb_pin(prio._h, 4) == S
    for e2 in (full, plain, empty, wrapped, prio):
        assert e2.mix_stats()["mixed_draws"] == 0 and e2.rb_pinned() == (PIN if e2 is full else 0)
    # ... and the refused engine runs a normal iteration, and a mixed one
    eng.step(True)
    eng.step_sampled(True, prior_rows=B // 2)
    assert not same_bits(eng.get_params(_lib.CRITICS), before["params.critics"])
    assert eng.mix_stats()["mixed_draws"] == 1 and eng.step_sampled_stats()["graph_captures"] == 1


# ------------------------------------------------------------------------------------------ 6. the untouched paths
def test_the_uniform_paths_do_not_notice_a_pinned_ring():
    """on a pinned ring whose live region has wrapped, rb_sample and step draw sample_indices(seed, ctr, B, len) as before"""
    (eng,), shape, B = twins("sac-hopper-64", PIN + 20, use_graphs=(True,))
    eng.rb_extend(*some_rows(shape, 31, 2))       # 20 live slots: wrapped
    length = eng.rb_len()
    assert length == PIN + 20 and eng.mix_stats()["pinned_wraps"] == 1
    ring = ring_flat(eng, length)
    eng.rb_sample()
    b = eng.read_batch()
    want = sample_indices(SEED, 0, B, length)
    assert np.array_equal(b["index"], want)
    assert same_bits(flat([b[k] for k in ("observations", "actions", "rewards", "next_observations", "dones")]), ring[want])
    eng.step(True)
    assert np.array_equal(eng.read_batch()["index"], sample_indices(SEED, 1, B, length))
    eng.step_sampled(False)                       # uniform, n_step 1: sactd3_step itself
    assert np.array_equal(eng.read_batch()["index"], sample_indices(SEED, 2, B, length))
    eng.rb_sample_with_indices(np.arange(B) % length)
    assert np.array_equal(eng.read_batch()["index"], np.arange(B) % length)
    assert eng.mix_stats()["mixed_draws"] == 0


# ------------------------------------------------------------------------------------------ 7. the loop
def test_train_one_launch_equals_the_call_by_call_loop():
    """12 segments of 4 envs on top of 40 pinned rows in a 64-slot ring (the live region wraps), half of every batch prior data, two
    updates per segment: one_launch=True gives the parameters and counters of the call sequence, bit for bit"""
    o, a, n = 11, 3, 4
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 8,
                             "num_timesteps": 12 * n - 1, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 64})
    obs, act, rew, nobs, done = [np.asarray(t) for t in rows(40, o, a, 1.0, 8)]
    data = dict(observations=obs, actions=act, rewards=rew, next_observations=nobs, terminations=done)
    res = []
    for one_launch in (False, True):
        env = loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5)
        env.action_space.seed(0)
        torch.manual_seed(0)
        np.random.seed(0)
        agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                        torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
        assert loop.load_dataset(agent, data, pin=True) == 40 and agent.rb.pinned == 40
        loop.train(cfg, env, agent, fused=False, prior_fraction=0.5, updates_per_step=2, one_launch=one_launch)
        eng = track(agent.engine)
        res.append(engine_state(eng, extra=dict(
            ring_and_counters(eng),
            counters=np.float32([agent.qnet_updates_so_far, agent.actor_updates_so_far, agent.timesteps_so_far, len(agent.rb)]))))
        assert agent.qnet_updates_so_far == 20 and len(agent.rb) == 64 and agent.rb.pinned == 40
        assert eng.mix_stats() == dict(mixed_draws=20, prior_rows_drawn=20 * 32, live_rows_drawn=20 * 32, pinned_wraps=2)
        launches = eng.step_sampled_stats()
        assert launches["launches"] == (20 if one_launch else 0) and launches["graph_captures"] <= 2
        eng.close()
    assert_same_state(res[0], res[1], what="one_launch against the call sequence")
