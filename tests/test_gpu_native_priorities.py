"""GPU: proportional prioritised replay as engine state (include/sactd3.h: sactd3_prio_enable, sactd3_rb_sample_prioritized,
sactd3_prio_set_uniforms, sactd3_prio_update_from_td, sactd3_prio_update_device, sactd3_prio_stats) against the numpy restatement of
tests/priorities_ref.py and against twin engines.

Engines are shape_engines() of tests/gpu_support.py (the oracle's perturbed parameters), the critic site's noise injected, with a
5000-slot ring that holds 2500 rows: two whole groups of 1024 leaves, a partial third, unfilled slots behind it, two empty groups.
Shapes: SAC Hopper at B = 64 and B = 40, TD3 HalfCheetah at B = 64, SAC Hopper at B = 1024 (the weights kernel's loop, 1024 draw and
write-back workgroups)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import priorities_ref as pref
from tests.gpu_support import (BOUND_REL, CAP, DEV, HELD, PRIO_CASES as CASES, SEED, P, _lib, assert_same_bits, assert_same_state,  # noqa: F401
                               boundary_uniforms, close_engines, cuda, extend_device, integer_priorities, loop, ring_rows, same_bits, shape_engines,
                               slot, stage, td_of, track, upload_priorities)
from tests.helpers import observe

pytestmark = pytest.mark.gpu

ALL = list(CASES)
U24 = 2.0 ** -24


def build(case, count, enable=(1.0, 1e-6)):
    """`count` twin engines: same parameters, the same 2500 rows in a 5000-slot ring, the same injected critic noise; priorities
    enabled with `enable` = (alpha, eps) unless None"""
    shape, B = CASES[case]
    _, engs, (o, a, bound) = shape_engines(shape, count, B=B, cap=CAP)
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for eng in engs:
        eng.rb_extend(*[t.numpy() for t in ring_rows(shape)])
        eng.set_noise(_lib.SITE_CRITIC, eps)
        if enable is not None:
            eng.prio_enable(*enable)
    return engs, (o, a, bound), B


def drawn(eng):
    return eng.read_batch()["index"]


def assert_sums_consistent(eng, what=""):
    """the group sums against float64 sums of the leaves read back: within 1024 * 2^-24 relative, the bound of any summation order of
    1024 non-negative float32 terms"""
    leaf, sums = eng.debug_read("prio_leaf"), eng.debug_read("prio_sums")
    want = pref.group_sums(leaf)
    assert sums.shape == want.shape == ((CAP + pref.GROUP - 1) // pref.GROUP,)
    assert (np.abs(sums - want) <= pref.GROUP * U24 * want).all(), (what, sums, want)
    return leaf, sums


# ------------------------------------------------------------------------------------------ 1. exact selection, injected uniforms
@pytest.mark.parametrize("case", ALL)
def test_injected_uniforms_select_exactly_the_restatements_slots(case):
    (eng,), _, B = build(case, 1)
    prio = integer_priorities()
    keep = upload_priorities(eng, np.arange(HELD), prio)
    leaf = eng.debug_read("prio_leaf")
    assert np.array_equal(leaf[:HELD], prio) and not leaf[HELD:].any()          # alpha == 1: the priority itself
    T = float(leaf.sum())
    assert T < 4096
    u = boundary_uniforms(B)
    eng.prio_set_uniforms(u)
    eng.rb_sample_prioritized(0.4)
    got, want = drawn(eng), pref.select(leaf, HELD, u)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert (got >= 0).all() and (got < HELD).all() and (prio[got] > 0).all()
    on_boundary = (u.astype(np.float64) * T) % 1 == 0
    assert on_boundary.sum() >= B // 2 - 8 and got[0] == 1 and got[1] == HELD - 2      # u = 0 skips the zero at slot 0; the largest skips the last
    eng.prio_set_uniforms(None)
    assert eng.prio_stats() == dict(samples=1, write_backs=1, rows_refused=0, rows_entered_at_max=HELD)
    del keep


# ------------------------------------------------------------------------------------------ 2. exact selection, native draws
@pytest.mark.parametrize("case", ALL)
def test_native_draws_follow_the_philox_stream_and_leave_the_uniform_sampler_alone(case):
    (A, Bt, N), _, B = build(case, 3)
    prio = integer_priorities()
    keep = [upload_priorities(e, np.arange(HELD), prio) for e in (A, Bt)]
    leaf = A.debug_read("prio_leaf")
    for ctr in range(3):                                            # the draw counter advances once per call
        A.rb_sample_prioritized(0.4)
        Bt.rb_sample_prioritized(0.4)
        want = pref.select(leaf, HELD, pref.native_uniforms(SEED, ctr, B))
        assert np.array_equal(drawn(A), want), (ctr, np.flatnonzero(drawn(A) != want))
        assert_same_bits(slot(A), slot(Bt), what=f"twin, call {ctr}")
    A.rb_sample()                                                   # the uniform sampler's counter was not consumed
    N.rb_sample()
    assert_same_bits(slot(A), slot(N), what="uniform sample behind three prioritised ones")
    del keep


# ------------------------------------------------------------------------------------------ 3. the slot is what index staging leaves
@pytest.mark.parametrize("case", ALL)
def test_the_slot_is_what_index_staging_leaves(case):
    (D, H), _, B = build(case, 2)
    keep = upload_priorities(D, np.arange(HELD), integer_priorities())
    D.rb_sample_prioritized(0.4)
    idx = drawn(D)
    keep2 = stage(H, idx)
    assert_same_bits(slot(D), slot(H), what="prioritised sample against rb_sample_indices_device")
    D.update_qnets()
    H.rb_sample()
    H.update_qnets()
    assert D.graph_kernel_count(8) == H.graph_kernel_count(0) > 0 and D.graph_kernel_count(0) == 0      # the weighted graph, the plain count
    del keep, keep2


# ------------------------------------------------------------------------------------------ 4. weights
def float_priorities(seed=21):
    return np.random.default_rng(seed).uniform(0.1, 1.0, HELD).astype(np.float32)


@pytest.mark.parametrize("case", ALL)
def test_importance_weights(case):
    """general float priorities, alpha = 0.6; beta 0: all exactly 1; every batch's largest weight exactly 1; otherwise the float64
    restatement on the leaves read back and the slots actually drawn, within BOUND_REL["weights"]"""
    (eng,), _, B = build(case, 1, enable=(0.6, 1e-6))
    keep = upload_priorities(eng, np.arange(HELD), float_priorities())
    leaf = eng.debug_read("prio_leaf")
    worst = 0.0
    for beta in (0.0, 0.4, 1.0):
        eng.rb_sample_prioritized(beta)
        idx = drawn(eng)
        w = weights_of(eng, B)
        assert (idx >= 0).all() and (idx < HELD).all() and w.max() == 1.0
        if beta == 0.0:
            assert (w == 1.0).all()
            continue
        want = pref.weights(leaf, HELD, idx, beta)
        rel = float((np.abs(w - want) / want).max())
        worst = max(worst, rel)
        print(f"weights[{case}] beta {beta}: max relative delta {rel:.3e}")
        observe("native_priorities_weights", f"{case} beta {beta}: max relative delta", rel)
        assert rel <= BOUND_REL["weights"], (beta, rel)
    del keep


def weights_of(eng, B):
    """the loss weights batch slot 0 carries (debug_read "prio_weights")"""
    w = eng.debug_read("prio_weights")
    assert w.shape == (B,)
    return w


# ------------------------------------------------------------------------------------------ 5. distribution
def test_draws_follow_the_priorities():
    """16 priority classes over the 2500 rows (row i in class i % 16, priority 0.2 + 0.1 class, alpha 0.6), 200 native calls at B = 64
    pooled by class: Pearson's chi-square against class mass / total at the 1 - 1e-6 quantile of chi-square(15).  The smallest
    expected count is 12800 * 0.38 / 15.3 > 300.  The restatement fed with the same Philox uniforms passes the same test (checked here, on
    the host); the run is deterministic."""
    (eng,), _, B = build("sac-hopper-64", 1, enable=(0.6, 1e-6))
    cls = np.arange(HELD) % 16
    keep = upload_priorities(eng, np.arange(HELD), (0.2 + 0.1 * cls).astype(np.float32))
    leaf = eng.debug_read("prio_leaf")
    mass = np.array([leaf[:HELD][cls == c].astype(np.float64).sum() for c in range(16)])
    calls = 200
    expect = calls * B * mass / mass.sum()
    assert expect.min() >= 20
    got, ref = np.zeros(16), np.zeros(16)
    for ctr in range(calls):
        eng.rb_sample_prioritized(0.4)
        idx = drawn(eng)
        assert (idx >= 0).all() and (idx < HELD).all()
        got += np.bincount(cls[idx], minlength=16)
        ref += np.bincount(cls[pref.select(leaf, HELD, pref.native_uniforms(SEED, ctr, B))], minlength=16)
    crit = pref.chi2_quantile(15, 1 - 1e-6)
    chi_dev, chi_ref = float(((got - expect) ** 2 / expect).sum()), float(((ref - expect) ** 2 / expect).sum())
    print(f"chi-square(15): device {chi_dev:.2f}, restatement {chi_ref:.2f}, critical {crit:.2f}")
    assert chi_ref < crit and chi_dev < crit, (chi_dev, chi_ref, crit)
    assert eng.prio_stats()["samples"] == calls
    del keep


# ------------------------------------------------------------------------------------------ 6. write-back from the TD errors
@pytest.mark.parametrize("case", ALL)
def test_write_back_from_td_errors(case):
    eps = 1e-6
    (E1, E6), _, B = build(case, 2, enable=None)
    E1.prio_enable(1.0, eps)
    E6.prio_enable(0.6, eps)
    for eng, alpha in ((E1, 1.0), (E6, 0.6)):
        eng.rb_sample_prioritized(0.4)
        with pytest.raises(P.EngineError, match="-3"):             # no critic update has run on these rows yet
            eng.prio_update_from_td()
        before = eng.debug_read("prio_leaf")
        assert (before[:HELD] == 1.0).all() and not before[HELD:].any()
        idx = drawn(eng)
        eng.update_qnets()
        td = td_of(eng)
        eng.prio_update_from_td()
        leaf = eng.debug_read("prio_leaf")
        p32 = np.abs(td).max(0).astype(np.float32) + np.float32(eps)
        touched = np.zeros(CAP, bool)
        touched[idx] = True
        assert np.array_equal(leaf[~touched], before[~touched])    # untouched leaves are unchanged
        if alpha == 1.0:                                            # bit for bit; where a slot repeats, the highest batch position wins
            want = before.copy()
            for b in range(B):
                want[idx[b]] = p32[b]
            assert same_bits(leaf, want), np.flatnonzero(leaf != want)
        else:
            want = pref.write_back(before, idx, pref.td_priorities(td, eps), alpha)
            rel = float((np.abs(leaf[touched] - want[touched]) / want[touched]).max())
            print(f"leaves[{case}] alpha {alpha}: max relative delta {rel:.3e}")
            observe("native_priorities_leaves", f"{case}: max relative delta", rel)
            assert rel <= BOUND_REL["leaves"], rel
        assert eng.debug_read("prio_max")[0] == max(np.float32(1.0), p32.max())
        assert_sums_consistent(eng, f"alpha {alpha}")
        eng.rb_sample()                                             # a refill of the slot: its TD errors are gone
        with pytest.raises(P.EngineError, match="-3"):
            eng.prio_update_from_td()
        assert eng.prio_stats() == dict(samples=1, write_backs=1, rows_refused=0, rows_entered_at_max=HELD)


# ------------------------------------------------------------------------------------------ 7. duplicates and refused rows
def test_duplicates_resolve_by_batch_position_and_bad_rows_are_refused():
    engs, _, B = build("sac-hopper-64", 3, enable=(0.6, 1e-6))
    rng = np.random.default_rng(31)
    idx = rng.integers(0, HELD, 64)
    prio = rng.uniform(0.1, 2.0, 64).astype(np.float32)
    idx[[3, 10, 50]] = 7                                            # one slot at three positions with three priorities
    idx[[0, 63]] = 1030                                             # ... and one at both ends of the batch
    prio[[3, 10, 50]] = [0.5, 1.75, 0.25]
    keeps = [upload_priorities(e, idx, prio) for e in engs]
    leaves = [e.debug_read("prio_leaf") for e in engs]
    sums = [e.debug_read("prio_sums") for e in engs]
    for k in (1, 2):
        assert same_bits(leaves[0], leaves[k]) and same_bits(sums[0], sums[k])
    want = pref.write_back(np.where(np.arange(CAP) < HELD, 1.0, 0.0), idx, prio, 0.6)
    assert np.allclose(leaves[0], want, rtol=1e-6, atol=0)
    assert abs(leaves[0][7] - 0.25 ** 0.6) < 1e-6 and abs(leaves[0][1030] - float(prio[63]) ** 0.6) < 1e-6      # the highest position won
    E = engs[0]
    before, max_before = leaves[0], E.debug_read("prio_max")[0]
    assert max_before == max(np.float32(1.0), prio.max())
    # refused rows between good ones: bad priorities on valid slots, good priorities on bad slots
    bad_idx = np.array([100, 101, 102, -1, HELD, 2 ** 40, 200, 201], np.int64)
    bad_prio = np.array([-1.0, np.nan, np.inf, 0.5, 0.5, 0.5, 0.75, 0.0], np.float32)
    keep = upload_priorities(E, bad_idx, bad_prio)
    leaf = E.debug_read("prio_leaf")
    want = before.copy()
    want[200], want[201] = np.float32(0.75) ** np.float32(0.6), 0.0                    # (0 excludes the row)
    assert np.array_equal(leaf[[100, 101, 102]], before[[100, 101, 102]]) and not leaf[HELD:].any()
    assert np.allclose(leaf, want, rtol=1e-6, atol=0) and leaf[201] == 0.0
    assert E.debug_read("prio_max")[0] == max_before
    assert E.prio_stats() == dict(samples=0, write_backs=2, rows_refused=6, rows_entered_at_max=HELD)
    assert_sums_consistent(E)
    for _ in range(3):                                              # the engine stays usable, and finite
        E.rb_sample_prioritized(0.4)
        got = drawn(E)
        assert (got >= 0).all() and (got < HELD).all() and 201 not in got
        E.update_qnets()
        E.prio_update_from_td()
    assert np.isfinite(list(E.read_metrics().values())).all() and np.isfinite(E.debug_read("prio_leaf")).all()
    assert E.priority_stats()["rows_refused"] == 0
    del keeps, keep


def test_nothing_to_draw_from_is_refused_rows_not_a_fault():
    (eng,), _, B = build("sac-hopper-64", 1)
    keep = upload_priorities(eng, np.arange(HELD), np.zeros(HELD, np.float32))
    eng.rb_sample_prioritized(0.4)
    assert (drawn(eng) == -1).all() and not eng.debug_read("X").any()
    assert eng.priority_stats()["rows_refused"] == B                # stored as refused rows by the staging kernel, and counted
    eng.update_qnets()
    assert np.isfinite(list(eng.read_metrics().values())).all()
    del keep


# ------------------------------------------------------------------------------------------ 8. the sums never drift
def test_sums_depend_on_the_leaves_not_on_the_history():
    (A, Bt), _, B = build("sac-hopper-64", 2, enable=(0.6, 1e-6))
    rng = np.random.default_rng(41)
    final = {}
    keep = []
    for k in range(20):                                             # 20 overlapping write-backs of 64 rows over 400 slots around a group boundary
        idx = rng.integers(800, 1200, 64)
        prio = rng.uniform(0.05, 3.0, 64).astype(np.float32)
        keep.append(upload_priorities(A, idx, prio))
        for s, p in zip(idx, prio):
            final[int(s)] = p
    slots = np.array(sorted(final), np.int64)
    keep.append(upload_priorities(Bt, slots, np.array([final[int(s)] for s in slots], np.float32)))      # ... and the same leaves in one
    la, lb = A.debug_read("prio_leaf"), Bt.debug_read("prio_leaf")
    assert same_bits(la, lb) and len(slots) > 300
    assert same_bits(A.debug_read("prio_sums"), Bt.debug_read("prio_sums"))
    assert_sums_consistent(A)
    assert A.prio_stats()["write_backs"] == 20 and Bt.prio_stats()["write_backs"] == 1
    del keep


# ------------------------------------------------------------------------------------------ 9. appends
def test_every_append_path_enters_rows_at_the_maximum_priority():
    shape = "sac-hopper"
    (eng,), (o, a, bound), B = build("sac-hopper-64", 1, enable=None)
    eng.prio_enable(0.6, 1e-6)                                      # on a ring that holds rows: they enter at priority 1
    leaf = eng.debug_read("prio_leaf")
    assert (leaf[:HELD] == 1.0).all() and not leaf[HELD:].any() and eng.prio_stats()["rows_entered_at_max"] == HELD
    p0 = np.zeros(HELD, np.float32)
    p0[0] = 3.0                                                     # the running maximum becomes 3; nothing else can be drawn
    keep = [upload_priorities(eng, np.arange(HELD), p0)]
    fresh = float(np.float32(3.0) ** np.float32(0.6))
    entered, length = HELD, HELD

    def check(lo, hi, what):
        leaf, _ = assert_sums_consistent(eng, what)
        span = np.arange(lo, hi) % CAP
        assert (leaf[span] == leaf[span[0]]).all() and abs(leaf[span[0]] - fresh) <= 2e-7 * fresh, what
        assert not leaf[length:].any() and eng.prio_stats()["rows_entered_at_max"] == entered, what
        return leaf

    five = ring_rows(shape, 300, 51)
    eng.rb_extend(*[t.numpy() for t in five])                       # 1. host arrays: slots 2500 .. 2799
    entered, length = entered + 300, length + 300
    leaf = check(2500, 2800, "rb_extend")
    assert leaf[0] == leaf[2500] and not leaf[1:HELD].any()
    eng.rb_sample_prioritized(0.4)                                  # a freshly appended row is drawable at once
    got = drawn(eng)
    assert np.isin(got, np.r_[0, 2500:2800]).all() and (got >= 2500).sum() > B // 2
    rec = torch.as_tensor(eng.pack_records(*[t.numpy() for t in ring_rows(shape, 200, 52)]), device=DEV)
    eng.rb_extend_device(rec.data_ptr(), 200)                       # 2. packed device records: 2800 .. 2999
    entered, length = entered + 200, length + 200
    check(2800, 3000, "rb_extend_device")
    extend_device(eng, cuda(ring_rows(shape, 100, 53)))             # 3. device fields: 3000 .. 3099
    entered, length = entered + 100, length + 100
    check(3000, 3100, "rb_extend_fields_device")
    eng.rb_extend(*[t.numpy() for t in ring_rows(shape, 2000, 54)])                   # 4. across the wrap: 3100 .. 4999, 0 .. 99
    entered, length = entered + 2000, CAP
    leaf = check(3100, 5100, "rb_extend across the wrap")
    assert not leaf[100:HELD].any() and eng.rb_len() == CAP
    extend_device(eng, cuda(ring_rows(shape, 1000, 55)))            # ... and device fields across a group boundary: 100 .. 1099
    entered += 1000
    leaf = check(100, 1100, "rb_extend_fields_device over a group boundary")
    assert not leaf[1100:HELD].any()
    eng.rb_fill_synthetic(1300, 5)                                  # 5. the synthetic fill: rows 0 .. 1299
    entered += 1300
    leaf = check(0, 1300, "rb_fill_synthetic")
    assert not leaf[1300:HELD].any() and (leaf[HELD:] == leaf[0]).all()
    del keep, rec


# ------------------------------------------------------------------------------------------ 10. invisible when off, harmless when on
def test_priorities_do_not_change_what_the_other_paths_compute():
    """the same sequence (extend, single steps, chained periods, update_qnets, predict) on an engine that never enables priorities and on
    one that does -- and writes priorities back between two chained periods: parameters, Adam state, metrics, sampled slots, actions
    and graphs are the same"""
    (N, E), (o, a, bound), B = build("sac-hopper-64", 2, enable=None)
    E.prio_enable(0.6, 1e-6)
    res, keep = [], []
    for eng in (N, E):
        eng.rb_extend(*[t.numpy() for t in ring_rows("sac-hopper", 8, 61)])
        eng.step(True)
        eng.step(False)
        it = eng.run_iterations(0, 3)
        if eng is E:                                                # behind a period that left the next one's opening pair precomputed
            keep.append(upload_priorities(E, np.arange(64), np.linspace(0.1, 2.0, 64)))
        it = eng.run_iterations(it, 3)
        samples = eng.read_batch()["index"]
        eng.rb_sample()
        eng.update_qnets()
        act = eng.predict(ring_rows("sac-hopper")[0][:4].numpy(), True)
        res.append((samples, act, [eng.graph_kernel_count(w) for w in range(9)]))
    assert_same_state(N, E)
    assert np.array_equal(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    assert E.prio_stats() == dict(samples=0, write_backs=1, rows_refused=0, rows_entered_at_max=HELD + 8)
    assert N.prio_stats() == dict(samples=0, write_backs=0, rows_refused=0, rows_entered_at_max=0)
    with pytest.raises(P.EngineError, match="-3"):                 # never enabled
        N.rb_sample_prioritized(0.4)
    with pytest.raises(P.EngineError, match="-3"):
        N.debug_read("prio_leaf")
    del keep


def test_write_back_behind_a_cut_short_period_goes_to_the_rows_it_trained_on():
    """run_iterations(0, 4) at delay 2 is a period, then step_prefix(1) on the opening pair that period left in batch slot 3: the
    write-back behind it takes that slot's ring rows, as behind four single steps -- not the stale rows of slot 0.  SAC Hopper, B = 64,
    3000 rows held, native draws."""
    _, (P4, S4), _ = shape_engines("sac-hopper", 2, B=64, cap=CAP)
    for eng in (P4, S4):
        eng.rb_extend(*[t.numpy() for t in ring_rows("sac-hopper", 3000)])
        eng.prio_enable(1.0, 1e-6)
    before = S4.debug_read("prio_leaf")
    assert P4.run_iterations(0, 4) == 4
    for i in range(4):
        S4.step(i % 3 == 0)
    for eng in (P4, S4):
        eng.prio_update_from_td()
    got, want, rows = P4.debug_read("prio_leaf"), S4.debug_read("prio_leaf"), S4.read_batch()["index"]
    assert np.array_equal(np.flatnonzero(want.view(np.uint32) != before.view(np.uint32)), np.unique(rows))      # (|TD| + eps is never exactly 1)
    assert same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert same_bits(P4.debug_read("prio_sums"), S4.debug_read("prio_sums")) and np.array_equal(P4.read_batch()["index"], rows)


def test_bad_arguments_are_refused_and_leave_the_engine_usable():
    (eng,), _, B = build("sac-hopper-64", 1, enable=None)
    lib, h = eng.lib, eng._h
    for alpha, eps in ((-0.1, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (0.6, 0.0), (0.6, -1.0), (0.6, float("nan"))):
        assert lib.sactd3_prio_enable(h, alpha, eps) == _lib.EINVAL
    assert lib.sactd3_prio_set_uniforms(h, None, 0) == _lib.ESTATE and lib.sactd3_prio_update_from_td(h) == _lib.ESTATE
    eng.prio_enable(0.6, 1e-6)
    eng.prio_enable(0.6, 1e-6)                                      # the same values again: nothing happens
    assert lib.sactd3_prio_enable(h, 0.7, 1e-6) == _lib.ESTATE
    idx, prio = torch.arange(B, device=DEV), torch.ones(B, device=DEV)
    host_i, host_p = np.arange(B, dtype=np.int64), np.ones(B, np.float32)
    vp = lambda t: t.data_ptr()
    call = lambda i, il, p, pl, n, fl: lib.sactd3_prio_update_device(h, i, il, p, pl, n, None, fl)
    assert call(host_i.ctypes.data, 1, vp(prio), 1, B, 0) == _lib.EINVAL                # host pointers
    assert call(vp(idx), 1, host_p.ctypes.data, 1, B, 0) == _lib.EINVAL
    assert call(None, 1, vp(prio), 1, B, 0) == _lib.EINVAL and call(vp(idx), 1, None, 1, B, 0) == _lib.EINVAL
    assert call(vp(idx), 1, vp(prio), 1, 0, 0) == _lib.EINVAL                           # n < 1
    assert call(vp(idx), 0, vp(prio), 1, B, 0) == _lib.EINVAL and call(vp(idx), 1, vp(prio), 0, B, 0) == _lib.EINVAL
    assert call(vp(idx), 1, vp(prio), 1, B, 2) == _lib.EINVAL                           # an unknown flag
    assert lib.sactd3_rb_sample_prioritized(h, -0.5) == _lib.EINVAL and lib.sactd3_rb_sample_prioritized(h, float("nan")) == _lib.EINVAL
    assert lib.sactd3_prio_set_uniforms(h, host_p.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), B - 1) == _lib.EINVAL
    torch.cuda.synchronize()
    assert call(vp(idx), 1, vp(prio), 1, B, 0) == 0                                     # the next call works
    eng.rb_sample_prioritized(0.4)
    eng.update_qnets()
    eng.prio_update_from_td()
    assert eng.prio_stats() == dict(samples=1, write_backs=2, rows_refused=0, rows_entered_at_max=HELD)
    assert eng.time_kernel("prio_sample", 5) > 0 and eng.time_kernel("prio_update", 5) > 0


# ------------------------------------------------------------------------------------------ 11. end to end
def test_train_with_engine_owned_priorities():
    """loop.train(fused=False, prioritized=...) on SyntheticVecEnv: finite losses, one sample and one write-back per iteration, and the
    only ring length there is is the engine's"""
    o, a, n, iters = 11, 3, 4, 60
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 200 + iters * n - 1, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 1000})
    env = loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5)
    env.action_space.seed(0)
    torch.manual_seed(0)
    agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                    torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
    with pytest.raises(ValueError, match="fused=False"):
        loop.train(cfg, env, agent, fused=True, prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6))
    metrics = loop.train(cfg, env, agent, fused=False, prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6))
    eng = track(agent.engine)
    assert all(np.isfinite(v) for v in metrics.values()), metrics
    updates = agent.qnet_updates_so_far
    assert updates >= iters
    held = len(agent.rb)
    assert eng.prio_stats() == dict(samples=updates, write_backs=updates, rows_refused=0, rows_entered_at_max=held)
    assert eng.priority_stats()["rows_refused"] == 0 and held == eng.rb_len() > 200
    leaf = eng.debug_read("prio_leaf")
    assert (leaf[:held] > 0).all() and np.isfinite(leaf).all() and not leaf[held:].any()
    assert eng.debug_read("prio_max")[0] >= 1.0 and len(np.unique(leaf[:held])) > iters      # the write-backs moved them
