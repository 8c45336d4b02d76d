"""GPU: the engine-owned priority table at full ring sizes (csrc/prio_kernels.h) against tests/prio_model.py, its restatement in
numpy float32 -- bit for bit: group sums, drawn slots, leaves and sums behind appends and write-backs -- and, independently of that
model, every drawn slot against the a-priori float64 interval of tests/bounds.py:prio_draw_interval.  Both are kept: a reading
of the kernel that model and test share cannot hide a draw from the wrong group from the float64 running sums.

Rings, leaves and uniforms are the case table of tests/prio_model.py (tests/test_prio_model.py shows on the CPU that they take the leaf fall-back, the
group fall-back in either chunk, the second top-level chunk and uniforms whose m is a running sum): one group; one group and a
leaf; the reference's 1 000 000 slots (977 groups); 1 050 076 slots with 1 050 039 held (1026 groups: two chunks, the last group
partly filled); 1 100 000 slots (1075 groups: the group fall-back inside the second chunk).  SAC Hopper, B = 64; the rings are
filled on the device (rb_fill_synthetic), priorities enabled with alpha = 1 -- no powf between a priority and its leaf.

Filling: EVERY leaf is written, by prio_update_device in calls of 8192 rows.  On an MI355X the 129 calls of the 1 050 039-row ring
took 0.045 s together (123 calls for 1 000 000 rows: 0.043 s; printed by every test and recorded through helpers.observe), so no
group is left at the entry priority; a whole test takes 0.1 to 0.3 s."""
import time

import numpy as np
import pytest
import torch

from tests import bounds
from tests import priorities_ref as pref
from tests import prio_model as pm
from tests.gpu_support import (BOUND_REL, DEV, SEED, SHAPES, _lib, call_sequence, close_engines, cuda, extend_device, same_bits,  # noqa: F401
                               sampled_draw, shape_engines, stream, td_of)
from tests.helpers import observe, synth_transitions

pytestmark = pytest.mark.gpu

SHAPE, B, EPS, BETA = "sac-hopper", 64, 1e-6, 0.4
CALL_ROWS = 8192
F32, G = np.float32, pm.G
BIG = (1_050_076, 1_050_039)
RINGS = [r + (fill,) for r in ((1024, 1024), (1025, 1025), (1_000_000, 1_000_000), BIG) for fill in pm.FILLS]
RINGS += [(1_100_000, 1_100_000, "uniform"), (1_100_000, 1_100_000, "spike")]
GROUPS = {1024: 1, 1025: 2, 1_000_000: 977, 1_050_076: 1026, 1_100_000: 1075}


def write_chunked(eng, idx, prio):
    """prio_update_device on device tensors, at most CALL_ROWS rows a call (one workgroup per row walks all rows of its call)"""
    for lo in range(0, idx.shape[0], CALL_ROWS):
        n = min(CALL_ROWS, idx.shape[0] - lo)
        eng.prio_update_device(idx[lo:].data_ptr(), 1, prio[lo:].data_ptr(), 1, n, stream())


def ring(cap, held, fill, count=1, alpha=1.0):
    """`count` twin engines whose ring holds `held` synthetic rows and whose priorities are the leaves of the CPU case (alpha == 1: its
    leaves); -> (engines, case, the model's table for the leaves read back)"""
    k = pm.case(cap, held, fill)
    _, engs, (o, a, bound) = shape_engines(SHAPE, count, B=B, cap=cap)
    noise = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    idx, prio = torch.arange(held, device=DEV), torch.as_tensor(k.leaf.copy(), device=DEV)
    for eng in engs:
        eng.rb_fill_synthetic(held, 5)
        eng.set_noise(_lib.SITE_CRITIC, noise)
        eng.prio_enable(alpha, EPS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        write_chunked(eng, idx, prio)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"{cap}-{held}-{fill}: {(held + CALL_ROWS - 1) // CALL_ROWS} prio_update_device calls wrote {held} leaves in {dt:.4f} s")
        observe("prio_scale_leaf_write_seconds", f"{cap}-{held}", dt)
    return engs, k, table_of(engs[0], cap)


def table_of(eng, cap):
    """the model's table for the leaves the engine holds now (read back): its leaves, and the sums they have to have"""
    leaf = eng.debug_read("prio_leaf")
    assert leaf.shape == (cap,)
    return pm.table(leaf, cap)


def assert_table(eng, t, what):
    """leaves and sums of the engine are the table's, as uint32"""
    leaf, sums = eng.debug_read("prio_leaf"), eng.debug_read("prio_sums")
    assert sums.shape == (t.ngroups,) and same_bits(leaf, t.leaf[:t.capacity]), (what, np.flatnonzero(leaf != t.leaf[:t.capacity])[:8])
    bad = np.flatnonzero(sums.view(np.uint32) != t.sums[:t.ngroups].view(np.uint32))
    assert bad.size == 0, (what, bad[:8], sums[bad[:8]], t.sums[bad[:8]])


def draw(eng, u):
    """64 injected uniforms -> the slots drawn"""
    eng.prio_set_uniforms(u)
    eng.rb_sample_prioritized(BETA)
    return eng.read_batch()["index"]


def batches(u):
    """the uniforms in calls of 64, the last one filled up with random ones"""
    pad = (-len(u)) % B
    u = np.minimum(np.concatenate([u, np.random.default_rng(3).random(pad).astype(F32)]), pm.U_MAX)
    return u.reshape(-1, B)


def into_groups(t, C, groups, n=B):
    """n uniforms whose m falls inside the given groups, well away from their edges; every fourth repeats its neighbour (the same slot twice)"""
    T = float(pm.draw(t, t.capacity, 0.0)[1])
    out = []
    for i in range(n):
        g = groups[i % len(groups)]
        lo, hi = (C[g * G - 1] if g else 0.0), C[min((g + 1) * G, len(C)) - 1]
        out.append((lo + (hi - lo) * (0.05 + 0.9 * ((i // len(groups)) + 0.5) / (n // len(groups) + 1))) / T)
    u = np.array(out, F32)
    u[3::4] = u[2::4]
    return u


# ------------------------------------------------------------------------------------------ 1. sums, draws, weights per ring
@pytest.mark.parametrize("cap,held,fill", RINGS, ids=[pm.case_id(r) for r in RINGS])
def test_sums_and_draws_have_the_models_bits_and_lie_in_the_float64_interval(cap, held, fill):
    """prio_sums equal the model's sums of the leaves read back as uint32; the CPU case's directed uniforms, 64 a call, and one native
    call draw exactly the model's slots; each slot lies in its float64 interval for m = fl32(u T), T the total the model predicts (the
    engine exposes none); the weights have their maximum exactly 1 and match float64 within BOUND_REL["weights"]; no row is refused"""
    (eng,), k, t = ring(cap, held, fill)
    assert same_bits(t.leaf[:held], k.leaf) and not t.leaf[held:].any()      # alpha == 1: the leaf is the priority written
    assert (t.ngroups, t.nch) == (GROUPS[cap], 1 if cap <= G * G else 2) and len(eng.debug_read("prio_sums")) == GROUPS[cap]
    assert_table(eng, t, "after the leaf writes")                            # the fixed order of prio_scan: no tolerance
    C = np.cumsum(t.leaf[:held].astype(np.float64))
    worst_iv = worst_w = 0.0
    slots, T, m, paths = pm.draws(t, held, k.u)
    assert np.array_equal(slots, k.slots)                                    # (the CPU case: its fall-back draws are among these)
    observe("prio_draw_interval_model", pm.case_id((cap, held, fill)), bounds.prio_draw_interval("model", t.leaf, held, slots, m, t.nch, C))
    for j, u in enumerate(batches(k.u)):
        want, _, m, _ = pm.draws(t, held, u)
        got = draw(eng, u)
        assert np.array_equal(got, want), (j, np.flatnonzero(got != want), got[got != want], want[got != want])
        worst_iv = max(worst_iv, bounds.prio_draw_interval(f"{cap}-{held}-{fill} call {j}", t.leaf, held, got, (u * T).astype(F32), t.nch, C))
        w = eng.debug_read("prio_weights")
        ref = pref.weights(t.leaf, held, got, BETA)
        assert w.shape == (B,) and w.max() == 1.0
        rel = float((np.abs(w - ref) / ref).max())
        worst_w = max(worst_w, rel)
        assert rel <= BOUND_REL["weights"], (j, rel)
    eng.prio_set_uniforms(None)                                              # ... and a native call: Philox uniforms, draw counter 0
    eng.rb_sample_prioritized(BETA)
    un = pref.native_uniforms(SEED, 0, B)
    want, _, m, _ = pm.draws(t, held, un)
    got = eng.read_batch()["index"]
    assert np.array_equal(got, want), ("native", np.flatnonzero(got != want))
    worst_iv = max(worst_iv, bounds.prio_draw_interval(f"{cap}-{held}-{fill} native", t.leaf, held, got, m, t.nch, C))
    print(f"{cap}-{held}-{fill}: {len(k.u)} directed draws, worst interval err / tol {worst_iv:.4f}, worst weight delta {worst_w:.3e}, "
          f"fall-backs: group {sum(p.group_fallback for p in paths)}, leaf {sum(p.leaf_fallback for p in paths)}, chunk 1: {sum(p.chunk == 1 for p in paths)}")
    observe("prio_draw_interval_device", pm.case_id((cap, held, fill)), worst_iv)
    observe("prio_scale_weights", pm.case_id((cap, held, fill)) + ": max relative delta", worst_w)
    st = eng.prio_stats()
    assert st["rows_refused"] == 0 and st["samples"] == len(batches(k.u)) + 1 and eng.priority_stats()["rows_refused"] == 0


# ------------------------------------------------------------------------------------------ 2. appends at scale
def test_appends_in_the_second_chunk_and_across_the_wrap_leave_the_models_table():
    """1 050 076 slots, 1 050 039 held: 2000 rows by rb_extend_fields_device end the ring and wrap (k_prio_refresh's first range in
    group 1025 of chunk 1, its second in groups 0 and 1); then rb_fill_synthetic over rows 0 .. 1 048 999, across slot 1 048 576"""
    cap, held = BIG
    (eng,), k, t = ring(cap, held, "wide")
    mx = eng.debug_read("prio_max")[0]
    assert mx == max(F32(1), k.leaf.max())
    _, (o, a, bound), _ = SHAPES[SHAPE]
    extend_device(eng, cuda(synth_transitions(2000, o, a, bound, seed=71)))
    t = pm.refresh(t, held, 2000, mx)
    assert eng.rb_len() == cap and (t.leaf[held:cap] == mx).all() and (t.leaf[:1963] == mx).all() and t.leaf[1963] == k.leaf[1963]
    assert_table(eng, t, "append over the end of the ring")
    eng.rb_fill_synthetic(1_049_000, 6)
    t = pm.refresh(t, 0, 1_049_000, mx)
    assert_table(eng, t, "fill across the chunk boundary")
    assert eng.prio_stats() == dict(samples=0, write_backs=(held + CALL_ROWS - 1) // CALL_ROWS, rows_refused=0, rows_entered_at_max=held + 2000 + 1_049_000)
    u = into_groups(t, np.cumsum(t.leaf[:cap].astype(np.float64)), [1023, 1024, 1025, 0])
    assert np.array_equal(draw(eng, u), pm.draws(t, cap, u)[0])              # ... and the table draws like the model's


# ------------------------------------------------------------------------------------------ 3. write-backs in the second chunk
def test_write_backs_in_the_second_chunk_leave_the_models_table():
    cap, held = BIG
    (eng,), k, t = ring(cap, held, "wide")
    # one call whose rows straddle slots 1 048 575 / 1 048 576 and repeat a slot on either side: the highest batch position wins
    idx = np.array([1_048_574, 1_048_575, 1_048_576, 1_048_577, 1_048_575, 1_050_038, 1_048_576, 1_049_600, 1_048_575], np.int64)
    prio = np.array([0.5, 0.25, 4.0, 0.0, 1.5, 2.0, 0.125, 3.0, 0.75], F32)
    keep = torch.as_tensor(idx, device=DEV), torch.as_tensor(prio, device=DEV)
    write_chunked(eng, *keep)
    t1, refused = pm.write_back(t, held, idx, prio)
    assert refused == 0 and t1.leaf[1_048_575] == 0.75 and t1.leaf[1_048_576] == 0.125 and t1.leaf[1_048_577] == 0.0
    assert_table(eng, t1, "prio_update_device across the chunk boundary")
    # the TD write-back behind a draw into groups 1024 and 1025
    C = np.cumsum(t1.leaf[:held].astype(np.float64))
    u = into_groups(t1, C, [1024, 1025])
    rows = draw(eng, u)
    assert np.array_equal(rows, pm.draws(t1, held, u)[0]) and (rows >= 1024 * G).all() and len(np.unique(rows)) < B
    assert {int(r) // G for r in rows} == {1024, 1025}
    eng.update_qnets()
    p32 = np.abs(td_of(eng)).max(0).astype(F32) + F32(EPS)
    eng.prio_update_from_td()
    t2, refused = pm.write_back(t1, held, rows, p32)
    assert refused == 0
    assert_table(eng, t2, "prio_update_from_td in chunk 1")
    touched = np.zeros(len(t2.leaf), bool)
    touched[rows] = True
    assert same_bits(t2.leaf[~touched], t1.leaf[~touched]) and set(np.flatnonzero(t2.sums != t1.sums)) <= {1024, 1025}
    for b in range(B):                                                       # the highest batch position wins
        assert t2.leaf[rows[b]] == p32[np.flatnonzero(rows == rows[b])[-1]]
    assert eng.prio_stats()["rows_refused"] == 0
    del keep


# ------------------------------------------------------------------------------------------ 4. the graph forms at nch = 2
def test_the_graph_forms_draw_and_write_back_like_the_call_sequence_at_two_chunks():
    """k_prio_draw_g, k_prio_weights_g, k_prio_update_g on the 1026-group ring: one step_sampled(False, beta) on a twin against
    rb_sample_prioritized, update_qnets, prio_update_from_td, update_targ_nets, with the same injected uniforms into groups 1023 .. 1025"""
    cap, held = BIG
    (A, Bt), k, t = ring(cap, held, "wide", count=2)
    assert len(Bt.debug_read("prio_sums")) == 1026
    C = np.cumsum(t.leaf[:held].astype(np.float64))
    u = into_groups(t, C, [1023, 1024, 1025])
    u[:2] = [0.0, pm.U_MAX]
    for eng in (A, Bt):
        eng.prio_set_uniforms(u)
    call_sequence(A, False, sampled_draw(BETA), 1, write_back=True)
    Bt.step_sampled(False, beta=BETA)
    want, T, m, paths = pm.draws(t, held, u)
    rows = Bt.read_batch()["index"]
    assert np.array_equal(rows, want) and np.array_equal(A.read_batch()["index"], want) and sum(p.chunk == 1 for p in paths) > B // 2
    bounds.prio_draw_interval("graph form", t.leaf, held, rows, m, t.nch, C)
    assert same_bits(A.debug_read("prio_weights"), Bt.debug_read("prio_weights")) and Bt.debug_read("prio_weights").max() == 1.0
    assert same_bits(td_of(A), td_of(Bt))
    p32 = np.abs(td_of(Bt)).max(0).astype(F32) + F32(EPS)
    t2, refused = pm.write_back(t, held, rows, p32)
    assert refused == 0
    assert_table(A, t2, "the call sequence")
    assert_table(Bt, t2, "step_sampled")
    assert same_bits(A.debug_read("prio_max"), Bt.debug_read("prio_max"))
    assert A.prio_stats() == Bt.prio_stats() and Bt.prio_stats()["rows_refused"] == 0 and Bt.step_sampled_stats()["launches"] == 1


# ------------------------------------------------------------------------------------------ 5. alpha != 1
def test_behind_a_power_the_sums_and_draws_are_still_the_models():
    """alpha = 0.6 on the 1026-group ring: a leaf is powf(p, 0.6) and is held to the float64 power within BOUND_REL["leaves"] (0 stays
    0); the sums and the draws are predicted from the leaves read back, and have the model's bits"""
    cap, held = BIG
    (eng,), k, t = ring(cap, held, "wide", alpha=0.6)
    want = k.leaf.astype(np.float64) ** 0.6
    live = want > 0
    rel = float((np.abs(t.leaf[:held][live] - want[live]) / want[live]).max())
    print(f"leaves at alpha 0.6: max relative delta {rel:.3e}")
    observe("prio_scale_leaves", "alpha 0.6: max relative delta", rel)
    assert rel <= BOUND_REL["leaves"] and not t.leaf[:held][~live].any() and not t.leaf[held:].any()
    assert_table(eng, t, "alpha 0.6")
    C = np.cumsum(t.leaf[:held].astype(np.float64))
    for u in list(batches(k.u)[:2]) + [into_groups(t, C, [1022, 1023, 1024, 1025])]:
        slots, T, m, _ = pm.draws(t, held, u)
        got = draw(eng, u)
        assert np.array_equal(got, slots), np.flatnonzero(got != slots)
        bounds.prio_draw_interval("alpha 0.6", t.leaf, held, got, m, t.nch, C)
    assert eng.prio_stats()["rows_refused"] == 0
