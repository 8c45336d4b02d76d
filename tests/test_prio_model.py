"""CPU: the checker of the prioritised draw checked -- tests/prio_model.py (the table of csrc/prio_kernels.h in numpy float32) and
tests/bounds.py:prio_draw_interval (the a-priori float64 interval), before tests/test_gpu_priorities_scale.py holds the device to both.

The case table: seven rings (one group; one group and a leaf; a partial group; the 5000-slot ring of the other priority tests; the
reference's 1 000 000 slots = 977 groups; 1 050 076 slots = 1026 groups, two top-level chunks, partly and wholly filled; 1 100 000
slots = 1075 groups), each filled four ways (FILLS).  The last ring is there for the group fall-back inside the second chunk: at 1026
groups the two sums of that chunk sit in one thread, whose compare path makes the very adds of the total path -- carry + (v0 + v1) --
so m = the float32 below T can never reach the last running sum; with 51 sums there, over 13 threads, it does.  Every draw of the model on directed uniforms has to lie in its float64 interval; the table has to hold
draws that take the leaf fall-back, the group fall-back and the second chunk, and draws whose m IS one of the running sums; a copy
of the model with one line changed (DEFECTS) has to be told apart; and what a 24-bit uniform and an fp32 m can reach at all in the
largest ring is characterised.

The seeds of the uniform(0.05, 3) fills are found by search (fallback_seed): with u = 1 - 2^-24, m is the float32 below T, and a
draw falls back where the running sum of the compare path ends below the T of the total path.  That happens in about one ring of
eight at one group and one of ten at 977 groups."""
import inspect
import types

import numpy as np
import pytest

from tests import bounds
from tests import prio_model as pm
from tests.helpers import observe
from tests.prio_model import FILLS, case, case_id, fallback_seed, uniform_leaves

F32, G = np.float32, pm.G
RINGS = [(1024, 1024), (1025, 1025), (1000, 777), (5000, 2500), (1_000_000, 1_000_000), (1_050_076, 1_050_039), (1_050_076, 1_050_076),
         (1_100_000, 1_100_000)]
CASES = [(cap, held, fill) for cap, held in RINGS for fill in FILLS]


# ------------------------------------------------------------------------------------------ 1. the model inside the interval
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_model_draws_lie_in_their_float64_interval(c):
    k = case(*c)
    t = k.table
    assert (t.ngroups, t.nch) == ((k.cap + G - 1) // G, 1 if k.cap <= G * G else 2)
    assert k.T == pm.draw(t, k.held, 0.5)[1] and abs(float(k.T) - k.C[-1]) <= bounds.gamma(2 * bounds.PRIO_ADDS_GROUP + t.nch) * k.C[-1]
    ratio = bounds.prio_draw_interval(case_id(c), k.leaf, k.held, k.slots, k.m, t.nch, k.C)
    print(f"{case_id(c)}: {len(k.u)} draws, T {float(k.T)!r}, worst err / tol {ratio:.4f}")
    observe("prio_draw_interval_model", case_id(c), ratio)
    live = np.flatnonzero(k.leaf > 0)
    assert k.slots[0] == live[0]                                             # u = 0: the first positive slot
    if fill_is_dense(k.fill):                                                # the largest u: the last one (no leaf there is below T 2^-24)
        assert k.slots[1] == live[-1]
    for i, (level, p) in k.exact.items():                                    # m on a running sum: the test is in > m, the draw goes past it
        beyond = np.searchsorted(live, (p + 1) * G if level == "top" else p + 1)
        if beyond == len(live):                                              # ... m on the LAST running sum: the fall-back, the last positive slot
            assert k.slots[i] == live[-1] and k.paths[i].leaf_fallback, (i, level, p, k.slots[i])
            continue
        assert k.slots[i] > ((p + 1) * G - 1 if level == "top" else p), (i, level, p, k.slots[i])
        nxt = live[beyond]
        if fill_is_dense(k.fill) and (p + 1) % 4:                            # the next position is in the same thread: no rounding between
            assert k.slots[i] == nxt, (i, level, p, k.slots[i], nxt)


def fill_is_dense(fill):
    """leaves of one magnitude: no running sum absorbs the next value"""
    return fill == "uniform"


# ------------------------------------------------------------------------------------------ 2. what the table has to hold
def test_the_case_table_reaches_every_path():
    """conditions on the table above, so that the GPU tests that take their rings from it run the same paths"""
    paths = {c: case(*c).paths for c in CASES}
    leaf_fb = [c for c, ps in paths.items() if any(p.leaf_fallback and not p.group_fallback for p in ps)]
    group_fb = [c for c, ps in paths.items() if any(p.group_fallback for p in ps)]
    chunk1 = [c for c, ps in paths.items() if any(p.chunk == 1 for p in ps)]
    exact = {c: case(*c).exact for c in CASES}
    print("leaf fall-back:", [case_id(c) for c in leaf_fb], "\ngroup fall-back:", [case_id(c) for c in group_fb])
    print("seeds:", {f"{cap}-{held}": fallback_seed(cap, held) for cap, held in RINGS})
    assert leaf_fb and group_fb and len(chunk1) >= 9
    assert any(p.group_fallback and p.chunk == 1 for c in group_fb for p in paths[c])         # glast taken from the second chunk
    assert any(p.group_fallback and p.chunk == 0 for c in group_fb for p in paths[c])
    assert fallback_seed(1024, 1024)[1] and fallback_seed(1000, 777)[1] and fallback_seed(1_000_000, 1_000_000)[1] and fallback_seed(1_100_000, 1_100_000)[1]
    assert all(p.leaf_fallback for ps in paths.values() for p in ps if p.group_fallback)      # resid stays +inf behind the group fall-back
    for c in CASES:                                                          # exact-boundary uniforms at both levels, everywhere
        levels = [lv for lv, _ in exact[c].values()]
        assert levels.count("leaf") >= 4 or c[2] == "spike", (case_id(c), exact[c])
        assert levels.count("top") >= (2 if c[0] > 8 * G else 1 if c[0] > 2 * G else 0) or c[2] == "spike", (case_id(c), exact[c])
    for c in CASES:                                                          # both sides of the chunk boundary where there is one
        if c[1] > G * G:
            groups = {p.group for p in paths[c]}
            assert {1021, 1025} <= groups or c[2] != "uniform", (case_id(c), sorted(groups))
            assert {1023, 1024} <= groups or c[2] == "zero-groups", (case_id(c), sorted(groups))
    for c in CASES:                                                          # a zero group is never drawn from
        if c[2] == "zero-groups":
            k = case(*c)
            assert all(k.table.sums[p.group] > 0 for p in k.paths)


# ------------------------------------------------------------------------------------------ 3. defects that must not pass
# name -> (the line of tests/prio_model.py, what a defective kernel would have there, which occurrence)
DEFECTS = {
    "carry_not_reset": ("    carry = F32(0)", "    carry = T", 1),
    "chunk_base_256": ("base = c * G", "base = c * 256", 0),
    "ngroups_limit_dropped_in_chunk_1": ("m, base, t.ngroups)", "m, base, t.ngroups if c == 0 else NONE)", 0),
    "resid_without_carry": ("resid = F32(m - f.excl)", "resid = F32(m - (f.excl - carry))", 0),
    "glast_from_chunk_0_only": ("if f.last >= 0:", "if f.last >= 0 and c == 0:", 0),
    "in_ge_m": ("ok & (inc > m)", "ok & (inc >= m)", 0),
    "zero_leaf_selectable": ("ok = (v > 0) & (pos < limit)", "ok = pos < limit", 0),
    "woff_wave_3_without_w2": ("w0 + w1, (w0 + w1) + w2], -1)", "w0 + w1, w0 + w1], -1)", 0),
    "length_not_applied": ("resid, g * G, length)", "resid, g * G, NONE)", 0),
}


def mutant(name):
    """tests/prio_model.py with one line changed, as a module of its own"""
    old, new, which = DEFECTS[name]
    src = inspect.getsource(pm)
    parts = src.split(old)
    assert len(parts) == which + 2 if which else len(parts) == 2, (name, len(parts) - 1)
    src = old.join(parts[:which + 1]) + new + old.join(parts[which + 1:])
    mod = types.ModuleType(f"prio_model_{name}")
    exec(compile(src, f"<prio_model with {name}>", "exec"), mod.__dict__)
    return mod


def poisoned():
    """Two tables that break what the kernel's two limits guard: with zero padding and zero leaves behind the ring's length the
    `v > 0` condition alone keeps a draw inside, so dropping a limit changes nothing that any well-formed table could show.
    (1) the top level's padding behind the 1026 sums holds mass; (2) 1000 positive leaves in a ring that holds 777 rows.
    -> [(table, length, uniforms)]"""
    k = case(1_050_076, 1_050_076, "uniform")
    sums = k.table.sums.copy()
    sums[k.table.ngroups:] = 1000.0
    t2 = pm.table(uniform_leaves(1000, 3), 1000)
    us = np.array([0.0, 0.3, 0.9, 0.999, pm.U_MAX], F32)
    return [(k.table._replace(sums=sums), k.held, us), (t2, 777, us)]


def told_apart(mod, t, held, u, C=None, leaf=None):
    """does the mutated model differ from the model on these draws, leave the table, or break the interval?"""
    want = pm.draws(t, held, u)[0]
    try:
        got, T, m, _ = mod.draws(mod.Table(*t), held, u)
    except (IndexError, ValueError):                       # a group behind the table: the kernel would have read out of bounds
        return "left the table"
    if not np.array_equal(got, want):
        return f"draws differ at {np.flatnonzero(got != want)[:4]}"
    if C is not None:
        try:
            bounds.prio_draw_interval("mutant", leaf, held, got, m, t.nch, C)
        except bounds.Violation as e:
            return str(e)
    return None


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_each_defect_is_told_apart(defect):
    mod = mutant(defect)
    why = None
    for c in sorted(CASES, key=lambda c: (c[1] <= G * G, c[1])):      # (the rings of two chunks first: most defects live there)
        k = case(*c)
        why = told_apart(mod, k.table, k.held, k.u, k.C, k.leaf)
        if why:
            print(f"{defect}: {case_id(c)}: {why}")
            break
    if not why and defect in ("ngroups_limit_dropped_in_chunk_1", "length_not_applied"):
        for t, held, u in poisoned():
            want = pm.draws(t, held, u)[0]
            assert (want >= 0).all() and (want < held).all()          # the model itself stays inside on the same table
            why = why or told_apart(mod, t, held, u)
        print(f"{defect}: only on a table that breaks the padding: {why}")
    assert why, f"{defect} passes every check"


def test_interval_refuses_what_it_must():
    k = case(1000, 777, "wide")
    C, s = k.C, int(np.flatnonzero(k.leaf > 0)[5])
    mid = 0.5 * (C[s - 1] + C[s])
    tol = bounds.prio_draw_tol(C[-1], 1)
    assert 40 * bounds.U * C[-1] < tol < 64 * bounds.U * C[-1]               # a few tens of units of 2^-24 T, derived (bounds.py)
    bounds.prio_draw_interval("ok", k.leaf, 777, [s], [mid], 1, C)
    bounds.prio_draw_interval("edges", k.leaf, 777, [s, s], [C[s - 1] - 0.9 * tol, C[s] + 0.9 * tol], 1)
    zero = int(np.flatnonzero(k.leaf == 0)[0])
    for what, slot, m in (("zero leaf", zero, C[zero]), ("at the length", 777, C[-1]), ("negative", -1, 0.0),
                          ("below", s, C[s - 1] - 1.1 * tol), ("above", s, C[s] + 1.1 * tol)):
        with pytest.raises(bounds.Violation):
            bounds.prio_draw_interval(what, k.leaf, 777, [slot], [m], 1, C)


# ------------------------------------------------------------------------------------------ 4. refresh and write-back
def test_refresh_and_write_back_resum_only_the_groups_they_touch():
    k = case(1_050_076, 1_050_039, "wide")
    t = pm.refresh(k.table, 1_050_039, 2000, 2.5)                            # ends the ring and wraps: group 1025, then groups 0 and 1
    changed = np.flatnonzero(t.sums.view(np.uint32) != k.table.sums.view(np.uint32))
    assert set(changed) == {0, 1, 1025} and (t.leaf[:1963] == 2.5).all() and (t.leaf[1_050_039:1_050_076] == 2.5).all()
    assert t.leaf[1963] == k.table.leaf[1963] and not t.leaf[1_050_076:].any()
    assert np.array_equal(pm.resum(t).sums.view(np.uint32), t.sums.view(np.uint32))       # the other sums were the leaves' already
    idx = np.array([1_048_575, 1_048_576, 1_048_575, 7, 1_050_076, -1], np.int64)
    w, refused = pm.write_back(t, 1_050_076, idx, np.array([0.5, 0.25, 4.0, np.nan, 1.0, 1.0], F32))
    assert refused == 3 and w.leaf[1_048_575] == 4.0 and w.leaf[1_048_576] == 0.25 and w.leaf[7] == t.leaf[7]
    assert set(np.flatnonzero(w.sums != t.sums)) == {1023, 1024}


# ------------------------------------------------------------------------------------------ 5. what a 24-bit uniform can reach
def test_reachability_of_the_largest_ring():
    """All 2^24 uniforms k 2^-24 through m = fl32(u T) and a float64 searchsorted over the 1 050 076-slot wide-range ring.  From first
    principles: consecutive m differ by at most T 2^-24 plus one rounding of m (at most ulp(T) / 2 on each side), so every row whose
    leaf is at least 2 max(T 2^-24, ulp(T)) and whose interval ends at or below the largest m is selected by some uniform.  How many
    positive rows none selects, and their share of the mass, is a property of the 24-bit uniform and the fp32 m, not an error: it is
    recorded (helpers.observe), not asserted."""
    k = case(1_050_076, 1_050_039, "wide")
    T, C = k.T, k.C
    hit = np.zeros(k.held, bool)
    m_max = 0.0
    for lo in range(0, 1 << 24, 1 << 21):
        u = (np.arange(lo, lo + (1 << 21), dtype=np.float64) * 2.0 ** -24).astype(F32)
        m = (u * T).astype(np.float64)                                       # (float32 array times float32 scalar: one float32 multiply)
        assert (u * T).dtype == F32
        m_max = max(m_max, float(m.max()))
        s = np.searchsorted(C, m, side="right")
        hit[s[s < k.held]] = True
    step = 2.0 * max(float(T) * 2.0 ** -24, float(np.spacing(T)))
    assert not hit[k.leaf == 0].any()
    must = (k.leaf >= step) & (C <= m_max)
    assert hit[must].all(), np.flatnonzero(must & ~hit)[:8]
    positive = k.leaf > 0
    missed = positive & ~hit
    share = float(k.leaf[missed].astype(np.float64).sum() / C[-1])
    print(f"T {float(T)!r}: step of m {step / 2:.4f}; {int(missed.sum())} of {int(positive.sum())} positive rows are selected by none of the "
          f"2^24 uniforms, {share:.3e} of the mass; {int(((k.leaf >= step) & ~must).sum())} large rows end above the largest m")
    observe("prio_reachability_1050076_wide", "positive rows no uniform selects", int(missed.sum()))
    observe("prio_reachability_1050076_wide", "their share of the mass", share)
    observe("prio_reachability_1050076_wide", "positive rows", int(positive.sum()))
