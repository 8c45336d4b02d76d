"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The two-level priority table of csrc/prio_kernels.h restated in numpy float32, operation for operation: the same adds in the same
order, one float32 multiply for m = u T, one float32 subtract for the residue.  Nothing in that code can be contracted or
reassociated (adds only; csrc/Makefile has no fast-math), so for ANY float leaves the device's group sums, its total T, m and the
slot it selects are predicted here bit for bit -- tests/test_gpu_priorities_scale.py compares uint32 views, with no tolerance.
tests/priorities_ref.py is the float64 restatement (what the table ought to compute); this file is what it does compute.

    scan(v)                         prio_scan: front of every thread, total of the 1024 values
    running(v, front)               the running sums prio_find compares with m: one add onto `front` each
    find(v, front, m, base, limit)  prio_find: first / last position, the chosen one's exclusive sum and value
    table(leaf, capacity)           zero-padded leaves, group sums (padded to whole chunks of 1024)
    draw(table, length, u)          prio_draw_body -> (slot, T, m, path)
    refresh / write_back            the leaves and re-summed groups k_prio_refresh / k_prio_update leave at alpha == 1 (no powf)
    resum                           the sums of a table from its leaves (alpha != 1: leaves as read back, sums predicted)

tests/test_prio_model.py checks this file on the CPU: against tests/bounds.py:prio_draw_interval in float64, and by showing that a
copy of this source with one line changed (its DEFECTS) is told apart."""
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

F32 = np.float32
G = 1024                         # PRIO_G
NONE = 0x7FFFFFFF                # PRIO_NONE
HUGE = F32(np.inf)
U_MAX = F32(1.0) - F32(2.0 ** -24)      # what the kernel keeps every uniform below


def scan(v):
    """prio_scan over the last axis (1024 values; thread t = 64 wave + lane owns 4t .. 4t+3) -> (front [..., 256], tot [...])"""
    v = np.asarray(v, F32)
    lead = v.shape[:-1]
    q = v.reshape(lead + (4, 64, 4))                               # wave, lane, k
    s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    for d in (1, 2, 4, 8, 16, 32):                                 # Kogge-Stone inside a wave: all lanes at once
        t = s.copy()
        t[..., d:] = s[..., d:] + s[..., :-d]
        s = t
    before = np.zeros_like(s)
    before[..., 1:] = s[..., :-1]                                  # (lane 0: 0)
    w0, w1, w2, w3 = (s[..., i, 63] for i in range(4))
    tot = ((w0 + w1) + w2) + w3
    woff = np.stack([np.zeros_like(w0), w0, w0 + w1, (w0 + w1) + w2], -1)
    front = woff[..., None] + before
    return front.reshape(lead + (256,)), tot


class Find(NamedTuple):
    first: int
    last: int
    excl: float
    val: float


def running(v, front):
    """the inclusive and exclusive running sums prio_find forms for its 1024 positions: one add onto `front` each -> ([1024], [1024])"""
    v = np.asarray(v, F32).reshape(256, 4)
    front = np.asarray(front, F32)
    v0, v1, v2, v3 = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    a01 = v0 + v1
    a012 = a01 + v2
    a0123 = a012 + v3
    inc = np.stack([front + v0, front + a01, front + a012, front + a0123], 1)
    exc = np.stack([front, front + v0, inc[:, 1], inc[:, 2]], 1)
    return inc.reshape(-1), exc.reshape(-1)


def find(v, front, m, base, limit):
    """prio_find on one block: v [1024], front [256] (what the caller adds to it included), positions base .. base + 1023"""
    v, m = np.asarray(v, F32), F32(m)
    inc, exc = running(v, front)
    pos = base + np.arange(G)
    ok = (v > 0) & (pos < limit)
    hit = np.flatnonzero(ok & (inc > m))
    live = np.flatnonzero(ok)
    first = base + int(hit[0]) if hit.size else NONE
    last = base + int(live[-1]) if live.size else -1
    chosen = first if first != NONE else last
    if chosen < 0:                                                 # (the kernel's s_excl / s_val are stale then, and unused)
        return Find(first, last, HUGE, F32(0))
    return Find(first, last, exc[chosen - base], v[chosen - base])


class Table(NamedTuple):
    leaf: np.ndarray             # [ngroups * 1024]
    sums: np.ndarray             # [nch * 1024]
    capacity: int
    ngroups: int
    nch: int


def group_sums(leaf):
    """the sum prio_scan leaves for every whole group of 1024 leaves"""
    return scan(np.asarray(leaf, F32).reshape(-1, G))[1]


def table(leaf, capacity):
    """the table for the leaves of slots [0, len(leaf)) in a ring of `capacity` slots"""
    ngroups = (capacity + G - 1) // G
    nch = (ngroups + G - 1) // G
    lf = np.zeros(ngroups * G, F32)
    lf[:len(leaf)] = np.asarray(leaf, F32)
    sums = np.zeros(nch * G, F32)
    sums[:ngroups] = group_sums(lf)
    return Table(lf, sums, int(capacity), ngroups, nch)


def resum(t, groups=None):
    """the table with the sums of `groups` (default: all) taken again from its leaves"""
    sums = t.sums.copy()
    gs = np.arange(t.ngroups) if groups is None else np.unique(np.asarray(groups, np.int64))
    sums[gs] = group_sums(t.leaf.reshape(-1, G)[gs])
    return t._replace(sums=sums)


class Path(NamedTuple):
    group_fallback: bool         # if (g < 0) g = glast
    leaf_fallback: bool          # chosen = f.last at the leaf stage
    chunk: int
    group: int


def top_scans(t):
    """prio_scan of every chunk of the top level: the same for every draw from one table"""
    return [scan(t.sums[c * G:(c + 1) * G]) for c in range(t.nch)]


def top_running(t):
    """the inclusive running sums the second pass of a draw compares m with, for every position of the top level -> [nch * 1024]"""
    out, carry = [], F32(0)
    for c, (front, tot) in enumerate(top_scans(t)):
        out.append(running(t.sums[c * G:(c + 1) * G], carry + front)[0])
        carry = carry + tot
    return np.concatenate(out)


def leaf_running(t, g):
    """the inclusive running sums of the leaf stage inside group g -> [1024]"""
    v = t.leaf[g * G:(g + 1) * G]
    return running(v, scan(v)[0])[0]


def draw(t, length, u, chunks=None):
    """prio_draw_body for one uniform -> (slot, T, m, Path); slot -1: nothing to draw from"""
    u = min(F32(u), U_MAX)
    chunks = top_scans(t) if chunks is None else chunks
    carry = F32(0)
    for c in range(t.nch):                                         # first pass: the total
        carry = carry + chunks[c][1]
    T = carry
    m = F32(u * T)
    carry = F32(0)                                                 # second pass
    g, glast, resid = -1, -1, HUGE
    for c in range(t.nch):
        front, tot = chunks[c]
        if g < 0:
            base = c * G
            f = find(t.sums[c * G:(c + 1) * G], carry + front, m, base, t.ngroups)
            if f.last >= 0:
                glast = f.last
            if f.first != NONE:
                g = f.first
                resid = F32(m - f.excl)
        carry = carry + tot
    fell_g = g < 0
    if fell_g:
        g = glast
    if g < 0:
        return -1, T, m, Path(True, True, -1, -1)
    v = t.leaf[g * G:(g + 1) * G]
    f = find(v, scan(v)[0], resid, g * G, length)
    chosen = f.first if f.first != NONE else f.last
    return chosen, T, m, Path(fell_g, f.first == NONE, g // G, g)


def draws(t, length, us):
    """draw for every uniform of `us` -> (slots int64, T, m float32 [n], [Path])"""
    chunks = top_scans(t)
    out = [draw(t, length, u, chunks) for u in us]
    T = out[0][1] if out else F32(0)
    return np.array([o[0] for o in out], np.int64), T, np.array([o[2] for o in out], F32), [o[3] for o in out]


def refresh(t, first, n, value):
    """k_prio_refresh behind an append of rows [first, first + n), wrapping at the capacity, at alpha == 1: the leaves set to
    `value` (max_prio), the groups that hold one of them summed again, every other sum untouched"""
    cap = t.capacity
    if n >= cap:
        first, n = 0, cap
    slots = (first + np.arange(n)) % cap
    leaf = t.leaf.copy()
    leaf[slots] = F32(value)
    return resum(t._replace(leaf=leaf), slots // G)


def write_back(t, length, idx, prio):
    """k_prio_update at alpha == 1: rows with a slot in [0, length) and a finite priority >= 0 are accepted, in batch order (the
    highest position wins a slot); the groups of accepted rows are summed again.  -> (table, rows refused)"""
    idx, prio = np.asarray(idx, np.int64), np.asarray(prio, F32)
    ok = (idx >= 0) & (idx < length) & (prio >= 0) & (prio < HUGE)
    leaf = t.leaf.copy()
    for s, p in zip(idx[ok], prio[ok]):
        leaf[s] = p
    return resum(t._replace(leaf=leaf), idx[ok] // G), int((~ok).sum())


# ------------------------------------------------------------------------------------------ the case table
# rings, leaves, directed uniforms and the model's draws of them: tests/test_prio_model.py checks them on the CPU,
# tests/test_gpu_priorities_scale.py holds the device to the same cases
FILLS = ["uniform", "wide", "zero-groups", "spike"]
NAMED_GROUPS = (0, 1, 511, 975, 976, 1022, 1023, 1024, 1025)
# how many seeds fallback_seed tries: 400 where a ring costs microseconds, 40 where it costs 20 ms
SEEDS = {1024: 400, 1025: 400, 1000: 400, 5000: 400, 1_000_000: 40, 1_050_076: 40, 1_100_000: 40}


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


def uniform_leaves(held, seed):
    return np.random.default_rng(seed).uniform(0.05, 3.0, held).astype(F32)


@functools.lru_cache(maxsize=None)
def fallback_seed(cap, held):
    """the first seed of SEEDS[cap] whose uniform(0.05, 3) ring falls back at u = 1 - 2^-24: at the group stage where the ring has
    more than eight groups, at the leaf stage below.  -> (seed, found); seed 0 where none does"""
    want_group = cap > 8 * G
    for seed in range(SEEDS[cap]):
        path = draw(table(uniform_leaves(held, seed), cap), held, U_MAX)[3]
        if path.group_fallback if want_group else (path.leaf_fallback and not path.group_fallback):
            return seed, True
    return 0, False


def leaves(cap, held, fill):
    """the leaves of rows [0, held) of one case"""
    if fill == "uniform":
        return uniform_leaves(held, fallback_seed(cap, held)[0])
    rng = np.random.default_rng(1000 + held % 997)
    last_group = (held - 1) // G
    if fill == "wide":                        # exp(N(0, 1.5))^0.6 with exact zeros: 5000 in a million, the ends and group edges among them
        lf = (np.exp(rng.normal(0.0, 1.5, held)) ** 0.6).astype(F32)
        lf[rng.choice(held, max(held * 5000 // 1_050_039, 24), replace=False)] = 0.0
        edges = [0, held - 1, held - 2] + [s for g in NAMED_GROUPS[1:] for s in (g * G - 1, g * G, g * G + 4) if s < held]
        lf[edges] = 0.0
        return lf
    if fill == "zero-groups":                 # whole groups without mass: 1022, 1023, 1024 (around the chunk boundary) and the last
        lf = rng.uniform(0.05, 3.0, held).astype(F32)
        for g in (1022, 1023, 1024, last_group):
            if g * G < held and last_group > 0:
                lf[g * G:(g + 1) * G] = 0.0
        if last_group == 0:                   # (one group: its second half)
            lf[held // 2:] = 0.0
        return lf
    lf = np.full(held, 1e-3, F32)             # spike: one leaf of 1e6 among leaves of 1e-3
    lf[(2 * held) // 3] = 1e6
    return lf


def aim(T, target):
    """a float32 u <= U_MAX with fl32(u T) == target exactly, or None"""
    u = F32(np.float64(target) / np.float64(T))
    cand = [u]
    lo = hi = u
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(2))
        cand += [lo, hi]
    for c in cand:
        if 0 <= c <= U_MAX and F32(c * T) == F32(target):
            return c
    return None


def directed(t, held, C):
    """the uniforms of one case -> (u float32 [n], exact): 0 and the largest; the centre and both edges of the first and last
    positive slot and of the slots on both sides of every named group boundary (the chunk boundary is group 1024's); the edges and
    centres of the named groups; 32 random ones; and `exact`, {index into u: (level, position)} for the uniforms whose m equals one of
    the model's own inclusive running sums -- at the top level (of a named group) and at the leaf level (inside group 0)."""
    leaf = t.leaf[:held]
    T64, T = C[-1], draw(t, held, 0.0)[1]
    live = np.flatnonzero(leaf > 0)
    slots = {int(live[0]), int(live[-1]), held - 1}
    groups = [g for g in NAMED_GROUPS if g * G < held] + [(held - 1) // G]
    for g in groups:
        slots.update(s for s in (g * G - 1, g * G, (g + 1) * G - 1, (g + 1) * G) if 0 <= s < held)
    us = [0.0, float(U_MAX)]
    for s in sorted(slots):
        lo, hi = (C[s - 1] if s else 0.0), C[s]
        us += [lo / T64, 0.5 * (lo + hi) / T64, hi / T64]
    for g in groups:
        lo, hi = (C[g * G - 1] if g else 0.0), C[min((g + 1) * G, held) - 1]
        us += [lo / T64, 0.5 * (lo + hi) / T64, hi / T64]
    us += list(np.random.default_rng(7).random(32))
    us = [min(max(F32(u), F32(0)), U_MAX) for u in us]
    exact = {}
    top = top_running(t)
    for g in groups:
        u = aim(T, top[g]) if t.sums[g] > 0 else None
        if u is not None:
            exact[len(us)] = ("top", g)
            us.append(u)
    inc0 = leaf_running(t, 0)
    for s in [s for s in (0, 1, 2, 5, 6, 254, 257, 258, 509, 510, 513, 769, 770, 1021, 1022) if s < held and leaf[s] > 0]:
        u = aim(T, inc0[s])
        if u is not None:
            exact[len(us)] = ("leaf", s)
            us.append(u)
    return np.array(us, F32), exact


@functools.lru_cache(maxsize=None)
def case(cap, held, fill):
    """one case, computed once and never written: leaves, table, float64 running sums, directed uniforms, the model's draws"""
    leaf = leaves(cap, held, fill)
    t = table(leaf, cap)
    C = np.cumsum(leaf.astype(np.float64))
    u, exact = directed(t, held, C)
    slots, T, m, paths = draws(t, held, u)
    for a in (leaf, t.leaf, t.sums, C, u, slots, m):
        a.setflags(write=False)
    return SimpleNamespace(cap=cap, held=held, fill=fill, leaf=leaf, table=t, C=C, u=u, exact=exact, slots=slots, T=T, m=m, paths=paths)
