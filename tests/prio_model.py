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
