"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Plain sequential float64 restatement of the returns-to-go call (include/sactd3_returns.h), over host copies of the ring's fields
indexed by ring SLOT (obs [cap, o], nobs [cap, o], rew [cap], done [cap] -- what tests/nstep_ref.place leaves):

* whole ring (count None): n = length, base = 0 while length < cap, else cursor; range: n = count, base = first; slot(age) = (base + age) % cap.
* link age g -> g + stride holds iff g + stride < n, done[slot(g)] == 0 and nobs[slot(g)] equals obs[slot(g + stride)] as 32-bit patterns.
* ages in reverse: a row whose link is broken is a chain's last row; every other row adds its reward to gamma x its successor's sums.
"""
from __future__ import annotations

import numpy as np

from tests.nstep_ref import bits

TERMINATED, TRUNCATED, OPEN, START = 1, 2, 4, 8


def returns_to_go(obs, nobs, rew, done, gamma, stride, length, cursor, cap, first=0, count=None):
    """-> dict of arrays by ring slot, [cap]: G, U, A = sum_j gamma^j |r_{t+j}| (float64), L, last, ends (int64), and `rows`, the
    slots of the range in age order; slots outside the range hold 0"""
    n, base = (length, 0 if length < cap else cursor) if count is None else (count, first)
    assert 1 <= n <= length and stride >= 1 and (count is None or first + count <= length)
    gamma = float(gamma)
    slot = (base + np.arange(n)) % cap
    G, U, A = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    L, last, ends = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    start = np.ones(cap, bool)
    for g in range(n - 1, -1, -1):
        s, r = slot[g], float(rew[slot[g]])
        if done[s] != 0:
            kind = TERMINATED
        elif g + stride >= n:
            kind = OPEN
        elif not np.array_equal(bits(nobs[s]), bits(obs[slot[g + stride]])):
            kind = TRUNCATED
        else:
            kind = 0
        if kind:
            G[s], U[s], A[s], L[s], last[s], ends[s] = r, r, abs(r), 1, s, kind
        else:
            t = slot[g + stride]
            with np.errstate(invalid="ignore"):
                G[s], U[s], A[s] = r + gamma * G[t], r + U[t], abs(r) + gamma * A[t]
            L[s], last[s], ends[s] = L[t] + 1, last[t], ends[t]
            start[t] = False
    ends[slot] |= np.where(start[slot], START, 0)
    return dict(G=G, U=U, A=A, L=L, last=last, ends=ends, rows=slot)
