"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

numpy restatement of the n-step staging (include/sactd3.h: sactd3_rb_sample_nstep*), over host copies of the ring's fields indexed by
ring SLOT (obs [cap, o], nobs [cap, o], rew [cap], done [cap] as float32 0/1 -- what the ring holds):

* age(i) = i while length < cap, else (i - cursor) mod cap; slot_j = (i0 + j * stride) mod cap exists iff age(i0) + j * stride < length.
* link j -> j+1 holds iff slot_{j+1} exists, done[slot_j] == 0 and nobs[slot_j] equals obs[slot_{j+1}] as 32-bit patterns
  (-0.0 != +0.0, equal NaN patterns are equal).
* k = 1 + the number of leading links that hold, 1 <= k <= steps.
* R_0 = r_0, G_0 = 1, G_j = G_{j-1} * gamma, R_j = R_{j-1} + G_j * r_j, every operation a float32 one in this order;
  mask = 1 - (1 - d_{k-1}) * G_{k-1}, and d_0 itself when k = 1.
* a start slot outside [0, length) is refused: (0, -1, 0, 0).
"""
from __future__ import annotations

import numpy as np

MAX_STEPS = 16
F1 = np.float32(1.0)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def age(i: int, length: int, cursor: int, cap: int) -> int:
    return i if length < cap else (i - cursor) % cap


def chain(obs, nobs, rew, done, i0, steps, stride, length, cursor, cap, gamma):
    """-> (k, last, R, mask): int, int, np.float32, np.float32"""
    assert 1 <= steps <= MAX_STEPS and stride >= 1
    i0 = int(i0)
    if not 0 <= i0 < length:
        return 0, -1, np.float32(0.0), np.float32(0.0)
    a0 = age(i0, length, cursor, cap)
    slots = [i0]
    for j in range(1, steps):
        if a0 + j * stride >= length:
            break
        nxt = (i0 + j * stride) % cap
        cur = slots[-1]
        if done[cur] != 0 or not np.array_equal(bits(nobs[cur]), bits(obs[nxt])):
            break
        slots.append(nxt)
    k = len(slots)
    g = np.float32(gamma)
    G, R = F1, np.float32(rew[slots[0]])
    for j in range(1, k):
        G = np.float32(G * g)
        R = np.float32(R + np.float32(G * np.float32(rew[slots[j]])))
    d = np.float32(done[slots[-1]])
    mask = d if k == 1 else np.float32(F1 - np.float32(np.float32(F1 - d) * G))
    return k, slots[-1], R, mask


def chains(obs, nobs, rew, done, idx, steps, stride, length, cursor, cap, gamma):
    """chain() over an index array -> dict of arrays k, last (int32), R, mask (float32)"""
    out = [chain(obs, nobs, rew, done, i, steps, stride, length, cursor, cap, gamma) for i in np.asarray(idx).reshape(-1)]
    return dict(k=np.array([c[0] for c in out], np.int32), last=np.array([c[1] for c in out], np.int32),
                R=np.array([c[2] for c in out], np.float32), mask=np.array([c[3] for c in out], np.float32))


def place(fields, cap):
    """rows in append order (obs, act, rew, nobs, done) -> the same fields indexed by ring slot ([cap, ...], unfilled slots zero), and
    (length, cursor): row r lands in slot r % cap"""
    n = len(fields[0])
    out = [np.zeros((cap,) + np.asarray(f).shape[1:], np.float32) for f in fields]
    for f, o in zip(fields, out):
        f = np.asarray(f, np.float32)
        for lo in range(0, n, cap):                     # later rows overwrite earlier ones
            hi = min(lo + cap, n)
            o[np.arange(lo, hi) % cap] = f[lo:hi]
    return out, min(n, cap), n % cap
