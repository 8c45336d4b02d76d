"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

numpy restatement of the engine-owned proportional prioritised replay (include/sactd3.h: sactd3_prio_*, sactd3_rb_sample_prioritized;
Schaul et al. 2016, proportional variant, draws with replacement):

* selection: with c the inclusive running sum of the leaves of rows [0, len) and T = c[-1], row b gets the smallest slot i with
  c[i] > m_b, m_b = float32(u_b * T) -- np.searchsorted(c, m, side="right").  Evaluated in float64; where the leaves are small
  integers the float32 sums of the device are exact too, so the slots must be EQUAL.
* the native uniforms: Philox4x32-10 (oracle.replay_ref), stream 0x300, counter words (draw counter, 0, 0x300, b >> 2), word b & 3,
  mapped by oracle.replay_ref._u01 and kept below 1 (the 24-bit map rounds its largest value up to 1.0).
* weights (N leaf / T)^(-beta) over the batch's largest, and the write-back p = max_k |td_k| + eps, leaf = p^alpha, in float64.
"""
from __future__ import annotations

import numpy as np

from oracle.replay_ref import _u01, philox4x32_10

STREAM_PRIO = 0x300
GROUP = 1024                       # leaves per partial sum (csrc/prio_kernels.h: PRIO_G)
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)


def native_uniforms(seed: int, draw_ctr: int, batch: int) -> np.ndarray:
    b = np.arange(batch, dtype=np.uint64)
    r = philox4x32_10(np.full(batch, draw_ctr), 0, STREAM_PRIO, b >> np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    word = np.choose((b & np.uint64(3)).astype(np.int64), r).astype(np.uint32)
    return np.minimum(_u01(word), U_MAX).astype(np.float32)


def select(leaf, length: int, u) -> np.ndarray:
    """-> the slots drawn for the uniforms u (float32, in [0, 1)); -1 everywhere if nothing can be drawn"""
    c = np.cumsum(np.asarray(leaf[:length], np.float64))
    T = np.float32(c[-1])
    if not T > 0:
        return np.full(len(u), -1, np.int64)
    m = (np.asarray(u, np.float32) * T).astype(np.float32)      # one float32 multiply
    return np.searchsorted(c, m.astype(np.float64), side="right").astype(np.int64)


def weights(leaf, length: int, slots, beta: float) -> np.ndarray:
    """float64 importance weights of the drawn slots, normalised by the batch's largest"""
    lf = np.asarray(leaf[:length], np.float64)
    T = lf.sum()
    w = (length * lf[np.asarray(slots)] / T) ** (-float(beta))
    return w / w.max()


def td_priorities(td, eps: float) -> np.ndarray:
    """float64 unscaled priorities of a [2, B] array of TD errors"""
    return np.abs(np.asarray(td, np.float64)).max(0) + float(eps)


def write_back(leaf, slots, prio, alpha: float) -> np.ndarray:
    """float64 leaves after a write-back; where a slot repeats, the highest batch position wins"""
    out = np.asarray(leaf, np.float64).copy()
    for s, p in zip(np.asarray(slots), np.asarray(prio, np.float64)):      # in batch order: later positions overwrite
        out[s] = 0.0 if p == 0 else p ** float(alpha)
    return out


def group_sums(leaf) -> np.ndarray:
    """float64 sum of every group of GROUP consecutive leaves"""
    lf = np.asarray(leaf, np.float64)
    n = (len(lf) + GROUP - 1) // GROUP
    return np.array([lf[g * GROUP:(g + 1) * GROUP].sum() for g in range(n)])


def chi2_quantile(df: int, p: float) -> float:
    """the p-quantile of chi-square(df): scipy if it imports, else Wilson-Hilferty"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(p, df))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(p)
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3
