"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

numpy restatement of the pinned ring and the mixed draw (include/sactd3.h: sactd3_rb_pin, sactd3_rb_sample_mixed), built on the
oracle's Philox: what tests/test_prior_data_host.py checks against itself and tests/test_gpu_prior_data.py against the engine."""
import numpy as np

from oracle.replay_ref import STREAM_INDEX, philox4x32_10


def index_words(seed: int, ctr: int, batch: int) -> np.ndarray:
    """w_b: the 32-bit word csrc/philox.h:philox_index selects for batch row b at sample counter `ctr`"""
    b = np.arange(batch, dtype=np.uint64)
    r = philox4x32_10(np.full(batch, ctr), 0, STREAM_INDEX, b >> np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    return np.choose((b & np.uint64(3)).astype(np.int64), r).astype(np.uint64)


def mixed_indices(seed: int, ctr: int, B: int, m: int, P: int, length: int) -> np.ndarray:
    """rows b < m: (w_b * P) >> 32; rows b >= m: P + ((w_b * (length - P)) >> 32)"""
    assert 0 <= m <= B and 0 <= P <= length
    assert m == 0 or P > 0, "prior rows need pinned rows"
    assert m == B or length > P, "live rows need a live row"
    w = index_words(seed, ctr, B)
    prior = np.arange(B) < m
    span = np.where(prior, np.uint64(P), np.uint64(length - P))
    return (np.where(prior, 0, P) + ((w * span) >> np.uint64(32)).astype(np.int64)).astype(np.int64)


class PinnedRing:
    """The ring's cursor with P pinned slots: rows are values of any shape, appends go round-robin over [P, cap), the cursor comes
    back to P, len saturates at cap.  `wraps` counts how often the cursor came back to P while rows were pinned (the engine counts
    the launches that reached the end of the live region: a launch holds at most cap - P rows, so the two counts are one)."""

    def __init__(self, cap: int, width: int = 1):
        self.cap, self.len, self.cursor, self.P, self.wraps = int(cap), 0, 0, 0, 0
        self.rows = np.zeros((cap, width), np.float32)

    def pin(self, n: int):
        assert 0 <= n <= self.len and n < self.cap
        self.P = int(n)
        if self.len == self.cap:      # full and never wrapped: the oldest live row is the first one behind the pinned rows
            self.cursor = self.P

    def extend(self, rows):
        rows = np.asarray(rows, np.float32).reshape(len(rows), -1)
        for r in rows:
            self.rows[self.cursor] = r
            self.cursor += 1
            if self.cursor == self.cap:
                self.cursor = self.P
                self.wraps += self.P > 0
            self.len = min(self.cap, self.len + 1)
