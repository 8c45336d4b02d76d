"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A plain brute-force restatement of sactd3_ring_knn_device (include/sactd3_ring_knn.h):
transform both sides, the full selector and distance matrices, a stable sort by (value, slot).  It runs in a dtype of the caller's
choice: float64 is the reference, float32 on the CPU -- the same xn - 2 dot expansion in torch's own summation order -- the yardstick
of the tolerance.  Used by tests/test_gpu_ring_knn.py and tests/test_ring_knn_host.py."""
import numpy as np
import torch


def matrices(queries, keys, offset=None, scale=None, dtype=torch.float64):
    """-> (sel [n, L] = |x'|^2 - 2 q'.x', dist2 [n, L] = sum_d (q'_d - x'_d)^2), both in `dtype`"""
    q, x = (torch.as_tensor(np.asarray(v), dtype=dtype) for v in (queries, keys))
    c = torch.zeros(q.shape[1], dtype=dtype) if offset is None else torch.as_tensor(np.asarray(offset), dtype=dtype)
    w = torch.ones(q.shape[1], dtype=dtype) if scale is None else torch.as_tensor(np.asarray(scale), dtype=dtype)
    q, x = (q - c) * w, (x - c) * w
    return (x * x).sum(1)[None, :] - 2.0 * (q @ x.T), ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def knn(queries, keys, k, offset=None, scale=None, exclude=None, first=0, last=None, dtype=torch.float64):
    """-> index [n, k] (int64, -1 where fewer than k exist), dist2 [n, k] (+inf there), sel [n, L], dist2 of every pair [n, L].  The
    winners are the k smallest (sel, slot) among the finite selectors of [first, last) but `exclude`; they are written by (dist2, slot)."""
    sel, d2 = (m.numpy() for m in matrices(queries, keys, offset, scale, dtype))
    n, L = sel.shape
    live = np.zeros((n, L), bool)
    live[:, first:L if last is None else last] = True
    live &= np.isfinite(sel)
    if exclude is not None:
        for i, e in enumerate(np.asarray(exclude)):
            if 0 <= e < L:
                live[i, e] = False
    index, dist2 = np.full((n, k), -1, np.int64), np.full((n, k), np.inf, sel.dtype)
    for i in range(n):
        slots = np.flatnonzero(live[i])
        win = slots[np.argsort(sel[i, slots], kind="stable")[:k]]
        win = win[np.lexsort((win, d2[i, win]))]
        index[i, :len(win)], dist2[i, :len(win)] = win, d2[i, win]
    return index, dist2, sel, d2
