"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A plain restatement of the feature-rank call (include/sactd3_feature_rank.h) in torch at a
dtype of the caller's choice (float64: the reference; float32 on the CPU: the yardstick of the tolerance).  Used by
tests/test_gpu_feature_rank.py and tests/test_feature_rank_host.py.  Not a test module: pytest does not rewrite its asserts."""
import numpy as np
import torch

from tests import dormant_model, init_model


def gram_and_spectrum(params, o, a, td3, ln, x, dtype):
    """([3, 256, 256], [3, 256] descending) float64 numpy: M = h2^T h2 / V and its eigenvalues per net (actor, Q1, Q2) over the rows
    x = [s | a], computed in `dtype`; V == 0 gives zeros"""
    grams, lams = [], []
    for _, K, nh, flat in init_model.nets_of(params, o, a, td3):
        h = dormant_model.hidden(flat, K, nh, ln, x, dtype)[1]
        m = h.T @ h / max(len(x), 1)
        grams.append(m.double().numpy())
        lam = torch.linalg.eigvalsh(m).flip(0)
        if not torch.isfinite(lam).all():      # (LAPACK's float32 driver has returned NaN on a rank-1 matrix: the singular values of a
            lam = torch.linalg.svdvals(m)      # symmetric positive semi-definite matrix are its eigenvalues, descending already)
        lams.append(lam.clamp_min(0).double().numpy())
    return np.stack(grams), np.stack(lams)


def summary(lam, delta=0.01, floor=1e-4):
    """the header's formulas in float64 on one descending spectrum -> dict(rank, srank, erank, stable, lambda_sum, sigma, share):
    `share` the cumulative share of sigma (what srank thresholds at 1 - delta)"""
    lam = np.maximum(np.asarray(lam, np.float64), 0.0)
    if lam[0] <= 0.0:
        return dict(rank=0, srank=0, erank=0.0, stable=0.0, lambda_sum=0.0, sigma=np.zeros_like(lam), share=np.zeros_like(lam))
    sigma = np.where(lam > floor * lam[0], np.sqrt(lam), 0.0)
    share = np.cumsum(sigma) / sigma.sum()
    p = sigma[sigma > 0] / sigma.sum()
    return dict(rank=int((sigma > 0).sum()), srank=int(np.argmax(share >= 1.0 - delta)) + 1, erank=float(np.exp(-(p * np.log(p)).sum())),
                stable=float(lam.sum() / lam[0]), lambda_sum=float(lam.sum()), sigma=sigma, share=share)
