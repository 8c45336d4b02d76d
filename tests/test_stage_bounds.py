"""The checker of tests/test_gpu_large_batch.py on the CPU: the a-priori bounds of tests/bounds.py accept correct fp32 computations
in every summation order the engine uses (torch's matmul, a sequential reversed sum, 64-row chunks dealt unevenly over slices as
k_tn64 + k_adam_red do) and reject each defect listed below.  The bounds are worst-case, so the outcome does not depend on the CPU."""
import numpy as np
import pytest
import torch

from tests import bounds as bd

F32 = np.float32


def _data(B, N=48, K=40, seed=0):
    """dY rows scaled by TD errors whose last 64-row tile is 'loud' (tests/bounds.py:make_loud), X rows of ReLU-like activations"""
    rng = np.random.default_rng(seed + B)
    td = bd.make_loud(rng.standard_normal(B).astype(F32), B)
    dY = (td[:, None] * rng.standard_normal((B, N))).astype(F32)
    X = np.maximum(rng.standard_normal((B, K)), 0.0).astype(F32)
    return dY, X


def _torch_wgrad(dY, X):
    return (torch.from_numpy(dY).T @ torch.from_numpy(X)).numpy(), torch.from_numpy(dY).sum(0).numpy()


def _sequential_reversed(dY, X):
    w, b = np.zeros((dY.shape[1], X.shape[1]), F32), np.zeros(dY.shape[1], F32)
    for r in range(dY.shape[0] - 1, -1, -1):
        w = w + np.outer(dY[r], X[r]).astype(F32)
        b = b + dY[r]
    return w, b


def _blocked_slices(dY, X, S=3):
    """64-row chunks, each an fp32 product; ceil(B/64) chunks dealt over S slices (unevenly: 17 and 64 chunks over 3), each slice
    summing its chunks in order, then the S slice partials summed"""
    B = dY.shape[0]
    nch = (B + 63) // 64
    parts = []
    for s in range(S):
        w, b = np.zeros((dY.shape[1], X.shape[1]), F32), np.zeros(dY.shape[1], F32)
        for c in range(s * nch // S, (s + 1) * nch // S):
            cw, cb = _torch_wgrad(dY[64 * c:64 * (c + 1)], X[64 * c:64 * (c + 1)])
            w, b = w + cw, b + cb
        parts.append((w, b))
    w, b = parts[0]
    for pw, pb in parts[1:]:
        w, b = w + pw, b + pb
    return w, b


def _check_wgrad(dY, X, got_w, got_b):
    ww, bw = bd.batch_wgrad(dY, X)
    wb, bb = bd.batch_sum(dY)
    return max(bd.check("dW", got_w, ww, bw), bd.check("db", got_b, wb, bb))


@pytest.mark.parametrize("B", [1025, 4095])
@pytest.mark.parametrize("order", ["torch", "sequential_reversed", "blocked_slices"])
def test_weight_gradient_bounds_accept_every_summation_order(B, order):
    dY, X = _data(B)
    w, b = {"torch": _torch_wgrad, "sequential_reversed": _sequential_reversed, "blocked_slices": _blocked_slices}[order](dY, X)
    assert _check_wgrad(dY, X, w, b) <= 1.0


@pytest.mark.parametrize("B", [1025, 4095])
@pytest.mark.parametrize("defect", ["last_row_dropped", "row_counted_twice", "chunk_dropped"])
def test_weight_gradient_bounds_catch_lost_or_repeated_rows(B, defect):
    dY, X = _data(B)
    if defect == "last_row_dropped":
        w, b = _torch_wgrad(dY[:-1], X[:-1])
    elif defect == "row_counted_twice":
        w, b = _torch_wgrad(np.concatenate([dY, dY[-1:]]), np.concatenate([X, X[-1:]]))
    else:                                                   # one 64-row chunk of ordinary (not loud) rows
        c = (B // 64) // 2
        keep = np.r_[0:64 * c, 64 * (c + 1):B]
        w, b = _torch_wgrad(dY[keep], X[keep])
    with pytest.raises(bd.Violation):
        _check_wgrad(dY, X, w, b)


@pytest.mark.parametrize("B", [1025, 4095])
def test_gemm_and_layernorm_forward_bounds_accept_fp32(B):
    rng = np.random.default_rng(B)
    K, H = 40, 256
    X = rng.standard_normal((B, K)).astype(F32)
    W1, b1 = (rng.standard_normal((H, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    z = (torch.from_numpy(X) @ torch.from_numpy(W1).T + torch.from_numpy(b1)).numpy()
    want, bound = bd.gemm(X, W1, b1)
    assert bd.check("z1", z, want, bound) <= 1.0
    zt = torch.from_numpy(z)
    mu = zt.mean(1, keepdim=True)
    xhat = ((zt - mu) * torch.rsqrt(((zt - mu) ** 2).mean(1, keepdim=True) + 1e-5)).numpy()
    g, be = (1 + 0.1 * rng.standard_normal(H)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    h = np.maximum(xhat * g + be, F32(0))
    want, y, bound = bd.ln_affine_relu(xhat, g, be)
    assert bd.check("h1", h, want, bound, accept=bd.relu_accept(h, y, bound)) <= 1.0


def _ln_case(seed=3, B=96, K=40, H=256):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, K)).astype(F32)
    W1, b1 = (rng.standard_normal((H, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    g = (1 + 0.1 * rng.standard_normal(H)).astype(F32)
    be = (0.1 * rng.standard_normal(H)).astype(F32)
    zt = torch.from_numpy(X) @ torch.from_numpy(W1).T + torch.from_numpy(b1)
    mu = zt.mean(1, keepdim=True)
    rstd = torch.rsqrt(((zt - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    xhat = (zt - mu) * rstd
    h = torch.relu(xhat * torch.from_numpy(g) + torch.from_numpy(be))
    dh = torch.from_numpy((rng.standard_normal((B, H)) * bd.make_loud(np.ones(B, F32), B, 29.0)[:, None]).astype(F32))
    return X, W1, b1, g, xhat, rstd, h, dh


@pytest.mark.parametrize("mean_term", [True, False])
def test_layernorm_backward_bound(mean_term):
    X, W1, b1, g, xhat, rstd, h, dh = _ln_case()
    dxh = dh * (h > 0) * torch.from_numpy(g)
    m1 = dxh.mean(1, keepdim=True) if mean_term else 0.0
    dz = (rstd * (dxh - m1 - xhat * (dxh * xhat).mean(1, keepdim=True))).numpy()
    r64, rho = bd.ln_rstd(X, W1, b1)
    want, bound = bd.ln_bwd(dh.numpy(), h.numpy(), xhat.numpy(), g, r64, rho)
    if mean_term:
        assert bd.check("dz1", dz, want, bound) <= 1.0
        (wg, bg), (wb, bb) = bd.ln_affine_grads(dh.numpy(), h.numpy(), xhat.numpy())
        dy = dh * (h > 0)
        assert bd.check("dgamma", (dy * xhat).sum(0).numpy(), wg, bg) <= 1.0 and bd.check("dbeta", dy.sum(0).numpy(), wb, bb) <= 1.0
        with pytest.raises(bd.Violation):                    # the last (loud) row left out of the affine gradients
            bd.check("dgamma", (dy[:-1] * xhat[:-1]).sum(0).numpy(), wg, bg)
    else:
        with pytest.raises(bd.Violation):
            bd.check("dz1", dz, want, bound)


def _adam_fp32(p, g, m, v, t0, lr, b1, b2, eps, swap=False, bc_lag=0, eps_inside=False):
    """the engine's Adam (csrc/kernels.h: adam_commit) in fp32 numpy, with the listed defects as options"""
    b1f, b2f = F32(b1), F32(b2)
    if swap:
        b1f, b2f = b2f, b1f
    t = t0 + 1 - bc_lag
    with np.errstate(divide="ignore", invalid="ignore"):
        step = F32(np.float64(lr) / (1.0 - np.float64(b1f) ** t))       # (t = 0: an infinite step)
        sq2 = F32(np.sqrt(1.0 - np.float64(b2f) ** t))
        m1 = m + (g - m) * (F32(1) - b1f)
        v1 = v * b2f + g * g * (F32(1) - b2f)
        den = np.sqrt(v1 / sq2 / sq2 + F32(eps)) if eps_inside else np.sqrt(v1) / sq2 + F32(eps)
        return (p - step * (m1 / den)).astype(F32), m1.astype(F32), v1.astype(F32)


def _adam_state(n=20000, seed=5):
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(F32)
    g = (1e-2 * rng.standard_normal(n)).astype(F32)
    m = (1e-3 * rng.standard_normal(n)).astype(F32)
    v = ((1e-2 * rng.standard_normal(n)) ** 2 + 1e-6).astype(F32)
    return p, g, m, v


def _adam_check(p0, g, m0, v0, t0, got, lr=3e-4, coef=1.0, coef_rel=0.0):
    p, m, v = got
    ex = bd.adam_expected(p0, m0, v0, t0, g, lr, m_got=m, v_got=v, coef=coef, coef_rel=coef_rel)
    return max(bd.check("m", m, *ex["m"]), bd.check("v", v, *ex["v"]), bd.check("p", p, *ex["p"]))


@pytest.mark.parametrize("t0", [0, 1000])
def test_adam_bound_accepts_the_fp32_step(t0):
    p, g, m, v = _adam_state()
    if t0 == 0:
        m, v = np.zeros_like(m), np.zeros_like(v)
    assert _adam_check(p, g, m, v, t0, _adam_fp32(p, g, m, v, t0, 3e-4, 0.9, 0.999, 1e-8)) <= 1.0


@pytest.mark.parametrize("t0", [0, 1000])
@pytest.mark.parametrize("defect", ["betas_swapped", "bias_correction_at_t_minus_1", "eps_inside_sqrt"])
def test_adam_bound_catches_defects(t0, defect):
    p, g, m, v = _adam_state()
    if t0 == 0:
        m, v = np.zeros_like(m), np.zeros_like(v)
    got = _adam_fp32(p, g, m, v, t0, 3e-4, 0.9, 0.999, 1e-8, swap=defect == "betas_swapped", bc_lag=int(defect == "bias_correction_at_t_minus_1"),
                     eps_inside=defect == "eps_inside_sqrt")
    with pytest.raises(bd.Violation):
        _adam_check(p, g, m, v, t0, got)


def test_clipped_adam_bound():
    """k_adam: the stored gradient is the unclipped G; coef = min(1, clip / (||G|| + 1e-6)) from an fp32 norm"""
    p, g, m, v = _adam_state(seed=6)
    G = 20.0 * g
    norm = F32(np.sqrt((G.astype(F32) * G.astype(F32)).sum(dtype=F32)))
    coef32 = F32(min(1.0, 0.05 / (float(norm) + 1e-6)))
    got = _adam_fp32(p, (G * coef32).astype(F32), m, v, 1000, 3e-4, 0.9, 0.999, 1e-8)
    coef, rel = bd.clip_coef(G, 0.05)
    assert coef < 1.0
    assert _adam_check(p, G, m, v, 1000, got, coef=coef, coef_rel=rel) <= 1.0
    with pytest.raises(bd.Violation):                      # the step taken with the unclipped gradient
        _adam_check(p, G, m, v, 1000, _adam_fp32(p, G.astype(F32), m, v, 1000, 3e-4, 0.9, 0.999, 1e-8), coef=coef, coef_rel=rel)


@pytest.mark.parametrize("twice", [False, True])
def test_polyak_bound(twice):
    rng = np.random.default_rng(7)
    t0 = (0.1 * rng.standard_normal(50000)).astype(F32)
    w = (t0 + 1e-3 * rng.standard_normal(50000)).astype(F32)
    tau = F32(0.005)
    t = t0 + (w - t0) * tau
    if twice:
        t = t + (w - t) * tau
    want, bound = bd.polyak_expected(t0, w, 0.005)
    if twice:
        with pytest.raises(bd.Violation):
            bd.check("target", t, want, bound)
    else:
        assert bd.check("target", t, want, bound) <= 1.0


@pytest.mark.parametrize("B", [1025, 4095])
def test_alpha_gradient_bound(B):
    rng = np.random.default_rng(B)
    logp = (rng.standard_normal(B) * 3).astype(F32)
    la = F32(np.log(0.2))
    s = F32(0)
    for x in logp:
        s = F32(s + (-x - F32(-3.0)))
    g = F32(np.exp(la) * (s / F32(B)))
    want, bound = bd.alpha_grad_expected(logp, la, -3.0)
    assert bd.check("alpha grad", g, want, bound) <= 1.0
