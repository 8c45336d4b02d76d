"""The checker of tests/test_gpu_large_batch.py and tests/test_gpu_small_batch.py on the CPU: the a-priori bounds of tests/bounds.py
accept correct fp32 computations in every summation order the engine uses (torch's matmul, a sequential reversed sum, 64-row chunks
dealt unevenly over slices as k_tn64 + k_adam_red do, 256-row slabs of four interleaved chunk groups as k_tn does, a K split into 4 or
2 parts as k_nt does) and reject each defect listed below, at large batch sizes and at the small ones where a switch of the
small-batch dispatch leaves a one-row block (17, 113, 257).  The bounds are worst-case, so the outcome does not depend on the CPU."""
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


def _slab_groups(dY, X):
    """k_tn's order below B = 1024: the rows in 256-row slabs, summed slab after slab; inside a slab the 16-row chunks (each an fp32
    product) are dealt round-robin over four groups that accumulate separately and are summed as (a + b) + (c + d).  The bias: 16
    partials (row r in partial r mod 16, each summed in order), then the partials in order."""
    B = dY.shape[0]
    w = np.zeros((dY.shape[1], X.shape[1]), F32)
    for s in range(0, B, 256):
        grp = [np.zeros_like(w) for _ in range(4)]
        for j, c in enumerate(range(s, min(s + 256, B), 16)):
            grp[j % 4] = grp[j % 4] + _torch_wgrad(dY[c:c + 16], X[c:c + 16])[0]
        w = w + ((grp[0] + grp[1]) + (grp[2] + grp[3]))
    b = np.zeros(dY.shape[1], F32)
    for p in range(16):
        part = np.zeros(dY.shape[1], F32)
        for r in range(p, B, 16):
            part = part + dY[r]
        b = b + part
    return w, b


def _split_k(A, W, b, parts):
    """k_nt's order: K in `parts` (4, 2) contiguous parts, each summed in order in fp32, the parts combined as a tree, then the bias"""
    K = A.shape[1]
    acc = []
    for q in range(parts):
        y = np.zeros((A.shape[0], W.shape[0]), F32)
        for k in range(q * K // parts, (q + 1) * K // parts):
            y = y + A[:, k:k + 1] * W[None, :, k]
        acc.append(y)
    while len(acc) > 1:
        acc = [acc[i] + acc[i + 1] for i in range(0, len(acc), 2)]
    return acc[0] + b


ORDERS = {"torch": _torch_wgrad, "sequential_reversed": _sequential_reversed, "blocked_slices": _blocked_slices, "slab_groups": _slab_groups}
BATCHES = [17, 113, 257, 1025, 4095]


def _check_wgrad(dY, X, got_w, got_b):
    ww, bw = bd.batch_wgrad(dY, X)
    wb, bb = bd.batch_sum(dY)
    return max(bd.check("dW", got_w, ww, bw), bd.check("db", got_b, wb, bb))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("order", list(ORDERS))
def test_weight_gradient_bounds_accept_every_summation_order(B, order):
    dY, X = _data(B)
    w, b = ORDERS[order](dY, X)
    assert _check_wgrad(dY, X, w, b) <= 1.0


def _defective_wgrad(dY, X, defect, order):
    B = dY.shape[0]
    if defect == "last_row_dropped":
        return ORDERS[order](dY[:-1], X[:-1])
    if defect == "row_counted_twice":
        return ORDERS[order](np.concatenate([dY, dY[-1:]]), np.concatenate([X, X[-1:]]))
    c = (B // 64) // 2                                      # chunk_dropped: one 64-row chunk of ordinary (not loud) rows
    keep = np.r_[0:64 * c, 64 * (c + 1):B]
    return ORDERS[order](dY[keep], X[keep])


# (B = 17 has fewer than two 64-row chunks: no chunk of ordinary rows to drop)
DEFECTS = [pytest.param(B, d, id=f"{d}-{B}") for B in BATCHES for d in ("last_row_dropped", "row_counted_twice", "chunk_dropped")
           if not (d == "chunk_dropped" and B < 64)]


@pytest.mark.parametrize("B,defect", DEFECTS)
def test_weight_gradient_bounds_catch_lost_or_repeated_rows(B, defect):
    dY, X = _data(B)
    with pytest.raises(bd.Violation):
        _check_wgrad(dY, X, *_defective_wgrad(dY, X, defect, "torch"))


@pytest.mark.parametrize("B,defect", DEFECTS)
def test_weight_gradient_bounds_catch_lost_or_repeated_rows_in_the_slab_order(B, defect):
    """the same defects in k_tn's small-batch summation order"""
    dY, X = _data(B)
    with pytest.raises(bd.Violation):
        _check_wgrad(dY, X, *_defective_wgrad(dY, X, defect, "slab_groups"))


@pytest.mark.parametrize("B", [17, 113, 257])
@pytest.mark.parametrize("parts", [4, 2])
def test_gemm_bound_accepts_a_split_k_and_catches_a_lost_part(B, parts):
    """z2 = h1 W2^T + b2 over K = 256 in k_nt's KS = 4 and KS = 2 orders; a defect: the last sixteenth of K left out"""
    rng = np.random.default_rng(B + parts)
    K = N = 256
    A = np.maximum(rng.standard_normal((B, K)), 0.0).astype(F32)
    W, b = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.standard_normal(N)).astype(F32)
    want, bound = bd.gemm(A, W, b)
    assert bd.check("z2", _split_k(A, W, b, parts), want, bound) <= 1.0
    with pytest.raises(bd.Violation):
        bd.check("z2", _split_k(A[:, :K - 16], W[:, :K - 16], b, parts), want, bound)


@pytest.mark.parametrize("B", BATCHES)
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
    want, bound = bd.ln_xhat(X, W1, b1)
    assert bd.check("xhat1", xhat, want, bound) <= 1.0
    g, be = (1 + 0.1 * rng.standard_normal(H)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    h = np.maximum(xhat * g + be, F32(0))
    want, y, bound = bd.ln_affine_relu(xhat, g, be)
    assert bd.check("h1", h, want, bound, accept=bd.relu_accept(h, y, bound)) <= 1.0


def _xhat_partials(X, W1, b1, parts=16):
    """k_nt's LayerNorm prologue in fp32: z in k order, (mean, M2) per group of 256 / parts columns, the mean of the partial means,
    M2 combined as Chan et al. do, xhat = (z - mean) * rstd"""
    z = _split_k(X, W1, b1, 1)
    H = z.shape[1]
    n = H // parts
    zp = z.reshape(z.shape[0], parts, n)
    ml = zp.sum(2, dtype=F32) * F32(1.0 / n)
    m2 = ((zp - ml[:, :, None]) ** 2).sum(2, dtype=F32)
    mean = ml.sum(1, dtype=F32, keepdims=True) * F32(1.0 / parts)
    M2 = (m2 + F32(n) * (ml - mean) ** 2).sum(1, dtype=F32, keepdims=True)
    rstd = F32(1) / np.sqrt(M2 * F32(1.0 / H) + F32(1e-5))
    return ((z - mean) * rstd).astype(F32)


@pytest.mark.parametrize("B", [17, 113, 257])
@pytest.mark.parametrize("K", [3, 14, 48, 65])
def test_xhat_bound_ties_the_stored_rows_to_the_input_rows(B, K):
    """bounds.ln_xhat accepts the fp32 prologue of the fused trunk form and rejects a first layer that leaves out the last input
    column (a mask one short), one whose last row read the row in front of it, and a mean taken over 255 of the 256 columns"""
    rng = np.random.default_rng(100 * B + K)
    X = rng.standard_normal((B, K)).astype(F32)
    W1, b1 = (rng.standard_normal((256, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.standard_normal(256)).astype(F32)
    want, bound = bd.ln_xhat(X, W1, b1)
    assert bd.check("xhat1", _xhat_partials(X, W1, b1), want, bound) <= 1.0
    masked = X.copy()
    masked[:, -1] = 0
    shifted = X.copy()
    shifted[-1] = X[-2]
    for what, bad in (("column", _xhat_partials(masked, W1, b1)), ("row", _xhat_partials(shifted, W1, b1))):
        with pytest.raises(bd.Violation):
            bd.check(f"xhat1 ({what})", bad, want, bound)
    z = _split_k(X, W1, b1, 1)
    mean = z[:, :255].mean(1, keepdims=True, dtype=F32)
    rstd = F32(1) / np.sqrt(((z - mean) ** 2).mean(1, keepdims=True, dtype=F32) + F32(1e-5))
    with pytest.raises(bd.Violation):
        bd.check("xhat1 (mean)", (z - mean) * rstd, want, bound)


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


@pytest.mark.parametrize("B", BATCHES)
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
