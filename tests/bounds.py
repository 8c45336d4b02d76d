"""A-priori float64 error bounds for the engine's fp32 stages (tests/test_gpu_large_batch.py; checked on the CPU by
tests/test_stage_bounds.py).

Every stage is recomputed in float64 from the inputs the engine itself read (debug_read / get_params taken before the step), so
the only difference left is the engine's own fp32 rounding.  For that the classical worst-case bound holds whatever the
summation order (sequential, blocked, split over slices, MFMA tiles): with u = 2^-24 and gamma(n) = n u / (1 - n u),
    sum_i a_i b_i  in fp32  differs from the exact value by at most  gamma(n) sum_i |a_i b_i|       (Higham, Thm. 3.5 / 4.4).
The bounds below are that bound times SAFETY = 2, set before any run; none of them is taken from an observed error, and none
allows a fraction of elements to be outside.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def f32c(x):
    """the float64 value of an fp32 constant (what the engine's float config fields hold)"""
    return float(np.float32(x))


class Violation(AssertionError):
    pass


def check(name, got, want, bound, accept=None):
    """every element: |got - want| <= bound (or accept[i]).  Returns the worst |err| / bound."""
    got, want, bound = f64(got), f64(want), np.broadcast_to(f64(bound), np.shape(want))
    got = got.reshape(want.shape)
    err = np.abs(got - want)
    ok = err <= bound
    if accept is not None:
        ok = ok | accept
    if not ok.all():
        i = np.unravel_index(int(np.argmax(np.where(ok, -np.inf, err - bound))), err.shape)
        raise Violation(f"{name}: {int((~ok).sum())} of {ok.size} elements outside the bound; worst at {tuple(int(x) for x in i)}: "
                        f"got {got[i]!r} want {want[i]!r} err {err[i]:.3e} bound {bound[i]:.3e}")
    ratio = np.where(err <= bound, err / np.maximum(bound, 1e-300), 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------- GEMMs and reductions

def gemm(A, W, b=None):
    """y = A W^T (+ b) over K = A.shape[1]: float64 value and the bound SAFETY gamma(K + 1) (|A| |W|^T + |b|)"""
    A, W = f64(A), f64(W)
    y = A @ W.T
    mag = np.abs(A) @ np.abs(W).T
    if b is not None:
        y = y + f64(b)
        mag = mag + np.abs(f64(b))
    return y, SAFETY * gamma(A.shape[1] + 1) * mag


def batch_wgrad(dY, X):
    """dW = dY^T X, a reduction over the B rows: K -> B"""
    return gemm(f64(dY).T, f64(X).T)


def batch_sum(dY):
    """db = sum over the B rows"""
    dY = f64(dY)
    return dY.sum(0), SAFETY * gamma(dY.shape[0] + 1) * np.abs(dY).sum(0)


# ---------------------------------------------------------------------------------------------------- LayerNorm

def ln_affine_relu(xhat, g, b):
    """h = relu(xhat g + b) from the engine's own xhat: value, pre-activation y and an elementwise bound (at most three roundings
    of any association of (z - mu) rstd g + b).  Where |y| is inside the bound either side of the ReLU is accepted."""
    xhat, g, b = f64(xhat), f64(g), f64(b)
    y = xhat * g + b
    bound = SAFETY * gamma(3) * (np.abs(xhat * g) + np.abs(b))
    return np.maximum(y, 0.0), y, bound


def relu_accept(got, y, bound):
    """inside the bound around y = 0 the fp32 result may sit on either side of the ReLU: 0, or y within the bound"""
    got = f64(got).reshape(y.shape)
    return (np.abs(y) <= bound) & ((got == 0.0) | (np.abs(got - y) <= bound))


def ln_rstd(X, W1, b1, eps=1e-5):
    """rstd of the layer-1 LayerNorm, recomputed in float64 from the layer's input rows X (rstd is not read back), and the bound
    rho on the engine's relative rstd error: its z1 differs from z64 by the GEMM bound dz, which moves the variance by at most
    2 sqrt(var) (2 max dz) + (2 max dz)^2; the variance's own rounding (one- or two-pass) is within gamma(H + 3) (mean z^2 + mu^2);
    the reciprocal square root adds 2 u."""
    z, dz = gemm(X, W1, b1)
    dz = dz / SAFETY
    H = z.shape[1]
    mu = z.mean(1, keepdims=True)
    var = ((z - mu) ** 2).mean(1, keepdims=True)
    dmax = 2.0 * dz.max(1, keepdims=True)
    dvar = 2.0 * np.sqrt(var) * dmax + dmax * dmax + gamma(H + 3) * ((z * z).mean(1, keepdims=True) + mu * mu)
    rho = 0.5 * dvar / (var + eps) + 2.0 * U
    return 1.0 / np.sqrt(var + eps), rho


def ln_bwd(dh, h, xhat, g, rstd, rho):
    """dz = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = relu'(y) dh g, from the engine's dh, h (ReLU mask), xhat, with the
    float64 rstd of ln_rstd.  First-order bound: the rounding of dxh, of the two row means (gamma(H + 2), gamma(H + 3)), of the
    three-term combination (gamma(3)), and the relative error rho of the engine's rstd (plus its final product)."""
    dh, xhat, g, rstd = f64(dh), f64(xhat), f64(g), f64(rstd)
    H = dh.shape[1]
    dy = dh * (f64(h) > 0)
    dxh = dy * g
    adx = np.abs(dxh)
    m1 = dxh.mean(1, keepdims=True)
    m2 = (dxh * xhat).mean(1, keepdims=True)
    t = dxh - m1 - xhat * m2
    dt = (U * adx + gamma(H + 2) * adx.mean(1, keepdims=True) + np.abs(xhat) * gamma(H + 3) * (adx * np.abs(xhat)).mean(1, keepdims=True)
          + gamma(3) * (adx + np.abs(m1) + np.abs(xhat * m2)))
    rho = f64(rho)
    bound = SAFETY * (rstd * (1.0 + rho) * dt + np.abs(t) * rstd * (rho + U))
    return rstd * t, bound


def ln_affine_grads(dh, h, xhat):
    """dgamma = sum_rows dy xhat, dbeta = sum_rows dy (dy = relu'(y) dh), reductions over the batch"""
    dy = f64(dh) * (f64(h) > 0)
    B = dy.shape[0]
    prod = dy * f64(xhat)
    return (prod.sum(0), SAFETY * gamma(B + 1) * np.abs(prod).sum(0)), (dy.sum(0), SAFETY * gamma(B + 1) * np.abs(dy).sum(0))


# ---------------------------------------------------------------------------------------------------- optimiser, targets

def adam_expected(p0, m0, v0, t0, g, lr, b1=0.9, b2=0.999, eps=1e-8, m_got=None, v_got=None, coef=1.0, coef_rel=0.0):
    """torch.optim.Adam (non-amsgrad, no weight decay) on one tensor from (p0, m0, v0, step t0) with gradient coef g, in float64,
    with the fp32 values of the configured constants (the engine's config holds them as float; so does its bias correction).
    Returns {m, v, p: (value, bound)}.
        |m - m64| <= 4u (|m0| + |g|),  |v - v64| <= 4u (v0 + g^2),  |p - p64| <= u |p64| + 8u |p64 - p0|
    p64 is the step taken with the engine's own m and v (m_got, v_got: each checked against m64, v64 above), so a cancellation in
    m cannot inflate its relative error into p.  coef_rel: the relative error of a gradient scale computed in fp32 (the clip
    coefficient's norm, gamma(n)): it widens m, v and p by the matching amount."""
    b1, b2, eps, lr = f32c(b1), f32c(b2), f32c(eps), f32c(lr)
    p0, m0, v0, g = f64(p0), f64(m0), f64(v0), f64(g) * coef
    t = int(t0) + 1
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * g * g
    bm = 4.0 * U * (np.abs(m0) + np.abs(g)) + (1.0 - b1) * np.abs(g) * coef_rel
    bv = 4.0 * U * (v0 + g * g) + (1.0 - b2) * g * g * 2.0 * coef_rel
    mu = m if m_got is None else f64(m_got).reshape(m.shape)
    vu = v if v_got is None else f64(v_got).reshape(v.shape)
    step = lr / (1.0 - b1 ** t)
    sq2 = np.sqrt(1.0 - b2 ** t)
    p = p0 - step * (mu / (np.sqrt(vu) / sq2 + eps))
    bp = U * np.abs(p) + (8.0 * U + coef_rel) * np.abs(p - p0)
    return {"m": (m, bm), "v": (v, bv), "p": (p, bp)}


def polyak_expected(t0, w, tau):
    """t = t0 + tau (w - t0) from the engine's own post-step online parameters w: |t - t64| <= 3u (|t64| + tau |w - t0|)"""
    t0, w = f64(t0), f64(w)
    tau = f32c(tau)
    t = t0 + tau * (w - t0)
    return t, 3.0 * U * (np.abs(t) + tau * np.abs(w - t0))


def alpha_grad_expected(logp, log_alpha, targ_ent):
    """d alpha_loss / d log_alpha = exp(log_alpha) mean(-logp - targ_ent) (oracle/manual_grads.py: update_actor) from the engine's
    own log-probs: the batch mean's rounding gamma(B + 2) plus 3 u for exp, the product and the division"""
    logp = f64(logp)
    terms = -logp - float(targ_ent)
    alpha = float(np.exp(f64(log_alpha)))
    g = alpha * terms.mean()
    return g, SAFETY * (alpha * gamma(logp.size + 2) * np.abs(terms).mean() + 3.0 * U * abs(g))


def clip_coef(G, clip):
    """coef = min(1, clip / (||G||_2 + 1e-6)) in float64 and the relative error of the engine's fp32 norm, gamma(n)"""
    G = f64(G)
    return min(1.0, float(clip) / (float(np.sqrt((G * G).sum())) + 1e-6)), gamma(G.size + 2)


# ---------------------------------------------------------------------------------------------------- inputs

def loud_rows(B):
    """the rows whose TD errors are made to dominate: the last (partial or full) 64-row tile, which contains the last 16-row block"""
    return np.arange(64 * ((B - 1) // 64), B)


def make_loud(rew, B, offset=30.0):
    rew = np.array(rew, np.float32, copy=True)
    rew[loud_rows(B)] += offset
    return rew
