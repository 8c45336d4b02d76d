"""A-priori float64 error bounds for the engine's fp32 stages (tests/test_gpu_large_batch.py; checked on the CPU by
tests/test_stage_bounds.py).

Every stage is recomputed in float64 from the inputs the engine itself read (debug_read / get_params taken before the step), so
the only difference left is the engine's own fp32 rounding.  For that the classical worst-case bound holds whatever the
summation order (sequential, blocked, split over slices, MFMA tiles): with u = 2^-24 and gamma(n) = n u / (1 - n u),
    sum_i a_i b_i  in fp32  differs from the exact value by at most  gamma(n) sum_i |a_i b_i|       (Higham, Thm. 3.5 / 4.4).
The bounds below are that bound times SAFETY = 2, set before any run; none of them is taken from an observed error, and none
allows a fraction of elements to be outside.  (prio_draw_tol is the plain worst case of its add count, without SAFETY: see there.)
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


def ln_xhat(X, W1, b1, eps=1e-5):
    """xhat1 = (z - mean z) rstd of the layer-1 LayerNorm, z = X W1^T + b1, in float64 from the layer's input rows X -- what ties the
    stored xhat1 (every later check's input) to the batch rows: a first-layer tile masked one column short or a row block reading
    another block's rows moves z by whole terms.  First-order bound, every kernel form computing (z - mean) * rstd:
      z     within dz, the GEMM bound (gemm, without SAFETY);
      mean  within dm = mean(dz) + gamma(H + 2) (mean |z| + mean(dz)): the shift of its terms, then its own rounding in any order
            (sequential, or a mean of partial means);
      d = z - mean  within dd = dz + dm + u (|d| + dz + dm);
      rstd  within the relative rho of ln_rstd;
      the product adds u:   |xhat - xhat64| <= rstd (1 + rho) dd + |xhat64| (rho + u)."""
    z, dz = gemm(X, W1, b1)
    dz = dz / SAFETY
    H = z.shape[1]
    rstd, rho = ln_rstd(X, W1, b1, eps)
    mu = z.mean(1, keepdims=True)
    d = z - mu
    mdz = dz.mean(1, keepdims=True)
    dm = mdz + gamma(H + 2) * (np.abs(z).mean(1, keepdims=True) + mdz)
    dd = dz + dm + U * (np.abs(d) + dz + dm)
    xhat = d * rstd
    return xhat, SAFETY * (rstd * (1.0 + rho) * dd + np.abs(xhat) * (rho + U))


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


# ---------------------------------------------------------------------------------------------------- row-local kernels
# (the tails and head backwards around the trunks: tests/test_gpu_tail_edges.py; checked on the CPU by tests/test_tail_bounds.py)

# Worst error of the device's tanhf / expf / logf in units of the float32 spacing at the exact result: profiles/libm_ulp.json
# (tools/libm_ulp.py on an MI355X, 2^22 points per function: 1.33, 0.86, 2.30), rounded up to an integer, plus 1 ulp for the
# rounding of that comparison itself.
LIBM_ULP = {"tanhf": 3, "expf": 2, "logf": 4}
ULP = 2.0 * U                 # the float32 spacing at v is at most 2^-23 |v|
# The pieces of the engine's normal draws, measured EXHAUSTIVELY over the 2^24 arguments of philox_u01 against float64
# (profiles/libm_ulp.json under "noise", tools/libm_ulp.py on an MI355X), each rounded up to the next power of two -- the margin covers
# only the rounding of the comparison itself.  tests/test_noise_model.py ties the record to these constants.
#   rad_rel       sqrtf(-2 ln2 v_log_f32(u)), relative to sqrt(-2 ln u)                    measured 1.278e-7  (> 2^-23)
#   trig_rev_abs  v_sin_f32(u) / v_cos_f32(u), absolute against sin / cos(2 pi u)          measured 1.253e-7 both  (> 2^-23)
#   rad_libm_rel  sqrtf(-2.f logf(u)) of k_rb_fill, relative                               measured 1.500e-7
#   sinf_abs, cosf_abs   the library's sinf / cosf at t = fl32(2 pi_f32 u), absolute against float64 at that t    6.29e-8, 7.03e-8
# logf over the same 2^24 arguments (down to 2^-25, below the 1e-6 where the entry above starts): 2.14 ulp, under LIBM_ULP["logf"].
NOISE = {"rad_rel": 2.0 ** -22, "trig_rev_abs": 2.0 ** -22, "rad_libm_rel": 2.0 ** -22, "sinf_abs": 2.0 ** -23, "cosf_abs": 2.0 ** -23}
LN_EPS = float(np.float32(1e-5))
LOGP_CONST = float(np.float32(0.9189385332046727))
TANH_EPS = float(np.float32(1e-6))


def check_interval(name, got, lo, hi):
    """every element: lo <= got <= hi.  Returns the worst |got - mid| / half-width (0 where the interval is a point that got hits)."""
    got, lo, hi = f64(got), f64(lo), f64(hi)
    got = got.reshape(lo.shape)
    ok = (got >= lo) & (got <= hi)
    if not ok.all():
        out = np.where(ok, -np.inf, np.maximum(lo - got, got - hi))
        i = np.unravel_index(int(np.argmax(out)), out.shape)
        raise Violation(f"{name}: {int((~ok).sum())} of {ok.size} elements outside their interval; worst at {tuple(int(x) for x in i)}: "
                        f"got {got[i]!r} interval [{lo[i]!r}, {hi[i]!r}]")
    hw = 0.5 * (hi - lo)
    ratio = np.where(hw > 0, np.abs(got - 0.5 * (lo + hi)) / np.maximum(hw, 1e-300), 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def ln2_fwd(z2, g, b, ln):
    """The layer-2 LayerNorm + ReLU of a row-local kernel (csrc/kernels.h: ln_fwd), in float64 from the engine's own z2 rows:
    {xhat, rstd, y: (value, bound); h: value; rho}.  The kernel is two-pass: mean (error dm <= gamma(H + 1) mean |z|), d = z - mean,
    var = mean d^2 -- which a shifted mean moves by dm^2 only, mean(d) being 0 -- rounded within gamma(H + 3) (var + dm^2 + eps) (two
    for d, one for the square, H - 1 for the sum, one for + eps); eps = 1e-5f inside the square root; the square root and the
    reciprocal are correctly rounded: 2u.  So rho, the relative error of rstd, has no GEMM term (unlike ln_rstd).
    Without LayerNorm xhat = y = z and rstd = 1 exactly."""
    z = f64(z2)
    if not ln:
        zero = np.zeros_like(z)
        one = np.ones((z.shape[0], 1))
        return {"xhat": (z, zero), "rstd": (one, 0.0 * one), "y": (z, zero), "h": np.maximum(z, 0.0), "rho": 0.0 * one}
    g, b = f64(g), f64(b)
    H = z.shape[1]
    mu = z.mean(1, keepdims=True)
    d = z - mu
    var = (d * d).mean(1, keepdims=True)
    dm = gamma(H + 1) * np.abs(z).mean(1, keepdims=True)
    dvar = dm * dm + gamma(H + 3) * (var + dm * dm + LN_EPS)
    rho = 0.5 * dvar / (var + LN_EPS) + 2.0 * U
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    xhat = d * rstd
    exh = rstd * (1.0 + rho) * (dm + U * np.abs(d)) + np.abs(xhat) * (rho + U)
    y = xhat * g + b
    ey = np.abs(g) * exh + 2.0 * U * (np.abs(xhat * g) + np.abs(b))
    return {"xhat": (xhat, SAFETY * exh), "rstd": (rstd, SAFETY * rho * rstd), "y": (y, SAFETY * ey), "h": np.maximum(y, 0.0), "rho": rho}


def head_dot(h2, Wh, bh):
    """u = h2 Wh^T + bh from the engine's own h2: gemm with K = 256"""
    return gemm(h2, Wh, bh)


def q_head(f, Wh, bh):
    """q = relu(y) . Wh + bh of a critic row whose h2 is not stored, from ln2_fwd's result f: the ReLU is 1-Lipschitz, so h inherits
    y's bound whichever side of 0 an undecided element falls; plus the dot product's gamma(H + 1)"""
    h, (y, ey) = f["h"], f["y"]
    w = f64(Wh).reshape(-1)
    q = h @ w + float(bh)
    return q, np.abs(w) @ ey.T + SAFETY * gamma(h.shape[1] + 1) * (h @ np.abs(w) + abs(float(bh)))


class _Iv:
    """An interval [lo, hi] in float64 that every float32 operation widens outwards by SAFETY roundings (or SAFETY k ulps for a
    library function).  More roundings than the kernel makes (a contracted multiply-add makes one where two are counted here) only
    widen it, so it holds for either code."""

    def __init__(self, lo, hi=None):
        self.lo = f64(lo)
        self.hi = self.lo if hi is None else f64(hi)

    def rnd(self, k=1.0, ulp=U):
        w = SAFETY * k * ulp
        return _Iv(self.lo - w * np.abs(self.lo), self.hi + w * np.abs(self.hi))

    def __add__(self, o):
        o = o if isinstance(o, _Iv) else _Iv(o)
        return _Iv(self.lo + o.lo, self.hi + o.hi).rnd()

    def __neg__(self):
        return _Iv(-self.hi, -self.lo)

    def __sub__(self, o):
        o = o if isinstance(o, _Iv) else _Iv(o)
        return self + (-o)

    def __mul__(self, o):
        o = o if isinstance(o, _Iv) else _Iv(o)
        c = np.stack(np.broadcast_arrays(self.lo * o.lo, self.lo * o.hi, self.hi * o.lo, self.hi * o.hi))
        return _Iv(c.min(0), c.max(0)).rnd()

    def sq(self):
        a, b = self.lo * self.lo, self.hi * self.hi
        lo = np.where((self.lo <= 0) & (self.hi >= 0), 0.0, np.minimum(a, b))
        return _Iv(lo, np.maximum(a, b)).rnd()

    def div_pos(self, o):
        """self / o for o > 0"""
        c = np.stack(np.broadcast_arrays(self.lo / o.lo, self.lo / o.hi, self.hi / o.lo, self.hi / o.hi))
        return _Iv(c.min(0), c.max(0)).rnd()

    def fn(self, f, name):
        """a monotonically increasing library function"""
        return _Iv(f(self.lo), f(self.hi)).rnd(LIBM_ULP[name], ULP)

    def clip(self, a, b):
        return _Iv(np.clip(self.lo, a, b), np.clip(self.hi, a, b))

    def pair(self):
        return self.lo, self.hi


def squash(u, eps, scale, bias):
    """The tanh-squashed Gaussian of the SAC tails (actor_tail_body) as intervals.  u = (value, bound) of the head outputs [B, 2a]
    (head_dot), eps the injected draws [B, a], scale / bias per action dimension.  Returns {tt, sd, x, y, action, logp_el: (lo, hi)
    [B, a]; logp: (lo, hi) [B]}: [lo, hi] goes through tanh, the affine map -5 + 3.5 (tt + 1), exp, x = mean + e sd, tanh,
    1 - y^2 and log(scale (1 - y^2) + 1e-6f) by the monotonicity of each piece, y clipped to [-1, 1]; a first-order bound blows up
    where y saturates.  dx = x - mean is taken as e sd plus the rounding of x (u |x|) and its own, not as the difference of two
    intervals: the kernel subtracts the very mean it added.  The row log-prob is the sum of the elements with gamma(16) on top."""
    uv, ub = f64(u[0]), f64(u[1])
    a = uv.shape[1] // 2
    e, sc, bi = f64(eps), f64(scale), f64(bias)
    u0, u1 = _Iv(uv[:, :a] - ub[:, :a], uv[:, :a] + ub[:, :a]), _Iv(uv[:, a:] - ub[:, a:], uv[:, a:] + ub[:, a:])
    tt = u1.fn(np.tanh, "tanhf").clip(-1.0, 1.0)
    log_std = ((tt + 1.0) * 3.5) + (-5.0)
    sd = log_std.fn(np.exp, "expf")
    p = sd * e
    x = u0 + p
    y = x.fn(np.tanh, "tanhf").clip(-1.0, 1.0)
    action = y * sc + bi
    ax = np.maximum(np.abs(x.lo), np.abs(x.hi))
    dx = _Iv(p.lo - SAFETY * U * ax, p.hi + SAFETY * U * ax).rnd()
    quad = dx.sq().div_pos((sd * sd) * 2.0)
    lg = ((-quad) - sd.fn(np.log, "logf")) - LOGP_CONST
    omy2 = (_Iv(1.0) - y.sq()).clip(0.0, 1.0)
    arg = (omy2 * sc) + TANH_EPS
    el = lg - arg.fn(np.log, "logf")
    mag = np.maximum(np.abs(el.lo), np.abs(el.hi)).sum(1)
    logp = (el.lo.sum(1) - SAFETY * gamma(16) * mag, el.hi.sum(1) + SAFETY * gamma(16) * mag)
    return {"tt": tt.pair(), "sd": sd.pair(), "x": x.pair(), "y": y.pair(), "action": action.pair(), "logp_el": el.pair(), "logp": logp}


def td3_policy(u, scale, bias):
    """TD3's deterministic head: th = tanh(u), action = th scale + bias, as intervals from u = (value, bound)"""
    uv, ub = f64(u[0]), f64(u[1])
    th = _Iv(uv - ub, uv + ub).fn(np.tanh, "tanhf").clip(-1.0, 1.0)
    return {"th": th.pair(), "action": (th * f64(scale) + f64(bias)).pair()}


def smooth_clip(act, eps, td3_std, td3_c, lo, hi):
    """TD3 target smoothing from the unsmoothed action interval act = (lo, hi): clip(act + clip(e std, -c, c), lo, hi).  The clamps are
    exact; the product and the one addition carry u each."""
    std, c = f32c(td3_std), f32c(td3_c)
    nz = (_Iv(f64(eps)) * std).clip(-c, c)
    return (_Iv(*act) + nz).clip(f64(lo), f64(hi)).pair()


def bellman(qt0, qt1, logp_next, log_alpha, rew, done, gamma_, bcq):
    """y = rew + (1 - done) gamma (mix(qt0, qt1) - alpha logp_next) from the engine's own target values (logp_next / log_alpha None:
    TD3): the minimum and maximum are exact, the BCQ mix is three roundings, alpha = expf(log_alpha), two for alpha logp and its
    subtraction, three for the outer products and sum.  done == 1: y == rew bit for bit (the bound is 0)."""
    q0, q1, rew, done = f64(qt0), f64(qt1), f64(rew), f64(done)
    g = f32c(gamma_)
    qmin, qmax = np.minimum(q0, q1), np.maximum(q0, q1)
    if bcq:
        qp = f32c(0.75) * qmin + f32c(0.25) * qmax
        eq = 3.0 * U * (0.75 * np.abs(qmin) + 0.25 * np.abs(qmax))
    else:
        qp, eq = qmin, 0.0 * qmin
    if logp_next is not None:
        alpha = float(np.exp(f64(log_alpha)))
        t = alpha * f64(logp_next)
        eq = eq + (LIBM_ULP["expf"] * ULP + U) * np.abs(t) + U * np.abs(qp - t)
        qp = qp - t
    c = (1.0 - done) * g
    y = rew + c * qp
    bound = np.where(c == 0.0, 0.0, SAFETY * (np.abs(c) * eq + 2.0 * U * np.abs(c * qp) + U * np.abs(y)))
    return y, bound


def tail_dq(q, y, B, w=None):
    """dq = w 2 (q - y) / B from the engine's own q and y: the subtraction, the division (the doubling is exact) and the weight.
    w == 0: dq == 0 exactly."""
    err = f64(q) - f64(y)
    dq = 2.0 * err / float(B)
    if w is not None:
        dq = f64(w) * dq
    return dq, SAFETY * (3.0 if w is None else 4.0) * U * np.abs(dq), err


def ln2_bwd(dy, edy, xhat, exh, g, rstd, rho, ln):
    """dz = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = dy g (ln_bwd of csrc/kernels.h) -- the existing ln_bwd, with the rho
    of ln2_fwd (0 where the engine's own rstd is an input) and two more first-order terms: edy, the error bound of the gated upstream
    gradient dy as the caller computed it, and exh, that of xhat where the kernel did not store it.  edy, exh without SAFETY.
    Without LayerNorm dz = dy."""
    dy, edy = f64(dy), np.broadcast_to(f64(edy), np.shape(dy))
    if not ln:
        return dy, SAFETY * edy
    xhat, exh, g, rstd, rho = f64(xhat), np.broadcast_to(f64(exh), np.shape(dy)), f64(g), f64(rstd), f64(rho)
    H = dy.shape[1]
    dxh = dy * g
    adx, edx = np.abs(dxh), edy * np.abs(g)
    axh = np.abs(xhat)
    m1 = dxh.mean(1, keepdims=True)
    m2 = (dxh * xhat).mean(1, keepdims=True)
    t = dxh - m1 - xhat * m2
    dt = (U * adx + gamma(H + 2) * adx.mean(1, keepdims=True) + axh * gamma(H + 3) * (adx * axh).mean(1, keepdims=True)
          + gamma(3) * (adx + np.abs(m1) + np.abs(xhat * m2))
          + edx + edx.mean(1, keepdims=True) + axh * (edx * axh).mean(1, keepdims=True)
          + exh * np.abs(m2) + axh * (adx * exh).mean(1, keepdims=True))
    return rstd * t, SAFETY * (rstd * (1.0 + rho) * dt + np.abs(t) * rstd * (rho + U))


def tail_colsums(terms, eterms):
    """Column (or scalar) sums over the B rows of a row-local kernel's per-row terms -- sum dy xhat and sum dy (the LayerNorm-2 affine
    gradients), sum h dq and sum dq (the head weight and bias gradients), whatever the block structure: gamma(B + 1) sum |terms|,
    plus the terms' own error bounds eterms (without SAFETY)."""
    t = f64(terms)
    return t.sum(0), SAFETY * (gamma(t.shape[0] + 1) * np.abs(t).sum(0) + np.broadcast_to(f64(eterms), t.shape).sum(0))


def _one_minus_sq(v):
    """1 - v^2 as the kernel's float32 code can produce it: with the square rounded first, or contracted into one multiply-add.
    v^2 is exact in float64 (two 24-bit factors), so both are reproduced bit for bit: (centre, half-width) of their hull.
    v == +-1 gives exactly (0, 0)."""
    v = f64(v)
    sq = v * v
    a = (1.0 - sq.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    b = (1.0 - sq).astype(np.float32).astype(np.float64)
    return 0.5 * (a + b), 0.5 * np.abs(a - b)


def head_bwd(dA, tg, eps, log_alpha, scale, B, sac=True, dA_rel=0.0, edA=0.0):
    """du, the gradient at the actor head's outputs, from the engine's own dA (summed over its critics), a_tg (SAC: tt, sd, yt;
    TD3: th) and the injected draws (actor_head_bwd*_body.inc):
        SAC  g0 = dA sc omy2 + dlogp (2 sc yt omy2) / (sc omy2 + 1e-6f),  omy2 = 1 - yt^2,  dlogp = exp(log_alpha) / B
             mean half g0, log-std half (g0 e sd - dlogp) 3.5 (1 - tt^2)
        TD3  dA sc (1 - th^2)
    1 - v^2 by _one_minus_sq, so that omy2 == 0 gives g0 == 0 exactly.  dA_rel: the relative error of dA itself (u where the kernel
    adds two critics' dA), edA its absolute error bound without SAFETY (the TD3+BC mix).  Returns (value [B, nh], bound)."""
    dA, sc = f64(dA), f64(scale)
    if not sac:
        om, eom = _one_minus_sq(tg)
        v = dA * sc * om
        return v, SAFETY * ((3.0 * U + dA_rel) * np.abs(v) + np.abs(dA * sc) * eom + f64(edA) * sc * om)
    tt, sd, yt = (f64(x) for x in tg)
    e = f64(eps)
    alpha = float(np.exp(f64(log_alpha)))
    dlogp = alpha / float(B)
    r_dl = LIBM_ULP["expf"] * ULP + U                       # relative error of dlogp
    om, eom = _one_minus_sq(yt)
    A = dA * sc * om
    N = 2.0 * sc * yt * om
    D = sc * om + TANH_EPS
    Q = dlogp * N / D
    g0 = A + Q
    dQ_dom = dlogp * 2.0 * sc * np.abs(yt) * TANH_EPS / (D * D)
    eg0 = f64(edA) * sc * om + (3.0 * U + dA_rel) * np.abs(A) + (r_dl + 7.0 * U) * np.abs(Q) + U * np.abs(g0) + (np.abs(dA * sc) + dQ_dom) * eom
    omt, eomt = _one_minus_sq(tt)
    s = g0 * e * sd
    inner = s - dlogp
    raw = inner * 3.5 * omt
    einner = eg0 * np.abs(e * sd) + 2.0 * U * np.abs(s) + r_dl * dlogp + U * np.abs(inner)
    eraw = 3.5 * (einner * omt + np.abs(inner) * eomt) + 2.0 * U * np.abs(raw)
    return np.concatenate([g0, raw], 1), SAFETY * np.concatenate([eg0, eraw], 1)


def bc_mix(dA, q, pi, act, bc_alpha, bc_weight):
    """TD3+BC: the head backward's upstream gradient lambda dA + bc_weight 2 (pi - a) / (B A), lambda = bc_alpha / max(mean |q|, 1e-8f)
    (tests/td3bc_ref.py: closed_form_dpi, with dq/da = -B dA), from the engine's own dA, q_pi, pi and the batch actions.  Bound as
    tests/test_gpu_td3bc.py derives it: lambda carries gamma(B + 2) and its product one rounding, the BC term four, the sum one.
    Returns (value, bound without SAFETY, lambda)."""
    import torch
    from tests import td3bc_ref
    dA, q, pi, act = f64(dA), f64(q), f64(pi), f64(act)
    B, A = dA.shape
    al, w = f32c(bc_alpha), f32c(bc_weight)
    lam = al / max(np.abs(q).mean(), f32c(1e-8))
    v = td3bc_ref.closed_form_dpi(torch.from_numpy(-B * dA), torch.from_numpy(pi), torch.from_numpy(act), lam, w).numpy()
    t1, t2 = lam * dA, (2.0 * w / (B * A)) * (pi - act)
    return v, np.abs(t1) * (gamma(B + 2) + U) + 4.0 * U * np.abs(t2) + U * np.abs(v), lam


def dqda_folded(f2, takes, Wh, W2, h1, xh1, gains, rstd1, rho1, W1, o, a, B, ln):
    """dA_i on the folded path (B < 1024, narrow head, a <= 7), where neither dz2, dh1 nor dz1 of the Q(s, pi) pass is stored: the
    chain composed in float64 from the critic's z2 (f2 = ln2_fwd of it), each stage's bound carried through the next --
    dq = -1/B on the rows the critic takes, dy2 = gate(Wh dq) (an undecided gate: the midpoint, half the step as its error), dz2 =
    ln2_bwd, dh1 = dz2 W2 (gemm, K = 256), the layer-1 gate from the stored h1, dz1 = ln2_bwd with the stored xhat1 and the rstd / rho
    of ln_rstd on the rows of Xp, dA = dz1 W1[:, o : o + a] (gemm, K = 256).  gains: {g2, g1}, the two LayerNorm weights (None without)."""
    wh = f64(Wh).reshape(-1)
    dq = np.where(takes, -1.0 / B, 0.0)
    (xh, exh), (y, ey) = f2["xhat"], f2["y"]
    und = np.abs(y) <= ey
    full = wh[None, :] * dq[:, None]
    dy = np.where(und, 0.5 * full, full * (y > 0))
    edy = np.where(und, 0.5 * np.abs(full), 0.0) + 2.0 * U * np.abs(dy)
    dz2, bz2 = ln2_bwd(dy, edy, xh, exh / SAFETY, None if not ln else gains["g2"], f2["rstd"][0], f2["rho"], ln)
    dh1, bh1 = gemm(dz2, f64(W2).T)
    bh1 = bh1 + bz2 @ np.abs(f64(W2))
    mask = f64(h1) > 0
    dz1, bz1 = ln2_bwd(dh1 * mask, bh1 * mask / SAFETY, xh1, 0.0, None if not ln else gains["g1"], rstd1, rho1, ln)
    W1a = f64(W1)[:, o:o + a]
    dA, bA = gemm(dz1, W1a.T)
    return dA, bA + bz1 @ np.abs(W1a)


def dqda(dz1, W1, o, a):
    """dA_i = dz1_i W1_i[:, o : o + a] on the stored path (k_ln_bwd<16>'s epilogue), from the engine's own c_dz1: gemm over K = 256"""
    return gemm(dz1, f64(W1)[:, o:o + a].T)


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


# ---------------------------------------------------------------------------------------------------- prioritised draw
# (csrc/prio_kernels.h: prio_draw_body; tests/test_gpu_priorities_scale.py; checked on the CPU by tests/test_prio_model.py)

# fp32 adds on the longest path to ...
PRIO_ADDS_GROUP = 3 + 6 + 3         # a group sum: in the thread, the Kogge-Stone steps of a wave, the four wave sums
PRIO_ADDS_LEAF = 16                 # a running sum inside a group: 3 + 6 + 2 (woff) + 1 (woff + before) + 3 (in the thread) + 1 (front + ...)


def prio_draw_tol(T, nch):
    """How far m may lie outside the float64 running-sum interval of the slot a draw selects.  The draw compares m with fp32
    running sums of non-negative terms; a sum reached by n adds is within gamma(n) of the exact one, and none exceeds T.
      top level: the group sums themselves (PRIO_ADDS_GROUP), the same depth again for the scan over them, nch carry adds, the
                 carry + front add and up to 4 adds in the thread                                  -> 2 * 12 + nch + 1 + 4
      residue:   m - excl, one subtract of two values below T                                      -> 1
      leaves:    the running sums inside the chosen group                                          -> PRIO_ADDS_LEAF
    The top level's error moves the group boundary m is compared with, the subtract and the leaf level move the boundary inside
    the group: the three add up.  gamma(n) is already the worst case of every order of n adds, so no SAFETY factor is put on top;
    the count is generous instead (the in-thread adds are counted in the scan depth and again)."""
    return gamma(2 * PRIO_ADDS_GROUP + nch + 1 + 4 + 1 + PRIO_ADDS_LEAF) * float(T)


def prio_draw_interval(name, leaf, length, slots, m, nch, C=None):
    """Every drawn slot s with its m = fl32(u T), as the device or the fp32 model formed it from its own T, against the float64
    inclusive running sums C of the leaves of [0, length):  C[s-1] - tol <= m <= C[s] + tol, tol = prio_draw_tol(C[-1], nch).
    Refused outright: a slot outside [0, length), a slot whose leaf is not positive.  Returns the worst err / tol."""
    leaf = f64(leaf)[:length]
    C = np.cumsum(leaf) if C is None else C
    slots, m = np.asarray(slots, np.int64).reshape(-1), f64(m).reshape(-1)
    assert C.shape == (length,) and slots.shape == m.shape
    bad = (slots < 0) | (slots >= length)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise Violation(f"{name}: draw {i} selected slot {int(slots[i])}, outside the {length} rows held")
    zero = ~(leaf[slots] > 0)
    if zero.any():
        i = int(np.flatnonzero(zero)[0])
        raise Violation(f"{name}: draw {i} selected slot {int(slots[i])}, whose leaf is {leaf[slots[i]]!r}")
    tol = prio_draw_tol(C[-1], nch)
    lo = np.where(slots > 0, C[np.maximum(slots - 1, 0)], 0.0)
    err = np.maximum(np.maximum(lo - m, m - C[slots]), 0.0)
    if (err > tol).any():
        i = int(np.argmax(err))
        raise Violation(f"{name}: {int((err > tol).sum())} of {err.size} draws outside their interval; worst draw {i}: slot {int(slots[i])}, "
                        f"m {m[i]!r} against [{lo[i]!r}, {C[slots[i]]!r}], err {err[i]:.3e} tol {tol:.3e}")
    return float((err / tol).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------- inputs

def loud_rows(B):
    """the rows whose TD errors are made to dominate: the last (partial or full) 64-row tile, which contains the last 16-row block"""
    return np.arange(64 * ((B - 1) // 64), B)


def make_loud(rew, B, offset=30.0):
    rew = np.array(rew, np.float32, copy=True)
    rew[loud_rows(B)] += offset
    return rew
