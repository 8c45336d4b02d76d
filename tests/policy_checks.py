"""The float64 intervals of a policy query (csrc/policy_kernels.h: k_pi_head; include/sactd3.h: sactd3_policy_device), shared by
tests/test_gpu_policy.py, which feeds them what the engine wrote, and tests/test_policy_bounds.py, which feeds them an fp32 emulation of
the kernel on the CPU -- so the checker that judges the GPU is itself checked, on the same inputs.

Everything is derived from the engine's own z2 rows (debug_read "pi_z2"): tail_checks.head_from_z2 (bounds.ln2_fwd, the head's gemm
bound), then bounds.squash for mode / sample / sample_logp and the intervals below for the inverse squash and action_logp.  Every
operation widens its interval outwards by bounds.SAFETY roundings (bounds._Iv), logf by bounds.LIBM_ULP["logf"] ulps, the one division by
one rounding; no tolerance is taken from an observed error, and no element is left out.
"""
import numpy as np

from tests import bounds as bd
from tests import tail_checks as tc

F32 = np.float32
M32 = F32(1.0 - 1e-6)        # the clamp of the inverse squash: 1 - 17 * 2^-24
assert M32.view(np.uint32) == 0x3F7FFFEF
M = float(M32)


def unscale32(g, scale, bias):
    """v = (g - bi) / sc exactly as the kernel forms it: one float32 subtraction, one IEEE float32 division"""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((np.asarray(g, F32) - np.asarray(bias, F32)) / np.asarray(scale, F32)).astype(F32)


def row_flags(g, scale, bias):
    """(rows the kernel counts as clamped, rows it counts as NaN): any |v_j| > M; any NaN component"""
    v = unscale32(g, scale, bias)
    with np.errstate(invalid="ignore"):
        return (np.abs(v) > M32).any(1), np.isnan(np.asarray(g, F32)).any(1)


def inverse_squash(g, scale, bias):
    """The inverse squash as intervals: v = (g - bi) / sc (a subtraction and a division, one rounding each), c = clamp(v, -M, M)
    (exact), x' = 0.5 (logf(1 + c) - logf(1 - c)): the two sums, the two logf, their difference, the halving.  -> (c, x') as _Iv.
    NaN components are replaced by 0 here: their rows are judged by their NaN alone."""
    g, sc, bi = bd.f64(g), bd.f64(scale), bd.f64(bias)
    g = np.where(np.isnan(g), 0.0, g)
    big = 3.0e38                                              # (an infinite component: any value beyond the clamp will do)
    g = np.clip(g, -big, big)
    v = (bd._Iv(g) - bi).div_pos(bd._Iv(np.broadcast_to(sc, g.shape)))
    c = v.clip(-M, M)
    up = (bd._Iv(1.0) + c).fn(np.log, "logf")
    dn = (bd._Iv(1.0) - c).fn(np.log, "logf")
    return c, (up - dn) * 0.5


def head_intervals(u, a):
    uv, ub = bd.f64(u[0]), bd.f64(u[1])
    return bd._Iv(uv[:, :a] - ub[:, :a], uv[:, :a] + ub[:, :a]), bd._Iv(uv[:, a:] - ub[:, a:], uv[:, a:] + ub[:, a:])


def action_logp_interval(u, g, scale, bias):
    """log pi(g | s) = sum_j [-(x' - mean)^2 / (2 sd^2) - logf(sd) - C - logf(sc (1 - c^2) + 1e-6f)] as an interval [n]: mean and sd
    from the head intervals exactly as bounds.squash forms them, x' and c from inverse_squash; d' = x' - mean is a genuine difference
    of two independent values (unlike the sample's dx).  The row sum carries gamma(16) on top, as the sample's does."""
    a = np.shape(g)[1]
    u0, u1 = head_intervals(u, a)
    tt = u1.fn(np.tanh, "tanhf").clip(-1.0, 1.0)
    sd = (((tt + 1.0) * 3.5) + (-5.0)).fn(np.exp, "expf")
    c, xp = inverse_squash(g, scale, bias)
    d = xp - u0
    quad = d.sq().div_pos((sd * sd) * 2.0)
    lg = ((-quad) - sd.fn(np.log, "logf")) - bd.LOGP_CONST
    omc2 = (bd._Iv(1.0) - c.sq()).clip(0.0, 1.0)
    el = lg - ((omc2 * bd.f64(scale)) + bd.TANH_EPS).fn(np.log, "logf")
    mag = np.maximum(np.abs(el.lo), np.abs(el.hi)).sum(1)
    return el.lo.sum(1) - bd.SAFETY * bd.gamma(16) * mag, el.hi.sum(1) + bd.SAFETY * bd.gamma(16) * mag


def log_std_interval(u, a):
    _, u1 = head_intervals(u, a)
    tt = u1.fn(np.tanh, "tanhf").clip(-1.0, 1.0)
    return (((tt + 1.0) * 3.5) + (-5.0)).pair(), tt.pair()


def check_policy_outputs(rec, z2, params, case, io):
    """Every output of a policy query held to its float64 interval.  z2 [n, 256]: the trunk rows the head kernel read; params: the actor's
    {key: array}; case: ln, sac, a, scale, bias; io: the outputs that were asked for, under the names of sactd3_policy_io (mode, mean,
    log_std, sample, sample_logp, action_logp) with the inputs they belong to (`eps`: the draws the sample used, given or eps_out;
    `actions`).  A row with a NaN action must hold a NaN action_logp, every other row a value inside its interval.  Returns
    {name: worst position inside the interval} and what saturated: {tt, y: whether any |.| == 1 lies inside the intervals' reach}."""
    a, ln = case["a"], case["ln"]
    sc, bi = case["scale"], case["bias"]
    u = tc.head_from_z2(z2, params, ln)
    seen = {}
    if not case["sac"]:
        s = bd.td3_policy(u, sc, bi)
        seen["mode"] = tc._chi(rec, "policy mode", io["mode"], s["action"])
        assert set(io) <= {"mode"}, "TD3 has `mode` only"
        return seen
    zero = np.zeros((np.shape(z2)[0], a))
    s0 = bd.squash(u, zero, sc, bi)
    if "mode" in io:
        seen["mode"] = tc._chi(rec, "policy mode", io["mode"], s0["action"])
    if "mean" in io:
        uv, ub = bd.f64(u[0])[:, :a], bd.f64(u[1])[:, :a]
        seen["mean"] = tc._chk(rec, "policy mean", io["mean"], uv, ub)
    if "log_std" in io:
        seen["log_std"] = tc._chi(rec, "policy log_std", io["log_std"], log_std_interval(u, a)[0])
    if "sample" in io or "sample_logp" in io:
        s = bd.squash(u, io["eps"], sc, bi)
        if "sample" in io:
            seen["sample"] = tc._chi(rec, "policy sample", io["sample"], s["action"])
        if "sample_logp" in io:
            seen["sample_logp"] = tc._chi(rec, "policy sample_logp", np.asarray(io["sample_logp"]).reshape(-1), s["logp"])
    if "action_logp" in io:
        got = np.asarray(io["action_logp"], F32).reshape(-1)
        _, nan_rows = row_flags(io["actions"], sc, bi)
        tc._exact(np.array_equal(np.isnan(got), nan_rows), "action_logp must be NaN on exactly the rows with a NaN action component")
        lo, hi = action_logp_interval(u, io["actions"], sc, bi)
        ok = ~nan_rows
        seen["action_logp"] = tc._chi(rec, "policy action_logp", got[ok], (lo[ok], hi[ok]))
    return seen
