"""The checker of tests/test_gpu_policy.py on the CPU.  k_pi_head (csrc/policy_kernels.h) is restated here in fp32 numpy in its
documented order of operations -- ln_fwd, the head product in the form of the acting tail of the same head shape (tests/tail_checks.py:
head), the squash, the inverse squash with its clamp at M = float32(1 - 1e-6), the row sums as a 16-lane tree -- on the edge inputs of
tail_checks.make_case (saturating head-bias offsets, per-dimension asymmetric action bounds) at the GPU test's shapes, with benign and
with degenerate nets.  policy_checks.check_policy_outputs must accept every one of them and raise bounds.Violation for each defect of
DEFECTS, one at a time, on the same inputs."""
import functools

import numpy as np
import pytest

from tests import bounds as bd
from tests import policy_checks as pc
from tests import tail_checks as tc
from tests.helpers import DIMS
from tests.tail_checks import head, ln_fwd, ln_of, tree16, trunk

F32 = np.float32
N = 67
# name -> (algo, env, layer_norm): the shapes of tests/test_gpu_policy.py
SHAPES = {"sac-hopper": ("sac", "hopper", True), "sac-humanoid": ("sac", "humanoid", True), "sac-hopper-noln": ("sac", "hopper", False),
          "td3-halfcheetah": ("td3", "halfcheetah", True)}
SAC = [k for k, v in SHAPES.items() if v[0] == "sac"]
DEFECTS = ["eps_dropped", "half_missing", "no_division_by_scale", "no_clamp", "clamp_at_1", "jacobian_from_mode_y", "jacobian_sign",
           "log_std_constants_swapped", "log_sd_dropped", "dx_from_rerounded_mean", "scale_bias_of_dim_0"]


@functools.lru_cache(maxsize=None)
def make(shape, degenerate):
    """the case, its z2 rows and the given actions: rows 0 .. 4 carry the edges -- every component at its upper bound, at its lower
    bound, at hi + 1, one +inf component, one NaN component; rows 5 .. 35 are the policy's own samples for the case's draws (where a
    dimension's std is exp(-5) only an action next to its mean keeps the quadratic term, and with it the interval, small enough to
    show an error in the other terms); the rest are drawn uniformly inside the bounds"""
    algo, env, ln = SHAPES[shape]
    o, a, _ = DIMS[env]
    c = tc.make_case(algo, o, a, N, ln, 2000 + list(SHAPES).index(shape), degenerate_nets=degenerate)
    z2 = trunk(c["actor"], c["obs"], ln)
    g = c["act"].copy()
    g[0], g[1], g[2] = c["hi"], c["lo"], c["hi"] + F32(1)
    g[3, a - 1], g[4, 0] = np.inf, np.nan
    if c["sac"]:
        g[5:36] = emu_pi_head(z2, c["actor"], c, c["eps_a"], g)["sample"][5:36]
    return c, z2, g


def emu_pi_head(z2, p, c, eps, g, defect=None):
    """k_pi_head in fp32 numpy -> the outputs under the names of sactd3_policy_io"""
    a, ln, sac = c["a"], c["ln"], c["sac"]
    narrow = c["nh"] <= 8 and a <= 8
    _, y, _ = ln_fwd(z2, *ln_of(p, ln), ln)
    u = head(np.maximum(y, F32(0)), p["head.weight"], p["head.bias"], narrow).astype(F32)
    sc, bi = c["scale"], c["bias"]
    if defect == "scale_bias_of_dim_0":
        sc, bi = np.full_like(sc, sc[0]), np.full_like(bi, bi[0])
    if not sac:
        return dict(mode=(np.tanh(u) * sc + bi).astype(F32))
    C, M = F32(0.9189385332046727), pc.M32

    def rowsum(l):
        lp = np.zeros((z2.shape[0], 16), F32)
        for j in range(a):
            lp[:, j % 16] = lp[:, j % 16] + l[:, j]
        return tree16(lp)

    with np.errstate(all="ignore"):
        u0, u1 = u[:, :a], u[:, a:]
        tt = np.tanh(u1)
        log_std = F32(3.5) + F32(-5.0) * (tt + F32(1)) if defect == "log_std_constants_swapped" else F32(-5.0) + F32(3.5) * (tt + F32(1))
        sd = np.exp(log_std)
        lsd = F32(0) if defect == "log_sd_dropped" else np.log(sd)
        te = F32(0) if defect == "eps_dropped" else F32(1e-6)
        x = u0 + eps * sd
        yt = np.tanh(x)
        # (a mean that went through a half-precision copy on its way to the subtraction)
        dx = x - (u0.astype(np.float16).astype(F32) if defect == "dx_from_rerounded_mean" else u0)
        jac = np.log(sc * (F32(1) - yt * yt) + te)
        el = -(dx * dx) / (F32(2) * sd * sd) - lsd - C
        el = el + jac if defect == "jacobian_sign" else el - jac
        v = (g - bi) if defect == "no_division_by_scale" else (g - bi) / sc
        cl = {"no_clamp": None, "clamp_at_1": F32(1)}.get(defect, M)
        cc = v if cl is None else np.minimum(np.maximum(v, -cl), cl)       # (fmaxf / fminf: a NaN gives way to the bound)
        cc = np.where(np.isnan(v) & (cl is not None), -(cl or F32(0)), cc).astype(F32)
        xp = (F32(1.0) if defect == "half_missing" else F32(0.5)) * (np.log(F32(1) + cc) - np.log(F32(1) - cc))
        dp = xp - (u0.astype(np.float16).astype(F32) if defect == "dx_from_rerounded_mean" else u0)
        yj = np.tanh(u0) if defect == "jacobian_from_mode_y" else cc
        jac_a = np.log(sc * (F32(1) - yj * yj) + te)
        ela = -(dp * dp) / (F32(2) * sd * sd) - lsd - C
        ela = ela + jac_a if defect == "jacobian_sign" else ela - jac_a
        alp = rowsum(ela.astype(F32))
        alp = np.where(np.isnan(g).any(1), F32(np.nan), alp)
        out = dict(mode=np.tanh(u0) * sc + bi, mean=u0, log_std=log_std, sample=yt * sc + bi, sample_logp=rowsum(el.astype(F32)), action_logp=alp)
    return {k: np.asarray(v, F32) for k, v in out.items()}


def run(shape, degenerate, defect=None):
    c, z2, g = make(shape, degenerate)
    out = emu_pi_head(z2, c["actor"], c, c["eps_a"], g, defect)
    io = dict(out, eps=c["eps_a"], actions=g) if c["sac"] else out
    return c, out, pc.check_policy_outputs(None, z2, c["actor"], c, io)


def test_the_clamp_constant_and_the_inverse_on_the_cpu():
    """M = float32(1 - 1e-6) = 0x3F7FFFEF = 1 - 17 * 2^-24, and the fp32 formula 0.5 (log(1 + c) - log(1 - c)) stays within 4.7e-7 of
    atanh over [-M, M] (2^16 points and both ends); its interval contains the float64 atanh of every point"""
    assert float(pc.M32) == 1.0 - 17 * 2.0 ** -24
    c = np.concatenate([np.linspace(-pc.M, pc.M, 1 << 16), [pc.M, -pc.M, 0.0]]).astype(F32)
    x = F32(0.5) * (np.log(F32(1) + c) - np.log(F32(1) - c))
    assert np.abs(x.astype(np.float64) - np.arctanh(c.astype(np.float64))).max() <= 4.7e-7
    ci, xi = pc.inverse_squash(c[None, :], np.ones(1, F32), np.zeros(1, F32))
    assert (xi.lo <= np.arctanh(bd.f64(c))).all() and (np.arctanh(bd.f64(c)) <= xi.hi).all()
    assert (xi.lo <= x).all() and (x <= xi.hi).all()


@pytest.mark.parametrize("degenerate", [False, True], ids=["benign", "degenerate"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_emulated_kernel_passes_every_interval(shape, degenerate):
    c, out, seen = run(shape, degenerate)
    if not c["sac"]:
        assert set(seen) == {"mode"}
        return
    assert set(seen) == {"mode", "mean", "log_std", "sample", "sample_logp", "action_logp"}
    clamped, nan = pc.row_flags(make(shape, degenerate)[2], c["scale"], c["bias"])
    assert nan.sum() == 1 and nan[4] and clamped[2] and clamped[3] and clamped[0] and clamped[1] and not clamped[36:].any()
    assert np.isfinite(out["action_logp"][~nan]).all() and np.isfinite(out["sample_logp"]).all()
    if degenerate:      # both squashes saturate: tanh(raw) == +-1 <=> log_std is exactly 2 or -5; y == +-1 <=> sample == bi +- sc
        assert np.isin(out["log_std"], (F32(2), F32(-5))).any(), "tanh(raw log-std) did not saturate"
        assert ((out["sample"] == c["bias"] + c["scale"]) | (out["sample"] == c["bias"] - c["scale"])).any(), "y did not saturate"


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("shape", SAC)
def test_every_seeded_defect_is_caught(shape, defect):
    with pytest.raises(bd.Violation):
        run(shape, False, defect)


def test_the_dimension_0_defect_is_caught_for_td3():
    with pytest.raises(bd.Violation):
        run("td3-halfcheetah", False, "scale_bias_of_dim_0")
