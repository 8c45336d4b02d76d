"""The checker of tests/test_gpu_tail_edges.py on the CPU.  The row-local kernels (csrc/kernels.h: ln_fwd, ln_bwd, actor_tail_body,
actor_tail_s_body, critic_tail_body.inc, k_actorq_tail, actor_head_bwd*_body.inc) are restated here in fp32 numpy in the summation
orders they use (the building blocks at the end of tests/tail_checks.py) -- a 16-lane tree per row over per-lane partial sums, the
general tail's head dot product split over four waves, column sums per 4-row or 16-row block and then over the blocks -- on the edge inputs of tests/tail_checks.py:make_case with the GPU
cases' own seeds.  The checks of tests/tail_checks.py (bounds from tests/bounds.py) must accept every one of them and raise
bounds.Violation for each defect of DEFECTS, one at a time, on the same inputs.  They also show that no row of any case comes near
the limit of three undecided layer-2 ReLU gates."""
import numpy as np
import pytest

from tests import bounds as bd
from tests import tail_checks as tc
from tests.tail_checks import block_colsum, head, ln_bwd, ln_fwd, ln_of, row_dot, tree16, trunk

F32 = tc.F32
H = tc.H
K1, K2 = tc.K1, tc.K2

CASES, case_seed = tc.CASES, tc.case_seed      # (algo, o, a, B, layer_norm): the table of tests/test_gpu_tail_edges.py

DEFECTS = ["eps_outside_log", "scale_missing", "logstd_3_0", "ln_eps_outside_sqrt", "done_dropped", "tie_to_critic_1", "gate_ge_0",
           "dlogp_sign", "ragged_group_dropped", "weight_not_on_loss", "clip_before_noise"]


def actor_tail(z2, p, eps, c, mode, cfg, defect=None):
    """actor_tail_body / actor_tail_s_body: SAC mode 0 (sample), TD3 mode 0 (policy) or 1 (target smoothing)"""
    a, ln, sac = c["a"], c["ln"], c["sac"]
    narrow = c["nh"] <= 8 and a <= 8
    xh, y, rstd = ln_fwd(z2, *ln_of(p, ln), ln, eps_outside=defect == "ln_eps_outside_sqrt")
    h = np.maximum(y, F32(0))
    u = head(h, p["head.weight"], p["head.bias"], narrow).astype(F32)
    sc, bi = c["scale"], c["bias"]
    out = dict(a_h2=h, a_xh2=xh, a_rs2=rstd)
    a4 = (a + 3) // 4 * 4
    tg = np.zeros((z2.shape[0], 4, a4), F32)
    with np.errstate(divide="ignore", over="ignore"):
        if sac:
            u0, u1 = u[:, :a], u[:, a:]
            tt = np.tanh(u1)
            sd = np.exp(F32(-5.0) + F32(3.0 if defect == "logstd_3_0" else 3.5) * (tt + F32(1)))
            x = u0 + eps * sd
            yt = np.tanh(x)
            dx = x - u0
            l = -(dx * dx) / (F32(2) * sd * sd) - np.log(sd) - F32(0.9189385332046727)
            om = F32(1) - yt * yt
            if defect == "eps_outside_log":
                l = l - (np.log(sc * om) + F32(1e-6))
            elif defect == "scale_missing":
                l = l - np.log(om + F32(1e-6))
            else:
                l = l - np.log(sc * om + F32(1e-6))
            lp = np.zeros((z2.shape[0], 16), F32)
            for j in range(a):
                lp[:, j % 16] = lp[:, j % 16] + l[:, j]
            out["logp"] = tree16(lp)
            out["action"] = yt * sc + bi
            tg[:, 0, :a], tg[:, 1, :a], tg[:, 2, :a] = tt, sd, yt
        else:
            th = np.tanh(u)
            act = th * sc + bi
            if mode == 1:
                nz = np.clip(eps * F32(cfg["td3_std"]), -F32(cfg["td3_c"]), F32(cfg["td3_c"]))
                act = np.clip(act, c["lo"], c["hi"]) + nz if defect == "clip_before_noise" else np.clip(act + nz, c["lo"], c["hi"])
            out["action"] = act
            tg[:, 0, :a] = th
    out["a_tg"] = tg
    return {k: np.asarray(v, F32) for k, v in out.items()}


def critic_tail(R, c, cfg, w, rpb, defect=None):
    """critic_tail_body.inc (rpb = 16) and the fused k_ctail_nn form (16-row blocks as well); rpb = 4 is run too: the bounds do not
    depend on the block structure"""
    B, ln, sac = c["B"], c["ln"], c["sac"]
    eo = defect == "ln_eps_outside_sqrt"
    qt = []
    for i in range(2):
        p = c["critics_t"][i]
        _, y, _ = ln_fwd(R["t_z2"][i], *ln_of(p, ln), ln, eo)
        qt.append(row_dot(np.maximum(y, F32(0)), np.broadcast_to(p["head.weight"][0], y.shape)) + p["head.bias"][0])
    qmin = np.minimum(qt[0], qt[1])
    qp = F32(0.75) * qmin + F32(0.25) * np.maximum(qt[0], qt[1]) if cfg["bcq"] else qmin
    if sac:
        qp = qp - np.exp(F32(cfg["log_alpha"])) * R["logp_next"]
    dn = np.zeros(B, F32) if defect == "done_dropped" else R["done"].astype(F32)
    yv = (R["rew"] + (F32(1) - dn) * F32(cfg["gamma"]) * qp).astype(F32)
    out = dict(q_target=np.stack(qt), targ_q=yv, q=[], c_dz2=[], grads=[])
    loss = F32(0)
    for i in range(2):
        p = c["critics"][i]
        g2, b2 = ln_of(p, ln)
        xh, y, rstd = ln_fwd(R["c_z2"][i], g2, b2, ln, eo)
        h = np.maximum(y, F32(0))
        wo = p["head.weight"][0]
        qv = (row_dot(h, np.broadcast_to(wo, h.shape)) + p["head.bias"][0]).astype(F32)
        err = qv - yv
        dq = F32(2) * err / F32(B)
        if w is not None:
            dq = w * dq
        dy = np.where(y > 0, wo[None, :] * dq[:, None], F32(0)).astype(F32)
        out["q"].append(qv)
        out["c_dz2"].append(ln_bwd(dy, xh, rstd, g2, ln))
        drop = defect == "ragged_group_dropped"
        gr = {"head.weight": block_colsum(h * dq[:, None], rpb, drop)[None, :], "head.bias": block_colsum(dq, rpb, drop).reshape(1)}
        if ln:
            gr[f"{K2}.ln.weight"], gr[f"{K2}.ln.bias"] = block_colsum(dy * xh, rpb, drop), block_colsum(dy, rpb, drop)
        out["grads"].append(gr)
        e2 = err * err if (w is None or defect == "weight_not_on_loss") else w * (err * err)
        loss = loss + block_colsum(e2.astype(F32), rpb)
    out["qf_loss"] = F32(loss * (F32(1) / F32(B)))
    return out


def q_pi_tail(c_z2, c, defect=None):
    """k_actorq_tail: Q(s, pi) of the nq online critics, the minimum's critic per row, dz2"""
    B, ln, nq = c["B"], c["ln"], 2 if c["sac"] else 1
    st = []
    for i in range(nq):
        p = c["critics"][i]
        xh, y, rstd = ln_fwd(c_z2[i], *ln_of(p, ln), ln)
        qv = row_dot(np.maximum(y, F32(0)), np.broadcast_to(p["head.weight"][0], y.shape)) + p["head.bias"][0]
        st.append((xh, y, rstd, qv.astype(F32)))
    if nq == 2:
        first = st[0][3] < st[1][3] if defect == "tie_to_critic_1" else st[0][3] <= st[1][3]
    else:
        first = np.ones(B, bool)
    dz2 = []
    for i in range(nq):
        p = c["critics"][i]
        xh, y, rstd, _ = st[i]
        dq = np.where(first if i == 0 else ~first, -(F32(1) / F32(B)), F32(0)).astype(F32)
        dy = np.where(y > 0, p["head.weight"][0][None, :] * dq[:, None], F32(0)).astype(F32)
        dz2.append(ln_bwd(dy, xh, rstd, ln_of(p, ln)[0], ln))
    return np.stack([s[3] for s in st]), np.stack(dz2), first


def dqda_chain(dz2, p, h1, xh1, rs1, c):
    """what the folded dQ/da path computes per critic: dh1 = dz2 W2, the layer-1 gate and LayerNorm backward, dA = dz1 W1[:, o : o + a]"""
    dh1 = (dz2 @ p[f"{K2}.fc.weight"]).astype(F32)
    dz1 = ln_bwd(np.where(h1 > 0, dh1, F32(0)).astype(F32), xh1, rs1, p.get(f"{K1}.ln.weight"), c["ln"])
    return (dz1 @ p[f"{K1}.fc.weight"][:, c["o"]:c["o"] + c["a"]]).astype(F32)


def head_bwd(R, c, log_alpha, rpb, defect=None, bc=None):
    """actor_head_bwd*_body.inc: du, dh2 = du Wh, the ReLU gate on the stored h2, LayerNorm-2 backward with the stored xhat2 / rstd2,
    the block column sums and the head's weight / bias gradients"""
    B, ln, sac, a, nh = c["B"], c["ln"], c["sac"], c["a"], c["nh"]
    p = c["actor"]
    sc, e = c["scale"], c["eps_a"]
    dA = R["dA"][0] + R["dA"][1] if sac else R["dA"][0]
    if sac:
        tt, sd, yt = tc.split_tg(R["a_tg"], a, True)
        dlogp = np.exp(F32(log_alpha)) / F32(B)
        om = F32(1) - yt * yt
        sign = F32(-1) if defect == "dlogp_sign" else F32(1)
        g0 = dA * sc * om + sign * dlogp * (F32(2) * sc * yt * om) / (sc * om + F32(1e-6))
        raw = (g0 * e * sd - sign * dlogp) * F32(3.5) * (F32(1) - tt * tt)
        du = np.concatenate([g0, raw], 1).astype(F32)
    else:
        th = tc.split_tg(R["a_tg"], a, False)
        if bc is not None:      # kernels.h: bc_lambda, bc_mix
            lam = F32(bc[0]) / np.maximum(np.abs(R["q_pi"][0]).sum(dtype=F32) / F32(B), F32(1e-8))
            dA = lam * dA + (F32(2) * F32(bc[1]) * (F32(1) / (F32(B) * F32(a)))) * (R["action"] - c["act"])
            R["bc_lambda"] = F32(lam)
        du = (dA * sc * (F32(1) - th * th)).astype(F32)
    Wh = p["head.weight"]
    dh = np.zeros((B, H), F32)
    for n in range(nh):
        dh = dh + Wh[n][None, :] * du[:, n:n + 1]
    gate = R["a_h2"] >= 0 if defect == "gate_ge_0" else R["a_h2"] > 0
    dy = np.where(gate, dh, F32(0)).astype(F32)
    g2 = ln_of(p, ln)[0]
    out = dict(a_du=du, a_dz2=ln_bwd(dy, R["a_xh2"], R["a_rs2"], g2, ln))
    drop = defect == "ragged_group_dropped"
    gr = {"head.weight": (du.T.astype(F32) @ R["a_h2"]).astype(F32), "head.bias": block_colsum(du, rpb)}
    if ln:
        gr[f"{K2}.ln.weight"], gr[f"{K2}.ln.bias"] = block_colsum(dy * R["a_xh2"], rpb, drop), block_colsum(dy, rpb, drop)
    out["grads"] = gr
    return out


# ------------------------------------------------------------------------------------------ one emulated iteration, checked

def run_case(case, defect=None, rpb=16, weighted=False, tie=False, degenerate=False, log_alpha=None, bcq=None, bc=None, zero_q=False):
    algo, o, a, B, ln = case
    c = tc.make_case(algo, o, a, B, ln, case_seed(case), degenerate_nets=degenerate)
    sac = c["sac"]
    cfg = dict(gamma=0.99, bcq=(not sac) if bcq is None else bcq, log_alpha=float(np.log(0.2)) if log_alpha is None else log_alpha,
               td3_std=0.2, td3_c=0.5)
    if tie:
        c["critics_t"][1] = c["critics_t"][0]
        c["critics"][1] = c["critics"][0]
    w = c["w"] if weighted else None
    und = 0
    # next-action pass (SAC: the online actor samples a'; TD3: the target actor, smoothed and clamped)
    pn = c["actor"] if sac else c["actor_t"]
    z2n = trunk(pn, c["nobs"], ln)
    nx = actor_tail(z2n, pn, c["eps_c"], c, 0 if sac else 1, cfg, defect)
    tc.check_pass_from_z2(None, "next", z2n, pn, c, c["eps_c"], nx["action"], nx.get("logp"), cfg)
    # critic tail
    Xn, X = np.concatenate([c["nobs"], nx["action"]], 1), np.concatenate([c["obs"], c["act"]], 1)
    R = dict(t_z2=np.stack([trunk(p, Xn, ln) for p in c["critics_t"]]), c_z2=np.stack([trunk(p, X, ln) for p in c["critics"]]),
             rew=c["rew"], done=c["done"].astype(F32), logp_next=nx.get("logp"))
    R.update(critic_tail(R, c, cfg, w, rpb, defect))
    tc.check_critic_tail(None, R, c, cfg, w)
    for i in range(2):
        f = bd.ln2_fwd(R["c_z2"][i], *tc._ln2(c["critics"][i], ln), ln)
        und = max(und, int((np.abs(f["y"][0]) <= f["y"][1]).sum(1).max()))
    if tie:
        assert np.array_equal(R["q_target"][0], R["q_target"][1])
    # policy pass with its backward stores
    z2 = trunk(c["actor"], c["obs"], ln)
    A = actor_tail(z2, c["actor"], c["eps_a"], c, 0, cfg, defect)
    A["a_z2"], A["logp_pi"] = z2, A.get("logp")
    tc.check_policy_stores(None, A, c)
    tc.check_policy_tail(None, A, c, require_saturation=sac and not degenerate)
    # Q(s, pi): dA itself comes from the critics' layer-1 backward, which is not emulated: random, exact zeros where a critic loses
    Xp = np.concatenate([c["obs"], A["action"]], 1)
    if zero_q:
        for p in c["critics"]:
            p["head.weight"], p["head.bias"] = np.zeros_like(p["head.weight"]), np.zeros_like(p["head.bias"])
    st = [trunk(p, Xp, ln, stores=True) for p in c["critics"][:2 if sac else 1]]
    c_z2 = np.stack([s[0] for s in st])
    q_pi, c_dz2, first = q_pi_tail(c_z2, c, defect)
    rng = np.random.default_rng(99)
    dA = (rng.standard_normal((len(c_z2), B, a)) / B).astype(F32)
    dA[0][~first] = 0
    if sac:
        dA[1][first] = 0
    Q = dict(c_z2=c_z2, q_pi=q_pi, c_dz2=c_dz2, dA=dA)
    tc.check_q_pi_tail(None, Q, c, stored_dz2=True)
    for i in range(len(c_z2)):
        f = bd.ln2_fwd(c_z2[i], *tc._ln2(c["critics"][i], ln), ln)
        und = max(und, int((np.abs(f["y"][0]) <= f["y"][1]).sum(1).max()))
    # dQ/da through the critics' first layer, as the folded path composes it (the true dA then feeds the head backward)
    if defect is None:
        dA = np.stack([dqda_chain(c_dz2[i], c["critics"][i], *st[i][1:], c) for i in range(len(c_z2))])
        tc.check_dqda_folded(None, dict(c_z2=c_z2, c_h1=[s[1] for s in st], c_xh1=[s[2] for s in st], Xp=Xp, dA=dA), c, first)
        tc.check_q_pi_tail(None, dict(Q, dA=dA), c, stored_dz2=True)
    # head backward
    A["dA"], A["q_pi"] = dA, q_pi
    A.update(head_bwd(A, c, cfg["log_alpha"], 4 if (c["nh"] <= 8 and a <= 8 and rpb == 16 and B >= 1024) else rpb, defect, bc))
    if zero_q:
        assert not q_pi.any() and not dA.any() and A["bc_lambda"] == F32(F32(bc[0]) / F32(1e-8))
    tc.check_head_bwd(None, A, c, cfg["log_alpha"], bc)
    return und


# ------------------------------------------------------------------------------------------ tests

IDS = [f"{al}-o{o}a{a}-{B}-{'ln' if ln else 'noln'}" for al, o, a, B, ln in CASES]
SMALL = [c for c in CASES if c[3] <= 64]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bounds_accept_the_fp32_kernels_and_no_row_is_near_the_gate_limit(case):
    und = run_case(case)
    assert und <= 1, f"{und} undecided layer-2 gates in one row (limit {tc.MAX_UNDECIDED})"


VARIANTS = {"rpb4": dict(rpb=4), "weighted": dict(weighted=True), "tie": dict(tie=True, bcq=False), "tie_bcq": dict(tie=True, bcq=True),
            "degenerate": dict(degenerate=True), "alpha_lo": dict(log_alpha=-8.0), "alpha_hi": dict(log_alpha=2.0),
            "bc": dict(bc=(2.5, 1.0)), "bc_zero_q": dict(bc=(2.5, 0.5), zero_q=True)}
# (TD3 has no temperature, SAC no behaviour-cloning term)
VARIANT_CASES = [(c, v) for c in SMALL for v in VARIANTS if (c[0] == "sac" or not v.startswith("alpha")) and (c[0] == "td3" or not v.startswith("bc"))]


@pytest.mark.parametrize("case,variant", VARIANT_CASES, ids=[f"{IDS[CASES.index(c)]}-{v}" for c, v in VARIANT_CASES])
def test_bounds_accept_the_variants(case, variant):
    run_case(case, **VARIANTS[variant])


def _defect_case(defect):
    """the smallest case of the table on which the defect can show, and how it is run"""
    sac_ln, sac_noln, td3 = ("sac", 11, 3, 19, True), ("sac", 7, 5, 40, False), ("td3", 13, 7, 21, False)
    if defect == "clip_before_noise":
        return td3, {}
    if defect == "ln_eps_outside_sqrt":
        return sac_ln, dict(degenerate=True)
    if defect == "tie_to_critic_1":
        return sac_ln, dict(tie=True)
    if defect == "weight_not_on_loss":
        return sac_ln, dict(weighted=True)
    if defect == "ragged_group_dropped":
        return sac_ln, dict(rpb=4)
    return (sac_noln if defect == "gate_ge_0" else sac_ln), {}


@pytest.mark.parametrize("defect", DEFECTS)
def test_bounds_reject_each_defect(defect):
    case, kw = _defect_case(defect)
    run_case(case, **kw)                                     # the same inputs pass without the defect
    with pytest.raises(bd.Violation):
        run_case(case, defect=defect, **kw)


def test_exact_values_where_the_arithmetic_is_exact():
    q0, q1 = np.array([1.5, -2.0, 0.25], F32), np.array([1.0, 3.0, 0.25], F32)
    rew, done = np.array([0.1, 31.0, -7.0], F32), np.array([0.0, 1.0, 1.0], F32)
    y, b = bd.bellman(q0, q1, np.array([0.3, 0.2, 0.1], F32), -1.6, rew, done, 0.99, True)
    assert np.array_equal(y[1:], rew[1:].astype(np.float64)) and not b[1:].any() and b[0] > 0
    dq, edq, _ = bd.tail_dq(q0, y, 3, np.array([0.0, 2.0, 1.0], F32))
    assert dq[0] == 0 and edq[0] == 0
    z = np.zeros((1, H))
    dz, bz = bd.ln2_bwd(z, z, z, z, np.ones(H), np.ones((1, 1)), np.zeros((1, 1)), True)
    assert not dz.any() and not bz.any()
    v, e = bd._one_minus_sq(np.array([1.0, -1.0], F32))
    assert not v.any() and not e.any()
    g, bg = bd.head_bwd(np.ones((1, 1)), (np.zeros((1, 1)), np.ones((1, 1)), np.ones((1, 1))), np.ones((1, 1)), 0.0, np.ones(1), 4)
    assert g[0, 0] == 0 and bg[0, 0] == 0
