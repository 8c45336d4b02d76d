"""The edge inputs and the per-stage checks of the row-local kernels (the tails and head backwards around the trunks), shared by
tests/test_gpu_tail_edges.py, which feeds them what the engine wrote, and tests/test_tail_bounds.py, which feeds them an fp32
emulation of the kernels on the CPU -- so the checker that judges the GPU is itself checked, on the same inputs.

A check takes a dict R of buffers under their debug_read names, already reshaped, recomputes one stage in float64 from the buffers the
kernel read (tests/bounds.py) and holds every element of what it wrote to an a-priori bound or interval; nothing is left out, and the
worst err / bound per stage goes to helpers.observe.
"""
import itertools

import numpy as np

from tests import bounds as bd
from tests.helpers import DIMS, observe

H = 256
F32 = np.float32
K1, K2 = "fc_stack.fc_block_1", "fc_stack.fc_block_2"
MEAN_OFFSETS = (0.0, 3.0, -3.0, 6.0, -9.0, 12.0)
LOGSTD_OFFSETS = (0.0, 4.0, -4.0, 9.0, -9.0)
MAX_UNDECIDED = 3

# (algo, env, B, layer_norm): what the shape takes -- B ragged against both the 4-row and the 16-row grouping
CASE_TABLE = [
    ("sac", "hopper", 19, True),          # narrow tail and head backward, folded dQ/da with 8-wide partials
    ("sac", "sac4", 33, True),            # nh = 8, 16-wide partials
    ("sac", "sac5", 40, False),           # nh = 10: the general tail and k_actor_head_bwd below B = 1024
    ("td3", "td3_7", 21, False),          # the widest folded dQ/da
    ("td3", "td3_8", 35, True),           # narrow head without the fold: k_ln_bwd<16>.dQ/da at small B
    ("td3", "o48a17", 35, True),          # a second element per lane
    ("sac", "o3a32", 18, True),           # nh = 64
    ("sac", "hopper", 257, True),         # two 256-row slabs, the second with one row
    ("sac", "hopper", 1025, True),        # k_critic_tail<16>, k_actorq_tail<4>, k_actor_head_bwd_s<4>, k_ln_bwd<16>.dQ/da
    ("td3", "halfcheetah", 1030, True),   # the same forms for TD3, target-actor smoothing
    ("sac", "o3a32", 1030, False),        # the wide head in the large forms
]
CASES = [(al, DIMS[env][0], DIMS[env][1], B, ln) for al, env, B, ln in CASE_TABLE]


def case_seed(case):
    """a case's inputs are drawn from its index in the table (CPU emulation and GPU test use the same)"""
    return 1000 + CASES.index(tuple(case))


# ------------------------------------------------------------------------------------------ inputs

def action_bounds(a):
    """per-dimension, asymmetric: lo_j = -0.4 - 0.3 j, hi_j = 0.2 + 0.5 j; scale and bias as the engine forms them (fp32)"""
    j = np.arange(a)
    lo, hi = (-0.4 - 0.3 * j).astype(F32), (0.2 + 0.5 * j).astype(F32)
    return lo, hi, ((hi - lo) / F32(2)).astype(F32), ((hi + lo) / F32(2)).astype(F32)


def make_net(rng, in_dim, nh, ln):
    p = {"fc_stack.fc_block_1.fc.weight": rng.standard_normal((H, in_dim)) / np.sqrt(in_dim), "fc_stack.fc_block_1.fc.bias": 0.1 * rng.standard_normal(H)}
    if ln:
        p["fc_stack.fc_block_1.ln.weight"], p["fc_stack.fc_block_1.ln.bias"] = 1 + 0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal(H)
    p[f"{K2}.fc.weight"], p[f"{K2}.fc.bias"] = rng.standard_normal((H, H)) / 16.0, 0.1 * rng.standard_normal(H)
    if ln:
        p[f"{K2}.ln.weight"], p[f"{K2}.ln.bias"] = 1 + 0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal(H)
    p["head.weight"], p["head.bias"] = rng.standard_normal((nh, H)) / 8.0, 0.1 * rng.standard_normal(nh)
    return {k: np.asarray(v, F32) for k, v in p.items()}


def degenerate(p, ln, c=0.5):
    """W2 = 0: with LayerNorm b2 = c, so every row has variance 0, xhat 0, rstd 1 / sqrt(1e-5) and y == beta2 (kept >= 0.05 in
    magnitude, so that its ReLU is decided); without, b2 = -c < 0, so h2 == 0, the head's output == bh and dz2 == 0, all exactly"""
    p = dict(p)
    p[f"{K2}.fc.weight"] = np.zeros((H, H), F32)
    p[f"{K2}.fc.bias"] = np.full(H, c if ln else -c, F32)
    if ln:
        b = p[f"{K2}.ln.bias"]
        p[f"{K2}.ln.bias"] = np.where(np.abs(b) < 0.05, np.where(b < 0, -0.05, 0.05), b).astype(F32)
    return p


def make_case(algo, o, a, B, ln, seed, degenerate_nets=False):
    """Engine parameters as {key: fp32 array} per net, a batch and the injected draws, with the edges built in:
    SAC head-bias offsets that saturate both squashes; rows of exact-zero and of +-4 noise; per-dimension action bounds; the last
    16-row block and the 4-row group of rows 4 .. 7 done, with 30 added to their rewards; loss weights with exact zeros and one of 50"""
    rng = np.random.default_rng(seed)
    sac = algo == "sac"
    nh = 2 * a if sac else a
    lo, hi, sc, bi = action_bounds(a)
    actor = make_net(rng, o, nh, ln)
    if sac:     # the phase of the log-std cycle is chosen so that narrow heads still get a +-9 (|tanh| == 1 needs |u| > 9.01)
        j = np.arange(a)
        actor["head.bias"][:a] += np.asarray(MEAN_OFFSETS, F32)[j % 6]
        actor["head.bias"][a:] += np.asarray(LOGSTD_OFFSETS, F32)[(j + max(0, 5 - a)) % 5]
    critics = [make_net(rng, o + a, 1, ln) for _ in range(2)]
    if degenerate_nets:
        actor, critics[1] = degenerate(actor, ln), degenerate(critics[1], ln)
    perturb = lambda p: {k: (v + 0.01 * rng.standard_normal(v.shape)).astype(F32) for k, v in p.items()}
    c = dict(algo=algo, sac=sac, o=o, a=a, nh=nh, B=B, ln=ln, lo=lo, hi=hi, scale=sc, bias=bi,
             actor=actor, actor_t=perturb(actor), critics=critics, critics_t=[perturb(p) for p in critics])
    c["obs"], c["nobs"] = rng.standard_normal((B, o)).astype(F32), rng.standard_normal((B, o)).astype(F32)
    c["act"] = (lo + (hi - lo) * rng.random((B, a))).astype(F32)
    done = np.zeros(B, bool)
    done[16 * ((B - 1) // 16):] = True
    done[4:8] = True
    done[rng.random(B) < 0.05] = True
    rew = rng.standard_normal(B).astype(F32)
    rew[done] += F32(30.0)
    c["rew"], c["done"] = rew, done
    for k in ("eps_c", "eps_a", "eps_l"):
        e = rng.standard_normal((B, a)).astype(F32)
        e[1::5] = 0.0
        e[2::5] = np.where((np.arange(a) + np.arange(B)[2::5, None]) % 2 == 0, 4.0, -4.0)
        c[k] = e
    w = (0.5 + rng.random(B)).astype(F32)
    w[3::7] = 0.0
    w[B - 2] = 50.0
    c["w"] = w
    return c


# ------------------------------------------------------------------------------------------ helpers

def _ob(rec, name, ratio):
    if rec is not None:
        observe(rec, f"{name}: err / bound", ratio)
    return ratio


def _chk(rec, name, got, want, bound, accept=None):
    return _ob(rec, name, bd.check(name, got, want, bound, accept))


def _chi(rec, name, got, iv):
    return _ob(rec, name, bd.check_interval(name, got, *iv))


def _exact(cond, msg):
    if not cond:
        raise bd.Violation(msg)


def _ln2(p, ln):
    return (p[f"{K2}.ln.weight"], p[f"{K2}.ln.bias"]) if ln else (None, None)


def head_from_z2(z2, p, ln):
    """u = relu(LN2(z2)) Wh^T + bh of a pass whose h2 is not kept: ln2_fwd's bound on y carried through the head (the ReLU is
    1-Lipschitz), plus the dot products' own"""
    f = bd.ln2_fwd(z2, *_ln2(p, ln), ln)
    u, bu = bd.gemm(f["h"], p["head.weight"], p["head.bias"])
    return u, bu + f["y"][1] @ np.abs(bd.f64(p["head.weight"])).T


def gated_rows(name, got, y, ey, make_row, skip=None):
    """Rows of a backward stage behind a ReLU whose input y is known only within ey.  make_row(rows, mask) -> (want, bound) for those
    rows under the gate `mask`.  Every row is first tried with mask = y > 0; a row that fails and has undecided elements (|y| <= ey) is
    tried under every choice of them, at most MAX_UNDECIDED per row, and must match one.  Returns (worst ratio, the masks that matched).
    skip: rows whose result does not depend on the gate (upstream gradient exactly 0)."""
    got = bd.f64(got)
    mask = y > 0
    und = np.abs(y) <= ey
    if skip is not None:
        und = und & ~skip[:, None]
    many = np.nonzero(und.sum(1) > MAX_UNDECIDED)[0]
    if many.size:
        raise bd.Violation(f"{name}: row {int(many[0])} has {int(und[many[0]].sum())} undecided ReLU gates (more than {MAX_UNDECIDED})")
    rows = np.arange(y.shape[0])
    want, bound = make_row(rows, mask)
    err = np.abs(got - want)
    bad = np.nonzero((err > bound).any(1))[0]
    for r in bad:
        cols = np.nonzero(und[r])[0]
        hit = False
        for choice in itertools.product((False, True), repeat=len(cols)):
            m = mask[r:r + 1].copy()
            m[0, cols] = choice
            w1, b1 = make_row(np.array([r]), m)
            if (np.abs(got[r:r + 1] - w1) <= b1).all():
                mask[r], want[r], bound[r], hit = m[0], w1[0], b1[0], True
                break
        if not hit:
            break
    return bd.check(name, got, want, bound), mask


# ------------------------------------------------------------------------------------------ critic update

def check_critic_tail(rec, R, c, cfg, w=None):
    """k_ctail_nn<2> / k_critic_tail<16> and their weighted forms.  R: t_z2, c_z2 [2, B, H], rew, done, logp_next (SAC), q_target [2, B],
    targ_q [B], q [2, B], c_dz2 [2, B, H], grads [per net {key: array}], qf_loss.  cfg: gamma, bcq, log_alpha."""
    B, ln, sac = c["B"], c["ln"], c["sac"]
    for i in range(2):
        f = bd.ln2_fwd(R["t_z2"][i], *_ln2(c["critics_t"][i], ln), ln)
        _chk(rec, f"target q{i}", R["q_target"][i], *bd.q_head(f, c["critics_t"][i]["head.weight"], c["critics_t"][i]["head.bias"][0]))
    y, by = bd.bellman(R["q_target"][0], R["q_target"][1], R["logp_next"] if sac else None, cfg["log_alpha"] if sac else None,
                       R["rew"], R["done"], cfg["gamma"], cfg["bcq"])
    _chk(rec, "Bellman target", R["targ_q"], y, by)
    dn = np.asarray(R["done"]) != 0
    assert dn.any()
    _exact(np.array_equal(np.asarray(R["targ_q"])[dn], np.asarray(R["rew"])[dn]), "done rows: y must equal rew bit for bit")
    loss, eloss = 0.0, 0.0
    for i in range(2):
        p = c["critics"][i]
        f = bd.ln2_fwd(R["c_z2"][i], *_ln2(p, ln), ln)
        _chk(rec, f"q{i}", R["q"][i], *bd.q_head(f, p["head.weight"], p["head.bias"][0]))
        dq, edq, err = bd.tail_dq(R["q"][i], R["targ_q"], B, w)
        if w is not None:
            z = np.asarray(w) == 0
            assert z.any()
            _exact(not np.asarray(R["c_dz2"][i])[z].any(), "weight 0: the row's dz2 must be exact zeros")
        wh = bd.f64(p["head.weight"]).reshape(-1)
        (xh, exh), (yy, ey) = f["xhat"], f["y"]
        g2 = p[f"{K2}.ln.weight"] if ln else None

        def row(rows, mask, dq=dq, edq=edq, wh=wh, xh=xh, exh=exh, f=f, g2=g2):
            dy = wh[None, :] * dq[rows, None] * mask
            edy = (np.abs(wh)[None, :] * edq[rows, None] / bd.SAFETY + bd.U * np.abs(dy)) * mask
            return bd.ln2_bwd(dy, edy, xh[rows], exh[rows] / bd.SAFETY, g2, f["rstd"][0][rows], f["rho"][rows], ln)

        ratio, mask = gated_rows(f"critic{i} dz2", R["c_dz2"][i], yy, ey, row, skip=dq == 0)
        _ob(rec, f"critic{i} dz2", ratio)
        dy = wh[None, :] * dq[:, None] * mask
        edy = (np.abs(wh)[None, :] * edq[:, None] / bd.SAFETY + bd.U * np.abs(dy)) * mask
        hq = f["h"] * mask
        sums = {"head.weight": bd.tail_colsums(hq * dq[:, None], np.abs(dq)[:, None] * ey / bd.SAFETY + np.abs(hq) * edq[:, None] / bd.SAFETY),
                "head.bias": bd.tail_colsums(dq, edq / bd.SAFETY)}
        if ln:
            sums[f"{K2}.ln.weight"] = bd.tail_colsums(dy * xh, np.abs(dy) * exh / bd.SAFETY + edy * np.abs(xh))
            sums[f"{K2}.ln.bias"] = bd.tail_colsums(dy, edy)
        for k, (want, bound) in sums.items():
            _chk(rec, f"critic{i} grad {k}", R["grads"][i][k], want, bound)
        t = err * err if w is None else bd.f64(w) * err * err
        loss, eloss = loss + t.sum(), eloss + t.sum()
    # the loss: sum over both critics and all rows of w err^2, over B: the two-level sum's gamma(2 B + 2), 4 u per term
    _chk(rec, "qf_loss", R["qf_loss"], loss / B, bd.SAFETY * (bd.gamma(2 * B + 2) + 4 * bd.U) * eloss / B)


# ------------------------------------------------------------------------------------------ actor passes

def check_policy_stores(rec, R, c, who="policy"):
    """the policy pass's backward stores from its own z2 (readable only while no later pass has overwritten a_z2: TD3): xhat2, rstd2, h2"""
    p, ln = c["actor"], c["ln"]
    f = bd.ln2_fwd(R["a_z2"], *_ln2(p, ln), ln)
    _chk(rec, f"{who} xhat2", R["a_xh2"], *f["xhat"])
    _chk(rec, f"{who} rstd2", R["a_rs2"], f["rstd"][0].reshape(-1), f["rstd"][1].reshape(-1))
    y, ey = f["y"]
    _chk(rec, f"{who} h2", R["a_h2"], f["h"], ey, accept=bd.relu_accept(R["a_h2"], y, ey))


def check_sac_outputs(rec, who, u, eps, c, action, logp, tg=None, require_saturation=False):
    """squash's intervals around the head outputs u = (value, bound): the action, the row log-prob and, where stored, a_tg"""
    s = bd.squash(u, eps, c["scale"], c["bias"])
    if tg is not None:
        tt, sd, yt = tg
        _chi(rec, f"{who} tanh(raw log-std)", tt, s["tt"])
        _chi(rec, f"{who} std", sd, s["sd"])
        _chi(rec, f"{who} y", yt, s["y"])
        if require_saturation:
            assert (np.abs(np.asarray(yt)) == 1).any() and (np.abs(np.asarray(tt)) == 1).any(), "the saturation edge was not reached"
    _chi(rec, f"{who} action", action, s["action"])
    _chi(rec, f"{who} logp", logp, s["logp"])
    return s


def split_tg(tg, a, sac):
    a4 = (a + 3) // 4 * 4
    tg = np.asarray(tg).reshape(-1, 4, a4)
    return (tg[:, 0, :a], tg[:, 1, :a], tg[:, 2, :a]) if sac else tg[:, 0, :a]


def check_policy_tail(rec, R, c, require_saturation=True):
    """the training policy pass from its stored h2: R: a_h2, a_tg, action [B, a] (Xp's action columns), logp_pi (SAC)"""
    p, a = c["actor"], c["a"]
    u = bd.head_dot(R["a_h2"], p["head.weight"], p["head.bias"])
    tg = split_tg(R["a_tg"], a, c["sac"])
    if c["sac"]:
        check_sac_outputs(rec, "policy", u, c["eps_a"], c, R["action"], R["logp_pi"], tg, require_saturation)
    else:
        s = bd.td3_policy(u, c["scale"], c["bias"])
        _chi(rec, "policy tanh", tg, s["th"])
        _chi(rec, "policy action", R["action"], s["action"])


def check_pass_from_z2(rec, who, z2, p, c, eps, action, logp, cfg=None):
    """a pass that keeps nothing for a backward (the next-action pass of update_qnets, the temperature draw), end to end from its z2:
    SAC the sampled action and its log-prob; TD3 the target action with smoothing noise, clamped (cfg: td3_std, td3_c)"""
    u = head_from_z2(z2, p, c["ln"])
    if c["sac"]:
        s = bd.squash(u, eps, c["scale"], c["bias"])
        if action is not None:
            _chi(rec, f"{who} action", action, s["action"])
        _chi(rec, f"{who} logp", logp, s["logp"])
    else:
        s = bd.td3_policy(u, c["scale"], c["bias"])
        _chi(rec, f"{who} action", action, bd.smooth_clip(s["action"], eps, cfg["td3_std"], cfg["td3_c"], c["lo"], c["hi"]))
        act = np.asarray(action)
        assert (np.abs(bd.f64(eps) * bd.f32c(cfg["td3_std"])) > bd.f32c(cfg["td3_c"])).any() and ((act == c["lo"]) | (act == c["hi"])).any(), \
            "neither the noise clamp nor the action clip binds: the edge was not reached"


def check_q_pi_tail(rec, R, c, stored_dz2):
    """Q(s, pi) from c_z2 (the online critics on Xp); the critic that loses the minimum (a tie goes to critic 0) gets dq == 0: exact zeros in
    its dz2 (stored at B >= 1024) and its dA.  R: c_z2 [nq, B, H], q_pi [nq, B], c_dz2, dA [nq, B, a]"""
    B, ln, nq = c["B"], c["ln"], 2 if c["sac"] else 1
    fs = []
    for i in range(nq):
        p = c["critics"][i]
        f = bd.ln2_fwd(R["c_z2"][i], *_ln2(p, ln), ln)
        fs.append(f)
        _chk(rec, f"q_pi{i}", R["q_pi"][i], *bd.q_head(f, p["head.weight"], p["head.bias"][0]))
    first = (np.asarray(R["q_pi"][0]) <= np.asarray(R["q_pi"][1])) if nq == 2 else np.ones(B, bool)
    for i in range(nq):
        takes = first if i == 0 else ~first
        _exact(not np.asarray(R["dA"][i])[~takes].any(), f"critic {i}: dA of rows it does not take must be exact zeros")
        if not stored_dz2:
            continue
        _exact(not np.asarray(R["c_dz2"][i])[~takes].any(), f"critic {i}: dz2 of rows it does not take must be exact zeros")
        p, f = c["critics"][i], fs[i]
        wh = bd.f64(p["head.weight"]).reshape(-1)
        dq = np.where(takes, -1.0 / B, 0.0)
        (xh, exh), (yy, ey) = f["xhat"], f["y"]
        g2 = p[f"{K2}.ln.weight"] if ln else None

        def row(rows, mask, dq=dq, wh=wh, xh=xh, exh=exh, f=f, g2=g2):
            dy = wh[None, :] * dq[rows, None] * mask
            return bd.ln2_bwd(dy, 2.0 * bd.U * np.abs(dy), xh[rows], exh[rows] / bd.SAFETY, g2, f["rstd"][0][rows], f["rho"][rows], ln)

        _ob(rec, f"Q(s, pi) critic{i} dz2", gated_rows(f"Q(s, pi) critic{i} dz2", R["c_dz2"][i], yy, ey, row, skip=dq == 0)[0])
    return first


def check_dqda_stored(rec, R, c):
    """dA_i = dz1_i W1_i[:, o : o + a] where k_ln_bwd<16>'s epilogue forms it from the stored c_dz1"""
    for i in range(2 if c["sac"] else 1):
        want, bound = bd.dqda(R["c_dz1"][i], c["critics"][i]["fc_stack.fc_block_1.fc.weight"], c["o"], c["a"])
        _chk(rec, f"dA{i}", R["dA"][i], want, bound)


def check_dqda_folded(rec, R, c, first):
    """dA on the folded dQ/da path, composed from c_z2 (bounds.dqda_folded).  R: c_z2, c_h1, c_xh1 [nq, B, H], Xp [B, o + a], dA"""
    B, ln, o, a = c["B"], c["ln"], c["o"], c["a"]
    for i in range(2 if c["sac"] else 1):
        p = c["critics"][i]
        f2 = bd.ln2_fwd(R["c_z2"][i], *_ln2(p, ln), ln)
        W1, b1 = p["fc_stack.fc_block_1.fc.weight"], p["fc_stack.fc_block_1.fc.bias"]
        rstd1, rho1 = bd.ln_rstd(R["Xp"], W1, b1) if ln else (np.ones((B, 1)), np.zeros((B, 1)))
        g = {"g2": p[f"{K2}.ln.weight"], "g1": p["fc_stack.fc_block_1.ln.weight"]} if ln else None
        want, bound = bd.dqda_folded(f2, first if i == 0 else ~first, p["head.weight"], p[f"{K2}.fc.weight"], R["c_h1"][i], R["c_xh1"][i], g,
                                     rstd1, rho1, W1, o, a, B, ln)
        _chk(rec, f"dA{i} (folded)", R["dA"][i], want, bound)


def check_head_bwd(rec, R, c, log_alpha, bc=None):
    """the head backward: R: dA [nq, B, a], a_tg, a_h2, a_xh2, a_rs2, a_du [B, nh], a_dz2, grads {key: array} (the actor's).
    bc = (bc_alpha, bc_weight): TD3+BC -- the upstream gradient is bounds.bc_mix of dA, q_pi (R), the policy action (R) and the batch's"""
    B, ln, sac, a, nh = c["B"], c["ln"], c["sac"], c["a"], c["nh"]
    p = c["actor"]
    nq = 2 if sac else 1
    dA = bd.f64(R["dA"][0]) + (bd.f64(R["dA"][1]) if nq == 2 else 0.0)
    edA = 0.0
    if bc is not None:
        dA, edA, lam = bd.bc_mix(dA, R["q_pi"][0], R["action"], c["act"], *bc)
        _chk(rec, "bc lambda", R["bc_lambda"], lam, bd.gamma(B + 2) * lam)
    want, bound = bd.head_bwd(dA, split_tg(R["a_tg"], a, sac), c["eps_a"], log_alpha, c["scale"], B, sac, dA_rel=bd.U if nq == 2 else 0.0, edA=edA)
    _chk(rec, "head backward du", R["a_du"], want, bound)
    if sac:
        tt, sd, yt = split_tg(R["a_tg"], a, sac)
        sat = np.abs(yt) == 1
        _exact(not np.asarray(R["a_du"])[:, :a][sat].any(), "1 - y^2 == 0 must give a mean-half gradient of exactly 0")
    dh, bdh = bd.gemm(R["a_du"], bd.f64(p["head.weight"]).T)
    mask = bd.f64(R["a_h2"]) > 0
    dy, edy = dh * mask, bdh * mask / bd.SAFETY
    g2 = p[f"{K2}.ln.weight"] if ln else None
    rs = bd.f64(R["a_rs2"]).reshape(-1, 1)
    _chk(rec, "actor dz2", R["a_dz2"], *bd.ln2_bwd(dy, edy, R["a_xh2"], 0.0, g2, rs, 0.0, ln))
    if ln:
        xh = bd.f64(R["a_xh2"])
        _chk(rec, f"actor grad {K2}.ln.weight", R["grads"][f"{K2}.ln.weight"], *bd.tail_colsums(dy * xh, edy * np.abs(xh)))
        _chk(rec, f"actor grad {K2}.ln.bias", R["grads"][f"{K2}.ln.bias"], *bd.tail_colsums(dy, edy))
    _chk(rec, "actor grad head.weight", R["grads"]["head.weight"], *bd.batch_wgrad(R["a_du"], R["a_h2"]))
    _chk(rec, "actor grad head.bias", R["grads"]["head.bias"], *bd.batch_sum(R["a_du"]))


# ------------------------------------------------------------------------------------------ fp32 building blocks
# the kernels' summation orders in numpy float32, for the CPU emulations of tests/test_tail_bounds.py and tests/test_policy_bounds.py

def lanes(x):
    """[B, 256] -> [B, 16 lanes, 4 q, 4]: lane `sub` holds columns 4 sub + 64 q .. + 3 (Row16)"""
    return x.reshape(x.shape[0], 4, 16, 4).transpose(0, 2, 1, 3)


def tree16(v):
    """row16_sum: xor 1, xor 2, half mirror, mirror"""
    i = np.arange(16)
    for perm in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        v = v + v[:, perm]
    return v[:, 0]


def sum4(v):
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def row_total(x):
    s = sum4(lanes(x))
    return tree16((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]))


def row_dot(a, b):
    p = lanes(a) * lanes(b)
    d = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    return tree16((d[..., 0] + d[..., 1]) + (d[..., 2] + d[..., 3]))


def ln_fwd(z, g, be, ln, eps_outside=False):
    if not ln:
        return z, z, np.ones(z.shape[0], F32)
    mean = row_total(z) * F32(1.0 / H)
    d = z - mean[:, None]
    var = row_dot(d, d) * F32(1.0 / H)
    rstd = F32(1) / (np.sqrt(var) + F32(1e-5)) if eps_outside else F32(1) / np.sqrt(var + F32(1e-5))
    xh = d * rstd[:, None]
    return xh, xh * g + be, rstd.astype(F32)


def ln_bwd(dy, xh, rstd, g, ln):
    if not ln:
        return dy
    dxh = dy * g
    m1 = row_total(dxh) * F32(1.0 / H)
    m2 = row_dot(dxh, xh) * F32(1.0 / H)
    return (dxh - m1[:, None] - xh * m2[:, None]) * rstd[:, None]


def block_colsum(vals, rpb, drop_last_group=False):
    """column sums per rpb-row block (rows in order), then over the blocks in order"""
    B = vals.shape[0]
    if drop_last_group:
        B = 4 * ((B - 1) // 4)
    tot = np.zeros(vals.shape[1:], F32)
    for b0 in range(0, B, rpb):
        acc = np.zeros(vals.shape[1:], F32)
        for r in range(b0, min(b0 + rpb, B)):
            acc = acc + vals[r]
        tot = tot + acc
    return tot


def ln_of(p, ln):
    return (p[f"{K2}.ln.weight"], p[f"{K2}.ln.bias"]) if ln else (None, None)


def trunk(p, X, ln, stores=False):
    """z2 of a net on rows X (torch-free fp32: the trunk GEMMs have their own tests); stores: also h1, xhat1, rstd1"""
    z1 = (X @ p[f"{K1}.fc.weight"].T + p[f"{K1}.fc.bias"]).astype(F32)
    xh1, rs1 = z1, np.ones(len(X), F32)
    if ln:
        mu = z1.mean(1, keepdims=True)
        rs1 = (F32(1) / np.sqrt(((z1 - mu) ** 2).mean(1, keepdims=True) + F32(1e-5))).astype(F32)
        xh1 = ((z1 - mu) * rs1).astype(F32)
        z1, rs1 = (xh1 * p[f"{K1}.ln.weight"] + p[f"{K1}.ln.bias"]).astype(F32), rs1[:, 0]
    h1 = np.maximum(z1, F32(0))
    z2 = (h1 @ p[f"{K2}.fc.weight"].T + p[f"{K2}.fc.bias"]).astype(F32)
    return (z2, h1, xh1, rs1) if stores else z2


def head(h, Wh, bh, narrow):
    if narrow:        # one dot product per output, reduced over the row's 16 lanes
        return np.stack([row_dot(h, np.broadcast_to(Wh[n], h.shape)) for n in range(Wh.shape[0])], 1) + bh
    part = []         # K split over 4 waves of 64 columns, each accumulated in order; then ((p0 + p1) + (p2 + p3)) + bh
    for w in range(4):
        acc = np.zeros((h.shape[0], Wh.shape[0]), F32)
        for k in range(64 * w, 64 * w + 64):
            acc = acc + h[:, k:k + 1] * Wh[None, :, k]
        part.append(acc)
    return ((part[0] + part[1]) + (part[2] + part[3])) + bh
