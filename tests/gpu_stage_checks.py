"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The two families of whole-update checks that several GPU test modules run at their own
shapes: one update against the fp32 oracle, intermediate by intermediate (check_update_qnets_intermediates /
check_update_actor_intermediates: tests/test_gpu_engine.py, tests/test_gpu_large_batch.py), and one iteration stage by stage against
float64 from the engine's own inputs (run_one_iteration / run_fused_critic_iteration: tests/test_gpu_large_batch.py,
tests/test_gpu_small_batch.py, tests/test_gpu_tn_epilogue.py; the bounds are tests/bounds.py's).

Not a test module: every assert carries its own message."""
import numpy as np
import torch

from oracle.manual_grads import ManualAgent
from tests import bounds as bd
from tests.gpu_support import (P, _lib, actor_layout, close, crit_layout, flat_actor, flat_critics, gclose, logp_close, make_pair, same_bits,
                               schema)
from tests.helpers import DIMS, assert_params_close, observe, synth_transitions

K1, K2 = "fc_stack.fc_block_1", "fc_stack.fc_block_2"
H = 256

# the shapes of tests/test_gpu_large_batch.py, on either side of each switch point -- (algo, env, B, layer_norm): why
LARGE_BATCH_CASES = [
    ("sac", "hopper", 1023, True),        # the largest small-batch shape: 4 slabs, last row block of 15 rows (Adam from step 0)
    ("sac", "humanoid", 1025, True),      # one row into the 17th 64-row tile; split-M with uneven slices
    ("td3", "halfcheetah", 1025, True),   # narrow input at a ragged large B
    ("sac", "humanoid", 1472, True),      # below the 2-net tiling switch and the opening trunk's alpha / gather switch
    ("sac", "humanoid", 1473, True),      # past both
    ("td3", "humanoid", 1473, True),      # TD3 past the 2-net switch: target-actor next-action pass, actor-target Polyak
    ("sac", "humanoid", 2048, False),     # k_nt64_ln's ReLU-only prologue in the 64 x 64 form
    ("sac", "hopper", 3008, True),        # below the 1-net switch (fused k_nt, K = 11)
    ("sac", "hopper", 3009, True),        # past it: the tiled pair with K = 11
    ("sac", "humanoid", 3009, True),      # every trunk tiled
    ("td3", "halfcheetah", 4095, True),   # ragged at the top of the scope
    ("sac", "humanoid", 4096, True),      # the top of the scope, wide
    ("sac", "o3a32", 1030, True),         # the widest head (nh = 64) at a large B
    ("td3", "o48a17", 1041, True),        # odd widths at a large B
]


# ------------------------------------------------------------------------------------------ one update against the fp32 oracle

def manual_flat_critic_grads(man, ref):
    ln = ref.hps.layer_norm
    return np.concatenate([schema.dict_to_flat(g, ref.ob_dim + ref.ac_dim, 1, ln) for g in man.tr["q_grads"]])


def check_update_qnets_intermediates(algo, env, B, ln):
    ref, eng, (o, a, bound) = make_pair(algo, env, B, ln)
    man = ManualAgent(ref)
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=3)
    done[::5] = True
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_CRITIC, eps)
    eng.update_qnets()
    out = ref.update_qnets(ref.to_batch(obs, act, rew, nobs, done), eps)
    man.update_qnets(obs, act, rew, nobs, done.float(), eps)
    ldc = (o + a + 3) // 4 * 4
    Xn = eng.debug_read("Xn").reshape(B, ldc)
    close(Xn[:, :o], nobs, 0, 0, "s' in the batch slot")
    close(Xn[:, o:o + a], ref.trace["next_action"], name="next action")
    cond = np.zeros(B)
    if algo == "sac":
        cond = logp_close(eng.debug_read("logp_next"), ref.trace["next_logp"], ref.trace["next_action"], bound, 0.0, "next logp")
    close(eng.debug_read("q_target").reshape(2, B), ref.trace["q_target"], name="target Q")
    # y = r + (1 - d) gamma (q' - alpha logp'): carries gamma alpha x the conditioning bound of logp' (logp_close) on saturated rows
    tq, wq = eng.debug_read("targ_q").astype(np.float64), ref.trace["targ_q"].numpy().astype(np.float64)
    assert (np.abs(tq - wq) <= 1e-5 + 1e-5 * np.abs(wq) + ref.hps.gamma * ref.hps.alpha_init * cond).all(), "Bellman target"
    close(eng.debug_read("q").reshape(2, B), ref.trace["q"], name="online Q")
    for i, c in enumerate(man.tr["q_caches"]):
        if ln:
            close(eng.debug_read("c_xh1").reshape(2, B, H)[i], c["s1"][0], rtol=1e-4, atol=1e-4, name=f"critic{i} xhat1")
        close(eng.debug_read("c_h1").reshape(2, B, H)[i], c["h1"], atol=2e-5, name=f"critic{i} h1")
        close(eng.debug_read("c_z2").reshape(2, B, H)[i], c["z2"], atol=2e-5, name=f"critic{i} z2")
        gclose(eng.debug_read("c_dz2").reshape(2, B, H)[i], c["dz2"], name=f"critic{i} dz2")
        # below B = 1024 the dh1 GEMM's epilogue applies the ReLU gate (csrc/kernels.h: NnFold): c_dh1 holds relu'(z1) dh1 there
        want_dh1 = c["dh1"] if B >= 1024 else c["dh1"] * (c["h1"] > 0).to(c["dh1"].dtype)
        gclose(eng.debug_read("c_dh1").reshape(2, B, H)[i], want_dh1, name=f"critic{i} dh1")
        gclose(eng.debug_read("c_dz1").reshape(2, B, H)[i], c["dz1"], name=f"critic{i} dz1")
    got_g = eng.debug_read("grad_critics").reshape(2, -1)
    want_g = manual_flat_critic_grads(man, ref).reshape(2, -1)
    keys = schema.net_keys(o + a, 1, ln)
    for i in range(2):
        gd, wd = schema.flat_to_dict(got_g[i], o + a, 1, ln), schema.flat_to_dict(want_g[i], o + a, 1, ln)
        for k, _ in keys:
            gclose(gd[k], wd[k], name=f"critic{i} grad {k}")
    close(eng.read_metrics()["loss/qf_loss"], out["loss/qf_loss"], name="qf_loss")
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, 1, "critics after Adam",
                        layout=crit_layout(ref), record=f"update_qnets_intermediates[{algo}-{env}-{B}-{ln}]")
    m, v, step = eng.get_adam_state(_lib.CRITICS)
    assert step == 1, ("critics' Adam step", step)


def check_update_actor_intermediates(algo, env, B, ln):
    ref, eng, (o, a, bound) = make_pair(algo, env, B, ln)
    man = ManualAgent(ref)
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=5)
    g = torch.Generator().manual_seed(6)
    e_a, e_l = torch.randn(B, a, generator=g), torch.randn(B, a, generator=g)
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_ACTOR0, e_a)
    eng.set_noise(_lib.SITE_ALPHA0, e_l)
    eng.update_actor()
    out = ref.update_actor(ref.to_batch(obs, act, rew, nobs, done), e_a, e_l)
    man.update_actor(obs, e_a, e_l)
    ldc = (o + a + 3) // 4 * 4
    nq = 1 if algo == "td3" else 2
    c = man.tr["actor_cache"]
    close(eng.debug_read("a_h1").reshape(B, H), c["h1"], atol=2e-5, name="actor h1")
    close(eng.debug_read("a_h2").reshape(B, H), c["h2"], atol=2e-5, name="actor h2")
    close(eng.debug_read("Xp").reshape(B, ldc)[:, o:o + a], ref.trace["pi_action"], name="pi action")
    close(eng.debug_read("q_pi").reshape(2, B)[:nq], ref.trace["q_pi"][:nq], name="Q(s, pi)")
    if algo == "sac":
        logp_close(eng.debug_read("logp_pi"), ref.trace["pi_logp"], ref.trace["pi_action"], bound, 0.0, "pi logp")
    a4 = (a + 3) // 4 * 4
    dA = eng.debug_read("dA").reshape(2, B, a4)[:nq, :, :a].sum(0)
    gclose(dA, man.tr["dA"], name="dLoss/dAction")
    ldu = (c["u"].shape[1] + 3) // 4 * 4
    gclose(eng.debug_read("a_du").reshape(B, ldu)[:, :c["u"].shape[1]], man.tr["du"], name="d head out")
    gclose(eng.debug_read("a_dz2").reshape(B, H), c["dz2"], name="actor dz2")
    gclose(eng.debug_read("a_dz1").reshape(B, H), c["dz1"], name="actor dz1")
    nh = a if algo == "td3" else 2 * a
    got_g = schema.flat_to_dict(eng.debug_read("grad_actor"), o, nh, ln)
    for (k, _), gr in zip(ref.actor.named_parameters(), ref.trace["actor_grads"]):
        gclose(got_g[k], gr, name=f"actor grad {k}")
    met = eng.read_metrics()
    close(met["loss/actor_loss"], out["loss/actor_loss"], name="actor_loss")
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, 1, "actor after Adam",
                        layout=actor_layout(ref), record=f"update_actor_intermediates[{algo}-{env}-{B}-{ln}]")
    if algo == "sac":
        # drawn through the POST-step actor: inherits Adam's sign-like first step (tests/helpers.py), so per-sample
        # log-probs move by O(lr * |x|) when a near-zero-gradient weight steps the other way; the mean does not
        close(eng.debug_read("logp_alpha"), ref.trace["alpha_logp"].reshape(-1), rtol=2e-3, atol=3e-2, name="alpha logp")
        close(met["loss/alpha_loss"], out["loss/alpha_loss"], rtol=1e-4, atol=1e-4, name="alpha_loss")
        close(met["vitals/alpha"], out["vitals/alpha"], rtol=1e-6, atol=1e-7, name="alpha")
        close(eng.get_params(_lib.LOG_ALPHA)[0], ref.log_alpha, rtol=1e-6, atol=1e-7, name="log_alpha")


# ------------------------------------------------------------------------------------------ optimiser, targets, temperature

def evolve_adam(eng, which, step, seed):
    """non-trivial Adam state: m ~ 1e-3 N(0, 1), v = (1e-3 N(0, 1))^2 + 1e-7 > 0 at `step` (0: zero moments)"""
    n = eng.param_count(which)
    if step == 0:
        eng.set_adam_state(which, np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
        return
    rng = np.random.default_rng(seed)
    eng.set_adam_state(which, (1e-3 * rng.standard_normal(n)).astype(np.float32),
                       ((1e-3 * rng.standard_normal(n)) ** 2 + 1e-7).astype(np.float32), step)


def pre_step_state(eng, which):
    """parameters and Adam state of ONE set before a step: what check_adam steps forward in float64"""
    p = eng.get_params(which)
    try:
        m, v, t = eng.get_adam_state(which)
    except P.EngineError:
        m = v = t = None
    return dict(p=p, m=m, v=v, t=t)


def check_adam(rec, what, eng, which, pre, G, lr, coef=1.0, coef_rel=0.0):
    """every element of m, v, p after one Adam step from `pre` with the engine's own gradient G (tests/bounds.py:adam_expected)"""
    m, v, t = eng.get_adam_state(which)
    p = eng.get_params(which)
    assert t == pre["t"] + 1, (what, t, pre["t"])
    cfg = eng.cfg
    ex = bd.adam_expected(pre["p"], pre["m"], pre["v"], pre["t"], G, lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, m_got=m, v_got=v,
                          coef=coef, coef_rel=coef_rel)
    for k, got in (("m", m), ("v", v), ("p", p)):
        observe(rec, f"{what} Adam {k}: err / bound", bd.check(f"{what} Adam {k}", got, *ex[k]))


def check_polyak(rec, what, eng, which_t, which_w, t0):
    want, bound = bd.polyak_expected(t0, eng.get_params(which_w), eng.cfg.polyak)
    observe(rec, f"{what} Polyak: err / bound", bd.check(f"{what} Polyak", eng.get_params(which_t), want, bound))


def check_alpha(rec, eng, pre, B):
    """the temperature step: its gradient (the alpha loss the engine reports) from the engine's own log-probs, then Adam"""
    g_eng = eng.read_metrics()["loss/alpha_loss"]
    want, bound = bd.alpha_grad_expected(eng.debug_read("logp_alpha"), pre["p"][0], -eng.cfg.ac_dim)
    observe(rec, "alpha gradient: err / bound", bd.check("alpha gradient", np.float32(g_eng), want, bound))
    check_adam(rec, "log_alpha", eng, _lib.LOG_ALPHA, pre, np.array([g_eng], np.float32), eng.cfg.log_alpha_lr)


def check_fixed_alpha(rec, eng, pre):
    """autotune = 0: no temperature step -- log_alpha and its Adam words stay bit for bit what they were before the update, and the
    reported alpha is expf(log_alpha): one fp32 rounding of the float64 value plus the device's measured expf error (bounds.LIBM_ULP)"""
    post = pre_step_state(eng, _lib.LOG_ALPHA)
    for k in ("p", "m", "v"):
        assert same_bits(post[k], pre[k]), (rec, f"fixed temperature: log_alpha's {k} moved", post[k], pre[k])
    assert post["t"] == pre["t"], (rec, "fixed temperature: log_alpha's Adam step count moved", post["t"], pre["t"])
    want = float(np.exp(np.float64(pre["p"][0])))
    bound = (bd.U + bd.LIBM_ULP["expf"] * bd.ULP) * want
    observe(rec, "fixed alpha: err / bound", bd.check("vitals/alpha", np.float32(eng.read_metrics()["vitals/alpha"]), want, bound))


# ------------------------------------------------------------------------------------------ stages

def _nd(flat, in_dim, nh, ln):
    return {k: np.asarray(v, np.float64) for k, v in schema.flat_to_dict(flat, in_dim, nh, ln).items()}


def check_trunk_backward(rec, who, X, p, h1, xh1, dz2, dh1, dz1, grads, ln, B, gated_dh1):
    """dh1 = dz2 W2 (GEMM, K = 256), dz1 (LayerNorm backward, or the ReLU gate), and the layer-1 / layer-2 weight, bias and LayerNorm-affine
    gradients (reductions over the batch) from the engine's own dz2, h1, xhat1, dh1, dz1 and its batch rows X"""
    mask = h1 > 0
    want, bound = bd.gemm(dz2, p[f"{K2}.fc.weight"].T)
    got = np.asarray(dh1, np.float64)
    if gated_dh1:      # (below B = 1024 the critics' dh1 GEMM epilogue applies the ReLU gate: compare where the gate lets dh1 through)
        got, want, bound = got * mask, want * mask, bound * mask
    observe(rec, f"{who} dh1: err / bound", bd.check(f"{who} dh1", got, want, bound))
    if ln:
        rstd, rho = bd.ln_rstd(X, p[f"{K1}.fc.weight"], p[f"{K1}.fc.bias"])
        want, bound = bd.ln_bwd(dh1, h1, xh1, p[f"{K1}.ln.weight"], rstd, rho)
    else:
        want, bound = np.asarray(dh1, np.float64) * mask, 0.0
    observe(rec, f"{who} dz1: err / bound", bd.check(f"{who} dz1", dz1, want, bound))
    for key, (want, bound) in ((f"{K2}.fc.weight", bd.batch_wgrad(dz2, h1)), (f"{K2}.fc.bias", bd.batch_sum(dz2)),
                               (f"{K1}.fc.weight", bd.batch_wgrad(dz1, X)), (f"{K1}.fc.bias", bd.batch_sum(dz1))):
        observe(rec, f"{who} grad {key}: err / bound", bd.check(f"{who} grad {key}", grads[key], want, bound))
    if ln:
        (wg, bg), (wb, bb) = bd.ln_affine_grads(dh1, h1, xh1)
        observe(rec, f"{who} grad {K1}.ln.weight: err / bound", bd.check(f"{who} grad {K1}.ln.weight", grads[f"{K1}.ln.weight"], wg, bg))
        observe(rec, f"{who} grad {K1}.ln.bias: err / bound", bd.check(f"{who} grad {K1}.ln.bias", grads[f"{K1}.ln.bias"], wb, bb))


def check_trunk_forward(rec, who, X, p, h1, xh1, z2, ln):
    """xhat1 from the input rows X (LayerNorm), h1 (LayerNorm affine + ReLU from the engine's xhat1; without LayerNorm
    relu(X W1^T + b1)) and z2 = h1 W2^T + b2 (K = 256)"""
    if ln:
        want, bound = bd.ln_xhat(X, p[f"{K1}.fc.weight"], p[f"{K1}.fc.bias"])
        observe(rec, f"{who} xhat1: err / bound", bd.check(f"{who} xhat1", xh1, want, bound))
        want, y, bound = bd.ln_affine_relu(xh1, p[f"{K1}.ln.weight"], p[f"{K1}.ln.bias"])
    else:
        y, bound = bd.gemm(X, p[f"{K1}.fc.weight"], p[f"{K1}.fc.bias"])
        want = np.maximum(y, 0.0)
    observe(rec, f"{who} h1: err / bound", bd.check(f"{who} h1", h1, want, bound, accept=bd.relu_accept(h1, y, bound)))
    if z2 is not None:
        want, bound = bd.gemm(h1, p[f"{K2}.fc.weight"], p[f"{K2}.fc.bias"])
        observe(rec, f"{who} z2: err / bound", bd.check(f"{who} z2", z2, want, bound))


def run_one_iteration(algo, env, B, ln, rec, adam_step=1000, stages=True, **hp):
    """update_qnets, update_actor, update_targ_nets through the API from an evolved optimiser state, on a batch with loud rows; after each
    update every checkable stage (stages=True) and every optimiser / target / temperature output against float64.  `hp`: further Hps
    fields -- clip_norm (the clipped Adam step), autotune=False (the fixed temperature: check_fixed_alpha)"""
    o, a, bound = DIMS[env]
    ref, eng, _ = make_pair(algo, env, B, ln, rb_capacity=max(4096, B), **hp)
    sac = algo == "sac"
    nh = 2 * a if sac else a
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=3)
    done[::5] = True
    rew = bd.make_loud(rew.numpy(), B)
    g = torch.Generator().manual_seed(4)
    eps_c, eps_a, eps_l = (torch.randn(B, a, generator=g) for _ in range(3))
    for i, which in enumerate((_lib.CRITICS, _lib.ACTOR)):
        evolve_adam(eng, which, adam_step, 10 + i)
    if sac:
        eng.set_adam_state(_lib.LOG_ALPHA, np.array([0.0 if adam_step == 0 else 0.02], np.float32),
                           np.array([0.0 if adam_step == 0 else 4e-4], np.float32), adam_step)
    pre = {w: pre_step_state(eng, w) for w in (_lib.CRITICS, _lib.CRITICS_TARGET, _lib.ACTOR, _lib.ACTOR_TARGET) + ((_lib.LOG_ALPHA,) if sac else ())}

    # ---- critics
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_CRITIC, eps_c)
    eng.update_qnets()
    ldc = (o + a + 3) // 4 * 4
    X = eng.debug_read("X").reshape(B, ldc)[:, :o + a]
    assert np.array_equal(X[:, :o], obs.numpy()) and np.array_equal(X[:, o:], act.numpy()) and np.array_equal(eng.debug_read("rew"), rew), \
        (rec, "the batch slot is not the loaded batch")
    Gc = eng.debug_read("grad_critics").reshape(2, -1)
    if stages:
        rd = {k: eng.debug_read(k).reshape(2, B, H) for k in ("c_xh1", "c_h1", "c_z2", "c_dz2", "c_dh1", "c_dz1")}
        pc = pre[_lib.CRITICS]["p"].reshape(2, -1)
        for i in range(2):
            p = _nd(pc[i], o + a, 1, ln)
            gr = _nd(Gc[i], o + a, 1, ln)
            who = f"critic{i}"
            check_trunk_forward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_z2"][i], ln)
            check_trunk_backward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_dz2"][i], rd["c_dh1"][i], rd["c_dz1"][i], gr, ln, B,
                                 gated_dh1=B < 1024)
    check_adam(rec, "critics", eng, _lib.CRITICS, pre[_lib.CRITICS], Gc.reshape(-1), eng.cfg.qnets_lr)

    # ---- actor (+ temperature)
    eng.set_noise(_lib.SITE_ACTOR0, eps_a)
    eng.set_noise(_lib.SITE_ALPHA0, eps_l)
    eng.update_actor()
    Ga = eng.debug_read("grad_actor")
    if stages:
        p = _nd(pre[_lib.ACTOR]["p"], o, nh, ln)
        gr = _nd(Ga, o, nh, ln)
        Xo = X[:, :o]
        rd = {k: eng.debug_read(k).reshape(B, H) for k in ("a_xh1", "a_h1", "a_z2", "a_h2", "a_dz2", "a_dh1", "a_dz1")}
        ldu = (nh + 3) // 4 * 4
        du = eng.debug_read("a_du").reshape(B, ldu)[:, :nh]
        # (SAC: a_z2 afterwards holds the temperature pass's pre-activation through the stepped actor, whose h1 is not kept: z2 is
        #  checked for TD3 only)
        check_trunk_forward(rec, "actor", Xo, p, rd["a_h1"], rd["a_xh1"], None if sac else rd["a_z2"], ln)
        check_trunk_backward(rec, "actor", Xo, p, rd["a_h1"], rd["a_xh1"], rd["a_dz2"], rd["a_dh1"], rd["a_dz1"], gr, ln, B, gated_dh1=B < 1024)
        for key, (want, bnd) in (("head.weight", bd.batch_wgrad(du, rd["a_h2"])), ("head.bias", bd.batch_sum(du))):
            observe(rec, f"actor grad {key}: err / bound", bd.check(f"actor grad {key}", gr[key], want, bnd))
        # the Q(s, pi) pass: the nq online critics (SAC 2, TD3 1), as stepped above, over Xp = [s | pi(s)] -- a launch of its own shape
        # (2 or 1 nets), whose xhat1, h1 and z2 stay in the critics' buffers
        Xp = eng.debug_read("Xp").reshape(B, ldc)[:, :o + a]
        assert np.array_equal(Xp[:, :o], obs.numpy()), (rec, "the observation columns of Xp are not the loaded batch's")
        pq = eng.get_params(_lib.CRITICS).reshape(2, -1)
        rq = {k: eng.debug_read(k).reshape(2, B, H) for k in ("c_xh1", "c_h1", "c_z2")}
        for i in range(2 if sac else 1):
            check_trunk_forward(rec, f"Q(s, pi) critic{i}", Xp, _nd(pq[i], o + a, 1, ln), rq["c_h1"][i], rq["c_xh1"][i], rq["c_z2"][i], ln)
    if eng.cfg.clip_norm > 0:      # k_adam: the stored gradient is the unclipped G, scaled by the coefficient of its fp32 norm
        coef, rel = bd.clip_coef(Ga, eng.cfg.clip_norm)
        check_adam(rec, "actor (clipped)", eng, _lib.ACTOR, pre[_lib.ACTOR], Ga, eng.cfg.actor_lr, coef=coef, coef_rel=rel)
    else:
        check_adam(rec, "actor", eng, _lib.ACTOR, pre[_lib.ACTOR], Ga, eng.cfg.actor_lr)
    if sac and eng.cfg.autotune:
        check_alpha(rec, eng, pre[_lib.LOG_ALPHA], B)
    elif sac:
        check_fixed_alpha(rec, eng, pre[_lib.LOG_ALPHA])

    # ---- targets (k_polyak)
    eng.update_targ_nets(1)
    check_polyak(rec, "critic targets (k_polyak)", eng, _lib.CRITICS_TARGET, _lib.CRITICS, pre[_lib.CRITICS_TARGET]["p"])
    if not sac:
        check_polyak(rec, "actor target (k_polyak)", eng, _lib.ACTOR_TARGET, _lib.ACTOR, pre[_lib.ACTOR_TARGET]["p"])
    else:
        assert np.array_equal(eng.get_params(_lib.ACTOR_TARGET), pre[_lib.ACTOR_TARGET]["p"]), (rec, "SAC's actor target moved")
    eng.close()


def run_fused_critic_iteration(algo, env, B, ln, rec, adam_step=1000, stages=False):
    """one fused critic-only iteration (sactd3_step): the critic targets lerped in the weight-gradient launch's Adam epilogue (k_tn /
    k_adam_red) and, TD3, the actor target as riding blocks of that launch -- from the engine's own gradient and parameters.
    stages: also the batch slot against the ring rows of the sample it reports, bit for bit, and the critics' trunk forward and
    backward stages from the parameters before the step -- the launches whose opening trunk reads ring rows and carries the gather"""
    o, a, bound = DIMS[env]
    ref, eng, _ = make_pair(algo, env, B, ln, rb_capacity=2 * B)
    rows = [t.numpy() for t in synth_transitions(2 * B, o, a, bound, seed=7)]
    rows[2] = bd.make_loud(rows[2], 2 * B)
    eng.rb_extend(*rows)
    evolve_adam(eng, _lib.CRITICS, adam_step, 12)
    pre = {w: pre_step_state(eng, w) for w in (_lib.CRITICS, _lib.CRITICS_TARGET, _lib.ACTOR, _lib.ACTOR_TARGET)}
    eng.step(False)
    if stages:
        idx = eng.read_batch()["index"]
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < 2 * B, (idx.min(), idx.max())
        X = eng.debug_read("X").reshape(B, (o + a + 3) // 4 * 4)[:, :o + a]
        assert same_bits(X[:, :o], rows[0][idx]) and same_bits(X[:, o:], rows[1][idx]), "batch slot [s | a] != the sampled ring rows"
        assert same_bits(eng.debug_read("rew"), rows[2][idx]), "batch slot rewards != the sampled ring rows"
        assert same_bits(eng.debug_read("done"), rows[4][idx].astype(np.float32)), "batch slot done flags != the sampled ring rows"
        rd = {k: eng.debug_read(k).reshape(2, B, H) for k in ("c_xh1", "c_h1", "c_z2", "c_dz2", "c_dh1", "c_dz1")}
        pc, Gc = pre[_lib.CRITICS]["p"].reshape(2, -1), eng.debug_read("grad_critics").reshape(2, -1)
        for i in range(2):
            p, who = _nd(pc[i], o + a, 1, ln), f"fused critic{i}"
            check_trunk_forward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_z2"][i], ln)
            check_trunk_backward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_dz2"][i], rd["c_dh1"][i], rd["c_dz1"][i],
                                 _nd(Gc[i], o + a, 1, ln), ln, B, gated_dh1=B < 1024)
    check_adam(rec, "critics (fused step)", eng, _lib.CRITICS, pre[_lib.CRITICS], eng.debug_read("grad_critics"), eng.cfg.qnets_lr)
    check_polyak(rec, "critic targets (Adam epilogue)", eng, _lib.CRITICS_TARGET, _lib.CRITICS, pre[_lib.CRITICS_TARGET]["p"])
    assert np.array_equal(eng.get_params(_lib.ACTOR), pre[_lib.ACTOR]["p"]), (rec, "a critic-only iteration moved the actor")
    if algo == "td3":
        check_polyak(rec, "actor target (riding blocks)", eng, _lib.ACTOR_TARGET, _lib.ACTOR, pre[_lib.ACTOR_TARGET]["p"])
    eng.close()
