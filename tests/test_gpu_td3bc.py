"""GPU: TD3+BC (include/sactd3.h: sactd3_set_bc) -- the BC forms of the head-backward kernels and of the actor-loss finalisation,
stage by stage against float64; one computation through every route, bit for bit; node counts; boundaries; and the direction the
term is there for.  The float64 restatement is tests/td3bc_ref.py (checked against its closed form on the CPU)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import bounds as bd
from tests import td3bc_ref as R
from tests.gpu_support import (P, _lib, actor_layout, assert_same_state, build_engines, close_engines, engine_state, flat_actor,  # noqa: F401
                               flat_critics, gclose, push_params, schema, track)
from tests.helpers import DIMS, assert_params_close, observe, synth_transitions

pytestmark = pytest.mark.gpu

H = 256
SHAPES = dict(DIMS, o10a8=(10, 8, 1.0))      # tests/helpers.DIMS has no 8-action shape: the narrow head WITHOUT the dQ/da fold


def make_bc_pair(shape, B, ln=True, seed=0, use_graphs=True, bc_alpha=2.5, rb_capacity=4096, max_envs=8, randomize=True, **hp):
    """the oracle's TD3 agent (its modules carry the parameters) and an engine with the same parameters; bc_alpha = 0: plain TD3"""
    ref, (eng,), dims = build_engines("td3", SHAPES[shape], B, ln=ln, seed=seed, cap=rb_capacity, max_envs=max_envs, use_graphs=use_graphs,
                                      randomize=randomize, bc_alpha=bc_alpha, **hp)
    return ref, eng, dims


# ------------------------------------------------------------------------------------------ 1. stages against float64

# (shape, B, layer_norm, clip_norm, bc_weight): which kernel forms
CASES = [
    ("halfcheetah", 256, True, 0.0, 1.0),     # k_headbwd_nn_bc + QaFold, 16-float partials
    ("halfcheetah", 256, True, 1e-3, 1.0),    # ... with clip_norm: k_tn_bc stores the gradient, k_gradnorm + k_adam step
    ("td3_2", 64, True, 0.0, 0.25),           # 8-float partials; bc_weight through set_bc
    ("td3_7", 40, False, 0.0, 1.0),           # widest fold, ragged last row block, no LayerNorm
    ("o10a8", 48, True, 0.0, 1.0),            # narrow head without the fold: k_ln_bwd<16>.dQ/da + k_headbwd_nn_bc
    ("o48a17", 96, True, 0.0, 1.0),           # k_qtail_nn + the general k_actor_head_bwd_bc; actions 16.. in the element loop's second pass
    ("halfcheetah", 1024, True, 0.0, 1.0),    # k_actorq_tail<4> + k_actor_head_bwd_s_bc<4>
    ("o48a17", 1024, True, 0.0, 1.0),         # k_actorq_tail<4> + k_actor_head_bwd_bc
]
EXPECT_KERNEL = {("halfcheetah", 256): "k_headbwd_nn_bc", ("td3_2", 64): "k_headbwd_nn_bc", ("td3_7", 40): "k_headbwd_nn_bc",
                 ("o10a8", 48): "k_headbwd_nn_bc", ("o48a17", 96): "k_actor_head_bwd_bc", ("halfcheetah", 1024): "k_actor_head_bwd_s_bc<4>",
                 ("o48a17", 1024): "k_actor_head_bwd_bc"}


@pytest.mark.parametrize("shape,B,ln,clip,w", CASES, ids=[f"{s}-{b}-{'ln' if l else 'noln'}-clip{c:g}-w{w:g}" for s, b, l, c, w in CASES])
def test_stages_against_float64(shape, B, ln, clip, w):
    """One update_actor on a loaded batch (actions from synth_transitions: pi != a), TD3 with BC on.  lambda, bc, L_actor and a_du are
    recomputed in float64 from the engine's own read-backs -- q_pi, dA, Xp (pi), the batch actions, scale -- so what is left is the
    engine's fp32 rounding, bounded a priori with u = 2^-24, gamma(n) = n u / (1 - n u) (tests/bounds.py):

      lambda = alpha / max(sum|q| / B, 1e-8): a sum of B non-negative terms in any order (gamma(B - 1), relative), the division by B
        and the division alpha / mean, one rounding each; max() is exact.  Relative bound gamma(B + 2).
      bc = inv_ba sum (pi - a)^2: per term the difference (one rounding, squared: two) and the square (one); the sum of B A
        non-negative terms (gamma(B A - 1)); inv_ba = fl(1 / (B A)) and the product with it.  Relative bound gamma(B A + 5).
      L = lambda (s inv_b) + w bc, s = sum of -q over the B rows (gamma(B - 1) sum|q|), inv_b and its product (2 u), the product
        with lambda (u, plus lambda's own gamma(B + 2)), w bc (u, plus bc's bound), the sum (u):
          |dL| <= (gamma(B + 3) + gamma(B + 2)) lambda mean|q| + gamma(B A + 7) w bc + u (|lambda mean q| + w bc).
      a_du_bj = (lambda dA + k dif) sc f, k = 2 w inv_ba, dif = pi - a, f = 1 - th^2, th = (pi - bias) / sc as recomputed here:
        t1 = lambda dA carries lambda's gamma(B + 2) and one rounding; t2 = k dif carries inv_ba and its product (2 u), dif (u) and
        the product (u); the sum, the two products with sc and f: 3 u of the result.  f itself: the engine squares its own th (u th^2)
        and subtracts (u f); th recomputed from the stored pi = fl(th sc + bias) differs from the engine's by at most 2 u |th| (the
        product and the sum; the division here is float64), which moves f by 4 u th^2 -- the conditioning term of a saturated action.
          |d a_du| <= SAFETY sc [ f (|t1| (gamma(B + 2) + u) + 4 u |t2|) + (|t1| + |t2|) (3 u f + u th^2 + u f + 4 u th^2) ]
        (SAFETY = 2 as everywhere in tests/bounds.py; the bound on lambda is used as stated, without it).
    Then every per-key actor gradient and the post-Adam actor against the float64 autograd restatement of the whole update
    (td3bc_ref.actor_update64), at the existing tolerances of gclose / assert_params_close; with clip_norm the step is also
    checked element by element from the engine's own gradient and the float64 clip coefficient (bounds.clip_coef, adam_expected)."""
    alpha = 2.5
    ref, eng, (o, a, bound) = make_bc_pair(shape, B, ln, clip_norm=clip)
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=5)
    eng.load_batch(obs, act, rew, nobs, done)
    if w != 1.0:
        eng.set_bc(alpha, w)
    assert eng.bc() == (alpha, w)
    p0 = eng.get_params(_lib.ACTOR)
    eng.update_actor()
    ldc, a4, ldu = (o + a + 3) // 4 * 4, (a + 3) // 4 * 4, (a + 3) // 4 * 4
    q = bd.f64(eng.debug_read("q_pi").reshape(2, B)[0])
    dA = bd.f64(eng.debug_read("dA").reshape(2, B, a4)[0, :, :a])
    pi = bd.f64(eng.debug_read("Xp").reshape(B, ldc)[:, o:o + a])
    ab = bd.f64(eng.read_batch()["actions"])
    assert np.array_equal(ab, bd.f64(act.numpy())) and np.abs(pi - ab).max() > 1e-2
    du = eng.debug_read("a_du").reshape(B, ldu)[:, :a]
    met = eng.read_metrics()
    u, g = bd.U, bd.gamma
    a32, w32 = bd.f32c(alpha), bd.f32c(w)
    # lambda
    lam = a32 / max(np.abs(q).mean(), 1e-8)
    r = abs(met["vitals/bc_lambda"] - lam) / lam
    print(f"lambda {met['vitals/bc_lambda']!r} float64 {lam!r} rel err {r:.3e} bound {g(B + 2):.3e}")
    observe("td3bc_stages", f"{shape}-{B} lambda err / bound", r / g(B + 2))
    assert r <= g(B + 2)
    # bc
    bc = ((pi - ab) ** 2).sum() / (B * a)
    r = abs(met["loss/bc_loss"] - bc) / bc
    print(f"bc {met['loss/bc_loss']!r} float64 {bc!r} rel err {r:.3e} bound {g(B * a + 5):.3e}")
    assert r <= g(B * a + 5)
    # L_actor
    L = -lam * q.mean() + w32 * bc
    bL = (g(B + 3) + g(B + 2)) * lam * np.abs(q).mean() + g(B * a + 7) * w32 * bc + u * (abs(lam * q.mean()) + w32 * bc)
    print(f"L_actor {met['loss/actor_loss']!r} float64 {L!r} err {abs(met['loss/actor_loss'] - L):.3e} bound {bL:.3e}")
    assert abs(met["loss/actor_loss"] - L) <= bL
    # a_du
    sc, bias = bd.f32c(bound), 0.0
    th = (pi - bias) / sc
    f = np.abs(1.0 - th * th)
    t1, t2 = lam * dA, (2.0 * w32 / (B * a)) * (pi - ab)
    want = (t1 + t2) * sc * (1.0 - th * th)
    at1, at2 = np.abs(t1), np.abs(t2)
    bdu = bd.SAFETY * sc * (f * (at1 * (g(B + 2) + u) + 4 * u * at2) + (at1 + at2) * (3 * u * f + u * th * th + u * f + 4 * u * th * th))
    worst = bd.check("a_du", du, want, bdu)
    print(f"a_du worst err / bound {worst:.3f}")
    observe("td3bc_stages", f"{shape}-{B} a_du err / bound", worst)
    # the whole update against float64 autograd
    up = R.actor_update64(ref.actor, ref.qnets[0], obs, act, bc_alpha=a32, bc_weight=w32, lr=ref.hps.actor_lr, clip_norm=clip)
    assert met["vitals/bc_lambda"] == pytest.approx(up["lam"], rel=1e-5) and met["loss/bc_loss"] == pytest.approx(up["bc"], rel=1e-5)
    assert met["loss/actor_loss"] == pytest.approx(up["loss"], rel=1e-5, abs=1e-5)
    G = eng.debug_read("grad_actor")
    got_g = schema.flat_to_dict(G, o, a, ln)
    for k, gr in up["grads"].items():
        gclose(got_g[k], gr.float(), name=f"actor grad {k}")
    p1 = eng.get_params(_lib.ACTOR)
    assert_params_close(p1, flat_actor(ref, up["actor"]), ref.hps.actor_lr, 1, "actor after Adam", layout=actor_layout(ref))
    assert not np.array_equal(p0, p1)
    if clip > 0:
        coef, rel = bd.clip_coef(G, clip)
        assert coef < 0.5 and coef == pytest.approx(up["coef"], rel=1e-4)      # the clip is active
        m, v, step = eng.get_adam_state(_lib.ACTOR)
        assert step == 1
        exp = bd.adam_expected(p0, np.zeros_like(p0), np.zeros_like(p0), 0, G, ref.hps.actor_lr, m_got=m, v_got=v, coef=coef, coef_rel=rel)
        for key, got in (("m", m), ("v", v), ("p", p1)):
            bd.check(f"clipped Adam {key}", got, *exp[key])
    # which kernel ran: the node list of the fused iteration names the BC forms and not their plain twins
    if clip == 0:
        _, scratch, _ = make_bc_pair(shape, B, ln)
        scratch.rb_extend(*[t.numpy() for t in synth_transitions(B, o, a, bound, seed=7)])
        names = [n["name"].split(":")[0] for n in scratch.time_nodes(1, iters=1)]
        assert names.count(EXPECT_KERNEL[(shape, B)]) == 2, names
        assert sum(n.startswith(("k_tn_bc<", "k_adam_red_bc")) for n in names) == 2, names
        assert not any(n in ("k_headbwd_nn", "k_actor_head_bwd", "k_actor_head_bwd_s<4>") for n in names), names


# ------------------------------------------------------------------------------------------ 2. one computation, every route

def issue(eng, route, i0, n, agent=None):
    """iterations i0 .. i0 + n - 1 (actor updates at the multiples of 3) through one route"""
    if route == "periods":
        return eng.run_iterations(i0, n)
    for i in range(i0, i0 + n):
        if route == "calls":
            eng.rb_sample()
            eng.update_qnets()
            if i % 3 == 0:
                eng.update_actor()
                eng.update_actor()
            eng.update_targ_nets(i + 1)
        elif route == "agent":
            agent.iteration(i)
        else:      # "steps" (graphs) / "eager" (use_graphs=False)
            eng.step(i % 3 == 0)
    return i0 + n


@pytest.mark.parametrize("shape,B", [("halfcheetah", 256), ("o48a17", 1024)])
def test_every_route_computes_the_same_bits(shape, B):
    """TD3, BC on, native RNG: the call sequence, Agent.iteration, run_iterations (periods and a two-period run) and the eager
    launches leave identical parameters, Adam state and metrics after 6 iterations; then sactd3_set_bc between two periods, in the
    period route and in the single-step routes alike: still identical, and no graph was captured for it."""
    from sac_td3_cudagraphs_pytorch_amd.agent import Agent, ReplayBuffer
    o, a, bound = SHAPES[shape]
    rows = [t.numpy() for t in synth_transitions(2000, o, a, bound, seed=29)]
    res, engines = {}, {}
    for route in ("calls", "agent", "periods", "eager"):
        if route == "agent":
            hps = SimpleNamespace(**dict(vars(Hps.td3(batch_size=B)), bc_alpha=2.5, seed=4, num_envs=8))
            agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32),
                          torch.device("cuda", 0), hps, ReplayBuffer(4096), seed=4)
            ref, _, _ = make_bc_pair(shape, B, seed=4)
            eng = track(agent.engine)
            push_params(eng, ref)
            assert eng.cfg.bc_alpha == 2.5
        else:
            agent = None
            _, eng, _ = make_bc_pair(shape, B, seed=4, use_graphs=route != "eager")
        eng.rb_extend(*rows)
        assert issue(eng, route, 0, 6, agent) == 6
        res[route], engines[route] = engine_state(eng, "index"), (eng, agent)
    for route in ("agent", "periods", "eager"):
        assert_same_state(res["calls"], res[route], what=route)
    met = {k[len("metrics."):]: float(v[0]) for k, v in res["calls"].items() if k.startswith("metrics.")}
    assert [int(res["calls"][f"adam_t.{k}"][0]) for k in ("actor", "critics")] == [4, 6] and np.isfinite(list(met.values())).all()
    assert met["loss/bc_loss"] > 0 and met["vitals/bc_lambda"] > 0
    assert engines["agent"][1].qnet_updates_so_far == 6 and engines["agent"][1].actor_updates_so_far == 4
    st0 = engines["periods"][0].step_periods_stats()
    pipelined = B < 1024      # (where the period graph has its pipelined form two periods go out as one run graph; elsewhere one by one)
    assert (st0["run_graphs_captured"] >= 1 and st0["run_launches"] >= 1) if pipelined else st0["single_period_launches"] >= 2
    run_nodes = engines["periods"][0].graph_kernel_count(10)
    after = {}
    for route in ("periods", "calls", "eager"):
        eng, agent = engines[route]
        issue(eng, route, 6, 3, agent)                    # one period ...
        eng.set_bc(1.5, 0.25)                             # ... new values between two periods ...
        issue(eng, route, 9, 9, agent)                    # ... a two-period run and a period on the chained opening pair
        assert eng.bc() == (1.5, 0.25)
        after[route] = engine_state(eng, "index")
    for route in ("calls", "eager"):
        assert_same_state(after["periods"], after[route], what=f"{route} behind set_bc")
    assert not np.array_equal(after["periods"]["params.actor"], res["periods"]["params.actor"])
    st1 = engines["periods"][0].step_periods_stats()
    assert st1["run_graphs_captured"] <= 2      # (at most the other start variant; test_set_bc_between_periods_captures_nothing is the strict form)
    assert engines["periods"][0].graph_kernel_count(10) == run_nodes and (run_nodes > 0) == pipelined
    # the values did reach the kernels: the same 12 iterations WITHOUT the set_bc call end elsewhere
    _, other, _ = make_bc_pair(shape, B, seed=4)
    other.rb_extend(*rows)
    other.run_iterations(0, 18)
    assert not np.array_equal(other.get_params(_lib.ACTOR), after["periods"]["params.actor"])
    # Agent.update_actor hands the two BC metrics out as zero-copy tensors beside the loss
    eng, agent = engines["agent"]
    out = agent.update_actor(agent.rb.sample(B))
    assert set(out) == {"loss/actor_loss", "loss/bc_loss", "vitals/bc_lambda"}
    m = eng.read_metrics()
    for k, v in out.items():
        assert v.is_cuda and v.ndim == 0 and float(v) == m[k]


def test_set_bc_between_periods_captures_nothing():
    """the capture counters around set_bc alone: a run of periods, set_bc, the same run again -- no run graph, no period graph more"""
    _, eng, (o, a, bound) = make_bc_pair("halfcheetah", 256, seed=2)
    eng.rb_extend(*[t.numpy() for t in synth_transitions(1000, o, a, bound, seed=3)])
    eng.run_iterations(0, 12)
    eng.run_iterations(12, 12)
    st0, c0 = eng.step_periods_stats(), [eng.graph_kernel_count(k) for k in range(9)] + [eng.graph_kernel_count(10)]
    eng.set_bc(0.7, 2.0)
    eng.run_iterations(24, 12)
    st1, c1 = eng.step_periods_stats(), [eng.graph_kernel_count(k) for k in range(9)] + [eng.graph_kernel_count(10)]
    assert st1["run_graphs_captured"] == st0["run_graphs_captured"] and c1 == c0
    assert st1["run_launches"] == st0["run_launches"] + 2 and st1["single_period_launches"] == st0["single_period_launches"]


# ------------------------------------------------------------------------------------------ 3. node counts

@pytest.mark.parametrize("shape,B", [("halfcheetah", 256), ("o48a17", 1024), ("o10a8", 48)])
def test_bc_adds_no_graph_node(shape, B):
    counts = []
    for alpha in (2.5, 0.0):
        _, eng, (o, a, bound) = make_bc_pair(shape, B, bc_alpha=alpha)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(max(B, 600), o, a, bound, seed=3)])
        eng.instantiate_graphs()
        eng.rb_sample(); eng.update_qnets(); eng.update_actor()
        eng.step_prefix(1); eng.step_prefix(2)
        eng.step_periods(2)
        eng.step_sampled(True, n_step=2, stride=1)
        eng.step_sampled(False, n_step=2, stride=1)
        eng.sync()
        counts.append([eng.graph_kernel_count(k) for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 16, 17, 18, 19)])
    assert counts[0] == counts[1], counts
    assert all(counts[0][i] > 0 for i in (0, 1, 2, 3, 4)) and sum(c > 0 for c in counts[0][9:]) == 2, counts
    if B < 1024:      # the cut-short period graphs and the run graph exist where the period graph has its pipelined form
        assert all(counts[0][i] > 0 for i in (6, 7, 8)), counts


# ------------------------------------------------------------------------------------------ 4. boundaries

def test_boundaries():
    o, a, bound = DIMS["halfcheetah"]
    with pytest.raises(P.EngineError, match="bc_alpha"):      # SAC has no BC form; the message names the field
        track(P.Engine(P.Config(ob_dim=o, ac_dim=a, bc_alpha=2.5), -1.0, 1.0))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(P.EngineError, match=r"\(-1\).*bc_alpha"):
            track(P.Engine(P.Config(ob_dim=o, ac_dim=a, prefer_td3_over_sac=True, bc_alpha=bad), -1.0, 1.0))
    _, plain, _ = make_bc_pair("halfcheetah", 64, bc_alpha=0.0)
    with pytest.raises(P.EngineError, match="-3"):            # SACTD3_ESTATE: the kernel forms are chosen at create
        plain.set_bc(2.5, 1.0)
    ref, eng, _ = make_bc_pair("halfcheetah", 64)
    assert eng.bc() == (2.5, 1.0)                             # bc_weight starts at 1
    for al, w in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (2.5, -0.1), (2.5, float("nan")), (2.5, float("inf"))):
        with pytest.raises(P.EngineError, match="-1"):
            eng.set_bc(al, w)
        assert eng.bc() == (2.5, 1.0)                         # a refused call changes nothing
    eng.set_bc(3.0, 0.0)                                      # weight 0 is allowed
    assert eng.bc() == (3.0, 0.0)
    eng.set_bc(2.5, 1.0)
    # an engine without BC never writes the two slots; a BC engine does
    obs, act, rew, nobs, done = synth_transitions(64, o, a, bound, seed=5)
    raw = np.empty(_lib.NUM_METRICS, np.float32)
    fp = raw.ctypes.data_as(C.POINTER(C.c_float))
    plain.load_batch(obs, act, rew, nobs, done); plain.update_actor()
    plain._ck(plain.lib.sactd3_read_metrics(plain._h, fp))
    assert raw[_lib.M_BC_LOSS] == 0 and raw[_lib.M_BC_LAMBDA] == 0 and raw[_lib.M_ACTOR_LOSS] != 0
    assert set(plain.read_metrics()) == {"loss/qf_loss", "loss/actor_loss", "loss/alpha_loss", "vitals/alpha"}
    # a batch whose q_pi are all exactly 0 (zeroed critic head): lambda sits on its floor, every parameter stays finite
    with torch.no_grad():
        for qn in ref.qnets:
            qn.head.weight.zero_(); qn.head.bias.zero_()
    eng.set_params(_lib.CRITICS, flat_critics(ref, ref.qnets))
    eng.load_batch(obs, act, rew, nobs, done)
    p0 = eng.get_params(_lib.ACTOR)
    eng.update_actor()
    assert not eng.debug_read("q_pi").reshape(2, 64)[0].any()
    m = eng.read_metrics()
    assert m["vitals/bc_lambda"] == pytest.approx(2.5e8, rel=1e-6) and np.isfinite(list(m.values())).all()
    p1 = eng.get_params(_lib.ACTOR)
    assert np.isfinite(p1).all() and np.isfinite(eng.get_adam_state(_lib.ACTOR)[0]).all() and not np.array_equal(p0, p1)
    assert m["loss/actor_loss"] == pytest.approx(m["loss/bc_loss"], rel=1e-6)      # -lambda mean q = 0: what is left is the BC term


# ------------------------------------------------------------------------------------------ 5. it does what it is for

def test_bc_pulls_the_policy_onto_the_data_and_plain_td3_does_not():
    """HalfCheetah dims, B = 256, a ring of 4096 rows whose actions are a fixed linear-tanh function of the observations
    (td3bc_ref.direction_dataset; its seed was chosen on the CPU restatement, tests/test_td3bc_host.py shows the same ordering there).
    300 offline iterations with bc_alpha = 2.5: loss/bc_loss ends below its value after the first actor updates; the same run with
    plain TD3 from the same seed does not make (1 / (n A)) sum (pi(s) - a)^2 over the ring fall.  A direction, no magnitude."""
    d, seed = R.DIRECTION, R.DIRECTION_SEED
    obs, act, rew, nobs, done = R.direction_dataset(seed)
    out = {}
    for alpha in (d["bc_alpha"], 0.0):
        _, eng, _ = make_bc_pair("halfcheetah", d["B"], seed=seed, bc_alpha=alpha, rb_capacity=d["rows"], max_envs=d["rows"], randomize=False)
        eng.rb_extend(obs.numpy(), act.numpy(), rew.numpy(), nobs.numpy(), done.numpy())
        predict = lambda x: eng.predict(x.numpy(), False)
        before = R.dataset_bc(predict, obs, act)
        eng.run_iterations(0, 1)
        first = eng.read_metrics().get("loss/bc_loss")
        eng.run_iterations(1, d["iters"] - 1)
        out[alpha] = (before, R.dataset_bc(predict, obs, act), first, eng.read_metrics().get("loss/bc_loss"))
        print(alpha, out[alpha])
    before, after, first, last = out[d["bc_alpha"]]
    assert last < first and after < before
    p_before, p_after, _, _ = out[0.0]
    assert p_before == before and p_after >= p_before
