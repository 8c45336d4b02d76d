"""The row-local kernels around the trunks -- the actor tails, the critic tails, the Q(s, pi) tails, the head backwards and the dQ/da
epilogue -- stage by stage against float64 at their edge inputs (tests/tail_checks.py, tests/bounds.py; the checker itself is
checked on the CPU by tests/test_tail_bounds.py).

Per case the engine gets parameters drawn directly (no torch oracle), a batch and injected noise with the edges built in
(tail_checks.make_case): head-bias offsets that saturate both squashes (an element with |y| == 1 and one with |tanh(raw log-std)|
== 1 are required), rows of exact-zero and of +-4 noise, per-dimension asymmetric action bounds, all-done blocks with loud rewards.
update_qnets and update_actor run through the API; after each, every buffer a row-local kernel read and wrote is read back and
    * the next-action pass (a_z2 still holds its z2 after update_qnets): a' in Xn and log pi(a'|s'), TD3 the smoothed, clamped a';
    * the critic tail: q_target, targ_q (done rows: == rew bit for bit), q, c_dz2 (a row is tried under each choice of its undecided
      layer-2 gates, at most three), the head and LayerNorm-2 entries of grad_critics, loss/qf_loss;
    * the policy pass from its stored h2: a_tg, the action columns of Xp, logp_pi; TD3 also a_z2 -> a_xh2, a_rs2, a_h2 (SAC's a_z2 is
      overwritten by the temperature pass);
    * SAC the temperature draw, end to end from a_z2, the stepped actor and the injected noise -> logp_alpha;
    * the Q(s, pi) tail: q_pi; exact zeros in the dA (and, where stored, dz2) of the critic that loses the minimum; c_dz2 at
      B >= 1024; dA from c_dz1 where the dQ/da epilogue of k_ln_bwd<16> forms it;
    * the head backward: a_du (exactly 0 in the mean half where 1 - y^2 == 0), a_dz2, the head and LayerNorm-2 entries of grad_actor
are held, every element, to the a-priori bounds and intervals of tests/bounds.py; the worst err / bound per stage is recorded
(helpers.observe).  Variants on small cases: loss weights with exact zeros and one large value (k_ctail_nn_w<2>, k_critic_tail_w<16>),
twin ties (target net 1 = target net 0 for the critic update, plain and BCQ mix; online net 1 = net 0 for the actor update),
zero-variance LayerNorm rows / all-negative pre-activations without LayerNorm, and log_alpha = -8 and +2.

On the folded dQ/da path (B < 1024, narrow head, ac_dim <= 7) neither c_dz2, c_dh1 nor c_dz1 of the Q(s, pi) pass is stored: dA is checked
against the whole chain composed from c_z2 (bounds.dqda_folded).  TD3+BC variants run the BC forms of the three head-backward kernels,
one with every Q(s, pi) exactly 0 (lambda on its floor).  A dispatch assertion per case (Engine.time_nodes) requires the kernel forms
the case is there for.
"""
import numpy as np
import pytest
import torch

from tests import tail_checks as tc
from tests.gpu_support import _lib, close_engines, make_engine, schema  # noqa: F401

pytestmark = pytest.mark.gpu

H = 256
IDS = [f"{al}-{env}-{B}-{'ln' if ln else 'noln'}" for al, env, B, ln in tc.CASE_TABLE]


def expected_kernels(c):
    """the row-local kernel forms csrc/engine.hip picks for the case (enqueue_update_qnets, enqueue_update_actor, launch_tails)"""
    B, a, nh, sac = c["B"], c["a"], c["nh"], c["sac"]
    narrow = nh <= 8 and a <= 8
    big = B >= 1024
    want = ["k_critic_tail<16>", "k_actorq_tail<4>"] if big else ["k_ctail_nn<2>", "k_qtail_nn<2>" if sac else "k_qtail_nn<1>"]
    want.append(("k_actor_head_bwd_s<4>" if big else "k_headbwd_nn") if narrow else "k_actor_head_bwd")
    if big or not (narrow and a <= 7):
        want.append("k_ln_bwd<16>/dQ/da")
    return want, ("k_actor_tail_s" if narrow else "k_actor_tail")


def check_dispatch(c):
    eng = make_engine(c, rb_capacity=4096 + c["B"])
    eng.rb_fill_synthetic(4096 + c["B"], seed=3)
    names = set()
    for n in eng.time_nodes(True, 2):
        kernel, rest = n["name"].split(":", 1)
        names.add(kernel)
        if rest.endswith("/dQ/da"):
            names.add(kernel + "/dQ/da")
    eng.close()
    want, tails = expected_kernels(c)
    assert all(k in names for k in want), (want, sorted(names))
    tail_names = {k for k in names if k.startswith("k_actor_tail")}
    assert tail_names and all(k.startswith("k_actor_tail_s") == (tails == "k_actor_tail_s") for k in tail_names), (tails, sorted(tail_names))


def nets(flat, in_dim, nh, ln, n):
    flat = np.asarray(flat, np.float32).reshape(n, -1)
    return [dict(schema.flat_to_dict(flat[i], in_dim, nh, ln)) for i in range(n)]


def run_case(case, rec, log_alpha=None, bcq=None, weighted=False, tie=False, degenerate=False, dispatch=True, bc_alpha=0.0, zero_q=False):
    algo, o, a, B, ln = case
    c = tc.make_case(algo, o, a, B, ln, tc.case_seed(case), degenerate_nets=degenerate)
    sac, nh = c["sac"], c["nh"]
    if tie:
        c["critics_t"][1] = c["critics_t"][0]
    if dispatch:
        check_dispatch(c)
    eng = make_engine(c, log_alpha, bcq, bc_alpha=bc_alpha)
    la = float(eng.get_params(_lib.LOG_ALPHA)[0]) if sac else 0.0
    cfg = dict(gamma=eng.cfg.gamma, bcq=bool(eng.cfg.bcq_style_targ_mix), log_alpha=la, td3_std=eng.cfg.td3_std, td3_c=eng.cfg.td3_c)
    ldc, a4, ldu = (o + a + 3) // 4 * 4, (a + 3) // 4 * 4, (nh + 3) // 4 * 4
    rd = lambda k, *shape: eng.debug_read(k).reshape(*shape)

    # ---- critic update
    eng.load_batch(c["obs"], c["act"], c["rew"], c["nobs"], c["done"])
    keep = None
    if weighted:
        keep = torch.as_tensor(c["w"], device="cuda")
        eng.batch_weights_device(keep.data_ptr(), 1, B, torch.cuda.current_stream().cuda_stream)
    eng.set_noise(_lib.SITE_CRITIC, c["eps_c"])
    eng.update_qnets()
    if weighted:
        assert eng.graph_kernel_count(8) > 0        # the weighted form of the update_qnets graph was the one captured and run
    assert np.array_equal(rd("rew", B), c["rew"]) and np.array_equal(rd("done", B) != 0, c["done"])
    pn = c["actor"] if sac else c["actor_t"]
    tc.check_pass_from_z2(rec, "next", rd("a_z2", B, H), pn, c, c["eps_c"], rd("Xn", B, ldc)[:, o:o + a], rd("logp_next", B) if sac else None, cfg)
    R = dict(t_z2=rd("t_z2", 2, B, H), c_z2=rd("c_z2", 2, B, H), rew=rd("rew", B), done=rd("done", B), logp_next=rd("logp_next", B),
             q_target=rd("q_target", 2, B), targ_q=rd("targ_q", B), q=rd("q", 2, B), c_dz2=rd("c_dz2", 2, B, H),
             grads=nets(eng.debug_read("grad_critics"), o + a, 1, ln, 2), qf_loss=np.float32(eng.read_metrics()["loss/qf_loss"]))
    if tie:
        assert np.array_equal(R["q_target"][0], R["q_target"][1])
    tc.check_critic_tail(rec, R, c, cfg, c["w"] if weighted else None)

    # ---- actor update, with the critics as update_qnets left them
    c = dict(c, critics=nets(eng.get_params(_lib.CRITICS), o + a, 1, ln, 2))
    if zero_q:      # every Q(s, pi) exactly 0: lambda sits on its floor, bc_alpha / 1e-8
        for p in c["critics"]:
            p["head.weight"], p["head.bias"] = np.zeros_like(p["head.weight"]), np.zeros_like(p["head.bias"])
    if tie:
        c["critics"][1] = c["critics"][0]
    if tie or zero_q:
        eng.set_params(_lib.CRITICS, np.concatenate([schema.dict_to_flat(p, o + a, 1, ln) for p in c["critics"]]))
    eng.set_noise(_lib.SITE_ACTOR0, c["eps_a"])
    eng.set_noise(_lib.SITE_ALPHA0, c["eps_l"])
    eng.update_actor()
    nq = 2 if sac else 1
    A = dict(a_z2=rd("a_z2", B, H), a_h2=rd("a_h2", B, H), a_xh2=rd("a_xh2", B, H), a_rs2=rd("a_rs2", B), a_tg=rd("a_tg", B, 4 * a4),
             action=rd("Xp", B, ldc)[:, o:o + a], logp_pi=rd("logp_pi", B), dA=rd("dA", 2, B, a4)[:nq, :, :a], a_du=rd("a_du", B, ldu)[:, :nh],
             a_dz2=rd("a_dz2", B, H), grads=nets(eng.debug_read("grad_actor"), o, nh, ln, 1)[0])
    if sac:       # a_z2 now holds the temperature pass through the stepped actor
        stepped = nets(eng.get_params(_lib.ACTOR), o, nh, ln, 1)[0]
        tc.check_pass_from_z2(rec, "temperature draw", A["a_z2"], stepped, c, c["eps_l"], None, rd("logp_alpha", B))
    else:
        tc.check_policy_stores(rec, A, c)
    tc.check_policy_tail(rec, A, c, require_saturation=sac and not degenerate)
    Q = dict(c_z2=rd("c_z2", 2, B, H)[:nq], q_pi=rd("q_pi", 2, B)[:nq], c_dz2=rd("c_dz2", 2, B, H)[:nq], dA=A["dA"])
    first = tc.check_q_pi_tail(rec, Q, c, stored_dz2=B >= 1024)
    if tie:
        assert first.all() and not Q["dA"][1].any()
    if zero_q:
        assert not Q["q_pi"].any() and not A["dA"].any()
    if B >= 1024 or not (nh <= 8 and a <= 7):
        tc.check_dqda_stored(rec, dict(c_dz1=rd("c_dz1", 2, B, H)[:nq], dA=A["dA"]), c)
    else:
        tc.check_dqda_folded(rec, dict(c_z2=Q["c_z2"], c_h1=rd("c_h1", 2, B, H)[:nq], c_xh1=rd("c_xh1", 2, B, H)[:nq],
                                       Xp=rd("Xp", B, ldc)[:, :o + a], dA=A["dA"]), c, first)
    bc = None
    if bc_alpha > 0:
        bc = eng.bc()
        A["q_pi"], A["bc_lambda"] = Q["q_pi"], np.float32(eng.read_metrics()["vitals/bc_lambda"])
        if zero_q:
            assert A["bc_lambda"] == np.float32(np.float32(bc_alpha) / np.float32(1e-8))
    tc.check_head_bwd(rec, A, c, la, bc)
    eng.close()
    del keep


@pytest.mark.parametrize("case", tc.CASES, ids=IDS)
def test_tail_edges(case):
    run_case(case, f"tail_edges[{IDS[tc.CASES.index(case)]}]")


def _case(algo, env, B, ln):
    return tc.CASES[tc.CASE_TABLE.index((algo, env, B, ln))]


HOPPER, SAC4, SAC5, TD3_8 = _case("sac", "hopper", 19, True), _case("sac", "sac4", 33, True), _case("sac", "sac5", 40, False), _case("td3", "td3_8", 35, True)
VARIANTS = [
    ("weighted-small-sac", HOPPER, dict(weighted=True)),                                   # k_ctail_nn_w<2>
    ("weighted-small-td3", TD3_8, dict(weighted=True)),
    ("weighted-large-td3", _case("td3", "halfcheetah", 1030, True), dict(weighted=True)),  # k_critic_tail_w<16>
    ("tie-plain", HOPPER, dict(tie=True, bcq=False)),
    ("tie-bcq-mix", SAC4, dict(tie=True, bcq=True)),
    ("degenerate-ln-sac", HOPPER, dict(degenerate=True)),
    ("degenerate-noln-sac", SAC5, dict(degenerate=True)),
    ("degenerate-ln-td3", TD3_8, dict(degenerate=True)),
    ("log-alpha-minus-8", SAC4, dict(log_alpha=-8.0)),
    ("log-alpha-plus-2", SAC4, dict(log_alpha=2.0)),
    ("td3bc-narrow", TD3_8, dict(bc_alpha=2.5)),                                             # k_headbwd_nn_bc
    ("td3bc-wide", _case("td3", "o48a17", 35, True), dict(bc_alpha=2.5)),                    # k_actor_head_bwd_bc
    ("td3bc-large", _case("td3", "halfcheetah", 1030, True), dict(bc_alpha=2.5)),            # k_actor_head_bwd_s_bc<4>
    ("td3bc-zero-q", _case("td3", "td3_7", 21, False), dict(bc_alpha=2.5, zero_q=True)),     # lambda = bc_alpha / 1e-8
]


@pytest.mark.parametrize("name,case,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_tail_edge_variants(name, case, kw):
    run_case(case, f"tail_edges[{name}]", dispatch=False, **kw)
