"""The small-batch kernel forms (B < 1024) at their switch points, checked stage by stage in float64 from the engine's own inputs --
the path every published number takes (B = 256), with the checker of tests/test_gpu_large_batch.py (tests/gpu_stage_checks.py) and the
a-priori bounds of tests/bounds.py (checked on the CPU by tests/test_stage_bounds.py at these batch sizes and in these kernels'
summation orders).

Below B = 1024 csrc/engine.hip runs a trunk as the fused k_nt<pro,true,KS,c1,nt> (inputs of at most 64 columns: the first layer is
recomputed per output tile) or as k_nt_wide + k_nt<pro,false,KS,0,nt>, and every weight gradient, with the optimiser step and the
target updates behind it, as one k_tn<kt[,true]> launch.  launch_nt / launch_tn choose, from the rows M, the nets of the launch and
the CU count (an MI355X has 256; a launch has 16 column tiles per net):
  * KS = 4 -> 2 (K split over 4 or 2 waves; 16- or 32-row blocks) once ceil(M / 16) 16 nets >= 2 CUs: the 4-net twin-critic trunk
    from M = 113, a 2-net launch (SAC's Q(s, pi)) from 241, a 1-net launch (an actor pass, TD3's Q(s, pi)) from 497;
  * nt = 1 -> 2 (two column tiles per block) once KS = 2 and ceil(M / 32) 16 nets >= 2 CUs: 225, 481, 993;
  * c1 in {1, 2, 4} from ceil(K1 / 16): K1 in 33 .. 48 runs the c1 = 4 instance with a masked tile;
  * pro = 1 with LayerNorm, 2 with the ReLU alone;
  * the opening pair of an iteration with actor updates on narrow observations (next-action pass + first policy pass, 2 nets) keeps
    the KS = 4 sums of the 1-net passes: KS = 4, or from M = 241 with LayerNorm the <...,2,c1,nt,true> instance (its period-graph
    forms are tied to the single iterations bit for bit by test_period_graph_equals_single_iterations; here its instance is
    named by the model and its outputs pass through the checks of the stages that read them);
  * k_tn: kt = 2 once a launch has more than 2 CUs single tiles (every critic launch, the Humanoid actor), the layer-1 LayerNorm
    backward folded in (<kt,true>) behind the fused row + GEMM launches (the critics; actors with nh <= 8), rows in 256-row slabs (a
    new one at 257, 513, 769, the last one masked).
dispatch() restates these rules; test_small_batch_dispatch_coverage holds it against the node lists of both fused iteration graphs
(Engine.time_nodes) case by case, a form the model does not know counting apart and so failing, and the two tests behind it assert
that CASES really shows every switch on both sides.  The side past a switch is always = 1 (mod 16): it ends in a one-row block.

Every case then runs update_qnets, update_actor and update_targ_nets through the API and one fused critic-only iteration on ring
rows (run_one_iteration, run_fused_critic_iteration with stages=True): trunk forward (with LayerNorm from xhat1, which
bounds.ln_xhat ties to the input rows -- where a first-layer tile masked wrongly would show), dh1 (where the ReLU gate of the fused
row + GEMM launches lets it through), dz1, the layer-1 and layer-2 weight, bias and LayerNorm-affine gradients, the actor head gradients,
the Q(s, pi) pass of the online critics, every element of m, v and p from an evolved Adam state (step 0 at B = 17), the Polyak
targets in their three forms, the temperature step, and in the fused iteration the batch slot against the sampled ring rows bit
for bit.  No tolerance is taken from an observed error and none allows a fraction of bad elements; the only acceptance rule is
relu_accept at an undecidable ReLU gate.  The worst |err| / bound per stage goes to parity_observed.json (helpers.observe).

Not checkable here: dh1 where the layer-1 ReLU gate is shut (the fused launches store relu'(z1) dh1; those elements are checked
as exact zeros); rstd1 (not read back: recomputed in float64 from the input rows, its rounding carried as rho); dz2, dh1 and dz1 of the Q(s, pi) pass on the folded dQ/da route, which stores none of them
(tests/test_gpu_tail_edges.py composes that chain).
"""
import functools
import re

import pytest
import torch

from tests.gpu_stage_checks import run_fused_critic_iteration, run_one_iteration
from tests.gpu_support import close_engines, make_pair  # noqa: F401
from tests.helpers import DIMS

pytestmark = pytest.mark.gpu

NUM_CUS = 256          # the switch points of CASES are derived for this many CUs; dispatch() itself takes the device's

# (algo, env, B, layer_norm): what the shape straddles
CASES = [
    ("sac", "hopper", 17, True),            # two row blocks, the second of one row; all KS = 4 (Adam from step 0)
    ("sac", "hopper", 112, True),           # 4-net KS ...
    ("sac", "hopper", 113, True),
    ("td3", "halfcheetah", 224, True),      # 4-net nt; c1 = 2 ...
    ("td3", "halfcheetah", 225, True),
    ("sac", "sac4", 240, True),             # 2-net KS (SAC's Q(s, pi)) ...
    ("sac", "sac4", 241, True),
    ("sac", "hopper", 256, False),          # the second k_tn slab; pro = 2 ...
    ("sac", "hopper", 257, False),
    ("sac", "hopper", 480, True),           # 2-net nt ...
    ("sac", "hopper", 481, True),
    ("td3", "halfcheetah", 496, True),      # 1-net KS (actor passes, TD3's Q(s, pi)) ...
    ("td3", "halfcheetah", 497, True),
    ("sac", "hopper", 513, True),           # the third slab, one live row
    ("td3", "td3_7", 769, False),           # the fourth slab, one live row; pro = 2 past every KS switch
    ("sac", "hopper", 992, True),           # 1-net nt ...
    ("sac", "hopper", 993, True),
    ("sac", "humanoid", 225, True),         # K > 64: k_nt_wide + the unfused layer 2 (4-net nt = 2), k_gather, the kt = 2 actor launch
    ("td3", "humanoid", 257, True),         # ... under TD3, past one slab
    ("td3", "o48a17", 113, True),           # critics K = 65 (wide), actor K1 = 48: the c1 = 4 instance with a masked tile
    ("sac", "o3a32", 257, True),            # the widest head (nh = 64), K1 = 3; critics K1 = 35: c1 = 4
]
IDS = [f"{a}-{e}-{b}-{'ln' if ln else 'noln'}" for a, e, b, ln in CASES]


# ------------------------------------------------------------------------------------------ the dispatch model

def _cdiv(a, b):
    return -(-a // b)


def nt_instance(pro, fuse1, K1, M, nets, num_cus, force_ks=0):
    """launch_nt: the k_nt instance of a launch of `nets` nets over M rows (256 outputs: 16 column tiles per net)"""
    tiles = _cdiv(M, 16) * 16 * nets
    ks = 2 if tiles >= 2 * num_cus else 4
    if force_ks:
        ks = force_ks
    c4 = force_ks == 4 and fuse1 and pro == 1 and tiles >= 2 * num_cus       # KS = 2 blocks with KS = 4's summation tree
    if c4:
        ks = 2
    blocks_m = _cdiv(M, 64 // ks)
    nt = 2 if ks == 2 and blocks_m * 16 * nets >= 2 * num_cus else 1
    if force_ks and not c4:
        nt = 1
    if c4 and nt == 2 and blocks_m * 8 * nets > num_cus:
        nt = 1
    c1 = 0 if not fuse1 else {1: 1, 2: 2}.get(max(_cdiv(K1, 16), 1), 4)
    return f"k_nt<{pro},{'true' if fuse1 else 'false'},{ks},{c1},{nt}{',true' if c4 else ''}>"


def trunk(K, M, nets, ln, num_cus, force_ks=0):
    """enqueue_trunk below BIG_BATCH: the fused form for K <= 64, otherwise k_nt_wide + the unfused layer 2 (which takes no forced KS)"""
    pro = 1 if ln else 2
    if K <= 64:
        return [nt_instance(pro, True, K, M, nets, num_cus, force_ks) + "/layers1+2"]
    return ["k_nt_wide/layer1", nt_instance(pro, False, 0, M, nets, num_cus) + "/layer2"]


def tn_instance(tiles_per_net, nets, fold, num_cus):
    """launch_tn: two k tiles per block once the single 16 x 16 tiles of the launch exceed two per CU"""
    kt = 2 if tiles_per_net * nets > 2 * num_cus else 1
    return f"k_tn<{kt},true>" if fold else f"k_tn<{kt}>"


def dispatch(algo, o, a, B, ln, num_cus, with_actor, delay=2, autotune=True):
    """[(what, nets, node)] of one fused iteration with a target update (enqueue_step as Engine.time_nodes walks it) at B < 1024: every trunk
    launch, every weight-gradient launch, and the nodes that exist only on some routes (k_gather, k_nn, k_ln_bwd<16>).
    what: 'opening', 'twin', 'policy<j>', 'q_pi<j>', 'alpha<j>', 'critic_dW', 'actor_dW<j>', or '' (nets 0) for the route nodes."""
    assert B < 1024
    sac = algo == "sac"
    nh, nq, narrow = (2 * a if sac else a), (2 if sac else 1), o <= 64
    small_head = nh <= 8 and a <= 8                 # the fused head backward + dh1 launch, with layer 1's LayerNorm backward folded into k_tn
    qa_fold = small_head and a <= 7                 # dQ/da finished inside the fused launches: no k_ln_bwd<16> for it
    w1 = lambda K: 16 * _cdiv((K + 3) // 4 * 4, 16)                     # 16 x 16 tiles of a layer-1 weight gradient
    out = []
    if not narrow:
        out.append(("", 0, "k_gather"))                # narrow observations: the opening trunk reads the ring rows itself
    merged = with_actor and narrow                  # the first policy pass as a second group of the opening launch, KS = 4 sums kept
    out += [("opening", 2 if merged else 1, n) for n in trunk(o, B, 2 if merged else 1, ln, num_cus, 4 if merged else 0)]
    out += [("twin", 4, n) for n in trunk(o + a, B, 4, ln, num_cus)]
    polyak = "dW+adam+polyak" + (" & actor-target polyak" if not sac and not with_actor else "")
    out.append(("critic_dW", 2, tn_instance(2 * 8 * 16 + w1(o + a), 2, True, num_cus) + "/" + polyak))      # always folded below 1024
    for j in range(delay if with_actor else 0):
        if not (narrow if j == 0 else (sac and autotune)):       # otherwise the pass rode in the opening pair / the previous temperature pass
            out += [(f"policy{j}", 1, n) for n in trunk(o, B, 1, ln, num_cus)]
        out += [(f"q_pi{j}", nq, n) for n in trunk(o + a, B, nq, ln, num_cus)]
        if not qa_fold:
            out.append(("", 0, "k_ln_bwd<16>"))
        if not small_head:
            out += [("", 0, "k_nn"), ("", 0, "k_ln_bwd<16>")]
        last = j + 1 == delay
        out.append((f"actor_dW{j}", 1, tn_instance(_cdiv(nh, 16) * 16 + 16 * 16 + w1(o), 1, small_head, num_cus)
                    + ("/dW+adam+polyak" if not sac and last else "/dW+adam")))
        if sac and autotune:
            out += [(f"alpha{j}", 1, n) for n in trunk(o, B, 1, ln, num_cus)]
    return out


MODELLED = ("k_nt", "k_tn", "k_gather", "k_nn", "k_ln_bwd", "k_adam_red")


def node_key(name):
    """'instance:role/detail' -> the model's spelling: instance/detail for the trunk and weight-gradient launches, the instance alone
    for the route nodes; a detail the model does not expect stays in the key, so that it counts apart and fails"""
    kernel, rest = name.split(":", 1)
    if kernel.startswith(("k_nt", "k_tn")):
        for d in ("layers1+2", "layer1", "layer2", "dW+adam+polyak & actor-target polyak", "dW+adam+polyak", "dW+adam", "dW"):
            if rest.endswith("/" + d):
                return f"{kernel}/{d}"
        return f"{kernel}/{rest}"
    return kernel


def count(keys):
    c = {}
    for k in keys:
        c[k] = c.get(k, 0) + 1
    return c


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def graph_nodes(algo, env, B, ln):
    """(node names of the critic-only fused iteration, of the one with actor updates, actor_update_delay, autotune) of a scratch engine"""
    ref, eng, _ = make_pair(algo, env, B, ln, rb_capacity=2048 + B)
    eng.rb_fill_synthetic(2048 + B, seed=3)
    g0, g1 = [n["name"] for n in eng.time_nodes(False, 2)], [n["name"] for n in eng.time_nodes(True, 2)]
    cfg = (eng.cfg.actor_update_delay, eng.cfg.autotune)
    eng.close()
    return g0, g1, cfg


@pytest.mark.parametrize("algo,env,B,ln", CASES, ids=IDS)
def test_small_batch_dispatch_coverage(algo, env, B, ln):
    """per case and per fused-iteration graph: the instance of every trunk and weight-gradient launch, and the count of every route
    node, as dispatch() derives them from csrc/engine.hip's rules for this device's CU count"""
    o, a, _ = DIMS[env]
    g0, g1, (delay, autotune) = graph_nodes(algo, env, B, ln)
    for label, g, actor in (("critic-only", g0, False), ("with actor updates", g1, True)):
        want = count(n for _, _, n in dispatch(algo, o, a, B, ln, _cus(), actor, delay, autotune))
        got = count(k for k in map(node_key, g) if k.startswith(MODELLED))
        assert got == want, (label, {k: (got.get(k, 0), want.get(k, 0)) for k in set(got) | set(want) if got.get(k, 0) != want.get(k, 0)}, g)


def _args(node):
    """template arguments of 'k_nt<pro,fuse1,ks,c1,nt[,true]>...' / 'k_tn<kt[,true]>...'"""
    return re.match(r"k_\w+<([^>]*)>", node).group(1).split(",")


def _graph_args(nodes, role):
    """template arguments of the one k_nt node of `nodes` (names as time_nodes gives them) whose role contains `role`"""
    hit = [n for n in nodes if n.startswith("k_nt<") and role in n.split(":", 1)[1]]
    assert len(hit) == 1, (role, hit, nodes)
    return _args(hit[0])


# (algo, env, below, from, role of the launch in the graph with actor updates, its nets, template argument index, values either side)
KS, NT = 2, 4
SWITCHES = [
    ("sac", "hopper", 112, 113, "twin-q", 4, KS, "4", "2"),
    ("td3", "halfcheetah", 224, 225, "twin-q", 4, NT, "1", "2"),
    ("sac", "sac4", 240, 241, "actor0/q(s,pi)", 2, KS, "4", "2"),
    ("sac", "hopper", 480, 481, "actor0/q(s,pi)", 2, NT, "1", "2"),
    ("td3", "halfcheetah", 496, 497, "actor0/q(s,pi)", 1, KS, "4", "2"),
    ("td3", "halfcheetah", 496, 497, "actor1/policy", 1, KS, "4", "2"),
    ("sac", "hopper", 992, 993, "actor1/alpha", 1, NT, "1", "2"),
]


@pytest.mark.parametrize("algo,env,lo,hi,role,nets,arg,below,past", SWITCHES, ids=[f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-{s[5]}net-{'ks' if s[6] == KS else 'nt'}-{s[4].split('/')[-1].strip('()').replace(',', '-')}" for s in SWITCHES])
def test_switch_points_change_the_named_template_argument(algo, env, lo, hi, role, nets, arg, below, past):
    """the two sides of a switch run instances that differ in KS (or nt) for the launch the switch belongs to, and in nothing else"""
    if _cus() != NUM_CUS:
        pytest.skip(f"the switch points are derived for {NUM_CUS} CUs; this device has {_cus()}")
    assert (algo, env, lo, True) in CASES and (algo, env, hi, True) in CASES
    al, ah = _graph_args(graph_nodes(algo, env, lo, True)[1], role), _graph_args(graph_nodes(algo, env, hi, True)[1], role)
    assert (al[arg], ah[arg]) == (below, past), (al, ah)
    assert [x for i, x in enumerate(al) if i != arg] == [x for i, x in enumerate(ah) if i != arg], (al, ah)


def test_cases_show_every_switch_on_both_sides():
    """over CASES, by the model that test_small_batch_dispatch_coverage holds against the graphs: per launch size (4, 2, 1 nets) KS = 4
    and KS = 2 and, at KS = 2, nt = 1 and nt = 2; c1 = 1, 2, 4; both prologues; the wide route with both KS and both nt in its
    layer 2; the forced-KS opening pair in both of its instances; every k_tn instance; 1 to 4 slabs with a one-row last slab"""
    cus = _cus()
    if cus != NUM_CUS:
        pytest.skip(f"the switch points are derived for {NUM_CUS} CUs; this device has {cus}")
    seen, tn = set(), set()
    for algo, env, B, ln in CASES:
        o, a, _ = DIMS[env]
        for what, nets, node in dispatch(algo, o, a, B, ln, cus, True):
            if node.startswith("k_nt<"):
                pro, fuse1, ks, c1, nt = _args(node)[:5]
                forced = what == "opening" and nets == 2
                seen.add(("c4" if len(_args(node)) == 6 else "forced" if forced else "free", nets, fuse1, ks, nt))
                seen.add(("c1", c1))
                seen.add(("pro", pro, fuse1))
            elif node.startswith("k_tn<"):
                tn.add(node.split("/")[0])
            elif what == "" or node.startswith("k_nt_wide"):
                seen.add(node.split("/")[0])
    for nets in (4, 2, 1):
        for ks, nt in (("4", "1"), ("2", "1"), ("2", "2")):
            assert ("free", nets, "true", ks, nt) in seen, (nets, ks, nt, sorted(map(str, seen)))
    for ks, nt in (("4", "1"), ("2", "1"), ("2", "2")):
        assert any(("free", nets, "false", ks, nt) in seen for nets in (4, 2, 1)), ("unfused layer 2", ks, nt)
    assert ("forced", 2, "true", "4", "1") in seen and ("c4", 2, "true", "2", "1") in seen and ("c4", 2, "true", "2", "2") in seen
    assert {("c1", "1"), ("c1", "2"), ("c1", "4"), ("c1", "0")} <= seen
    assert {("pro", p, f) for p in ("1", "2") for f in ("true",)} <= seen and ("pro", "1", "false") in seen
    assert {"k_nt_wide", "k_gather", "k_nn", "k_ln_bwd<16>"} <= seen
    assert tn == {"k_tn<1>", "k_tn<1,true>", "k_tn<2>", "k_tn<2,true>"}, tn
    slabs = {(_cdiv(B, 256), B % 256) for _, _, B, _ in CASES}
    assert {(2, 1), (3, 1), (4, 1)} <= slabs and any(s == 1 for s, _ in slabs)


# ------------------------------------------------------------------------------------------ stages

@pytest.mark.parametrize("algo,env,B,ln", CASES, ids=IDS)
def test_small_batch_stages_against_float64(algo, env, B, ln):
    rec = f"small_batch_stages[{algo}-{env}-{B}-{ln}]"
    run_one_iteration(algo, env, B, ln, rec, adam_step=0 if B == 17 else 1000, stages=True)
    run_fused_critic_iteration(algo, env, B, ln, rec, stages=True)


def test_small_batch_stages_with_clip_norm_past_one_slab():
    """the clipped route (k_tn<1,true> without the optimiser step, k_gradnorm, k_adam) at 257 rows: the same stages, and Adam from the
    stored unclipped gradient scaled by the coefficient of its norm"""
    rec = "small_batch_stages[sac-hopper-257-clip]"
    run_one_iteration("sac", "hopper", 257, True, rec, adam_step=1000, stages=True, clip_norm=0.05)
    run_fused_critic_iteration("sac", "hopper", 257, True, rec, stages=True)
