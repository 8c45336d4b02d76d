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
import pytest
import torch

from tests.gpu_stage_checks import (LARGE_BATCH_CASES as CASES, H, check_update_actor_intermediates, check_update_qnets_intermediates,
                                    run_fused_critic_iteration, run_one_iteration)
from tests.gpu_support import close_engines, make_pair  # noqa: F401
from tests.helpers import DIMS

pytestmark = pytest.mark.gpu

NUM_CUS = 256

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
