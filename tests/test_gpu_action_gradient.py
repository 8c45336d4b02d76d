"""GPU: the action gradients of the twin critics and the in-kernel ascent (include/sactd3_action_gradient.h) against the plain float64
autograd restatement of tests/action_gradient_model.py, on perturbed parameters (the recipe of gpu_support.build_engines: the oracle's
nets, every bias and LayerNorm pair moved, targets apart from the online nets) and asymmetric per-dimension action bounds.

The tolerance is taken from no kernel: per quantity and case, K = 4 x the largest |float32 - float64| of the same restatement run in
torch float32 on the CPU, as for the dormant scan and the candidate scoring.  ReLU masks and the minimum are discontinuous, so rows whose
float64 kink margin is below 1e-5 are left out of the gradient comparisons (never of Q): none at n <= 17 and at most 5 % of a case, which
the float64 model alone satisfies with these seeds (asserted).

Measured on an MI355X, worst ratio kernel error / yardstick over the 32 cases of a row count: n = 17 -- q_start 2.5, q_min 2.9, grad 2.2,
grad_obs 1.9, columns 2 - 4 1.9 / 2.2 / 2.4; n = 1025 -- 1.5, 1.5, 1.2, 2.2, 1.3 / 1.5 / 2.5; the step: refined 1.4, q_end and column 5 below
0.9.  At n = 1 a quantity is one number (two for q_start, a for grad): its own yardstick is one rounding accident of the float32
restatement -- it lands within 3e-10 of float64 in some cases while the kernel is within one or two ulps, 1e-8 .. 4e-7 -- and the ratio
to it alone reaches 64 (q_min), 52 (column 3), 18 (column 4), 14 (column 2), 9.7 (q_start); 17 of the 32 one-row cases miss 4 x.  A
one-row case is therefore held to 4 x the larger of its own yardstick and that of the same restatement on the 17 rows of the same
engine and critics: still the float32 restatement's own error, sampled on 17 rows of the same distribution instead of one.  With it
the worst one-row ratio is 2.0 (q_min; 1.3 q_start, 0.9 grad, 1.1 grad_obs, 1.1 / 1.0 / 1.2 columns 2 - 4).  profiles/action_gradient.json
holds these figures, DESIGN section 5 the reason."""
import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps, RefAgent
from tests import action_gradient_model as am
from tests.gpu_support import DEV, MAXN, P, _lib, assert_same_state, close_engines, push_params, same_bits, track  # noqa: F401
from tests.helpers import randomize_ln, synth_transitions

pytestmark = pytest.mark.gpu
K_BOUND, SEED, KINK = 4.0, 3, 1e-5
SHAPES = ((3, 1), (11, 3), (61, 6), (376, 17))      # (61, 6): the action columns straddle a K chunk of 64; (376, 17): six chunks, a > 16
# input seeds other than 0: the first for which the float64 model alone leaves out no row at n <= 17 and at most 5 % at n = 1025 (found on the CPU)
SEEDS = {("sac", 3, 1, 0, "online", 17): 1, ("sac", 3, 1, 0, "online", 1025): 10, ("sac", 3, 1, 0, "target", 1025): 6,
         ("td3", 3, 1, 0, "online", 17): 1, ("td3", 3, 1, 0, "online", 1025): 11, ("td3", 3, 1, 0, "target", 17): 1,
         ("sac", 3, 1, 1, "target", 17): 1, ("sac", 11, 3, 0, "target", 17): 1, ("td3", 11, 3, 1, "online", 17): 1,
         ("td3", 61, 6, 0, "online", 17): 1}
OUT = ("q_start", "grad", "grad_obs", "refined", "q_end", "summary")


def bounds(a):
    d = np.arange(a, dtype=np.float32)
    return (-1.0 - 0.125 * d).tolist(), (0.5 + 0.25 * d).tolist()


def build(algo, o, a, ln, tracked=True):
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=bool(ln), batch_size=64)
    lo, hi = bounds(a)
    torch.manual_seed(SEED)
    ref = RefAgent(o, a, lo, hi, hps)
    randomize_ln(ref)
    eng = P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=1024, max_envs=MAXN, seed=SEED), lo, hi)
    if tracked:
        track(eng)
    push_params(eng, ref)
    return eng


def inputs(o, a, n, seed=0):
    g = torch.Generator().manual_seed(1000 * n + o + seed)
    lo, hi = (torch.tensor(b) for b in bounds(a))
    return torch.randn(n, o, generator=g), lo + (0.05 + 0.9 * torch.rand(n, a, generator=g)) * (hi - lo)


def call(eng, obs, act, **kw):
    got = eng.action_gradient(obs.to(DEV), act.to(DEV), grad_obs=True, **kw)
    return {k: got[k].cpu().numpy() for k in OUT}


def restate(eng, o, a, ln, obs, act, which="online", steps=0, lr=0.0):
    crit = eng.get_params(_lib.CRITICS_TARGET if which == "target" else _lib.CRITICS)
    return [am.action_gradient(crit, o, a, ln, obs, act, *bounds(a), steps, lr, t) for t in (torch.float64, torch.float32)]


def quantities(want, x):
    """the compared quantities of one result: Q on every row, the gradient quantities on the rows off the kinks"""
    keep = want["margin"] >= KINK
    out = {"q_start": x["q_start"], "q_min": x["summary"][:, 0], "grad": x["grad"][:, keep], "grad_obs": x["grad_obs"][:, keep]}
    out.update({f"summary{c}": x["summary"][keep, c] for c in (2, 3, 4)})
    return out


def held(tag, pairs, wide=None):
    """every (name, kernel, float64, float32) within K_BOUND x the float32 restatement's error (`wide`: name -> the same restatement's
    error on more rows, the yardstick's floor in a one-row case); each figure is printed first"""
    bad = []
    for name, got, want, f32 in pairs:
        err, yard = np.abs(got - want).max(), np.abs(f32 - want).max()
        yard = max(yard, wide[name]) if wide else yard
        print("action_gradient", tag, name, "kernel", float(err), "yardstick", float(yard), "ratio", float(err / yard) if yard else float("inf"))
        if not err <= K_BOUND * yard:
            bad.append((name, float(err), float(yard)))
    assert not bad, (tag, bad)


@pytest.fixture(scope="module", params=[(al, o, a, ln) for o, a in SHAPES for ln in (0, 1) for al in ("sac", "td3")], ids=str)
def case(request):
    eng = build(*request.param, tracked=False)
    yield eng, request.param
    eng.close()


@pytest.mark.parametrize("which", ["online", "target"])
@pytest.mark.parametrize("n", [1, 17, 1025])
def test_against_float64(case, n, which):
    eng, (algo, o, a, ln) = case
    obs, act = inputs(o, a, n, SEEDS.get((algo, o, a, ln, which, n), 0))
    got = call(eng, obs, act, which=which)
    want, f32 = restate(eng, o, a, ln, obs, act, which)
    keep = want["margin"] >= KINK
    assert (~keep).sum() <= (0 if n <= 17 else 0.05 * n)
    g, w, f = (quantities(want, x) for x in (got, want, f32))
    wide = None
    if n == 1:      # (the module docstring: one number's yardstick is one rounding accident)
        w17, f17 = restate(eng, o, a, ln, *inputs(o, a, 17, SEEDS.get((algo, o, a, ln, which, 17), 0)), which)
        wide = {k: np.abs(quantities(w17, f17)[k] - v).max() for k, v in quantities(w17, w17).items()}
    held((algo, o, a, ln, which, n), [(k, g[k], w[k], f[k]) for k in g], wide)
    assert same_bits(got["q_end"], got["q_start"]) and same_bits(got["refined"], act.numpy())      # steps == 0


@pytest.mark.parametrize("algo,o,a,ln,seed", [("sac", 61, 6, 1, 1), ("td3", 376, 17, 0, 2)], ids=str)
def test_steps(algo, o, a, ln, seed):
    eng, n, lr = build(algo, o, a, ln), 33, 0.07
    obs, act = inputs(o, a, n, seed)
    whole, cur = call(eng, obs, act, steps=3, lr=lr), act
    for _ in range(3):
        one = call(eng, obs, cur, steps=1, lr=lr)
        cur = torch.as_tensor(one["refined"])
    assert same_bits(whole["refined"], one["refined"]) and same_bits(whole["q_end"], one["q_end"])
    first = call(eng, obs, act, steps=1, lr=lr)
    want, f32 = restate(eng, o, a, ln, obs, act, steps=1, lr=lr)
    keep = want["margin"] >= KINK
    assert keep.all()
    held((algo, o, a, ln, "step"), [(k, first[k], want[k], f32[k]) for k in ("refined", "q_end")] + [("moved", *(x["summary"][:, 5] for x in (first, want, f32)))])
    far = call(eng, obs, act, steps=16, lr=0.5)
    lo, hi = (np.array(b, np.float32) for b in bounds(a))
    assert (far["refined"] >= lo).all() and (far["refined"] <= hi).all() and far["summary"][:, 6].max() >= 1 and (far["summary"][:, 7] == 0).all()
    still = call(eng, obs, act, steps=2, lr=0.0)
    assert same_bits(still["refined"], act.numpy()) and same_bits(still["q_end"], still["q_start"])
    assert eng.action_gradient_stats() == dict(calls=7, rows=7 * n, rows_nonfinite=0, ascent_steps=(3 + 3 + 1 + 16 + 2) * n)


def test_row_independence_invisibility_and_a_nan_row():
    algo, o, a, ln = "sac", 61, 6, 1
    R, Q = build(algo, o, a, ln), build(algo, o, a, ln)
    five = synth_transitions(1024, o, a, 0.5, seed=SEED + 1)
    obs, act = inputs(o, a, 1025)
    for eng in (R, Q):
        eng.rb_extend(*[t.numpy() for t in five])
        it = eng.run_iterations(0, 6)
        if eng is R:
            whole = call(R, obs, act, steps=2, lr=0.05)
            alone = call(R, obs[700:701], act[700:701], steps=2, lr=0.05)
            moved = call(R, obs[697:720], act[697:720], steps=2, lr=0.05)
        eng.run_iterations(it, 6)
    assert_same_state(R, Q, "index", "noise", "ring")
    assert all(same_bits(R.get_params(w), Q.get_params(w)) for w in (_lib.ACTOR, _lib.CRITICS, _lib.CRITICS_TARGET))
    row = lambda x, k, i: x[k][:, i:i + 1] if k in ("grad", "grad_obs") else x[k][i:i + 1]
    for k in OUT:
        assert same_bits(row(whole, k, 700), row(alone, k, 0)) and same_bits(row(whole, k, 700), row(moved, k, 3)), k
    bad = obs[:40].clone()
    bad[21, 5] = float("nan")
    clean, got = call(R, obs[:40], act[:40], steps=1, lr=0.05), call(R, bad, act[:40], steps=1, lr=0.05)
    others = [i for i in range(40) if i != 21]
    assert all(same_bits(got[k][:, others] if k in ("grad", "grad_obs") else got[k][others],
                         clean[k][:, others] if k in ("grad", "grad_obs") else clean[k][others]) for k in OUT)
    assert R.action_gradient_stats()["rows_nonfinite"] == 1 and Q.action_gradient_stats()["calls"] == 0
