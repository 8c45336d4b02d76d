"""GPU: the critics under N sampled candidate actions per state (include/sactd3_action_values.h) against the plain float64 restatement of
tests/action_values_model.py, on perturbed sactd3_init_params parameters (every bias and LayerNorm pair non-trivial) and asymmetric
action bounds [-1, 2].

The tolerance is taken from no kernel: per output column, K x the largest |float32 - float64| of the same restatement run in torch
float32 on the CPU, over the case; K = 4 as for the dormant scan.  A summary column is one number per row, so at n = 1 its own
yardstick is one rounding accident (measured on an MI355X: the float32 restatement lands within 5e-10 of float64 in some cases, the
kernel within 1 - 2 ulps, 2.4e-7, a ratio of 225).  Columns 0 - 5 are functions of the m_j with Lipschitz constant 1 (a maximum, means,
a soft maximum, a deviation), column 6 the mean of the logp_j and column 4 adds alpha times it: their yardstick is therefore the larger
of the column's own float32 error and that of the per-candidate values it is reduced from (all n N of them).  With it the worst
measured ratios over the 288 cases are 1.3, 0.8, 2.4, 0.4, 0.8, 1.5 for columns 0 - 5 (K = 4), 2.9 for cand_q, 2.3 for cand_logp,
7.6 x the yardstick for a policy candidate (K = 4 held it in every case but 2 of 144; see K_CAND).  Column 6 takes K = 16: with the
uniform source every logp_j is the same number, torch's pairwise mean of N equal terms is exact and leaves one rounding of the
logarithm as the yardstick, while the header's order (j ascending, N - 1 float32 additions) rounds at every step -- measured 13.0.  `cand` is held to 2 ulps of the float32 restatement for the uniform
source, where both sides perform the same three operations; for the policy source a candidate is a function of the actor's output,
whose float32 MFMA and CPU sums differ by more than ulps of the candidate, so it is held by the same K x bound per action dimension."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import action_values_model as am
from tests.gpu_support import DEV, P, _lib, assert_same_state, close_engines, engine_state, same_bits, track  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
K_SUMMARY = np.array([4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 16.0, 4.0])
K_CAND = 16.0      # a policy candidate: tanhf / expf of the device library against torch's, behind the actor's three layers; measured 7.6
K_BOUND, SEED, LO, HI, SIGMA, TAU, ALPHA = 4.0, 11, -1.0, 2.0, 0.3, 0.7, 0.2
SHAPES = ((3, 1), (17, 6), (70, 2))      # ob_dim below a float4, not a multiple of 4, above the LDS chunk of 64
OUT = ("summary", "best_index", "best_action", "cand", "cand_q", "cand_logp", "eps")


def build(algo, o, a, ln, tracked=True):
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=bool(ln), batch_size=64)
    eng = P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=1024, max_envs=96, seed=SEED), [LO] * a, [HI] * a)
    if tracked:
        track(eng)
    eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
    rng = np.random.default_rng(SEED)
    for which in (_lib.ACTOR, _lib.CRITICS, _lib.CRITICS_TARGET):
        flat = eng.get_params(which)
        eng.set_params(which, flat + 0.05 * rng.standard_normal(flat.size).astype(np.float32))
    if algo == "sac":
        eng.set_params(_lib.LOG_ALPHA, np.array([np.log(ALPHA)], np.float32))
    return eng


def inputs(o, a, N, n, source, seed=0):
    g = torch.Generator().manual_seed(1000 * n + N + seed)
    eps = torch.rand(n, N, a, generator=g) if source == "uniform" else torch.randn(n, N, a, generator=g)
    return torch.randn(n, o, generator=g), torch.rand(n, a, generator=g) * (HI - LO) + LO, eps


def call(eng, obs, act, eps, N, source, **kw):
    dev = lambda x: None if x is None else x.to(DEV)
    got = eng.action_values(dev(obs), dev(act), candidates=N, source=source, sigma=SIGMA, tau=TAU, eps=dev(eps), dump=True, **kw)
    return {k: got[k].cpu().numpy() for k in OUT}


def restate(eng, algo, o, a, ln, obs, act, eps, source, dtype, target=False):
    params = {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS_TARGET if target else _lib.CRITICS)}
    alpha = float(np.exp(np.float64(eng.get_params(_lib.LOG_ALPHA)[0]))) if algo == "sac" else 0.0
    return am.action_values(params, o, a, algo == "td3", ln, obs, eps, source, SIGMA, TAU, alpha, [LO] * a, [HI] * a, act, dtype)


@pytest.fixture(scope="module", params=[(al, o, a, ln) for o, a in SHAPES for ln in (0, 1) for al in ("sac", "td3")], ids=str)
def case(request):
    eng = build(*request.param, tracked=False)
    yield eng, request.param
    eng.close()


@pytest.mark.parametrize("source", ["policy", "uniform"])
@pytest.mark.parametrize("N", [16, 32, 64])
@pytest.mark.parametrize("rows", ["one", "full", "full+1", "chunk+3"])
def test_against_float64(case, rows, N, source):
    eng, (algo, o, a, ln) = case
    n = {"one": 1, "full": 64 // N, "full+1": 64 // N + 1, "chunk+3": 1027}[rows]
    obs, act, eps = inputs(o, a, N, n, source)
    got = call(eng, obs, act, eps, N, source)
    want, f32 = (restate(eng, algo, o, a, ln, obs, act, eps, source, t) for t in (torch.float64, torch.float32))
    yard = {key: np.abs(f32[key] - want[key]).max(axes) for key, axes in (("cand_q", (0, 1)), ("cand_logp", (0, 1)), ("summary", (0,)))}
    qy, ly = yard["cand_q"].max(), yard["cand_logp"].max()
    yard["summary"] = np.maximum(yard["summary"], [qy, qy, qy, qy, qy + ALPHA * ly, qy, ly, 0.0])
    for key, axes in (("cand_q", (0, 1)), ("cand_logp", (0, 1)), ("summary", (0,))):
        err, bound = np.abs(got[key] - want[key]).max(axes), (K_SUMMARY if key == "summary" else K_BOUND) * yard[key]
        print("action_values", (algo, o, a, ln, N, source, n), key, "kernel", np.atleast_1d(err).tolist(), "bound", np.atleast_1d(bound).tolist())
        assert (err <= bound).all(), (key, err, bound)
    if source == "uniform":
        assert (np.abs(got["cand"] - f32["cand"]) <= 2 * np.spacing(np.abs(f32["cand"]).astype(np.float32))).all()
    else:
        err, bound = np.abs(got["cand"] - want["cand"]).max((0, 1)), K_CAND * np.abs(f32["cand"] - want["cand"]).max((0, 1))
        print("action_values", (algo, o, a, ln, N, source, n), "cand", "kernel", err.tolist(), "bound", bound.tolist())
        assert (err <= bound).all(), ("cand", err, bound)
    assert same_bits(got["eps"], eps.numpy())
    row = np.arange(n)
    assert same_bits(got["best_action"], got["cand"][row, got["best_index"]])
    qb = K_BOUND * np.abs(f32["cand_q"] - want["cand_q"]).max()
    assert (want["m"].max(1) - want["m"][row, got["best_index"]] <= 2 * qb).all()


def test_row_independence_determinism_and_the_target_critics():
    algo, o, a, ln, N = "sac", 17, 6, 1, 16
    eng = build(algo, o, a, ln)
    obs, act, eps = inputs(o, a, N, 130, "policy")
    whole, again = call(eng, obs, act, eps, N, "policy"), call(eng, obs, act, eps, N, "policy")
    r = 77
    alone = call(eng, obs[r:r + 1], act[r:r + 1], eps[r:r + 1], N, "policy")
    moved = call(eng, obs[r - 2:r + 9], act[r - 2:r + 9], eps[r - 2:r + 9], N, "policy")
    for k in OUT:
        assert same_bits(whole[k], again[k]) and same_bits(whole[k][r:r + 1], alone[k]) and same_bits(whole[k][r:r + 1], moved[k][2:3]), k
    tgt = call(eng, obs, act, eps, N, "policy", target=True)
    want, f32 = (restate(eng, algo, o, a, ln, obs, act, eps, "policy", t, target=True) for t in (torch.float64, torch.float32))
    assert (np.abs(tgt["cand_q"] - want["cand_q"]).max((0, 1)) <= K_BOUND * np.abs(f32["cand_q"] - want["cand_q"]).max((0, 1))).all()
    assert not same_bits(tgt["cand_q"], whole["cand_q"])


@pytest.mark.parametrize("algo,source", [("sac", "policy"), ("td3", "policy"), ("sac", "uniform")])
def test_native_draws_reproduce_and_the_call_is_invisible(algo, source):
    o, a, N = 17, 6, 32
    R, Q = build(algo, o, a, 1), build(algo, o, a, 1)
    five = synth_transitions(1024, o, a, 1.0, seed=SEED + 1)
    obs, act, _ = inputs(o, a, N, 1030, source)
    for eng in (R, Q):
        eng.rb_extend(*[t.numpy() for t in five])
        it = eng.run_iterations(0, 6)
        if eng is R:
            first, second = call(R, obs, act, None, N, source), call(R, obs, act, None, N, source)
            replay = call(R, obs, act, torch.as_tensor(first["eps"]), N, source)
        eng.run_iterations(it, 6)
    assert_same_state(R, Q, "index", "noise", "ring")
    assert all(same_bits(first[k], replay[k]) for k in OUT) and not same_bits(first["eps"], second["eps"])
    st = R.action_values_stats()
    assert (st["calls"], st["rows"], st["native_draw_calls"], st["av_ctr"], st["rows_nonfinite"]) == (3, 3090, 2, 2, 0)
    e = first["eps"]
    assert np.isfinite(e).all() and ((0 < e.min() and e.max() <= 1 and abs(e.mean() - 0.5) < 0.01) if source == "uniform" else abs(e.std() - 1) < 0.01)


def test_edges_a_nan_row_no_actions_and_every_refusal():
    o, a, N = 17, 6, 16
    eng = build("sac", o, a, 1)
    obs, act, eps = inputs(o, a, N, 9, "policy")
    clean = call(eng, obs, act, eps, N, "policy")
    bad = obs.clone()
    bad[5, 3] = float("nan")
    got = call(eng, bad, act, eps, N, "policy")
    others = [i for i in range(9) if i != 5]
    assert all(same_bits(got[k][others], clean[k][others]) for k in OUT)      # (row 5 itself: whatever the arithmetic gives)
    assert eng.action_values_stats()["rows_nonfinite"] == 1
    bare = call(eng, obs, None, eps, N, "policy")
    assert np.isnan(bare["summary"][:, 5]).all() and same_bits(np.delete(bare["summary"], 5, 1), np.delete(clean["summary"], 5, 1))
    assert all(same_bits(bare[k], clean[k]) for k in OUT if k != "summary")
    calls = eng.action_values_stats()["calls"]
    x, out, host = obs.to(DEV), torch.full((9, 8), -7.0, device=DEV), np.zeros((9, 8), np.float32)

    def raw(obs_p=x.data_ptr(), obs_ld=o, n=9, cand=N, source=0, which=0, sigma=0.2, tau=1.0, flags=0, io=True, engine=eng, **fields):
        s = _lib.CActionValuesIO(summary=out.data_ptr(), summary_ld=8)
        for k, v in fields.items():
            setattr(s, k, v)
        return eng.lib.sactd3_action_values_device(engine._h if engine else None, C.c_void_p(obs_p), obs_ld, n, cand, source, which, sigma, tau,
                                                      C.byref(s) if io else None, None, flags)

    td3 = build("td3", o, a, 1)
    bad_calls = [dict(obs_p=0), dict(io=False), dict(summary=None), dict(n=0), dict(cand=8), dict(cand=48), dict(cand=128), dict(source=2),
                 dict(which=2), dict(flags=2), dict(engine=td3, sigma=-0.1), dict(engine=td3, sigma=float("nan")), dict(tau=0.0),
                 dict(tau=float("inf")), dict(obs_ld=o - 1), dict(summary_ld=7), dict(actions=x.data_ptr(), actions_ld=a - 1),
                 dict(eps=x.data_ptr(), eps_ld=N * a - 1), dict(best_action=out.data_ptr(), best_action_ld=a - 1), dict(obs_p=host.ctypes.data),
                 dict(summary=host.ctypes.data), dict(engine=None)]
    assert [raw(**b) for b in bad_calls] == [_lib.EINVAL] * len(bad_calls)
    assert eng.action_values_stats()["calls"] == calls and td3.action_values_stats()["calls"] == 0 and (out == -7.0).all()
    assert raw() == 0 and eng.action_values_stats()["calls"] == calls + 1


def test_through_the_loop_and_best_of_n():
    """loop.train on the native pendulum with ood_gap: the three vitals are there and finite, the run ends with the bits of the run
    without the keyword; predict_best_of returns a candidate of the policy inside the bounds"""
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    n, seed = 2, 3
    cfg = P.launcher.job_config("sac", "pendulum", seed, num_envs=n, learning_starts=10, batch_size=4, num_timesteps=150 * n - 1,
                                eval_every=100, rb_capacity=512)
    o, a, bound = envs.SPECS[envs.kind_of("pendulum")][:3]
    runs = []
    for kw in (dict(), dict(ood_gap=dict(rows=64, candidates=32))):
        agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV),
                        cfg, P.ReplayBuffer(cfg.rb_capacity), seed=seed, init="engine")
        track(agent.engine)
        env = track(envs.NativeVecEnv("pendulum", n, seed=seed, device=DEV, horizon=25))
        runs.append((agent, loop.train(cfg, env, agent, device_env=True, **kw)))
    (plain, _), (watched, out) = runs
    assert_same_state(plain.engine, watched.engine, "index", "noise", "ring")
    assert all(np.isfinite(out[k]) for k in loop.OodGap.KEYS) and watched.engine.action_values_stats()["calls"] >= 2
    obs = torch.randn(5, o, device=DEV)
    best = watched.predict_best_of({"observations": obs}, candidates=16)
    assert best.shape == (5, a) and bool((best.abs() <= bound).all()) and watched.engine.action_values_stats()["rows_nonfinite"] == 0
