"""GPU: the feature-rank call (include/sactd3_feature_rank.h) against the plain float64 restatement of tests/feature_rank_model.py, on a
ring of 4096 seeded transitions and the parameters of sactd3_init_params.

Every tolerance is M x the error of the same restatement run in torch float32 on the CPU against float64 (the rule of
tests/test_gpu_dormant.py): M_GRAM = 4 for the Gram matrix, M_LAMBDA = 16 -- the most the call's specification allows -- for the
eigenvalues, M_TRACE = 8 for the trace invariant.  Each case prints its figures before it asserts.

Measured on an MI355X over the 32 cases of test 1: the Gram matrix 0.32 .. 2.9 of its yardstick; the eigenvalues 0.08 .. 6.7 of
theirs (errors 3e-9 .. 2.6e-5; the worst ratio at (70, 2), no LayerNorm, n = 17, Q2 -- above 4, hence M_LAMBDA = 16); the trace invariant
at most 4.3 of its; 6 .. 15 sweeps of the 16 allowed, every case converged."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import feature_rank_model as fm, init_model
from tests.gpu_support import DEV, P, _lib, assert_same_state, engine_state, same_bits, track  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
CAP, SEED, M_GRAM, M_LAMBDA, M_TRACE = 4096, 7, 4.0, 16.0, 8.0
NS = (1, 17, 256, 16 * 16 + 5)      # rank 1, a partial second tile, full rank possible, 17 tiles: a workgroup walks two
NETS = ("actor", "q1", "q2")


def build(algo, o, a, ln, tracked=True):
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=bool(ln), batch_size=64)
    eng = P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=CAP, max_envs=96, seed=SEED), [-1.0] * a, [1.0] * a)
    if tracked:
        track(eng)
    eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
    five = synth_transitions(CAP, o, a, 1.0, seed=SEED + 1)
    eng.rb_extend(*[t.numpy() for t in five])
    return eng, torch.cat([five[0], five[1]], 1).numpy()


def rank(eng, idx, **kw):
    got = eng.feature_rank(torch.as_tensor(np.asarray(idx, np.int64), device=DEV), spectrum=True, gram=True, **kw)
    return got["lambda"].cpu().numpy(), got["gram"].cpu().numpy(), got


online = lambda eng: {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS)}


@pytest.fixture(scope="module", params=[(al, o, a, ln) for o, a in ((3, 1), (70, 2)) for ln in (0, 1) for al in ("sac", "td3")], ids=str)
def case(request):
    eng, x = build(*request.param, tracked=False)
    yield eng, x, request.param
    eng.close()


@pytest.mark.parametrize("n", NS)
def test_gram_and_spectrum_against_float64(case, n):
    eng, x, (algo, o, a, ln) = case
    idx = np.random.default_rng(n).integers(0, CAP, n)
    idx[-1] = idx[0]                                                          # (a duplicate wherever n > 1)
    lam, gram, info = rank(eng, idx)
    (g64, l64), (g32, l32) = (fm.gram_and_spectrum(online(eng), o, a, algo == "td3", ln, x[idx], t) for t in (torch.float64, torch.float32))
    tr64, tr32 = g64.trace(axis1=1, axis2=2), g32.trace(axis1=1, axis2=2)
    err_g, yard_g = np.abs(gram - g64).max((1, 2)), np.abs(g32 - g64).max((1, 2))
    err_l, yard_l = np.abs(lam - l64).max(1), np.abs(l32 - l64).max(1)
    # the invariant's yardstick.  The device's two sides each approximate tr64, and so do the restatement's: |tr32 - tr64| is its error
    # in the trace, |sum l32 - tr64| its error in the eigenvalue sum, |sum l32 - tr32| what the two leave between them (each alone can be
    # 0 by luck while the others are not).  The floor: both sides are float32 numbers near the trace, one spacing apart at the least.
    yard_t = np.maximum.reduce([np.abs(l32.sum(1) - tr32), np.abs(tr32 - tr64), np.abs(l32.sum(1) - tr64)])
    yard_t = np.maximum(yard_t, np.spacing(tr64.astype(np.float32)).astype(np.float64))
    err_t = np.array([abs(info["lambda_sum"][k] - info["trace"][k]) for k in NETS])
    print("feature rank", (algo, o, a, ln, n), "gram", (err_g / yard_g).tolist(), "lambda", (err_l / yard_l).tolist(), "err", err_l.tolist(),
          "trace", err_t.tolist(), yard_t.tolist(), "sweeps", info["sweeps"])
    assert info["valid_rows"] == n and info["refused_rows"] == 0 and all(info["converged"][k] == 1 for k in NETS)
    assert (gram == gram.transpose(0, 2, 1)).all()
    assert (err_g <= M_GRAM * yard_g).all(), (err_g, yard_g)
    assert (err_l <= M_LAMBDA * yard_l).all(), (err_l, yard_l)
    assert (err_t <= M_TRACE * yard_t).all(), (err_t, yard_t)


def test_summaries_refused_rows_and_invisibility():
    algo, o, a, ln, kw = "sac", 11, 3, 1, dict(delta=0.01, floor=1e-5)
    (R, x), (N, _) = build(algo, o, a, ln), build(algo, o, a, ln)
    valid = np.random.default_rng(3).integers(0, CAP, 24)
    _, l64 = fm.gram_and_spectrum(online(R), o, a, False, ln, x[valid], torch.float64)
    for l in l64:                                                             # the precondition, on the reference alone
        want = fm.summary(l, **kw)
        assert not ((l / l[0] > kw["floor"] / 2) & (l / l[0] < kw["floor"] * 2)).any() and (np.abs(want["share"] - 0.99) > 1e-5).all()
    R.dormant_scan(torch.as_tensor(valid, device=DEV))
    for eng in (R, N):
        it = eng.run_iterations(0, 6)
        if eng is R:
            before, scan_before = engine_state(R), R.dormant_stats()
            lam, gram, info = rank(R, valid, **kw)
            again = rank(R, valid, **kw)
            bad = rank(R, np.insert(valid, [0, 10, valid.size], [-1, CAP, 2 ** 40]), **kw)
            critics = rank(R, valid, what=("critics",), **kw)
            none = rank(R, [-1, CAP, 2 ** 40], **kw)
            assert_same_state(before, engine_state(R))
            assert R.dormant_stats() == scan_before
        eng.run_iterations(it, 6)
    assert_same_state(R, N, "index", "noise", "ring")
    R.redo(("actor", "critics"), seed=1, epoch=1)                             # the scan's masks are still pending
    for k, net in enumerate(NETS):
        want = fm.summary(lam[k], **kw)
        assert 1 <= info["srank"][net] == want["srank"] <= info["rank"][net] == want["rank"] <= 24
        assert info["erank"][net] == pytest.approx(want["erank"], rel=1e-5) and info["stable"][net] == pytest.approx(want["stable"], rel=1e-5)
    for other in (again, bad):
        assert same_bits(other[0], lam) and same_bits(other[1], gram)
        assert all(other[2][f] == info[f] for f in _lib.FEATURE_RANK_SUMMARY)
    assert bad[2]["refused_rows"] == 3 and bad[2]["valid_rows"] == 24 and info["refused_rows"] == 0
    assert same_bits(critics[0][1:], lam[1:]) and not critics[0][0].any() and set(critics[2]["rank"]) == {"q1", "q2"}
    assert not none[0].any() and not none[1].any() and none[2]["valid_rows"] == 0
    assert all(none[2][f][net] == 0 for f in ("rank", "srank", "erank", "stable", "trace", "lambda_sum") for net in NETS)


@pytest.mark.parametrize("r", [1, 5])
def test_a_planted_collapse(r):
    """all but r - 1 rows of W2 / b2 become row 0: the features have at most r distinct columns"""
    algo, o, a, ln, floor = "sac", 11, 3, 0, 1e-4
    eng, x = build(algo, o, a, ln)
    idx = np.random.default_rng(r).integers(0, CAP, 300)
    assert all(v > 5 for v in rank(eng, idx, floor=floor)[2]["rank"].values())
    params = online(eng)
    for _, K, nh, flat in init_model.nets_of(params, o, a, False):
        p = {(kind, layer): v for kind, layer, v in init_model.split(flat, K, nh, ln)}
        p[("weight", 1)][r - 1:], p[("bias", 1)][r - 1:] = p[("weight", 1)][0], p[("bias", 1)][0]
    eng.set_params(_lib.ACTOR, params["actor"])
    eng.set_params(_lib.CRITICS, params["critics"])
    lam, _, info = rank(eng, idx, floor=floor)
    print("planted", r, info["rank"], info["srank"], (lam[:, r] / lam[:, 0]).tolist(), info["sweeps"])
    assert all(info["rank"][k] <= r and info["srank"][k] <= r for k in NETS)
    assert (lam[:, r:] < floor * lam[:, :1]).all() and (lam[:, 0] > 0).all()


def test_refusals_come_before_any_side_effect():
    eng, _ = build("sac", 11, 3, 1)
    empty = track(P.Engine(eng.cfg, [-1.0] * 3, [1.0] * 3))
    idx, host, out = torch.zeros(8, dtype=torch.int64, device=DEV), np.zeros(8, np.int64), torch.zeros(3, 256, device=DEV)
    raw = lambda e, p, n, what, delta, floor, flags=0, ld=1, gram=0: e.lib.sactd3_feature_rank_device(
        e._h, C.c_void_p(p), ld, n, what, delta, floor, C.c_void_p(out.data_ptr()), C.c_void_p(gram), None, flags)
    d, nan, inf = idx.data_ptr(), float("nan"), float("inf")
    bad = [(eng, d, 0, 3, 0.01, 1e-4), (eng, d, 4097, 3, 0.01, 1e-4), (eng, d, 8, 0, 0.01, 1e-4), (eng, d, 8, 4, 0.01, 1e-4),
           (eng, d, 8, 3, 0.0, 1e-4), (eng, d, 8, 3, 1.0, 1e-4), (eng, d, 8, 3, nan, 1e-4), (eng, d, 8, 3, 0.01, 1e-7), (eng, d, 8, 3, 0.01, 1.0),
           (eng, d, 8, 3, 0.01, nan), (eng, d, 8, 3, 0.01, inf), (eng, d, 8, 3, 0.01, 1e-4, 4), (eng, d, 8, 3, 0.01, 1e-4, 0, 0),
           (eng, host.ctypes.data, 8, 3, 0.01, 1e-4), (eng, 0, 8, 3, 0.01, 1e-4), (eng, d, 8, 3, 0.01, 1e-4, 0, 1, host.ctypes.data)]
    assert [raw(*b) for b in bad] == [_lib.EINVAL] * len(bad) and raw(empty, d, 8, 3, 0.01, 1e-4) == _lib.ESTATE
    assert eng.feature_rank_stats()["calls"] == 0 and not out.any()
    assert raw(eng, d, 8, 3, 0.01, 1e-4) == 0 and eng.feature_rank_stats()["calls"] == 1 and out.any()
