"""GPU: the dormant-neuron scan over ring rows and ReDo recycling (include/sactd3_dormant.h) against the plain float64 restatement of
tests/dormant_model.py, on a ring of 4096 seeded transitions and the parameters of sactd3_init_params.

The tolerance of a layer's scores is taken from no kernel: 4 x the largest |float32 - float64| of the same restatement run in torch
float32 on the CPU (MFMA's summation order differs from the CPU GEMM's; both errors are of the same order in K).  Measured on an
MI355X over the 64 cases of test 1: the kernel's error 1.1e-7 .. 3.7e-6, the CPU float32 restatement's 1.6e-7 .. 1.9e-6, the worst
case at 0.81 of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import dormant_model as dm, init_model
from tests.gpu_support import DEV, P, _lib, assert_same_state, close_engines, engine_state, same_bits, score, track  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
CAP, SEED = 4096, 7
NS = (1, 16, 17, 16 * 128 + 21)                  # a partial tile, the tile edge, one row behind it, workgroups that walk two tiles
SHAPES = ((3, 1), (11, 3), (17, 6), (70, 2))     # K = 3 / 4, 11 / 14, 17 / 23, and 70 / 72: above the kernel's LDS chunk of 64
PLANTED = ((5, 200), (0, 77))                    # the neurons test 2 and test 4 silence, per layer


def build(algo, o, a, ln, tracked=True):
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=bool(ln), batch_size=64)
    eng = P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=CAP, max_envs=96, seed=SEED), [-1.0] * a, [1.0] * a)
    if tracked:
        track(eng)
    eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
    five = synth_transitions(CAP, o, a, 1.0, seed=SEED + 1)
    eng.rb_extend(*[t.numpy() for t in five])
    return eng, torch.cat([five[0], five[1]], 1).numpy()


def scan(eng, idx, what=("actor", "critics"), tau=0.025):
    got = eng.dormant_scan(torch.as_tensor(np.asarray(idx, np.int64), device=DEV), what=what, tau=tau, scores=True)
    return got["scores"].cpu().numpy(), got


online = lambda eng: {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS)}


def reference(eng, o, a, algo, ln, rows):
    """(float64 scores, the bound per pair): the restatement at float64, and 4 x its own float32 error"""
    want, f32 = (dm.scores(online(eng), o, a, algo == "td3", ln, rows, t) for t in (torch.float64, torch.float32))
    return want, 4.0 * np.abs(f32 - want).max(1)


def plant(eng, o, a, algo, ln):
    """silence PLANTED in every net: LayerNorm weight 0 and bias -1; without LayerNorm a zero weight row and bias -1000"""
    params = online(eng)
    for _, K, nh, flat in init_model.nets_of(params, o, a, algo == "td3"):
        p = {(kind, layer): v for kind, layer, v in init_model.split(flat, K, nh, ln)}
        for layer, neurons in enumerate(PLANTED):
            for i in neurons:
                if ln:
                    p[("ln_weight", layer)][i], p[("ln_bias", layer)][i] = 0.0, -1.0
                else:
                    p[("weight", layer)][i], p[("bias", layer)][i] = 0.0, -1000.0
    eng.set_params(_lib.ACTOR, params["actor"])
    eng.set_params(_lib.CRITICS, params["critics"])


@pytest.fixture(scope="module", params=[(al, o, a, ln) for o, a in SHAPES for ln in (0, 1) for al in ("sac", "td3")], ids=str)
def case(request):
    eng, x = build(*request.param, tracked=False)
    yield eng, x, request.param
    eng.close()


@pytest.mark.parametrize("n", NS)
def test_scores_against_float64(case, n):
    eng, x, (algo, o, a, ln) = case
    idx = np.random.default_rng(n).integers(0, CAP, n)
    idx[-1] = idx[0]                                                          # (a duplicate wherever n > 1)
    got, info = scan(eng, idx)
    want, bound = reference(eng, o, a, algo, ln, x[idx])
    err = np.abs(got - want).max(1)
    print("dormant scores", (algo, o, a, ln, n), "kernel", err.tolist(), "bound", bound.tolist())
    assert info["valid_rows"] == n and info["refused_rows"] == 0
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("ln", [0, 1])
def test_masks_counts_and_bad_rows(ln):
    algo, o, a = "sac", 11, 3
    eng, x = build(algo, o, a, ln)
    plant(eng, o, a, algo, ln)
    valid = np.random.default_rng(3).integers(0, CAP, NS[-1])
    bad = np.insert(valid, [0, 40, valid.size], [-1, CAP, 2 ** 40])
    want, bound = reference(eng, o, a, algo, ln, x[valid])
    for tau in (0.0, 0.025):
        got, info = scan(eng, bad, tau=tau)
        alone, info_alone = scan(eng, valid, tau=tau)
        assert same_bits(got, alone) and info["refused_rows"] == 3 and info_alone["refused_rows"] == 0
        assert info["valid_rows"] == info_alone["valid_rows"] == valid.size and info["dormant"] == info_alone["dormant"]
        far = np.abs(want - tau) > bound[:, None]
        assert (far.sum(1) >= 254).all(), far.sum(1)                          # the float64 reference alone: at most 2 per layer too close
        assert ((got <= tau) == (want <= tau))[far].all()
        for pair, count in enumerate(info["dormant"].values()):
            planted = list(PLANTED[pair % 2])
            assert (got[pair, planted] == 0.0).all() and count == int((got[pair] <= tau).sum()) >= 2
    got, info = scan(eng, [-1, CAP, 2 ** 40])
    assert not got.any() and info["valid_rows"] == 0 and info["refused_rows"] == 3 and not any(info["dormant"].values())


def test_a_scan_refuses_bad_arguments_before_any_side_effect():
    eng, _ = build("sac", 11, 3, 1)
    empty = track(P.Engine(eng.cfg, [-1.0] * 3, [1.0] * 3))
    idx, host, out = torch.zeros(8, dtype=torch.int64, device=DEV), np.zeros(8, np.int64), torch.zeros(6, 256, device=DEV)
    raw = lambda e, p, n, what, tau, flags=0, ld=1: e.lib.sactd3_dormant_scan_device(e._h, C.c_void_p(p), ld, n, what, tau, C.c_void_p(out.data_ptr()), None, flags)
    d = idx.data_ptr()
    bad = [(eng, d, 0, 3, 0.1), (eng, d, 65537, 3, 0.1), (eng, d, 8, 0, 0.1), (eng, d, 8, 4, 0.1), (eng, d, 8, 3, -0.1), (eng, d, 8, 3, float("nan")),
           (eng, d, 8, 3, float("inf")), (eng, d, 8, 3, 0.1, 2), (eng, d, 8, 3, 0.1, 0, 0), (eng, host.ctypes.data, 8, 3, 0.1), (eng, 0, 8, 3, 0.1)]
    assert [raw(*b) for b in bad] == [_lib.EINVAL] * len(bad) and raw(empty, d, 8, 3, 0.1) == _lib.ESTATE
    assert eng.dormant_stats()["scans"] == 0 and not out.any()
    with pytest.raises(P.EngineError):
        eng.redo(("actor",))                                                  # nothing above counted as a scan
    assert raw(eng, d, 8, 3, 0.1) == 0 and eng.dormant_stats()["scans"] == 1


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_a_scan_is_invisible_and_repeatable(algo):
    """two engines, one scans between two chained runs of periods: the same parameters, optimiser state, metrics, sampled indices,
    noise and ring; two scans give the same bits; the critics alone get the bits they get beside the actor"""
    o, a = 11, 3
    (R, _), (N, _) = build(algo, o, a, 1), build(algo, o, a, 1)
    idx = np.random.default_rng(5).integers(0, CAP, 300)
    for eng in (R, N):
        it = eng.run_iterations(0, 6)
        if eng is R:
            first, again, critics = scan(R, idx)[0], scan(R, idx)[0], scan(R, idx, what=("critics",))[0]
        eng.run_iterations(it, 6)
    assert_same_state(R, N, "index", "noise", "ring")
    assert same_bits(first, again) and same_bits(first[2:], critics[2:]) and not critics[:2].any() and first[:2].any()


@pytest.mark.parametrize("algo,ln", [("sac", 1), ("sac", 0), ("td3", 0)])
def test_recycle(algo, ln):
    o, a, td3 = 11, 3, algo == "td3"
    eng, x = build(algo, o, a, ln)
    with pytest.raises(P.EngineError):
        eng.redo(("actor", "critics"), seed=11, epoch=1)                      # before any scan
    plant(eng, o, a, algo, ln)
    for which in (_lib.ACTOR, _lib.CRITICS):
        ones = np.ones(eng.param_count(which), np.float32)
        eng.set_adam_state(which, ones, 2 * ones, 5)
    idx = np.random.default_rng(9).integers(0, CAP, 512)
    mask = scan(eng, idx, tau=0.0)[0] <= 0.0
    rows = torch.as_tensor(x[idx[:64]])
    outputs = lambda: (score(eng, rows[:, :o].to(DEV), rows[:, o:].to(DEV)), eng.predict(rows[:, :o].numpy(), False))
    out_before, before = outputs(), engine_state(eng, "ring")
    eng.redo(("actor", "critics"), seed=11, epoch=1)
    out_after, after = outputs(), engine_state(eng, "ring")
    if not ln:                                                                # (header: with LayerNorm the layer's statistics move)
        assert all(same_bits(u, v) for u, v in zip(out_before, out_after))
    # what a redo writes: value, bound (0: exact) and a tag per element, laid over the parameters of before
    want = {k: before[f"params.{k}"].astype(np.float64) for k in ("actor", "critics")}
    bnd, tag = ({k: np.zeros_like(v) for k, v in want.items()} for _ in range(2))
    got32 = {k: after[f"params.{k}"] for k in want}
    for four in zip(*(init_model.nets_of(d, o, a, td3) for d in (want, bnd, tag, got32))):
        net, K, nh = four[0][:3]
        w, b, t, g = ({(kind, layer): v for kind, layer, v in init_model.split(d[3], K, nh, ln)} for d in four)
        for layer in (0, 1):
            for i in np.flatnonzero(mask[2 * net + layer]):
                w[("weight", layer)][i], b[("weight", layer)][i], c = dm.redraw64(11, 3 * net + layer, 1, i, K if layer == 0 else 256)
                if layer == 0:                                                # (a layer-2 row loses the columns of recycled layer-1 neurons)
                    norm = np.linalg.norm(g[("weight", 0)][i].astype(np.float64))
                    assert abs(norm - c) <= np.linalg.norm(b[("weight", 0)][i]), (net, i, norm, c)
                t[("weight", layer)][i] = t[("bias", layer)][i] = 1
                w[("bias", layer)][i] = 0.0
                if ln:
                    w[("ln_weight", layer)][i], w[("ln_bias", layer)][i] = 1.0, 0.0
                    t[("ln_weight", layer)][i] = t[("ln_bias", layer)][i] = 1
        for layer in (0, 1):                                                  # the outgoing columns last: the zero wins
            for d, v in ((w, 0.0), (b, 0.0), (t, 1)):
                d[("weight", layer + 1)][:, mask[2 * net + layer]] = v
    assert mask[0::2][:, PLANTED[0]].all() and mask[1::2][:, PLANTED[1]].all()
    for k in want:
        got, t = after[f"params.{k}"], tag[k] > 0
        assert (np.abs(got - want[k]) <= bnd[k]).all(), (k, float((np.abs(got - want[k]) - bnd[k]).max()))
        assert same_bits(got[~t], before[f"params.{k}"][~t])
        for m in ("adam_m", "adam_v"):
            assert same_bits(after[f"{m}.{k}"], np.where(t, np.float32(0), before[f"{m}.{k}"]))
    untouched = [k for k in before if k not in ("params.actor", "params.critics", "adam_m.actor", "adam_v.actor", "adam_m.critics", "adam_v.critics")]
    assert_same_state({k: before[k] for k in untouched}, {k: after[k] for k in untouched})
    st = eng.dormant_stats()
    assert st["redo_calls"] == 1 and st["recycled"] == int(mask.sum()) and st["rows_left_zero"] == 0
    with pytest.raises(P.EngineError):
        eng.redo(("critics",), seed=11, epoch=2)                              # a mask is good for one redo
    scan(eng, idx)
    eng.init_params(_lib.INIT_CRITICS, epoch=1)
    with pytest.raises(P.EngineError):
        eng.redo(("critics",), seed=11, epoch=2)                              # ... and none behind init_params
    eng.redo(("actor",), seed=11, epoch=2)


def test_through_the_loop():
    """loop.train on the native pendulum: the vitals are there and are fractions; with redo_every the recycler ran; with
    redo_every=None the run ends with the bits of the run without the keyword"""
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    n, seed = 2, 3
    cfg = P.launcher.job_config("sac", "pendulum", seed, num_envs=n, learning_starts=10, batch_size=4, num_timesteps=150 * n - 1,
                                eval_every=100, rb_capacity=512)
    o, a, bound = envs.SPECS[envs.kind_of("pendulum")][:3]
    runs = []
    for kw in (dict(), dict(dormant=dict(rows=64, tau=0.025)), dict(dormant=dict(rows=64, tau=0.025), redo_every=50)):
        agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV),
                        cfg, P.ReplayBuffer(cfg.rb_capacity), seed=seed, init="engine")
        track(agent.engine)
        env = track(envs.NativeVecEnv("pendulum", n, seed=seed, device=DEV, horizon=25))
        runs.append((agent, loop.train(cfg, env, agent, device_env=True, **kw)))
    (plain, _), (watched, out), (recycled, red) = runs
    assert_same_state(plain.engine, watched.engine, "index", "noise", "ring")
    for got in (out, red):
        assert all(0.0 <= got[k] <= 1.0 for k in ("vitals/dormant_actor", "vitals/dormant_critics"))
    st = recycled.engine.dormant_stats()
    assert out["vitals/recycled"] == 0 and red["vitals/recycled"] == recycled.recycles_so_far == st["redo_calls"] >= 2
