"""GPU: the k nearest ring rows of each query (include/sactd3_ring_knn.h) against the plain brute-force restatement of
tests/ring_knn_model.py.  Rows are synth_transitions plus a constant shift of 3 on every state column, so the xn - 2 dot expansion
cancels; key widths 3 .. 72 (below a float4, not a multiple of 4, above the 64-column chunk), both keys; ring lengths 1, 15 / 16 / 17
(the MFMA row tile's edge), 150 (three slices of 64, the last ragged) and a wrapped ring full at 1 024 (16 slices).

The tolerance is taken from no kernel.  Per case (ring, key, transform, range; its 65 queries) b = 4 x the largest |sel32 - sel64| of
the float32 CPU restatement: every reported slot has a float64 selector <= the float64 k-th smallest + 2 b, every slot below the k-th
smallest - 2 b is reported, and dist2 lies within 4 x the restatement's largest |dist2_32 - dist2_64| of the float64 direct distance.
Nothing is left out; the 2 b band is the only slack.

Measured on an MI355X over the 1 296 (case, n, k) combinations: no reported slot's float64 selector lay above the float64 k-th smallest
at all (the band was never entered: worst 0.0 of the 2 b allowed); dist2 error over the yardstick, worst per shape: (3, 1) 1.0,
(17, 6) 2.3, (70, 2) 3.9 -- the last at a ring of one row, n = 65, k = 1, where the yardstick is the largest of 65 numbers; 2.3 at the
rings of 15 rows and more."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import ring_knn_model as km
from tests.gpu_support import DEV, MAXN, P, _lib, assert_same_state, build_engines, close_engines, engine_state, same_bits, track  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu
K_BOUND, CAP, NQ = 4.0, 1024, 65
SHAPES = ((3, 1), (17, 6), (70, 2))
RINGS = {"1": 1, "15": 15, "16": 16, "17": 17, "150": 150, "wrapped": CAP + 100}


def ring_data(o, a, rows, seed=7):
    """(the five arrays to extend with, the [s | a] keys by ring slot afterwards) of `rows` shifted rows through a ring of CAP slots"""
    five = [t.numpy().copy() for t in synth_transitions(rows, o, a, 0.5, seed=seed)]
    five[0] += 3.0
    sa = np.concatenate([five[0], five[1]], 1)
    keys = sa[:CAP].copy()
    keys[: max(rows - CAP, 0)] = sa[CAP:]
    return five, keys


def new_engine(o, a, five=None):
    eng = P.Engine(P.Config.from_hps(Hps.sac(batch_size=64), o, a, rb_capacity=CAP, max_envs=MAXN, seed=0), [-0.5] * a, [0.5] * a)
    if five is not None:
        eng.rb_extend(*five)
    return eng


@pytest.fixture(scope="module", params=[(o, a, r) for o, a in SHAPES for r in RINGS], ids=str)
def ring(request):
    o, a, r = request.param
    five, keys = ring_data(o, a, RINGS[r])
    eng = new_engine(o, a, five)
    yield eng, keys, request.param
    eng.close()


@functools.lru_cache(maxsize=None)
def reference(o, a, r, key, tf, sub):
    """once per case: the 65 queries, the transform, the range, the float64 selectors and distances, and the two yardsticks"""
    keys = ring_data(o, a, RINGS[r])[1][:, : o + (a if key == "state_action" else 0)]
    L, D = keys.shape
    g = np.random.default_rng(1000 * o + L + 7 * tf + sub)
    q = np.concatenate([3.0 + g.normal(size=(NQ, o)), g.uniform(-0.5, 0.5, size=(NQ, a))], 1)[:, :D].astype(np.float32)
    c, w = ((3.0 + 0.1 * g.normal(size=D)).astype(np.float32), g.uniform(0.5, 2.0, size=D).astype(np.float32)) if tf else (None, None)
    first, count = (L // 3, max(1, L // 2)) if sub else (0, None)
    last = L if count is None else min(L, first + count)
    s64, d64 = (m.numpy() for m in km.matrices(q, keys, c, w, torch.float64))
    s32, d32 = (m.numpy() for m in km.matrices(q, keys, c, w, torch.float32))
    return dict(q=q, c=c, w=w, first=first, count=count, last=last, s64=s64, d64=d64, keys=keys,
                b=K_BOUND * np.abs(s32 - s64)[:, first:last].max(), yard=np.abs(d32 - d64)[:, first:last].max())


def search(eng, q, k, key="state", c=None, w=None, exclude=None, first=0, count=None):
    dev = lambda x, t: None if x is None else torch.as_tensor(np.asarray(x), dtype=t, device=DEV)
    got = eng.ring_knn(dev(q, torch.float32), k, key=key, offset=dev(c, torch.float32), scale=dev(w, torch.float32),
                       exclude=dev(exclude, torch.int64), first=first, count=count)
    return got["index"].cpu().numpy(), got["dist2"].cpu().numpy()


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("tf", [0, 1])
@pytest.mark.parametrize("key", ["state", "state_action"])
def test_against_float64(ring, key, tf, sub):
    eng, _, (o, a, r) = ring
    R = reference(o, a, r, key, tf, sub)
    lo, hi, b = R["first"], R["last"], R["b"]
    for n, k in [(n, k) for n in (1, 17, NQ) for k in (1, 5, 16)]:
        index, dist2 = search(eng, R["q"][:n], k, key, R["c"], R["w"], first=lo, count=R["count"])
        worst_band = worst_dist = 0.0
        for i in range(n):
            sel, found = R["s64"][i, lo:hi], index[i][index[i] >= 0]
            assert len(found) == min(k, hi - lo) == len(set(found)) and ((found >= lo) & (found < hi)).all(), (n, k, i, index[i])
            assert (index[i, len(found):] == -1).all() and np.isinf(dist2[i, len(found):]).all(), (n, k, i)
            if hi - lo > k:
                kth = np.sort(sel)[k - 1]
                worst_band = max(worst_band, (R["s64"][i, found].max() - kth) / b)
                assert (R["s64"][i, found] <= kth + 2 * b).all() and set(lo + np.flatnonzero(sel < kth - 2 * b)) <= set(found), (n, k, i, index[i])
            worst_dist = max(worst_dist, np.abs(dist2[i, : len(found)] - R["d64"][i, found]).max() / R["yard"])
            assert (np.lexsort((found, dist2[i, : len(found)])) == np.arange(len(found))).all(), (n, k, i, index[i], dist2[i])
        print("ring_knn", (o, a, r, key, tf, sub, n, k), "band", float(worst_band), "of 2; dist ratio", float(worst_dist), "of", K_BOUND)
        assert worst_dist <= K_BOUND, (n, k)


def test_ties_and_exclude():
    """exact duplicates of three ring rows at higher slots: the lower slot first, equal dist2 bits; a query that is ring row j finds j
    first at distance 0, and with exclude = j what the model finds with row j removed"""
    o, a = 17, 6
    five, keys = ring_data(o, a, 150)
    for src, dst in ((5, 70), (20, 149), (64, 65)):
        for t in five:
            t[dst] = t[src]
        keys[dst] = keys[src]
    eng = track(new_engine(o, a, five))
    q = keys[[5, 20, 64], :o] + np.float32(1e-3)
    index, dist2 = search(eng, q, 2)
    assert index.tolist() == [[5, 70], [20, 149], [64, 65]] and same_bits(dist2[:, 0], dist2[:, 1])
    own = np.array([5, 33, 149, 64])
    index, dist2 = search(eng, keys[own, :o], 5)
    assert index[:, 0].tolist() == [5, 33, 20, 64] and (dist2[:, 0] == 0).all()
    index, dist2 = search(eng, keys[own, :o], 5, exclude=own)
    want = km.knn(keys[own, :o], keys[:, :o], 5, exclude=own)
    assert (index == want[0]).all() and np.allclose(dist2, want[1], rtol=1e-5)


def test_row_independence_and_slicing():
    """query i alone and inside n = 65: the same bits; the full ring against two sub-range calls that split it: every full-ring hit
    stands in the sub-range results with the same dist2 bits, and the full result is the union's k best by (dist2, slot) wherever the
    union's dist2 values are apart by more than the selector band"""
    o, a, r = 70, 2, "wrapped"
    five, keys = ring_data(o, a, RINGS[r])
    eng, R = track(new_engine(o, a, five)), reference(o, a, r, "state_action", 1, 0)
    q, kw = R["q"], dict(key="state_action", c=R["c"], w=R["w"])
    whole = search(eng, q, 5, **kw)
    for i in (0, 40, 64):
        alone = search(eng, q[i:i + 1], 5, **kw)
        assert same_bits(alone[0], whole[0][i:i + 1]) and same_bits(alone[1], whole[1][i:i + 1])
    lower, upper = search(eng, q, 5, first=0, count=391, **kw), search(eng, q, 5, first=391, **kw)
    for i in range(NQ):
        union = {int(s): d for idx, d2 in (lower, upper) for s, d in zip(idx[i], d2[i])}
        assert all(same_bits(np.float32(union[int(s)]), d) for s, d in zip(whole[0][i], whole[1][i])), i
        rest = [d for s, d in union.items() if s not in set(whole[0][i].tolist())]
        assert min(rest) >= whole[1][i, -1] - 2 * R["b"], i


def test_short_results_nonfinite_values_and_refusals():
    o, a = 3, 1
    five, keys = ring_data(o, a, 40)
    five[0][11, 1] = np.nan
    eng, one = track(new_engine(o, a, five)), track(new_engine(o, a, ring_data(o, a, 1)[0]))
    index, dist2 = search(one, keys[:2, :o], 5)
    assert (index[:, 0] == 0).all() and (index[:, 1:] == -1).all() and np.isinf(dist2[:, 1:]).all() and np.isfinite(dist2[:, 0]).all()
    assert one.ring_knn_stats() == dict(calls=1, queries=2, rows_scanned=1, queries_nonfinite=0, ring_keys_nonfinite=0, short_results=2)
    q = keys[:3, :o].copy()
    q[1, 2] = np.nan
    index, dist2 = search(eng, q, 16)
    assert (index[1] == -1).all() and np.isnan(dist2[1]).all() and 11 not in index and (index[[0, 2]] >= 0).all()
    assert eng.ring_knn_stats() == dict(calls=1, queries=3, rows_scanned=40, queries_nonfinite=1, ring_keys_nonfinite=1, short_results=0)
    before = engine_state(eng)
    qd, out = torch.as_tensor(q, device=DEV), torch.empty(3, 16, dtype=torch.int64, device=DEV)
    host = torch.zeros(3, 16, dtype=torch.int64)

    def raw(handle=eng._h, queries=qd.data_ptr(), ld=o, n=3, k=16, key=0, first=0, count=0, index=out.data_ptr(), index_ld=16, io=True, flags=0, **f):
        s = _lib.CRingKnnIO(index=index, index_ld=index_ld, **f)
        return eng.lib.sactd3_ring_knn_device(handle, queries, ld, n, k, key, first, count, C.byref(s) if io else None, None, flags)

    bad = [dict(handle=None), dict(queries=None), dict(io=False), dict(index=None), dict(n=0), dict(k=0), dict(k=17), dict(key=2), dict(flags=4),
           dict(first=-1), dict(count=-1), dict(ld=o - 1), dict(index_ld=15), dict(exclude=out.data_ptr(), exclude_ld=0), dict(index=host.data_ptr())]
    assert [raw(**b) for b in bad] == [_lib.EINVAL] * len(bad)
    assert raw(first=40) == _lib.ESTATE and raw(handle=track(new_engine(o, a))._h) == _lib.ESTATE
    assert_same_state(before, engine_state(eng))
    assert eng.ring_knn_stats()["calls"] == 1 and raw() == 0 and eng.ring_knn_stats()["calls"] == 2


def test_invisible_between_two_periods():
    _, (R, Q), (o, a, bound) = build_engines("sac", (17, 6, 0.5), 64, count=2, seed=3, cap=CAP, max_envs=MAXN)
    five, keys = ring_data(o, a, CAP)
    for eng in (R, Q):
        eng.rb_extend(*five)
        it = eng.run_iterations(0, 6)
        if eng is R:
            search(R, keys[:NQ], 16, key="state_action", exclude=np.arange(NQ))
            search(R, keys[:3, :o], 1, first=100, count=200)
        eng.run_iterations(it, 6)
    assert_same_state(R, Q, "index", "noise", "ring")


def test_through_the_agent_and_the_loop():
    """state_novelty and dataset_distance are their composition from Engine.ring_knn, rows and policy; loop.train with knn= ends with
    the bits of the run without the keyword and logs both vitals"""
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    n, seed = 2, 3
    cfg = P.launcher.job_config("sac", "pendulum", seed, num_envs=n, learning_starts=10, batch_size=4, num_timesteps=150 * n - 1,
                                eval_every=100, rb_capacity=512)
    o, a, bound = envs.SPECS[envs.kind_of("pendulum")][:3]
    runs = []
    for kw in (dict(), dict(knn=dict(rows=32, k=3, beta=1.5))):
        agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV),
                        cfg, P.ReplayBuffer(cfg.rb_capacity), seed=seed, init="engine")
        track(agent.engine)
        env = track(envs.NativeVecEnv("pendulum", n, seed=seed, device=DEV, horizon=25))
        runs.append((agent, loop.train(cfg, env, agent, device_env=True, **kw)))
    (plain, _), (watched, out) = runs
    assert_same_state(plain.engine, watched.engine, "index", "noise", "ring")
    assert all(np.isfinite(out[k]) for k in loop.Knn.KEYS) and watched.engine.ring_knn_stats()["calls"] >= 2
    index = torch.tensor([0, 7, 100, 7], device=DEV)
    obs = watched.rb.rows(index)["observations"]
    nov, got = watched.state_novelty(index, k=3), watched.engine.ring_knn(obs, 3, exclude=index)
    assert torch.equal(nov["dist2"], got["dist2"][:, 2]) and torch.equal(nov["bonus"], 0.5 * torch.log1p(got["dist2"][:, 2]))
    far, mode = watched.dataset_distance(obs, beta=1.5, k=2, count=200), watched.policy({"observations": obs})["mode"]
    inv = torch.as_tensor(2.0 / (watched.max_ac - watched.min_ac), dtype=torch.float32, device=DEV)
    scale = torch.cat([torch.full((o,), 1.5, device=DEV), inv])
    got = watched.engine.ring_knn(torch.cat([obs, mode], 1), 2, key="state_action", scale=scale, count=200)
    assert torch.equal(far["index"], got["index"]) and torch.equal(far["dist2"], got["dist2"]) and int(far["index"].max()) < 200
    acts = watched.rb.rows(got["index"].reshape(-1))["actions"].reshape(4, 2, a)
    assert torch.equal(far["action_dist2"], (((mode[:, None] - acts) * inv) ** 2).sum(-1)) and bool((far["action_dist2"] <= far["dist2"] * (1 + 1e-5) + 1e-6).all())
