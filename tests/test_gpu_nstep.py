"""GPU: n-step returns staged by the engine (include/sactd3.h: sactd3_rb_sample_nstep_device, sactd3_rb_sample_nstep,
sactd3_rb_sample_prioritized_nstep, sactd3_nstep_info_device, sactd3_nstep_stats) against the numpy restatement of tests/nstep_ref.py
and against twin engines.

Engines are shape_engines() of tests/gpu_support.py (the oracle's perturbed parameters) with the critic site's noise injected as in
tests/test_gpu_native_priorities.py.  Shapes: SAC Hopper at B = 64 and B = 40 (o % 4 = 3), TD3 HalfCheetah at B = 64 (o % 4 = 1), SAC
Humanoid at B = 64 (o % 4 = 0, 196 chunks per record: a block's span holds a handful of rows), SAC Hopper at B = 1024 (many blocks).

Ring U: 5000 slots, 2400 rows = 600 env steps of 4 envs, chained trajectories built on the host (gpu_support.trajectories).  Episode lengths cycle through
1, 2, 3, 4, 5, 6, 15, 16, 17 (steps - 1, steps, steps + 1 for the step counts in use); episodes end by termination or, alternately, by a
fresh s without a flag.  Planted: (a) a successor whose s differs from s' in element ob_dim - 1 only, (b) a -0.0 / +0.0 pair, (c) a pair
of equal NaN patterns (the link holds), (d) the newest step's s' zeroed and unflagged, so that only the length rule cuts it off from the
(all-zero) unfilled slots.
Ring W: 1001 slots, 1400 rows, cursor 399.  Every row of the oldest step has s equal to the s' of the matching row of the newest step,
so only the age rule cuts there."""
import functools

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import nstep_ref as nref
from tests.gpu_support import (DEV, MAXN, NSTEP_STRIDE as STRIDE, SEED, SHAPES, P, _lib, assert_same_bits, assert_same_state, close_engines,  # noqa: F401
                               info, loop, push_params, same_bits, shape_engines, slot, stage, stream, track, trajectories)

pytestmark = pytest.mark.gpu

CASES = {"sac-hopper-64": ("sac-hopper", 64), "sac-hopper-40": ("sac-hopper", 40), "td3-halfcheetah-64": ("td3-halfcheetah", 64),
         "sac-humanoid-64": ("sac-humanoid", 64), "sac-hopper-1024": ("sac-hopper", 1024)}
ALL = list(CASES)
STEPS = (1, 2, 3, 5, 16)
U_CAP, U_ROWS = 5000, 2400
W_CAP, W_ROWS = 1001, 1400


@functools.lru_cache(maxsize=None)
def ring_u(shape, planted=True):
    """-> dict: rows (append order), the slot-indexed fields, length / cursor / cap, and the planted rows.  planted=False: (d) only --
    no NaN anywhere, for the tests that run updates"""
    _, (o, a, _), _ = SHAPES[shape]
    rows = trajectories(o, a, U_ROWS, 21)
    obs, act, rew, nobs, done = rows
    nobs[U_ROWS - STRIDE:] = 0.0                                       # (d)
    done[U_ROWS - STRIDE:] = 0.0
    special = {}
    if planted:
        (f0, _, r0, n0, d0), length, cursor = nref.place(rows, U_CAP)
        k3 = nref.chains(f0, n0, r0, d0, np.arange(U_ROWS), 3, STRIDE, length, cursor, U_CAP, 0.99)["k"]
        mid = [int(r) for r in np.flatnonzero(k3 == 3) if 100 < r < 2000]      # rows whose next two links hold
        ra, rb, rc = mid[0], mid[40], mid[80]
        assert len({ra, rb, rc, ra + STRIDE, rb + STRIDE, rc + STRIDE}) == 6
        obs[ra + STRIDE, o - 1] = nobs[ra, o - 1] + np.float32(1.0)    # (a)
        nobs[rb, 0], obs[rb + STRIDE, 0] = np.float32(-0.0), np.float32(0.0)      # (b)
        nobs[rc, 1] = obs[rc + STRIDE, 1] = np.float32(np.nan)         # (c)
        special = dict(a=ra, b=rb, c=rc)
    fields, length, cursor = nref.place(rows, U_CAP)
    return dict(rows=rows, fields=fields, length=length, cursor=cursor, cap=U_CAP, special=special)


@functools.lru_cache(maxsize=None)
def ring_w(shape):
    _, (o, a, _), _ = SHAPES[shape]
    rows = trajectories(o, a, W_ROWS, 22)
    obs, act, rew, nobs, done = rows
    oldest = W_ROWS - W_CAP                                            # the oldest row the ring still holds: slot 399 = the cursor
    for i in range(STRIDE):                                            # slot of the newest step's row i, + STRIDE, wraps onto the oldest rows
        assert (W_ROWS - STRIDE + i + STRIDE) % W_CAP == (oldest + i) % W_CAP
        obs[oldest + i] = nobs[W_ROWS - STRIDE + i]
        done[W_ROWS - STRIDE + i] = 0.0
    fields, length, cursor = nref.place(rows, W_CAP)
    assert (length, cursor) == (W_CAP, 399)
    return dict(rows=rows, fields=fields, length=length, cursor=cursor, cap=W_CAP, special={})


def fill(eng, ring):
    rows, cap = ring["rows"], ring["cap"]
    for lo in range(0, len(rows[0]), cap - 1):                         # (at most the capacity per call)
        eng.rb_extend(*[f[lo:lo + cap - 1] for f in rows])
    assert eng.rb_len() == ring["length"]


def build(case, count, ring, prio=None):
    """`count` twin engines holding `ring`, the same critic noise injected"""
    shape, B = CASES[case]
    ref, engs, (o, a, bound) = shape_engines(shape, count, B=B, cap=ring["cap"])
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for eng in engs:
        fill(eng, ring)
        eng.set_noise(_lib.SITE_CRITIC, eps)
        if prio is not None:
            eng.prio_enable(*prio)
    return ref, engs, (o, a, bound), B, eps


def stage_n(eng, idx, w, steps, stride=STRIDE):
    """sactd3_rb_sample_nstep_device on CUDA tensors (any stride); -> what has to stay alive"""
    idx = idx if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx, np.int64), device=DEV)
    w = torch.as_tensor(np.asarray(w, np.float32), device=DEV) if w is not None and not torch.is_tensor(w) else w
    eng.rb_sample_nstep_device(idx.data_ptr(), max(idx.stride(0), 1), 0 if w is None else w.data_ptr(), 1 if w is None else max(w.stride(0), 1),
                               idx.shape[0], steps, stride, stream())
    return idx, w


def expected(eng, ring, idx, steps):
    """what the restatement says batch slot 0 holds after staging `idx` with `steps`"""
    obs, act, rew, nobs, done = ring["fields"]
    lay = eng.rb_layout()
    o, a = obs.shape[1], act.shape[1]
    c = nref.chains(obs, nobs, rew, done, idx, steps, STRIDE, ring["length"], ring["cursor"], ring["cap"], np.float32(eng.cfg.gamma))
    B = len(idx)
    ok = c["k"] > 0
    i0 = np.where(ok, np.asarray(idx), 0).astype(np.int64)
    X = np.zeros((B, lay["next_obs_offset"]), np.float32)
    X[:, :o], X[:, o:o + a] = obs[i0], act[i0]
    Xn = np.zeros((B, lay["next_obs_width"]), np.float32)
    Xn[:, :o] = nobs[np.where(ok, c["last"], 0)]
    X[~ok], Xn[~ok] = 0.0, 0.0
    return dict(X=X, Xn=Xn, rew=c["R"], done=c["mask"], index=np.where(ok, np.asarray(idx), -1).astype(np.int64), k=c["k"], last=c["last"])


def read_slot(eng):
    lay = eng.rb_layout()
    B = eng.cfg.batch_size
    d = slot(eng)
    d["X"] = d["X"].reshape(B, -1)[:, :lay["next_obs_offset"]]
    d["Xn"] = d["Xn"].reshape(B, -1)[:, :lay["next_obs_width"]]
    d["k"], d["last"] = info(eng)
    return d


def assert_slot_is(got, want, what):
    for key in ("X", "Xn", "rew", "done"):
        assert same_bits(np.asarray(got[key]), np.asarray(want[key])), (what, key, np.flatnonzero(
            (nref.bits(got[key]).reshape(len(want["k"]), -1) != nref.bits(want[key]).reshape(len(want["k"]), -1)).any(1))[:8])
    for key in ("index", "k", "last"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])


def start_slots(ring, B, steps):
    """start slots that cover the planted rows with their neighbours, the ring's ends, the slots around the cursor and a few slots the
    engine must refuse; filled up to B with random slots of the whole capacity (for U those >= length are refused)"""
    sp, length, cursor, cap = ring["special"], ring["length"], ring["cursor"], ring["cap"]
    want = []
    for r in sp.values():
        want += [r - STRIDE, r, r + STRIDE]
    want += [0, 1, 2, 3, cap - 1, length - 1, length - 2, length - 3, length - 4, length - 5, length - 8, -1, length, cap]
    want += [(cursor + d) % cap for d in range(-6, 5)]
    k16 = safe_rows(ring, 16, full=True)["k"]
    want += [int(np.flatnonzero(k16 == n)[0]) for n in (14, 15, 16)]      # chains of steps - 2, steps - 1 and steps rows at steps = 16
    rng = np.random.default_rng(100 + steps)
    idx = np.concatenate([np.asarray(want, np.int64), rng.integers(0, cap, max(B - len(want), 0))])[:B]
    assert len(idx) == B and len(want) <= 40
    return idx


def safe_rows(ring, steps, full=False):
    """start slots in [0, length) (full: whose chain has exactly `steps` rows)"""
    obs, act, rew, nobs, done = ring["fields"]
    c = nref.chains(obs, nobs, rew, done, np.arange(ring["length"]), steps, STRIDE, ring["length"], ring["cursor"], ring["cap"], 0.99)
    return c if full else np.arange(ring["length"])


# ------------------------------------------------------------------------------------------ 1. staging equals the restatement
@pytest.mark.parametrize("which", ["U", "W"])
@pytest.mark.parametrize("case", ALL)
def test_staging_equals_the_restatement_bit_for_bit(case, which):
    ring = (ring_u if which == "U" else ring_w)(CASES[case][0])
    _, (eng,), _, B, _ = build(case, 1, ring)
    if which == "U":                                                   # the plants do what they are there for
        sp, f = ring["special"], ring["fields"]
        k3 = lambda r: nref.chain(f[0], f[3], f[2], f[4], r, 3, STRIDE, ring["length"], ring["cursor"], ring["cap"], 0.99)[0]
        assert k3(sp["a"]) == 1 and k3(sp["b"]) == 1 and k3(sp["c"]) == 3 and k3(U_ROWS - 1) == 1
    else:
        f = ring["fields"]
        newest = (ring["cursor"] - 1) % ring["cap"]
        assert same_bits(f[3][newest], f[0][(newest + STRIDE) % ring["cap"]])      # the data would link the newest row to the oldest
    before = eng.nstep_stats()
    assert before == dict(stagings=0, rows_staged=0, rows_cut_short=0, rows_refused=0)
    cut = refused = 0
    keep = []
    for n, steps in enumerate(STEPS):
        idx = start_slots(ring, B, steps)
        keep.append(stage_n(eng, idx, None, steps))
        want = expected(eng, ring, idx, steps)
        assert_slot_is(read_slot(eng), want, (case, which, steps))
        cut += int(((want["k"] > 0) & (want["k"] < steps)).sum())
        refused += int((want["k"] == 0).sum())
        assert eng.nstep_stats() == dict(stagings=n + 1, rows_staged=(n + 1) * B, rows_cut_short=cut, rows_refused=refused)
        if steps == 16:
            assert (want["k"] == 16).any() and (want["k"] == 1).any()
    assert refused > 0 and cut > 0


# ------------------------------------------------------------------------------------------ 2. steps == 1 is the 1-step staging
@pytest.mark.parametrize("case", ALL)
def test_one_step_staging_is_the_index_staging_bit_for_bit(case):
    ring = ring_u(CASES[case][0], False)
    _, (A, T), _, B, _ = build(case, 2, ring, prio=(1.0, 1e-6))      # (priorities on: debug_read("prio_weights") reads the slot's weights)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, ring["length"], B)
    idx[:3] = [0, ring["length"] - 1, ring["length"] - 1]
    w = rng.uniform(0.1, 1.0, B).astype(np.float32)
    keep = [stage_n(A, idx, w, 1), stage(T, torch.as_tensor(idx, device=DEV), torch.as_tensor(w))]
    assert_same_bits(slot(A), slot(T), what=case)
    assert same_bits(A.debug_read("prio_weights"), T.debug_read("prio_weights"))
    k, last = info(A)
    assert (k == 1).all() and np.array_equal(last, idx)
    A.update_qnets()
    T.update_qnets()
    assert_same_state(A, T)
    assert same_bits(A.debug_read("targ_q"), T.debug_read("targ_q"))
    del keep


# ------------------------------------------------------------------------------------------ 3. bad indices, bad weights
@pytest.mark.parametrize("case", ALL)
def test_bad_indices_and_weights_are_neutralised_and_counted(case):
    ring = ring_u(CASES[case][0], False)
    _, (A, T), _, B, _ = build(case, 2, ring, prio=(1.0, 1e-6))
    rng = np.random.default_rng(6)
    good = rng.integers(0, ring["length"], B)
    idx, w = good.copy(), rng.uniform(0.1, 1.0, B).astype(np.float32)
    bad_i, bad_w = [1, 7, B - 1], [0, 9, 20]
    idx[bad_i] = [-1, ring["length"], 2 ** 40]
    w[bad_w] = [-1.0, np.nan, np.inf]
    padded = torch.full((B + 2,), 7, dtype=torch.int64, device=DEV)      # a sentinel row on either side of the index array
    padded[1:-1] = torch.as_tensor(idx, device=DEV)
    keep = [stage_n(A, padded[1:-1], w, 3)]
    got, want = read_slot(A), expected(A, ring, idx, 3)
    assert_slot_is(got, want, case)
    for b in bad_i:
        assert not got["X"][b].any() and not got["Xn"][b].any() and got["rew"][b] == 0 and got["done"][b] == 0
        assert (got["index"][b], got["k"][b], got["last"][b]) == (-1, 0, -1)
    ws = A.debug_read("prio_weights")
    w0 = w.copy()
    w0[bad_i + bad_w] = 0.0
    assert same_bits(ws, w0) and (got["k"][bad_w] >= 1).all()
    assert A.nstep_stats()["rows_refused"] == len(bad_i) + len(bad_w)
    assert padded[0].item() == 7 and padded[-1].item() == 7
    # a twin that staged the same rows (any valid row in place of a refused one) with weight 0
    twin_idx = np.where(want["k"] > 0, idx, 0)
    keep.append(stage_n(T, twin_idx, w0, 3))
    A.update_qnets()
    T.update_qnets()
    assert_same_state(A, T)
    del keep


# ------------------------------------------------------------------------------------------ 4. the engine's own uniform draw
@pytest.mark.parametrize("case", ALL)
def test_native_draw_starts_where_rb_sample_draws(case):
    ring = ring_u(CASES[case][0], False)
    _, (A, T, Cn), _, B, _ = build(case, 3, ring)
    A.rb_sample_nstep(3, STRIDE)
    T.rb_sample()
    first = read_slot(A)
    idx = T.read_batch()["index"]
    assert np.array_equal(first["index"], idx) and (idx >= 0).all() and (idx < ring["length"]).all()
    assert_slot_is(first, expected(A, ring, idx, 3), case)
    keep = stage_n(Cn, idx, None, 3)
    assert_slot_is(read_slot(Cn), first, case)
    A.rb_sample()                                                      # one tick, as rb_sample's
    T.rb_sample()
    assert np.array_equal(A.read_batch()["index"], T.read_batch()["index"]) and not np.array_equal(A.read_batch()["index"], idx)
    with pytest.raises(P.EngineError, match="-3"):                     # the slot is no n-step slot any more
        info(A)
    A.rb_sample_nstep(3, STRIDE)
    A.update_qnets()                                                   # no weights: the unweighted critic graph
    assert A.graph_kernel_count(8) == 0
    del keep


# ------------------------------------------------------------------------------------------ 5. prioritised
@pytest.mark.parametrize("case", ALL)
def test_prioritised_nstep_draws_weights_and_writes_back_like_the_one_step_call(case):
    ring = ring_u(CASES[case][0], False)
    _, (A, T, Cn), _, B, _ = build(case, 3, ring, prio=None)
    rng = np.random.default_rng(7)
    prio = rng.choice(np.float32([0.0, 1.0, 1.0, 1.0, 2.0, 3.0]), ring["length"]).astype(np.float32)
    u = rng.random(B).astype(np.float32)
    keep = []
    for eng in (A, T):
        eng.prio_enable(1.0, 1e-6)
        i = torch.arange(ring["length"], device=DEV)
        p = torch.as_tensor(prio, device=DEV)
        eng.prio_update_device(i.data_ptr(), 1, p.data_ptr(), 1, ring["length"], stream())
        eng.prio_set_uniforms(u)
        keep.append((i, p))
    A.rb_sample_prioritized_nstep(0.4, 3, STRIDE)
    T.rb_sample_prioritized(0.4)
    got = read_slot(A)
    idx, w = T.read_batch()["index"], T.debug_read("prio_weights")
    assert np.array_equal(got["index"], idx) and (prio[idx] > 0).all()
    assert same_bits(A.debug_read("prio_weights"), w)
    keep.append(stage_n(Cn, idx, w, 3))
    assert_slot_is(got, read_slot(Cn), case)
    assert_slot_is(got, expected(A, ring, idx, 3), case)
    leaf0 = A.debug_read("prio_leaf")
    A.update_qnets()
    A.prio_update_from_td()
    leaf1 = A.debug_read("prio_leaf")
    changed = np.flatnonzero(nref.bits(leaf0) != nref.bits(leaf1))
    assert len(changed) > 0 and np.isin(changed, idx).all()            # the start slots only
    assert A.prio_stats()["samples"] == 1 and A.nstep_stats()["stagings"] == 1
    del keep


# ------------------------------------------------------------------------------------------ 6. the target is the n-step target
@pytest.mark.parametrize("steps", [3, 16])
@pytest.mark.parametrize("case", ALL)
def test_the_critic_target_is_the_n_step_target(case, steps):
    """targ_q against a twin whose discount is gamma^steps and whose batch is (s_0, a_0, R, s'_last, d_last), loaded through load_batch.
    Terminated chains: equal bits.  The others: within 2 (steps + 4) 2^-24 max(1, |q'|, |y|) -- steps - 1 multiplies for G, two
    subtractions of the mask, the gamma multiply and the final add, against two roundings on the twin."""
    shape, B = CASES[case]
    ring = ring_u(shape, False)
    ref, (A,), (o, a, bound), _, eps = build(case, 1, ring)
    g32 = np.float32(A.cfg.gamma)
    gk = float(np.float32(np.float64(g32) ** steps))
    algo, _, ln = SHAPES[shape]
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=ln, batch_size=B)
    T = track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=ring["cap"], max_envs=MAXN, seed=SEED, gamma=gk), [-bound] * a, [bound] * a))
    push_params(T, ref)
    T.set_noise(_lib.SITE_CRITIC, eps)
    obs, act, rew, nobs, done = ring["fields"]
    c = safe_rows(ring, steps, full=True)
    full = c["k"] == steps
    term, cont = np.flatnonzero(full & (done[c["last"]] == 1)), np.flatnonzero(full & (done[c["last"]] == 0))
    assert len(term) > 0 and len(cont) > 0
    rng = np.random.default_rng(8)
    idx = np.concatenate([rng.choice(term, B // 2), rng.choice(cont, B - B // 2)])
    keep = stage_n(A, idx, None, steps)
    k, last = info(A)
    assert (k == steps).all() and np.array_equal(last, c["last"][idx])
    T.load_batch(obs[idx], act[idx], c["R"][idx], nobs[last], done[last].astype(np.uint8))
    A.update_qnets()
    T.update_qnets()
    y, yt = A.debug_read("targ_q").astype(np.float64), T.debug_read("targ_q").astype(np.float64)
    ended = done[last] == 1
    assert ended.sum() == B // 2
    assert same_bits(A.debug_read("targ_q")[ended], T.debug_read("targ_q")[ended])
    qp = (yt - c["R"][idx].astype(np.float64)) / gk                    # the twin's bootstrap value
    bound_b = 2.0 * (steps + 4) * 2.0 ** -24 * np.maximum(1.0, np.maximum(np.abs(qp), np.abs(yt)))
    err = np.abs(y - yt)
    print(f"{case} steps={steps}: max |y - y_twin| = {err[~ended].max():.3e}, smallest bound = {bound_b[~ended].min():.3e}, "
          f"largest ratio = {(err / bound_b)[~ended].max():.3f}")
    assert (err[~ended] <= bound_b[~ended]).all(), np.flatnonzero(err > bound_b)
    del keep


# ------------------------------------------------------------------------------------------ 7. host state
def test_n_step_state_is_set_by_the_three_calls_and_cleared_by_every_other_refill():
    ring = ring_u("sac-hopper", False)
    _, (A, T), _, B, _ = build("sac-hopper-64", 2, ring)
    for eng in (A, T):
        eng.rb_sample()                                                # (one tick of the sample counter on both)
    with pytest.raises(P.EngineError, match="-3"):
        info(A)
    idx = np.arange(B) * 3
    keep = [stage_n(A, idx, None, 3)]
    assert (info(A)[0] >= 1).all()
    A.step(True)                                                       # the fused iteration draws its own 1-step sample
    T.step(True)
    with pytest.raises(P.EngineError, match="-3"):
        info(A)
    x, y = A.read_batch(), T.read_batch()
    for key in x:
        assert np.array_equal(x[key], y[key]), key
    assert_same_state(A, T)
    # between two chained periods: the staging breaks the run-ahead chain, the second period equals single steps
    res = []
    for eng in (A, T):
        it = eng.run_iterations(0, 3)
        if eng is A:
            keep.append(stage_n(A, idx, None, 5))
        it = eng.run_iterations(it, 3)
        res.append(eng.read_batch()["index"])
    assert np.array_equal(res[0], res[1])
    assert_same_state(A, T)
    del keep


def test_slot_state_through_a_sequence_of_refills_and_updates():
    """what the host knows about batch slot 0 (n-step rows? loss weights? TD errors of its rows?) behind each call of a sequence that mixes
    the staging calls, the API-path update and a fused iteration: the return codes of sactd3_nstep_info_device and
    sactd3_td_errors_device, and the weighted graph (graph 8) captured by the first weighted update only.  SAC Hopper, B = 64."""
    ring = ring_u("sac-hopper", False)
    _, (eng,), _, B, _ = build("sac-hopper-64", 1, ring, prio=(0.6, 1e-6))
    lib, h = eng.lib, eng._h
    k, td = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(2, B, device=DEV)

    def state():
        """(nstep_info's code, td_errors' code, nodes of the weighted update graph)"""
        return (lib.sactd3_nstep_info_device(h, k.data_ptr(), 1, None, 1, None, 0), lib.sactd3_td_errors_device(h, td.data_ptr(), 1, B, None, 0),
                eng.graph_kernel_count(8))

    OK, NO = 0, _lib.ESTATE
    assert lib.sactd3_rb_sample_nstep(h, 3, STRIDE) == 0 and state() == (OK, NO, 0)           # an n-step slot; no update has seen its rows
    assert lib.sactd3_update_qnets(h) == 0 and state() == (OK, OK, 0)                         # the update keeps what the refill staged
    assert lib.sactd3_rb_sample_prioritized(h, 0.4) == 0 and state() == (NO, NO, 0)           # 1-step rows with weights
    assert lib.sactd3_batch_weights_device(h, None, 1, B, None, 0) == 0 and state() == (NO, NO, 0)      # weights dropped, nothing else
    assert lib.sactd3_update_qnets(h) == 0 and state() == (NO, OK, 0)                         # ... so this update was the unweighted one
    assert lib.sactd3_step(h, 1) == 0 and state() == (NO, OK, 0)                              # fused: its own 1-step sample
    assert lib.sactd3_rb_sample_prioritized(h, 0.4) == 0 and state() == (NO, NO, 0)
    assert lib.sactd3_update_qnets(h) == 0
    s = state()
    assert s[:2] == (NO, OK) and s[2] > 0                                                     # the weighted graph, at its first use
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 8. views and streams
@pytest.mark.parametrize("case", ["sac-hopper-64", "sac-humanoid-64"])
def test_strided_views_on_another_stream_give_the_same_bits(case):
    ring = ring_u(CASES[case][0], False)
    _, (A, V), _, B, _ = build(case, 2, ring, prio=(1.0, 1e-6))
    rng = np.random.default_rng(9)
    idx = rng.integers(0, ring["length"], B)
    w = rng.uniform(0.1, 1.0, B).astype(np.float32)
    keep = [stage_n(A, idx, w, 5)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wide_i = torch.full((B, 3), 5, dtype=torch.int64, device=DEV)
        wide_w = torch.full((B, 5), 0.5, device=DEV)
        wide_i[:, 1] = torch.as_tensor(idx, device=DEV)
        wide_w[:, 2] = torch.as_tensor(w, device=DEV)
        keep.append(stage_n(V, wide_i[:, 1], wide_w[:, 2], 5))         # SRC_ORDERED against the side stream
    side.synchronize()
    assert_slot_is(read_slot(V), read_slot(A), case)
    assert same_bits(V.debug_read("prio_weights"), A.debug_read("prio_weights"))
    del keep


# ------------------------------------------------------------------------------------------ 9. loop.train
@pytest.mark.parametrize("prioritized", [None, dict(alpha=0.6, beta=0.4, eps=1e-6)], ids=["plain", "prioritized"])
def test_train_runs_with_n_step_returns(prioritized):
    from types import SimpleNamespace
    o, a, bound = 11, 3, 1.0
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": 4, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 1200, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 4096})
    env = loop.SyntheticVecEnv(o, a, 4, horizon=7, term_at=2.5, bound=bound)
    env.action_space.seed(0)
    torch.manual_seed(0)
    agent = P.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32),
                    torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
    metrics = loop.train(cfg, env, agent, fused=False, prioritized=prioritized, n_step=3)
    assert all(np.isfinite(v) for v in metrics.values()), metrics
    st = track(agent.engine).nstep_stats()
    assert st["stagings"] == agent.qnet_updates_so_far > 100 and st["rows_staged"] == 64 * st["stagings"]
    assert st["rows_cut_short"] > 0 and st["rows_refused"] == 0
