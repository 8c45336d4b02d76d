"""GPU: the device boundary outwards (sactd3_read_batch_device / sactd3_rb_read_rows_device, include/sactd3.h) against the host
read-back it stands beside.  Everything here is an equality at small shapes: what a read-out leaves in the caller's device arrays is,
bit for bit, what sactd3_read_batch returns for the same slot or the same ring rows; nothing outside the destinations' windows is
written; a read-out is invisible to training; and the counters follow from the calls, not from timing."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests.gpu_support import (DEV, PACK_SHAPES, P, _lib, assert_same_state, close_engines, fields_of, make_pair, new_engine,  # noqa: F401
                               rows, stream, track)
from tests.helpers import DIMS

pytestmark = pytest.mark.gpu

KEYS = ("observations", "actions", "rewards", "next_observations", "dones", "index")
B, CAP = 64, 1000


def engine(env, td3=False, cap=CAP, seed=0):
    """an engine with the reference's initial parameters (so that it can step), batch_size 64"""
    o, a, bound = DIMS[env]
    eng = new_engine((Hps.td3 if td3 else Hps.sac)(batch_size=B), DIMS[env], rb_capacity=cap, max_envs=8, seed=seed)
    torch.manual_seed(seed)
    actor, critics = P.schema.reference_initial_params(o, a, td3, True)
    for which, flat in ((_lib.ACTOR, actor), (_lib.ACTOR_TARGET, actor), (_lib.CRITICS, critics), (_lib.CRITICS_TARGET, critics)):
        eng.set_params(which, flat)
    return eng, (o, a, bound)


def fill(eng, dims, n, seed=0):
    """n transitions into the ring through rb_extend, in pushes of at most 300 rows (every 7th flag done)"""
    o, a, bound = dims
    first = 0
    while first < n:
        k = min(300, n - first)
        eng.rb_extend(*[t.numpy() for t in rows(k, o, a, bound, seed=seed + first, first=first)])
        first += k


def outs(n, o, a, fill_value=None):
    """six contiguous destination tensors in the shapes read_batch() uses: rewards / dones / index flat"""
    mk = torch.empty if fill_value is None else (lambda *s, **k: torch.full(s, fill_value, **k))
    t = {"observations": mk(n, o, device=DEV), "actions": mk(n, a, device=DEV), "rewards": mk(n, device=DEV), "next_observations": mk(n, o, device=DEV),
         "dones": torch.zeros(n, dtype=torch.bool, device=DEV), "index": torch.full((n,), -7, dtype=torch.int64, device=DEV)}
    return t


def fields(ts, drop=()):
    """[(address, row stride in elements)] in the order of sactd3_device_fields_out; a dropped key is a NULL destination"""
    return [(0, 0) if k in drop else (ts[k].data_ptr(), ts[k].stride(0) if ts[k].shape[0] > 1 else (ts[k].shape[1] if ts[k].dim() == 2 else 1)) for k in KEYS]


def host(ts):
    return {k: ts[k].cpu().numpy() for k in KEYS}


def assert_equals_host(got, want, what):
    for k in KEYS:
        g, w = got[k].reshape(want[k].shape), want[k]
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k)
        if g.dtype == np.float32:                                # bit for bit: -0.0 and NaN payloads included
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, k, "bits")


def batch_out(eng, dims):
    ts = outs(B, dims[0], dims[1])
    eng.read_batch_device(fields(ts), stream())
    return host(ts)


def ring_rows(eng):
    """every ring row through the host path: rb_sample_with_indices + read_batch, 64 rows at a time"""
    n, parts = eng.rb_len(), []
    for lo in range(0, n, B):
        eng.rb_sample_with_indices(np.minimum(np.arange(lo, lo + B), n - 1))
        got = eng.read_batch()
        parts.append({k: got[k][:min(B, n - lo)] for k in KEYS})
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def rows_out(eng, dims, idx):
    """idx: an int64 CUDA tensor or view, 1-D"""
    n = idx.shape[0]
    ts = outs(n, dims[0], dims[1])
    eng.rb_read_rows_device(idx.data_ptr(), idx.stride(0) if n > 1 else 1, n, fields(ts), stream())
    return host(ts)


# ------------------------------------------------------------------------------------------ 1. the batch slot
@pytest.mark.parametrize("env", PACK_SHAPES)
def test_batch_readout_equals_read_batch(env):
    eng, dims = engine(env)
    o, a, bound = dims
    fill(eng, dims, 700)
    eng.rb_sample()
    assert_equals_host(batch_out(eng, dims), eng.read_batch(), "rb_sample")
    idx = (np.arange(B) * 37 + 5) % 700
    eng.rb_sample_with_indices(idx)
    got = batch_out(eng, dims)
    assert_equals_host(got, eng.read_batch(), "rb_sample_with_indices")
    assert np.array_equal(got["index"], idx)
    eng.load_batch(*[t.numpy() for t in rows(B, o, a, bound, seed=91)])
    got = batch_out(eng, dims)
    assert_equals_host(got, eng.read_batch(), "load_batch")
    assert np.array_equal(got["index"], np.arange(B))
    eng.step(True)
    assert_equals_host(batch_out(eng, dims), eng.read_batch(), "step(1)")
    s = eng.readout_stats()
    assert (s["batch_readouts"], s["row_readouts"], s["rows_requested"], s["rows_refused"]) == (4, 0, 0, 0)


@pytest.mark.parametrize("td3,env", [(False, "hopper"), (True, "td3_2")])
def test_batch_readout_after_a_period_reads_the_last_slot(td3, env):
    eng, dims = engine(env, td3=td3)
    assert eng.cfg.actor_update_delay == 2
    fill(eng, dims, 700)
    for _ in range(2):                                           # the second period starts from the chained opening pair (SAC)
        eng.step_period()
        got, want = batch_out(eng, dims), eng.read_batch()
        assert_equals_host(got, want, "step_period")
        assert_equals_host(batch_out(eng, dims), want, "step_period, again")


# ------------------------------------------------------------------------------------------ 2. strided, unaligned destinations
def slabs(n, o, a):
    """destinations as column slices of wider slabs pre-filled with sentinels: float rows that start at odd element offsets (row
    stride 2o + a + 6), flags in column 1 of an [n, 3] bool tensor, the index in column 1 of an [n, 2] int64 tensor"""
    wide = torch.full((n, 2 * o + a + 6), 7.0, device=DEV)
    fl8 = torch.full((n, 3), 7, dtype=torch.uint8, device=DEV)
    ix = torch.full((n, 2), -7, dtype=torch.int64, device=DEV)
    cols = {"observations": (1, 1 + o), "actions": (2 + o, 2 + o + a), "next_observations": (3 + o + a, 3 + 2 * o + a), "rewards": (4 + 2 * o + a, 5 + 2 * o + a)}
    ts = {k: wide[:, lo:hi] for k, (lo, hi) in cols.items()}
    ts["dones"], ts["index"] = fl8.view(torch.bool)[:, 1:2], ix[:, 1:2]
    return ts, wide, fl8, ix, cols


def check_slabs(made, want, drop, what):
    ts, wide, fl8, ix, cols = made
    wide, fl8, ix = wide.cpu().numpy(), fl8.cpu().numpy(), ix.cpu().numpy()
    outside = np.ones(wide.shape, bool)
    for k, (lo, hi) in cols.items():
        if k in drop:
            continue
        outside[:, lo:hi] = False
        w = want[k].reshape(wide.shape[0], -1)
        assert np.array_equal(wide[:, lo:hi].view(np.uint32), w.view(np.uint32)), (what, k)
    assert np.all(wide[outside] == 7.0), (what, "a float outside the windows was written")
    if "dones" in drop:
        assert np.all(fl8 == 7), (what, "dones is NULL but its slab was written")
    else:
        assert np.array_equal(fl8[:, 1], want["dones"].astype(np.uint8)) and np.all(fl8[:, [0, 2]] == 7), (what, "dones")      # bytes 0 / 1
    if "index" in drop:
        assert np.all(ix == -7), (what, "index is NULL but its slab was written")
    else:
        assert np.array_equal(ix[:, 1], want["index"]) and np.all(ix[:, 0] == -7), (what, "index")


@pytest.mark.parametrize("env", PACK_SHAPES)
def test_strided_unaligned_destinations_and_nothing_else_written(env):
    eng, dims = engine(env)
    o, a, _ = dims
    fill(eng, dims, 700)
    ring = ring_rows(eng)
    eng.rb_sample()
    want = eng.read_batch()
    req = (np.arange(150) * 13 + 3) % 700
    idx, want_rows = torch.as_tensor(req, device=DEV), {k: ring[k][req] for k in KEYS}
    for drop in ((), ("actions", "dones", "index"), ("observations", "rewards", "next_observations"), tuple(KEYS[1:])):
        made = slabs(B, o, a)
        assert made[0]["observations"].data_ptr() % 16 == 4      # rows start at odd element offsets
        eng.read_batch_device(fields(made[0], drop), stream())
        check_slabs(made, want, drop, ("batch", drop))
        made = slabs(150, o, a)
        eng.rb_read_rows_device(idx.data_ptr(), 1, 150, fields(made[0], drop), stream())
        check_slabs(made, want_rows, drop, ("rows", drop))


# ------------------------------------------------------------------------------------------ 3. ring rows
@pytest.mark.parametrize("env", PACK_SHAPES)
def test_ring_rows_equal_the_host_read_back(env):
    eng, dims = engine(env)
    fill(eng, dims, 1300)                                        # 1300 rows into 1000: the ring has wrapped
    assert eng.rb_len() == CAP
    ring = ring_rows(eng)
    assert np.array_equal(ring["index"], np.arange(CAP))
    g = torch.Generator().manual_seed(5)
    calls = 0
    for n in (1, 5, 64, 300, 1000):
        dup = torch.randint(0, max(CAP // 4, 1), (n,), generator=g)          # (drawn from 250 slots: duplicates from n = 64 on for certain)
        desc = torch.arange(CAP - 1, CAP - 1 - n, -1)
        wide = torch.randint(0, CAP, (3 * n,), generator=g).to(DEV)
        for name, idx in (("duplicates", dup.to(DEV)), ("descending", desc.to(DEV)), ("strided", wide[::3])):
            if name == "duplicates" and n >= 64:
                assert len(set(idx.tolist())) < n
            if name == "strided" and n > 1:
                assert idx.stride(0) == 3
            got, req = rows_out(eng, dims, idx), idx.cpu().numpy()
            assert np.array_equal(got["index"], req), (n, name, "index")
            assert_equals_host(got, {k: ring[k][req] for k in KEYS}, (n, name))
            calls += 1
    s = eng.readout_stats()
    assert (s["row_readouts"], s["rows_requested"], s["rows_refused"]) == (calls, 3 * (1 + 5 + 64 + 300 + 1000), 0)


# ------------------------------------------------------------------------------------------ 4. indices outside the ring
def test_out_of_range_indices_read_zero_rows_and_are_counted():
    eng, dims = engine("hopper")
    o, a, _ = dims
    fill(eng, dims, 500)                                         # half full: len 500 < capacity 1000
    ring = ring_rows(eng)
    small = [-1, 3, 500, 2 ** 40, 499, 0, -2 ** 40, 1000, 17, 999, 2 ** 31, 2 ** 32 + 5, -2 ** 31]
    big = [(-1 - k, 500 + k, 2 ** 40 + k)[(k // 3) % 3] if k % 3 == 0 else (k * 17) % 500 for k in range(400)]      # every third one is bad
    refused = 0
    for req in (small, big):
        req = np.asarray(req, np.int64)
        bad = (req < 0) | (req >= 500)                            # a count of the inputs
        assert bad.any() and (~bad).any()
        got = rows_out(eng, dims, torch.as_tensor(req, device=DEV))      # returns 0: no exception
        assert np.array_equal(got["index"], req)                 # echoed as given
        for k in KEYS[:-1]:
            assert np.array_equal(got[k][~bad], ring[k][req[~bad]]), k
            assert not got[k][bad].any(), (k, "a refused row is all-zero, flag False")
        for k in ("observations", "actions", "rewards", "next_observations"):
            assert np.array_equal(got[k][bad].view(np.uint32), np.zeros_like(got[k][bad]).view(np.uint32)), (k, "+0.0")
        refused += int(bad.sum())
        assert eng.readout_stats()["rows_refused"] == refused
    eng.step(True)                                               # the engine goes on
    eng.sync()
    assert eng.readout_stats()["rows_refused"] == refused and eng.rb_len() == 500


# ------------------------------------------------------------------------------------------ 5. a sampler of the caller's own
@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "td3_2")])
def test_external_sampler_round_trip_trains_like_the_engines_own_gather(algo, env):
    _, D, dims = make_pair(algo, env, B, rb_capacity=CAP)
    _, H, _ = make_pair(algo, env, B, rb_capacity=CAP)
    for e in (D, H):
        fill(e, dims, 700)
    rb = P.ReplayBuffer(CAP)
    rb._bind(D)
    for rnd in range(2):
        idx = (np.arange(B) * 29 + 11 * rnd) % 700
        td = rb.rows(torch.as_tensor(idx, device=DEV))
        assert all(td[k].is_cuda for k in KEYS) and np.array_equal(td["index"].cpu().numpy(), idx)
        got = fields_of(D, (td["observations"], td["actions"], td["rewards"], td["next_observations"], td["dones"]))
        D.load_batch_device(got[0], got[1], stream())
        H.rb_sample_with_indices(idx)
        for e in (D, H):
            e.update_qnets()
            e.update_actor()
            e.update_actor()
            e.update_targ_nets(rnd + 1)
        assert_same_state(D, H)


# ------------------------------------------------------------------------------------------ 6. read-outs are invisible to training
@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "td3_2")])
def test_readouts_between_chained_periods_change_nothing(algo, env):
    res = []
    for reads in (True, False):
        _, eng, dims = make_pair(algo, env, B, rb_capacity=CAP, seed=3)
        o, a, bound = dims
        fill(eng, dims, 600)
        idx = torch.as_tensor((np.arange(200) * 7) % 600, device=DEV)
        it, samples = 0, []

        def read():
            if reads:
                batch_out(eng, dims)
                rows_out(eng, dims, idx)
        for k in range(3):                                       # rb_extend every period
            eng.rb_extend(*[t.numpy() for t in rows(8, o, a, bound, seed=70 + k, first=600 + 8 * k)])
            read()
            it = eng.run_iterations(it, 3)
            read()
            samples.append(eng.read_batch()["index"])
        it = eng.run_iterations(it, 3)                           # ... and two periods with nothing but read-outs in between: the second
        read()                                                   # starts from the opening pair the first precomputed, if the chain holds
        it = eng.run_iterations(it, 3)
        samples.append(eng.read_batch()["index"])
        res.append((eng, samples, [eng.graph_kernel_count(w) for w in range(8)]))
    (R, sr, gr), (N, sn, gn) = res
    assert_same_state(R, N)
    assert all(np.array_equal(x, y) for x, y in zip(sr, sn)) and len(sr) == 4
    assert gr == gn and sum(gr) > 0                              # the same graphs were instantiated: no chain break, no counter consumed
    assert R.readout_stats()["batch_readouts"] == 7 and N.readout_stats()["batch_readouts"] == 0
    assert R.boundary_stats()["ordered_calls"] == 14 and N.boundary_stats()["ordered_calls"] == 0


# ------------------------------------------------------------------------------------------ 7. stream order, both directions
def test_readouts_are_ordered_against_the_consumer_stream():
    """The destinations are overwritten on a side stream behind a long matmul, handed over under that stream and read on it right after
    the call, with no host synchronisation: the engine must write after the overwrite, and the side stream must read after the write.
    (A missing wait reads the overwrite's values; nothing faults.)"""
    eng, dims = engine("hopper")
    o, a, _ = dims
    fill(eng, dims, 700)
    rb = P.ReplayBuffer(CAP)
    rb._bind(eng)
    big = torch.randn(4096, 4096, device=DEV)
    ts = outs(B, o, a)
    ts["rewards"], ts["dones"] = ts["rewards"].reshape(B, 1), ts["dones"].reshape(B, 1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    before = eng.boundary_stats()["ordered_calls"]
    kept = []
    for rep in range(50):
        batch = rb.sample(B)
        with torch.cuda.stream(side):
            big = (big @ big) * 1e-2                              # a large kernel queued on the side stream in front
            for k in KEYS:
                ts[k].fill_(True if ts[k].dtype == torch.bool else 5)
            got = batch.on_device(out=ts)
            assert all(got[k] is ts[k] for k in KEYS)
            kept.append({k: got[k].clone() for k in KEYS})       # read on the side stream at once
        assert eng.boundary_stats()["ordered_calls"] == before + rep + 1
        want = eng.read_batch()
        assert_equals_host({k: kept[-1][k].cpu().numpy() for k in KEYS}, want, rep)


# ------------------------------------------------------------------------------------------ 8. errors
def test_bad_arguments_are_refused_and_leave_the_engine_usable():
    eng, dims = engine("hopper")
    o, a, _ = dims
    names = ("obs", "actions", "rewards", "next_obs", "dones", "index")
    ts = outs(B, o, a)
    good = fields(ts)
    idx = torch.arange(B, device=DEV)
    pinned = {k: torch.zeros(B, max(o, a), dtype=ts[k].dtype).pin_memory() for k in KEYS}
    plain = np.zeros((B, max(o, a)), np.float64)
    # an empty ring: ESTATE for the rows call, whatever else is right
    with pytest.raises(P.EngineError, match=r"error -3.*empty"):
        eng.rb_read_rows_device(idx.data_ptr(), 1, B, good, stream())
    fill(eng, dims, 300)
    calls = (("read_batch_device", lambda f, **k: eng.read_batch_device(f, stream(), **k)),
             ("rb_read_rows_device", lambda f, **k: eng.rb_read_rows_device(idx.data_ptr(), 1, B, f, stream(), **k)))
    for what, call in calls:
        for j, name in enumerate(names):
            width = (o, a, 1, o, 1, 1)[j]
            for bad, text in (((pinned[KEYS[j]].data_ptr(), good[j][1]), "`%s` is not device memory" % name), ((plain.ctypes.data, good[j][1]), "`%s` is not device memory" % name),
                              ((good[j][0], width - 1), "stride of `%s`" % name)):
                with pytest.raises(P.EngineError, match=r"error -1.*" + what + ".*" + text):
                    call([f if i != j else bad for i, f in enumerate(good)])
        with pytest.raises(P.EngineError, match=r"error -1.*" + what + ".*all six destinations"):
            call([(0, 0)] * 6)
    if torch.cuda.device_count() >= 2:                           # another device's tensor
        there = torch.zeros(B, o, device="cuda:1")
        for what, call in calls:
            with pytest.raises(P.EngineError, match=r"error -1.*`obs` is not device memory of the engine's device"):
                call([(there.data_ptr(), o)] + good[1:])
        with pytest.raises(P.EngineError, match=r"error -1.*`idx` is not device memory of the engine's device"):
            eng.rb_read_rows_device(torch.arange(B, device="cuda:1").data_ptr(), 1, B, good, stream())
    for n in (0, -1):
        with pytest.raises(P.EngineError, match=r"error -1.*n >= 1"):
            eng.rb_read_rows_device(idx.data_ptr(), 1, n, good, stream())
    host_idx = np.arange(B, dtype=np.int64)
    with pytest.raises(P.EngineError, match=r"error -1.*`idx` is not device memory"):
        eng.rb_read_rows_device(host_idx.ctypes.data, 1, B, good, stream())
    with pytest.raises(P.EngineError, match=r"error -1.*`idx`"):
        eng.rb_read_rows_device(idx.data_ptr(), 0, B, good, stream())
    lib, f = eng.lib, eng._fields_out(good)
    for flags in (2, 3, -2):                                     # an unknown flag
        assert lib.sactd3_read_batch_device(eng._h, f, None, flags) == _lib.EINVAL
        assert b"read_batch_device: unknown flag" in lib.sactd3_last_error(eng._h)
        assert lib.sactd3_rb_read_rows_device(eng._h, C.c_void_p(idx.data_ptr()), 1, B, f, None, flags) == _lib.EINVAL
        assert b"rb_read_rows_device: unknown flag" in lib.sactd3_last_error(eng._h)
    assert lib.sactd3_read_batch_device(eng._h, None, None, 0) == _lib.EINVAL
    assert lib.sactd3_rb_read_rows_device(eng._h, None, 1, B, f, None, 0) == _lib.EINVAL
    assert lib.sactd3_readout_stats(eng._h, None) == _lib.EINVAL
    s = eng.readout_stats()
    assert (s["batch_readouts"], s["row_readouts"], s["rows_requested"], s["rows_refused"]) == (0, 0, 0, 0)
    assert eng.boundary_stats()["ordered_calls"] == 0
    # ... and the engine is as usable as before
    eng.step(True)
    assert_equals_host(batch_out(eng, dims), eng.read_batch(), "after the errors")
    ring = ring_rows(eng)
    got = rows_out(eng, dims, idx)
    assert_equals_host(got, {k: ring[k][:B] for k in KEYS}, "rows after the errors")
    torch.cuda.synchronize()
    eng.read_batch_device(good, 0, ordered=False)               # without the flag nothing is inserted
    eng.sync()
    assert eng.boundary_stats()["ordered_calls"] == 2


# ------------------------------------------------------------------------------------------ 9. the mirror
def test_mirror_hands_out_device_batches_like_the_reference():
    o, a, n = 11, 3, 4
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=B).__dict__, "seed": 0, "num_envs": n, "rb_capacity": 500})
    torch.manual_seed(0)
    ag = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                 torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity, device_batches=True))
    eng = track(ag.engine)
    fill(eng, (o, a, 1.0), 200)
    first = ag.rb.sample(B)                                      # never looked at
    batch = ag.rb.sample(B)
    obs = batch["observations"]
    assert obs.is_cuda and obs.dtype == torch.float32 and tuple(obs.shape) == (B, o)
    assert batch["dones"].dtype == torch.bool and tuple(batch["dones"].shape) == (B, 1) and batch["terminations"] is batch["dones"]
    assert tuple(batch["rewards"].shape) == (B, 1) and tuple(batch["actions"].shape) == (B, a) and tuple(batch["next_observations"].shape) == (B, o)
    assert batch["index"].dtype == torch.int64 and tuple(batch["index"].shape) == (B,)
    assert batch["observations"] is obs and eng.readout_stats()["batch_readouts"] == 1      # one launch filled every key; cached
    want = P.BatchHandle(eng, eng.batch_generation())            # a default handle on the same slot: numpy through read_batch
    for k in KEYS + ("terminations",):
        assert isinstance(want[k], np.ndarray) and np.array_equal(batch[k].cpu().numpy(), want[k]), k
    with pytest.raises(P.StaleBatchError):
        first["observations"]
    with pytest.raises(P.StaleBatchError):
        first.on_device()
    stats = eng.boundary_stats()["device_batches"]
    ag.update_qnets(batch)                                       # already in the slot: no restage
    ag.update_actor(batch)
    assert eng.boundary_stats()["device_batches"] == stats == 0
    td = ag.rb.rows(batch["index"])                              # the same rows through the ring
    for k in KEYS:
        assert torch.equal(td[k], batch[k]), k
    td2 = ag.rb.rows([5, 1, 5])                                  # anything torch can turn into an index
    assert tuple(td2["observations"].shape) == (3, o) and td2["index"].tolist() == [5, 1, 5]
    later = ag.rb.sample(B)
    assert np.array_equal(batch["rewards"].cpu().numpy(), want["rewards"])      # cached keys outlive the slot
    with pytest.raises(P.StaleBatchError):
        ag.update_qnets(batch)
    ag.update_qnets(later)


# ------------------------------------------------------------------------------------------ 10. timing names
@pytest.mark.parametrize("env", ["hopper", "humanoid"])
def test_time_kernel_knows_the_readout_kernels(env):
    eng, dims = engine(env)
    fill(eng, dims, 300)
    eng.rb_sample()
    for name in ("batch_to_fields", "rows_to_fields"):
        us = eng.time_kernel(name, 20)
        assert np.isfinite(us) and us > 0.0, (name, us)
    assert eng.readout_stats()["rows_refused"] == 0
    eng.step(True)
    eng.sync()


# ------------------------------------------------------------------------------------------ 11. the name tables cannot drift
STATE_REFUSALS = r"error -3.*(priorities are not enabled|no row is pinned|rows are pinned)"


def test_every_timing_and_debug_name_is_served_on_some_engine():
    """Every name sactd3_time_kernel lists in its own refusal, and every word of sactd3_debug_names(), is served by at least one of two
    tiny engines whose states exclude each other (priorities enabled / rows pinned with a mixed draw); the other engine serves it too
    or refuses it for its STATE -- never as an unknown name.  (Besides the two refusals a name can meet for a state it lacks,
    "priorities are not enabled" and "no row is pinned", the pinned engine has a third: "batch_from_index_nstep" stages chains, which
    a pinned ring refuses with "rows are pinned".)"""
    o, a, bound = DIMS["hopper"]

    def tiny(prepare):
        cfg = P.Config(ob_dim=o, ac_dim=a, batch_size=32, rb_capacity=256, max_envs=4, seed=0)
        eng = track(P.Engine(cfg, [-bound] * a, [bound] * a))
        torch.manual_seed(0)
        actor, critics = P.schema.reference_initial_params(o, a, False, True)
        for which, flat in ((_lib.ACTOR, actor), (_lib.ACTOR_TARGET, actor), (_lib.CRITICS, critics), (_lib.CRITICS_TARGET, critics)):
            eng.set_params(which, flat)
        eng.rb_fill_synthetic(64, seed=0)
        prepare(eng)
        eng.step(True)                                            # q, y and the slot exist
        eng.policy(np.zeros((4, o), np.float32))                  # ... and pi_z2
        return eng

    def pin_and_mix(eng):
        eng.rb_pin(16)
        eng.rb_set_mix(8)

    engines = [tiny(lambda eng: eng.prio_enable()), tiny(pin_and_mix)]
    with pytest.raises(P.EngineError, match=r"error -1.*time_kernel: unknown kernel \(") as refusal:
        engines[0].time_kernel("no_such_kernel", 1)
    kernels = str(refusal.value).split("(")[-1].split(")")[0].split(" | ")
    assert len(kernels) >= 18 and "gather" in kernels and "pi_head" in kernels, kernels

    def served(call, names, unknown):
        for name in names:
            ok = 0
            for eng in engines:
                try:
                    ok += bool(call(eng, name))
                except P.EngineError as err:
                    assert unknown not in str(err), (name, str(err))
                    assert re.search(STATE_REFUSALS, str(err)), (name, str(err))
            assert ok >= 1, name

    served(lambda eng, name: eng.time_kernel(name, 2) > 0.0, kernels, "unknown kernel")
    words = engines[0].lib.sactd3_debug_names().decode().split()
    assert len(words) >= 38 and len(set(words)) == len(words), words
    served(lambda eng, name: eng.debug_read(name).size > 0, words, "unknown buffer name")
    for eng in engines:
        eng.sync()
