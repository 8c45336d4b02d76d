"""GPU: the device boundary (sactd3_rb_extend_fields_device / sactd3_load_batch_device, include/sactd3.h) against the host
entry points it stands beside.  Everything here is an equality: a ring or a batch slot filled from five device arrays holds, bit
for bit, what the host route leaves there from the same values, and an update computed from it is the same update.  The counters
(sactd3_boundary_stats) follow from the schedule of the calls, not from timing."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests.gpu_support import (DEV, PACK_SHAPES, P, _lib, agent_mod, assert_same_state, close_engines, cuda, extend_device, load_device,  # noqa: F401
                               make_pair, rows, track)
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu


def raw_fields(five):
    """contiguous CUDA tensors -> [(address, row stride in elements)]"""
    return [(t.data_ptr(), t.shape[1] if t.dim() == 2 else 1) for t in five]


def strided(five):
    """the same values as column slices of wider CUDA tensors: row strides above the widths, rows that start at odd offsets,
    [n, 1] rewards and torch.bool flags"""
    obs, act, rew, nobs, done = five
    n, o, a = obs.shape[0], obs.shape[1], act.shape[1]
    wide = torch.full((n, 2 * o + a + 6), 7.0, device=DEV)
    wide[:, 1:1 + o], wide[:, 2 + o:2 + o + a], wide[:, 3 + o + a:3 + 2 * o + a], wide[:, 4 + 2 * o + a] = obs.to(DEV), act.to(DEV), nobs.to(DEV), rew.to(DEV)
    flags = torch.ones((n, 3), dtype=torch.bool, device=DEV)
    flags[:, 1] = done.to(DEV)
    return wide[:, 1:1 + o], wide[:, 2 + o:2 + o + a], wide[:, 4 + 2 * o + a:5 + 2 * o + a], wide[:, 3 + o + a:3 + 2 * o + a], flags[:, 1:2]


def assert_same_ring(A, B):
    assert A.rb_len() == B.rb_len()
    n, bs = A.rb_len(), A.cfg.batch_size
    for lo in range(0, n, bs):                                   # index sets that cover every row
        idx = np.minimum(np.arange(lo, lo + bs), n - 1)
        A.rb_sample_with_indices(idx)
        B.rb_sample_with_indices(idx)
        x, y = A.read_batch(), B.read_batch()
        for k in x:
            assert np.array_equal(x[k], y[k]), ("ring rows from", lo, k)


# ------------------------------------------------------------------------------------------ 1. the ring
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("env", PACK_SHAPES)
def test_ring_from_device_fields_equals_ring_from_host_arrays(env, layout):
    o, a, bound = DIMS[env]
    H, D = [track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=64, rb_capacity=1000, max_envs=8), [-bound] * a, [bound] * a))
            for _ in range(2)]
    first = 0
    for k, n in enumerate((1, 4, 4, 8, 300, 683, 300)):          # 1300 rows into 1000: one wrap, inside the 300-row push
        five = rows(n, o, a, bound, seed=k, first=first)
        first += n
        H.rb_extend(*[t.numpy() for t in five])
        extend_device(D, strided(five) if layout == "strided" else cuda(five))
        assert H.rb_len() == D.rb_len() == min(first, 1000)
    assert_same_ring(H, D)
    s = D.boundary_stats()
    assert (s["device_extends"], s["device_rows"], s["device_batches"], s["ordered_calls"]) == (7, 1300, 0, 7)
    assert list(H.boundary_stats().values()) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 2. the batch slot
@pytest.mark.parametrize("algo,env,B", [("sac", "hopper", 64), ("sac", "sac4", 300), ("sac", "humanoid", 128), ("td3", "halfcheetah", 64)])
def test_batch_slot_from_device_fields_equals_load_batch(algo, env, B):
    _, H, (o, a, bound) = make_pair(algo, env, B)
    _, D, _ = make_pair(algo, env, B)
    for rnd in range(2):       # twice in a row on the same engines: in the second round the action columns of Xn hold the first round's a'
        five = rows(B, o, a, bound, seed=20 + rnd)
        H.load_batch(*[t.numpy() for t in five])
        load_device(D, strided(five) if rnd else cuda(five))
        x, y = H.read_batch(), D.read_batch()
        for k in x:
            assert np.array_equal(x[k], y[k]), ("slot", rnd, k)
        assert np.array_equal(y["index"], np.arange(B))
        for name in ("X", "Xn", "rew", "done"):                  # the whole buffers, pads and the columns the fields do not own included
            assert np.array_equal(H.debug_read(name).view(np.uint32), D.debug_read(name).view(np.uint32)), ("buffer", rnd, name)
        for e in (H, D):
            e.update_qnets()
            e.update_actor()
            e.update_actor()
            e.update_targ_nets(rnd + 1)
        assert_same_state(H, D)
    assert D.boundary_stats()["device_batches"] == 2 and H.boundary_stats()["device_batches"] == 0


# ------------------------------------------------------------------------------------------ 3. the mirror, as the reference's loop drives it
def mirror_run(device_inputs, as_numpy=False):
    """12 iterations of orchestrator.py:317-352 on Agent + ReplayBuffer: rb.extend with a dict of CUDA tensors (:100-113), update_qnets /
    update_actor with a dict of CUDA tensors (:338-348), update_targ_nets.  `slot_refills` on the agent returned: how far the run moved
    the engine's batch generation."""
    o, a, n, B = 11, 3, 4, 64
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=B).__dict__, "seed": 0, "num_envs": n, "rb_capacity": 500})
    torch.manual_seed(0)
    ag = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                 torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
    track(ag.engine).device_inputs = device_inputs
    put = (lambda t: t.numpy()) if as_numpy else (lambda t: t.to(DEV))
    before = ag.engine.batch_generation()

    def td(five):
        obs, act, rew, nobs, done = five
        return {"observations": put(obs), "next_observations": put(nobs), "actions": put(act), "rewards": put(rew.reshape(-1, 1)),
                "terminations": put(done.reshape(-1, 1)), "dones": put(done.reshape(-1, 1))}
    for i in range(12):
        ag.rb.extend(td(rows(n, o, a, 1.0, seed=100 + i, first=n * i)))
        ag.timesteps_so_far += n
        batch = td(rows(B, o, a, 1.0, seed=200 + i))
        ag.update_qnets(batch)
        ag.qnet_updates_so_far += 1
        if i % (cfg.actor_update_delay + 1) == 0:
            for _ in range(cfg.actor_update_delay):
                ag.update_actor(batch)
                ag.actor_updates_so_far += 1
        ag.update_targ_nets()
    ag.slot_refills = ag.engine.batch_generation() - before
    return ag


def test_mirror_keeps_device_tensors_on_the_device():
    D, H, N = mirror_run(True), mirror_run(False), mirror_run(True, as_numpy=True)
    s = D.engine.boundary_stats()
    assert (s["device_extends"], s["device_rows"], s["device_batches"], s["ordered_calls"]) == (12, 48, 20, 32)
    assert list(H.engine.boundary_stats().values()) == [0, 0, 0, 0]
    assert list(N.engine.boundary_stats().values()) == [0, 0, 0, 0]      # numpy never takes the device route
    assert D.slot_refills == H.slot_refills == N.slot_refills == 12 + 8      # (StaleBatchError behaviour: a generation per staged caller-owned batch, on every route)
    for other in (H, N):
        assert_same_state(D.engine, other.engine)
        assert len(D.rb) == len(other.rb) == 48
        idx = np.arange(64) % 48
        for eng in (D.engine, other.engine):
            gen = eng.batch_generation()
            eng.rb_sample_with_indices(idx)
            assert eng.batch_generation() == gen + 1                    # a direct refill counts, exactly once
        x, y = D.engine.read_batch(), other.engine.read_batch()
        for k in x:
            assert np.array_equal(x[k], y[k]), ("ring", k)


# ------------------------------------------------------------------------------------------ 4. stream order, both directions
def test_reads_are_ordered_against_the_producer_stream():
    """The sources are WRITTEN on a side stream behind a long matmul, handed over under that stream, and zeroed on it right after the
    call: the engine must read after the write and before the zeroing.  (A missing wait reads stale or zeroed values; nothing faults.)"""
    o, a, bound = DIMS["hopper"]
    B = 64
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=256, max_envs=8), [-bound] * a, [bound] * a))
    want = rows(B, o, a, bound, seed=3)
    real = cuda(want)
    src = tuple(torch.full_like(t, True if t.dtype == torch.bool else 5.0) for t in real)
    big = torch.randn(6144, 6144, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for what in ("batch", "extend"):
        with torch.cuda.stream(side):
            for _ in range(4):
                big = (big @ big) * 1e-2                          # tens of milliseconds queued in front of the write
            for s_, r_ in zip(src, real):
                s_.copy_(r_)
            (load_device if what == "batch" else extend_device)(eng, src)
            for s_ in src:
                s_.zero_()
        if what == "extend":
            eng.rb_sample_with_indices(np.arange(B))
        got = eng.read_batch()
        for k, t in zip(("observations", "actions", "rewards", "next_observations", "dones"), want):
            assert np.array_equal(got[k], t.numpy()), (what, k)
        side.synchronize()
        for s_ in src:
            assert not s_.any(), "the zeroing on the producer stream did not run"
            s_.fill_(True if s_.dtype == torch.bool else 5.0)
        torch.cuda.synchronize()
    assert eng.boundary_stats()["ordered_calls"] == 2


# ------------------------------------------------------------------------------------------ 5. a precomputed opening pair is dropped
def test_device_extend_breaks_the_period_chain():
    _, A, (o, a, bound) = make_pair("sac", "hopper", 64)
    _, Bn, _ = make_pair("sac", "hopper", 64)
    pre, new = synth_transitions(512, o, a, bound, seed=5), rows(4, o, a, bound, seed=6)
    for e in (A, Bn):
        e.rb_extend(*pre)
    A.run_iterations(0, 3)                                       # one period graph: leaves the next period's opening pair precomputed
    extend_device(A, cuda(new))
    A.run_iterations(3, 3)
    for i in range(6):
        if i == 3:
            Bn.rb_extend(*[t.numpy() for t in new])
        Bn.step(i % 3 == 0)
    assert_same_state(A, Bn, "index")
    assert A.rb_len() == Bn.rb_len() == 516


# ------------------------------------------------------------------------------------------ 6. errors
def test_bad_arguments_are_refused_and_leave_the_engine_usable():
    o, a, bound = DIMS["hopper"]
    B = 32
    H, D = [track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=256, max_envs=8), [-bound] * a, [bound] * a))
            for _ in range(2)]
    want = rows(B, o, a, bound, seed=4)
    five = cuda(want)
    good = raw_fields(five)
    pinned = torch.zeros(B, o).pin_memory()
    plain = np.zeros((B, o), np.float32)
    cases = []
    for k in range(5):
        cases.append(([f if j != k else (0, f[1]) for j, f in enumerate(good)], B, "NULL"))
        cases.append(([f if j != k else (f[0], f[1] - 1) for j, f in enumerate(good)], B, "stride"))
    cases.append(([(pinned.data_ptr(), o)] + good[1:], B, "not device memory"))
    cases.append((good[:3] + [(plain.ctypes.data, o)] + good[4:], B, "not device memory"))
    for call in (D.load_batch_device, D.rb_extend_fields_device):
        for fields, n, text in cases:
            with pytest.raises(P.EngineError, match=r"error -1.*" + text):
                call(fields, n)
    for n in (B - 1, B + 1, 0):
        with pytest.raises(P.EngineError, match=r"error -1.*batch_size"):
            D.load_batch_device(good, n)
    with pytest.raises(P.EngineError, match=r"error -1"):
        D.rb_extend_fields_device(good, -1)
    assert list(D.boundary_stats().values()) == [0, 0, 0, 0] and D.rb_len() == 0
    lib, st = D.lib, (C.c_int64 * 4)()
    assert lib.sactd3_rb_extend_fields_device(D._h, None, 4, None, 0) == _lib.EINVAL
    assert lib.sactd3_load_batch_device(D._h, None, B, None, 0) == _lib.EINVAL
    assert lib.sactd3_boundary_stats(D._h, None) == _lib.EINVAL and lib.sactd3_boundary_stats(None, st) == _lib.EINVAL
    # ... and correct calls afterwards work
    D.rb_extend_fields_device(good, 0)                            # n = 0: nothing appended
    assert D.rb_len() == 0
    D.rb_extend_fields_device(good, B)
    H.rb_extend(*[t.numpy() for t in want])
    assert_same_ring(H, D)
    D.load_batch_device(good, B)
    H.load_batch(*[t.numpy() for t in want])
    x, y = H.read_batch(), D.read_batch()
    for k in x:
        assert np.array_equal(x[k], y[k]), k
    s = D.boundary_stats()
    assert (s["device_extends"], s["device_rows"], s["device_batches"]) == (2, B, 1)


def test_a_tensor_of_another_gpu_is_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    o, a, bound = DIMS["hopper"]
    B = 32
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=256, max_envs=8), [-bound] * a, [bound] * a))
    here = cuda(rows(B, o, a, bound, seed=4))
    there = tuple(t.to("cuda:1") for t in here)
    assert agent_mod._device_route(eng, *there) is None and agent_mod._device_route(eng, *(here[:1] + there[1:])) is None
    for call in (eng.load_batch_device, eng.rb_extend_fields_device):
        with pytest.raises(P.EngineError, match=r"error -1.*not device memory of the engine's device"):
            call(raw_fields(here[:2] + there[2:3] + here[3:]), B)
    eng.load_batch_device(raw_fields(here), B)
    assert np.array_equal(eng.read_batch()["observations"], here[0].cpu().numpy())


# ------------------------------------------------------------------------------------------ 7. acting overlap
def test_device_extend_does_not_meet_an_acting_call_in_flight():
    _, A, (o, a, bound) = make_pair("sac", "hopper", 32)
    _, Bn, _ = make_pair("sac", "hopper", 32)
    obs = torch.randn(4, o, generator=torch.Generator().manual_seed(9)).numpy()
    new = cuda(rows(4, o, a, bound, seed=8))
    want = A.predict(obs, True)
    Bn.predict_begin(obs, True)
    s0 = Bn.acting_stats()
    extend_device(Bn, new)
    assert Bn.acting_stats() == s0 and s0["begun"] == 1
    assert np.array_equal(Bn.predict_end(), want)
    assert Bn.rb_len() == 4 and Bn.boundary_stats()["device_extends"] == 1
