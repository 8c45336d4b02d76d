"""GPU: acting on device observations (sactd3_predict_device, include/sactd3.h) against the host call it stands beside.  Everything
here is an equality: the actions, the exploration draws and the learner's state are, bit for bit, what sactd3_predict gives at the
same position in the call sequence; the counters follow from the schedule of the calls, not from timing.

Shapes (max_envs = 96): SAC Hopper (o = 11: one pad column; narrow head, 4 rows per tail block), TD3 HalfCheetah (o = 17: three pad
columns; narrow head), SAC Humanoid (o = 376: no pad; wide head, 16 rows per tail block; 94 chunks per row, so 17 and 67 rows span
several blocks of the pack kernel).  Row counts 1, 4, 5, 16, 17, 67: single-block and multi-block tails of both head forms and a
partial last block."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests.gpu_support import (DEV, MAXN, SENTINEL, SETS, P, _lib, assert_same_state, build_engines, close_engines, loop, stream,  # noqa: F401
                               track)
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu

SHAPES = [("sac", "hopper"), ("td3", "halfcheetah"), ("sac", "humanoid")]
ROWS = (1, 4, 5, 16, 17, 67)


def twins(algo, env, count=2, B=64, use_graphs=True, seed=3):
    """`count` engines with the same seed and the same (perturbed, so that every parameter matters) parameters"""
    _, engs, dims = build_engines(algo, DIMS[env], B, count=count, seed=seed, cap=2048, max_envs=MAXN, use_graphs=use_graphs)
    return engs, dims


def obs_rows(n, o, seed):
    return torch.randn(n, o, generator=torch.Generator().manual_seed(seed))


def device_call(eng, obs, explore, out=None, ordered=True):
    """predict_device on a CUDA tensor `obs` [n, o] (any row stride) -> the actions as a host array"""
    n, a = obs.shape[0], eng.cfg.ac_dim
    out = torch.empty(n, a, device=DEV) if out is None else out
    eng.predict_device(obs.data_ptr(), obs.stride(0), n, explore, out.data_ptr(), out.stride(0), stream(), ordered)
    return out.cpu().numpy()            # (on the current stream, which the call made wait for the engine's)


# ------------------------------------------------------------------------------------------ 1. the same bits as the host call
@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("algo,env", SHAPES)
def test_device_calls_equal_host_calls(algo, env, explore):
    (H, D), (o, a, bound) = twins(algo, env)
    multi = 0
    for n in ROWS:
        for k in range(3):                                           # three in a row: the exploration counter ticks once per call
            obs = obs_rows(n, o, seed=100 * n + k)
            want, got = H.predict(obs.numpy(), explore), device_call(D, obs.to(DEV), explore)
            assert want.shape == got.shape == (n, a) and np.array_equal(want, got), (n, k)
            assert np.isfinite(got).all()
        assert np.array_equal(H.read_noise(_lib.SITE_PREDICT, n), D.read_noise(_lib.SITE_PREDICT, n)), n
        multi += 3 * (n > (16 if env == "humanoid" else 4))
    s = D.predict_device_stats()
    assert (s["calls"], s["rows"], s["ordered_calls"], s["multi_block_tails"]) == (3 * len(ROWS), 3 * sum(ROWS), 3 * len(ROWS), multi)
    assert list(H.predict_device_stats().values()) == [0, 0, 0, 0]
    if explore:                                                      # (the draws are in use: another call, other actions)
        obs = obs_rows(5, o, seed=1)
        assert not np.array_equal(device_call(D, obs.to(DEV), True), device_call(D, obs.to(DEV), True))


@pytest.mark.parametrize("algo,env", SHAPES)
def test_host_and_device_calls_share_one_noise_stream(algo, env):
    """host, device, device, host on one engine = four host calls on its twin"""
    (H, M), (o, a, bound) = twins(algo, env)
    for n in (4, 17):
        for k, on_device in enumerate((False, True, True, False)):
            obs = obs_rows(n, o, seed=7 * n + k)
            want = H.predict(obs.numpy(), True)
            got = device_call(M, obs.to(DEV), True) if on_device else M.predict(obs.numpy(), True)
            assert np.array_equal(want, got), (n, k)
        assert np.array_equal(H.read_noise(_lib.SITE_PREDICT, n), M.read_noise(_lib.SITE_PREDICT, n))


def test_eager_sequence_equals_host_calls():
    (H, D), (o, a, bound) = twins("sac", "hopper", use_graphs=False)
    for n in (4, 17):
        for k in range(3):
            obs = obs_rows(n, o, seed=n + k)
            assert np.array_equal(H.predict(obs.numpy(), True), device_call(D, obs.to(DEV), True)), (n, k)
    assert np.array_equal(H.read_noise(_lib.SITE_PREDICT, 17), D.read_noise(_lib.SITE_PREDICT, 17))


# ------------------------------------------------------------------------------------------ 2. views
@pytest.mark.parametrize("algo,env", SHAPES)
def test_views_in_and_out(algo, env):
    """obs = big[:, 1:1+o] (rows 4-byte aligned only, stride above the width), out = wide[:, 2:2+a] of a sentinel-filled tensor with
    more rows than n: the actions of the contiguous call, and not one byte outside the [n, a] window is touched"""
    (H, D), (o, a, bound) = twins(algo, env)
    ag = P.Agent.__new__(P.Agent)                                    # the mirror's method on an engine of this test
    ag.engine = D
    for n in (1, 5, 67):
        obs = obs_rows(n, o, seed=n)
        want = H.predict(obs.numpy(), False)
        big = torch.full((n, o + 5), float("nan"), device=DEV)
        big[:, 1:1 + o] = obs.to(DEV)
        wide = torch.full((n + 3, a + 7), SENTINEL, device=DEV)
        got = ag.predict_device({"observations": big[:, 1:1 + o]}, explore=False, out=wide[:, 2:2 + a])
        assert got.shape == (n, a) and got.data_ptr() == wide[:, 2:2 + a].data_ptr()
        host = wide.cpu().numpy()
        assert np.array_equal(host[:n, 2:2 + a], want), n
        host[:n, 2:2 + a] = np.float32(SENTINEL)
        assert np.array_equal(host.view(np.uint32), np.full_like(host, SENTINEL).view(np.uint32)), n
        # float64 and a transposed (inner stride) observation: converted on the device, same result; `out` made by the call
        for form in (obs.double().to(DEV), obs.t().contiguous().to(DEV).t()):
            assert form.dtype != torch.float32 or form.stride(1) != 1 or n == 1
            res = ag.predict_device({"observations": form}, explore=False)
            assert res.dtype == torch.float32 and res.device == torch.device(DEV) and np.array_equal(res.cpu().numpy(), want)
    # one row with an inner stride, in and out: the observation is made contiguous first, such an `out` is refused unwritten
    obs = obs_rows(1, o, seed=1)
    want = H.predict(obs.numpy(), False)
    spread = torch.full((1, 2 * o), float("nan"), device=DEV)
    spread[:, ::2] = obs.to(DEV)
    assert np.array_equal(ag.predict_device({"observations": spread[:, ::2]}, explore=False).cpu().numpy(), want)
    wide = torch.full((2, 2 * a), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="out"):
        ag.predict_device({"observations": obs.to(DEV)}, explore=False, out=wide[:1, ::2])
    D.sync()
    assert (wide == SENTINEL).all()
    with pytest.raises(TypeError):
        ag.predict_device({"observations": obs_rows(4, o, 0)}, explore=False)      # host data: predict() takes it


# ------------------------------------------------------------------------------------------ 3. ordering without synchronisation
def test_ordered_against_the_callers_stream_without_a_sync():
    """a side stream: a long producer, then obs.copy_(src); predict_device under that stream; obs overwritten with NaNs right after;
    the result read on that stream.  Nothing synchronises in between -- the event waits do the ordering."""
    (T, D), (o, a, bound) = twins("sac", "hopper")
    n = 16
    src = obs_rows(n, o, seed=9).to(DEV)
    want = device_call(T, src, True)                                 # the twin, fully synchronised
    torch.cuda.synchronize()
    ag = P.Agent.__new__(P.Agent)
    ag.engine = D
    side = torch.cuda.Stream(device=DEV)
    obs, out = torch.zeros(n, o, device=DEV), torch.zeros(n, a, device=DEV)
    m = torch.randn(2048, 2048, device=DEV)
    before, before_b = D.predict_device_stats(), D.boundary_stats()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(12):
            m = (m @ m) * 1e-3                                       # the producer: milliseconds of work ahead of the copy
        obs.copy_(src)
        got = ag.predict_device({"observations": obs}, explore=True, out=out)
        obs.fill_(float("nan"))                                      # must not overtake the engine's read
        result = got.clone()                                         # read on the side stream, at once
    after, after_b = D.predict_device_stats(), D.boundary_stats()
    assert after["ordered_calls"] - before["ordered_calls"] == 1 and after["calls"] - before["calls"] == 1
    assert after_b["ordered_calls"] - before_b["ordered_calls"] == 1
    side.synchronize()
    assert np.array_equal(result.cpu().numpy(), want)
    assert torch.isnan(obs).all()


# ------------------------------------------------------------------------------------------ 4. neutral to the learner
@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah")])
def test_device_acting_between_periods_leaves_the_learner_alone(algo, env):
    """4 periods through run_iterations with an acting call between them: predict on one engine, predict_device on its twin.
    Same parameters, Adam state, metrics and sampled indices; the period graph is the one captured at the start (a call that
    reset chain_ready would have sent the next period through the opening graph, whose draws sit elsewhere)."""
    (H, D), (o, a, bound) = twins(algo, env)
    for e in (H, D):
        e.rb_extend(*[t.numpy() for t in synth_transitions(1500, o, a, bound, seed=31)])
        e.instantiate_graphs()
    nodes = D.graph_kernel_count(4)
    assert nodes > 0
    for p in range(4):
        obs = obs_rows(4, o, seed=p)
        for e in (H, D):
            assert e.run_iterations(3 * p, 3) == 3 * p + 3
        assert np.array_equal(H.predict(obs.numpy(), True), device_call(D, obs.to(DEV), True)), p
    assert_same_state(H, D, "index")
    assert D.graph_kernel_count(4) == H.graph_kernel_count(4) == nodes


# ------------------------------------------------------------------------------------------ 5. the loop
def test_train_on_a_device_env_equals_train_on_the_host_env():
    """train(device_env=True) on SyntheticDeviceVecEnv against train() on SyntheticVecEnv, same seed, 60 iterations past
    learning_starts, a horizon and a termination threshold short enough for both kinds of episode end: the ring rows, every
    parameter set and the action of every step are the same bits."""
    o, a, n = 11, 3, 4
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 200 + 60 * n - 1, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 1000})
    logs = []
    for device_env in (False, True):
        env = (loop.SyntheticDeviceVecEnv(o, a, n, horizon=7, term_at=2.5, device=DEV) if device_env
               else loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5))
        env.action_space.seed(0)
        acts, flags, step = [], [], env.step

        def spy(actions, _step=step, _acts=acts, _flags=flags):
            res = _step(actions)
            _acts.append(actions)                                    # (device tensors are looked at after the run)
            _flags.append((res[2], res[3]))
            return res
        env.step = spy
        torch.manual_seed(0)
        agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                        torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
        m = loop.train(cfg, env, agent, fused=True, device_env=device_env)
        eng = track(agent.engine)
        st = eng.predict_device_stats()
        assert (st["calls"] > 0) == device_env and (eng.boundary_stats()["device_extends"] > 0) == device_env
        ring = []
        for lo in range(0, eng.rb_len(), 64):
            eng.rb_sample_with_indices(np.minimum(np.arange(lo, lo + 64), eng.rb_len() - 1))
            ring.append(eng.read_batch())
        host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        logs.append(dict(metrics=m, params=[eng.get_params(w) for w in SETS], rb=eng.rb_len(), ring=ring,
                         acts=[host(x) for x in acts], term=sum(int(host(t).sum()) for t, _ in flags), trunc=sum(int(host(t).sum()) for _, t in flags),
                         counters=(agent.timesteps_so_far, agent.qnet_updates_so_far, agent.actor_updates_so_far)))
        eng.close()
    x, y = logs
    assert x["term"] == y["term"] > 0 and x["trunc"] == y["trunc"] > 0
    assert x["counters"] == y["counters"] and x["counters"][1] >= 60 and x["rb"] == y["rb"] > 200
    assert len(x["acts"]) == len(y["acts"]) and all(np.array_equal(p, q) for p, q in zip(x["acts"], y["acts"]))
    assert x["metrics"] == y["metrics"] and all(np.array_equal(p, q) for p, q in zip(x["params"], y["params"]))
    for p, q in zip(x["ring"], y["ring"]):
        for k in p:
            assert np.array_equal(p[k], q[k]), k


# ------------------------------------------------------------------------------------------ 6. errors
def test_bad_arguments_and_the_acting_call_in_flight():
    (eng,), (o, a, bound) = twins("sac", "hopper", count=1)
    lib, h, ORD = eng.lib, eng._h, _lib.SRC_ORDERED
    obs, out = torch.zeros(8, o, device=DEV), torch.full((8, a), SENTINEL, device=DEV)
    host = np.zeros((8, o), np.float32)
    pinned = torch.zeros(8, o).pin_memory()
    po, pa, vp = C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p
    call = lambda *args: lib.sactd3_predict_device(h, *args)
    assert call(None, o, 4, 0, pa, a, None, ORD) == _lib.EINVAL                         # NULL pointers
    assert call(po, o, 4, 0, None, a, None, ORD) == _lib.EINVAL
    assert call(po, o, 0, 0, pa, a, None, ORD) == _lib.EINVAL                           # n out of range
    assert call(po, o, MAXN + 1, 0, pa, a, None, ORD) == _lib.EINVAL
    assert call(po, o - 1, 4, 0, pa, a, None, ORD) == _lib.EINVAL                       # strides below the widths
    assert call(po, o, 4, 0, pa, a - 1, None, ORD) == _lib.EINVAL
    assert call(vp(host.ctypes.data), o, 4, 0, pa, a, None, ORD) == _lib.EINVAL         # host pointers: pageable, pinned
    assert call(vp(pinned.data_ptr()), o, 4, 0, pa, a, None, ORD) == _lib.EINVAL
    assert call(po, o, 4, 0, vp(pinned.data_ptr()), a, None, ORD) == _lib.EINVAL
    assert call(po, o, 4, 0, pa, a, None, 2) == _lib.EINVAL                             # an unknown flag
    st = (C.c_int64 * 4)()
    assert lib.sactd3_predict_device_stats(h, None) == _lib.EINVAL
    assert lib.sactd3_predict_device_stats(h, st) == 0 and list(st) == [0, 0, 0, 0]     # none of those launched anything
    eng.sync()
    assert (out == SENTINEL).all()
    eng.predict_begin(host[:4], True)
    assert call(po, o, 4, 1, pa, a, None, ORD) == _lib.ESTATE                           # shares the exploration counter with that call
    with pytest.raises(P.EngineError, match="in flight"):
        eng.predict_device(obs.data_ptr(), o, 4, True, out.data_ptr(), a)
    first = eng.predict_end()
    assert call(po, o, 4, 1, pa, a, None, ORD) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got[:4]).all() and not np.array_equal(got[:4], first) and (got[4:] == np.float32(SENTINEL)).all()
    assert lib.sactd3_predict_device_stats(h, st) == 0 and list(st) == [1, 4, 1, 0]


@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah")])
def test_predict_begin_behind_a_device_call_waits_for_it(algo, env):
    """The device call returns with its kernels queued on the learner stream; they use the scratch, the draw buffer and the counter
    of the acting pair.  A predict_begin right behind it -- with nothing in between that writes the actor, after an earlier
    begin / end has cleared the pending wait -- must order the acting stream behind them: device, begin / end on one engine equal
    predict, begin / end on its twin, and the begin is counted among those that waited for the learner."""
    (H, D), (o, a, bound) = twins(algo, env)
    warm = obs_rows(4, o, seed=0).numpy()
    for e in (H, D):                                                 # clears the wait every engine starts with
        e.predict_begin(warm, True)
        e.predict_end()
    assert D.acting_stats()["begin_waited_for_learner"] == 1
    side = torch.cuda.Stream(device=DEV)
    m = torch.randn(2048, 2048, device=DEV)
    for k, n in enumerate((4, 67, 16, 5)):
        big, small = obs_rows(n, o, seed=10 + k), obs_rows(4, o, seed=20 + k)
        want = (H.predict(big.numpy(), True), None)
        H.predict_begin(small.numpy(), True)
        want = (want[0], H.predict_end())
        dev_obs, out = big.to(DEV), torch.empty(n, a, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                m = (m @ m) * 1e-3                                   # the device call's kernels stay queued behind this for a while
            D.predict_device(dev_obs.data_ptr(), o, n, True, out.data_ptr(), a, side.cuda_stream, True)
        D.predict_begin(small.numpy(), True)                         # at once: the device call has not run yet
        got_small = D.predict_end()
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(got_small, want[1]), (k, n)
        assert np.array_equal(H.read_noise(_lib.SITE_PREDICT, 4), D.read_noise(_lib.SITE_PREDICT, 4))
    assert D.acting_stats()["begin_waited_for_learner"] == 5 and H.acting_stats()["begin_waited_for_learner"] == 1


def test_device_env_on_the_gpu_equals_the_host_env_across_pool_refreshes():
    """SyntheticDeviceVecEnv on the GPU with small blocks of normals and a position copy requested every 5 steps (pinned copy + event
    query, never waited for): 600 steps equal the host env's -- checked from the tensors kept, after the run"""
    o, a, n = 5, 2, 3
    host = loop.SyntheticVecEnv(o, a, n, horizon=4, term_at=2.0)
    dev = loop.SyntheticDeviceVecEnv(o, a, n, horizon=4, term_at=2.0, device=DEV)
    dev._block, dev._refresh_every = 8 * n * o, 5
    host.reset(seed=11)
    dev.reset(seed=11)
    want, got = [], []
    for step in range(600):
        act = host.action_space.sample()
        want.append(host.step(act)[:4])
        got.append(dev.step(torch.from_numpy(act).to(DEV))[:4])
    assert dev._base > 0 and dev._pool.numel() == dev._drawn - dev._base
    for step, (w, g) in enumerate(zip(want, got)):
        for x, y in zip(w, g):
            assert np.array_equal(x, y.cpu().numpy()), step
