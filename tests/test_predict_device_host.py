"""CPU: everything of the device acting route that needs no GPU -- how Agent.predict_device hands an observation to the engine
(pointer, stride, conversions, refusals; on stand-ins that carry __cuda_array_interface__), the NULL-engine behaviour of the two new
entry points, the torch port of the synthetic env against the numpy one, DeviceRollout against Rollout, and train()'s flags."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, loop
from tests.helpers import FakeDeviceArray

O, A = 11, 3


class RecordingEngine:
    """what Agent.predict_device needs of an engine; records what it is handed"""
    device_inputs = True

    def __init__(self):
        self.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0)
        self.calls = []

    def predict_device(self, *args):
        self.calls.append(args)


def mirror(engine=None):
    ag = agent_mod.Agent.__new__(agent_mod.Agent)          # the method under test reads `engine` only
    ag.engine = engine or RecordingEngine()
    return ag


# ------------------------------------------------------------------------------------------ routing
def test_contiguous_observation_and_out_go_to_the_engine_as_they_are():
    ag, obs, out = mirror(), FakeDeviceArray((8, O)), FakeDeviceArray((8, A))
    assert ag.predict_device({"observations": obs}, explore=True, out=out) is out
    assert ag.engine.calls == [(obs.ptr, O, 8, True, out.ptr, A, 0)]      # (not a torch array: the default stream)


def test_row_strides_of_views_are_kept():
    ag = mirror()
    obs = FakeDeviceArray((8, O), strides=(4 * (O + 5), 4))
    out = FakeDeviceArray((8, A), strides=(4 * (A + 7), 4))
    ag.predict_device({"observations": obs}, explore=False, out=out)
    assert ag.engine.calls == [(obs.ptr, O + 5, 8, False, out.ptr, A + 7, 0)]
    assert obs.log == []                                                   # nothing converted


def test_conversions_happen_on_the_device():
    """not float32 -> .to(float32); an inner stride -> .contiguous(); FakeDeviceArray.cpu() raises"""
    for obs, log in ((FakeDeviceArray((8, O), "<f8"), [("to", "float32")]), (FakeDeviceArray((8, O), strides=(4, 32)), ["contiguous"]),
                     (FakeDeviceArray((8, O), "<f2", strides=(2, 16)), [("to", "float32")])):
        ag, out = mirror(), FakeDeviceArray((8, A))
        made = []
        for name in ("to", "contiguous"):
            def spy(self, *a, _f=getattr(FakeDeviceArray, name)):
                made.append(_f(self, *a))
                return made[-1]
            setattr(obs, name, spy.__get__(obs))
        ag.predict_device({"observations": obs}, explore=True, out=out)
        (ptr, ld, n, explore, optr, old, stream), = ag.engine.calls
        assert made and made[-1].log == log and ptr == made[-1].ptr != obs.ptr and (ld, n, optr, old) == (O, 8, out.ptr, A)


def test_one_row_with_an_inner_stride_is_not_contiguous():
    """n == 1: the row stride does not matter, the inner stride does -- a one-row `wide[:1, ::2]` must not be written as if it
    were contiguous, nor read"""
    ag = mirror()
    with pytest.raises(ValueError, match="out"):
        ag.predict_device({"observations": FakeDeviceArray((1, O))}, explore=True, out=FakeDeviceArray((1, A), strides=(64, 8)))
    obs, out = FakeDeviceArray((1, O), strides=(4 * 2 * O, 8)), FakeDeviceArray((1, A), strides=(4, 4))
    ag.predict_device({"observations": obs}, explore=True, out=out)
    (ptr, ld, n, _, optr, old, _), = ag.engine.calls
    assert ptr != obs.ptr and (ld, n, optr, old) == (O, 1, out.ptr, A)          # the observation was made contiguous first


def test_out_may_hold_more_rows_than_the_observation():
    class Sliceable(FakeDeviceArray):
        def __getitem__(self, key):
            return ("rows", key)
    ag, out = mirror(), Sliceable((12, A), strides=(4 * (A + 1), 4))
    assert ag.predict_device({"observations": FakeDeviceArray((8, O))}, explore=True, out=out) == ("rows", slice(None, 8))
    assert ag.engine.calls[0][2:] == (8, True, out.ptr, A + 1, 0)


def test_what_the_device_route_cannot_take_is_a_type_error():
    ok_out = FakeDeviceArray((8, A))
    with pytest.raises(TypeError, match="device"):                         # host data
        mirror().predict_device({"observations": np.zeros((8, O), np.float32)}, explore=True, out=ok_out)
    with pytest.raises(TypeError, match="device"):                         # a CPU torch tensor
        mirror().predict_device({"observations": torch.zeros(8, O)}, explore=True, out=ok_out)
    with pytest.raises(TypeError, match="device"):                         # another GPU's memory
        mirror().predict_device({"observations": FakeDeviceArray((8, O), device_index=1)}, explore=True, out=ok_out)
    off = RecordingEngine()
    off.device_inputs = False
    with pytest.raises(TypeError, match="device_inputs"):
        mirror(off).predict_device({"observations": FakeDeviceArray((8, O))}, explore=True, out=ok_out)
    for bad in (FakeDeviceArray((8, A), device_index=1), FakeDeviceArray((8, A), "<f8"), np.zeros((8, A), np.float32)):
        with pytest.raises(TypeError, match="out"):
            mirror().predict_device({"observations": FakeDeviceArray((8, O))}, explore=True, out=bad)
    for bad in (FakeDeviceArray((7, A)), FakeDeviceArray((8, A), strides=(4, 32))):      # too few rows; an inner stride
        with pytest.raises(ValueError, match="out"):
            mirror().predict_device({"observations": FakeDeviceArray((8, O))}, explore=True, out=bad)
    with pytest.raises(ValueError, match="expected"):
        mirror().predict_device({"observations": FakeDeviceArray((8, O + 1))}, explore=True, out=ok_out)
    assert off.calls == []


def test_without_torch_the_caller_brings_out(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torch", None)                        # `import torch` now raises ImportError
    with pytest.raises(TypeError, match="torch"):
        mirror().predict_device({"observations": FakeDeviceArray((8, O))}, explore=True)


def test_null_engine_is_refused_without_a_device():
    lib = pkg.load_library()
    st = (C.c_int64 * 4)()
    assert lib.sactd3_predict_device(None, C.c_void_p(4096), O, 4, 1, C.c_void_p(8192), A, None, _lib.SRC_ORDERED) == _lib.EINVAL
    assert lib.sactd3_predict_device_stats(None, st) == _lib.EINVAL


# ------------------------------------------------------------------------------------------ the env
@pytest.mark.parametrize("o,a,n,horizon,term_at", [(11, 3, 4, 7, 2.5), (5, 2, 3, 4, 1e9), (17, 6, 1, 9, 2.2)])
def test_device_env_on_the_cpu_reproduces_the_host_env(o, a, n, horizon, term_at):
    """same seed -> the same observations, rewards, flags and final observations, bit for bit, over 200 steps in which envs are
    truncated, terminated (where term_at allows it) and reset; the action space draws the same actions"""
    host = loop.SyntheticVecEnv(o, a, n, horizon=horizon, term_at=term_at)
    dev = loop.SyntheticDeviceVecEnv(o, a, n, horizon=horizon, term_at=term_at, device=torch.device("cpu"))
    for e in (host, dev):
        e.action_space.seed(3)
    x, _ = host.reset(seed=7)
    y, _ = dev.reset(seed=7)
    assert y.dtype == torch.float32 and np.array_equal(x, y.numpy())
    seen = dict(term=0, trunc=0)
    for step in range(200):
        act, act_d = host.action_space.sample(), dev.action_space.sample()
        assert np.array_equal(act, act_d.numpy())
        if step % 5 == 0:
            act, act_d = 3.0 * act, 3.0 * act_d                            # out of bounds: both clip
        x, r, te, tr, info = host.step(act)
        y, r_d, te_d, tr_d, info_d = dev.step(act_d)
        assert np.array_equal(x, y.numpy()) and np.array_equal(r, r_d.numpy()) and r_d.dtype == torch.float32, step
        assert np.array_equal(te, te_d.numpy()) and np.array_equal(tr, tr_d.numpy()), step
        ended = te | tr
        assert np.array_equal(ended, info_d["_final_observation"].numpy())
        assert tuple(info_d["final_observation"].shape) == (n, o)
        for k in np.flatnonzero(ended):
            assert np.array_equal(info["final_observation"][k], info_d["final_observation"][k].numpy()), (step, k)
        seen["term"] += int(te.sum())
        seen["trunc"] += int(tr.sum())
    assert seen["trunc"] > 0 and (seen["term"] > 0 or term_at > 100)


def test_device_env_drops_and_redraws_its_pool_of_normals():
    """small blocks and a refresh every 5 steps: over 600 steps the pool of normals is refilled and trimmed many times, from bounds
    that restart from a copy of the position taken steps earlier -- and the env still equals the host env, which draws as it goes"""
    o, a, n = 5, 2, 3
    host = loop.SyntheticVecEnv(o, a, n, horizon=4, term_at=2.0)
    dev = loop.SyntheticDeviceVecEnv(o, a, n, horizon=4, term_at=2.0, device="cpu")
    dev._block, dev._refresh_every = 8 * n * o, 5
    x, _ = host.reset(seed=11)
    y, _ = dev.reset(seed=11)
    trims, bases = 0, [0]
    for step in range(600):
        act = host.action_space.sample()
        x, r, te, tr, _ = host.step(act)
        y, r_d, te_d, tr_d, _ = dev.step(torch.from_numpy(act))
        assert np.array_equal(x, y.numpy()) and np.array_equal(te, te_d.numpy()) and np.array_equal(tr, tr_d.numpy()), step
        assert dev._base <= dev._lo <= int(dev._cur) <= dev._hi <= dev._drawn, step
        trims += dev._base != bases[-1]
        bases.append(dev._base)
        assert dev._pool.numel() == dev._drawn - dev._base <= 40 * n * o      # the window stays a few blocks wide
    assert trims > 20 and dev._base > 600 * n * o


def test_fold_sum_is_one_order_everywhere():
    g = np.random.default_rng(0)
    for k in (1, 2, 3, 7, 8, 11, 376):
        x = g.standard_normal((5, k, 3)).astype(np.float32)
        want = x.copy()
        kk = k
        while kk > 1:                                                      # the definition, written out column by column
            h = kk // 2
            for i in range(h):
                want[:, i] = want[:, i] + want[:, kk - h + i]
            kk -= h
        assert np.array_equal(loop._fold_sum(x.copy()), want[:, 0])
        assert np.array_equal(loop._fold_sum(torch.from_numpy(x.copy())).numpy(), want[:, 0])
        assert np.allclose(want[:, 0], x.astype(np.float64).sum(1), atol=1e-4)


# ------------------------------------------------------------------------------------------ the rollout
class StubRb:
    def __init__(self):
        self.got = []

    def extend(self, td):
        self.got.append({k: (v.numpy().copy() if hasattr(v, "numpy") else np.array(v)) for k, v in td.items()})


class StubAgent:
    """a deterministic 'policy' on either kind of array"""

    def __init__(self, a):
        self.a, self.rb, self.timesteps_so_far, self.asked = a, StubRb(), 0, 0

    def predict(self, td, *, explore):
        self.asked += 1
        return np.tanh(np.asarray(td["observations"])[:, :self.a] * np.float32(0.5)).astype(np.float32)

    def predict_device(self, td, *, explore, out=None):
        assert explore and isinstance(td["observations"], torch.Tensor)
        self.asked += 1
        return torch.from_numpy(np.tanh(td["observations"].numpy()[:, :self.a] * np.float32(0.5)).astype(np.float32))


@pytest.mark.parametrize("action_repeat", [1, 3])
def test_device_rollout_hands_the_ring_what_rollout_hands_it(action_repeat):
    o, a, n, starts = 11, 3, 4, 40
    host, dev = loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5), loop.SyntheticDeviceVecEnv(o, a, n, horizon=7, term_at=2.5, device="cpu")
    ag_h, ag_d = StubAgent(a), StubAgent(a)
    ro_h = loop.Rollout(host, ag_h, 5, starts, action_repeat)
    ro_d = loop.DeviceRollout(dev, ag_d, 5, starts, action_repeat)
    for step in range(120):
        for ro, ag in ((ro_h, ag_h), (ro_d, ag_d)):
            ro.choose()
            ro.advance()
            ag.timesteps_so_far += n
    assert ag_h.asked == ag_d.asked > 0 and len(ag_h.rb.got) == len(ag_d.rb.got) == 120
    cut = 0
    for x, y in zip(ag_h.rb.got, ag_d.rb.got):
        assert sorted(x) == sorted(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k
        cut += int((x["next_observations"] != x["observations"]).any())
    assert y["rewards"].shape == (n, 1) and y["dones"].dtype == np.bool_
    assert isinstance(ro_d.obs, torch.Tensor) and isinstance(ro_d.actions, torch.Tensor)


def test_device_rollout_needs_predict_device():
    class NoDevice:
        rb, timesteps_so_far = StubRb(), 0
    with pytest.raises(TypeError, match="predict_device"):
        loop.DeviceRollout(loop.SyntheticDeviceVecEnv(3, 1, 2, device="cpu"), NoDevice(), 0, 10, 1)


def test_overlap_and_device_env_exclude_each_other():
    cfg = SimpleNamespace(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=20)
    with pytest.raises(ValueError, match="device_env"):
        loop.train(cfg, loop.SyntheticDeviceVecEnv(3, 1, 2, device="cpu"), StubAgent(1), overlap=True, device_env=True)
