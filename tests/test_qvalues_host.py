"""CPU: everything of the scoring route that needs no GPU -- how Agent.q_values hands its rows and its `out` to the engine (pointers,
strides, the [2, n, 1] addressing, conversions, refusals; on stand-ins that carry __cuda_array_interface__), the host route, the
batch generation it leaves alone, and the NULL-engine behaviour of the three entry points."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod
from tests.helpers import FakeDeviceArray, SlotGeneration

O, A = 11, 3


class RecordingEngine(SlotGeneration):
    """what Agent.q_values needs of an engine; records what it is handed"""
    device_inputs = True

    def __init__(self):
        self.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0)
        self.calls, self.host_calls = [], []

    def q_values_device(self, *args):
        self.calls.append(args)

    def q_values(self, obs, act, target):
        self.host_calls.append((obs, act, target))
        return np.arange(2 * obs.shape[0], dtype=np.float32).reshape(2, -1)


def mirror(engine=None):
    ag = agent_mod.Agent.__new__(agent_mod.Agent)          # the method under test reads `engine` only
    ag.engine = engine or RecordingEngine()
    return ag


class Sliceable(FakeDeviceArray):
    def __getitem__(self, key):
        return ("rows", key)


def test_contiguous_fields_and_out_go_to_the_engine_as_they_are():
    ag, obs, act, out = mirror(), FakeDeviceArray((8, O)), FakeDeviceArray((8, A)), FakeDeviceArray((2, 8, 1))
    assert ag.q_values({"observations": obs, "actions": act}, out=out) is out
    assert ag.q_values({"observations": obs, "actions": act}, target=True, out=out) is out
    # (pointer, row stride) of obs and actions, n, target, then `out`: pointer, row stride, net stride; not a torch array: the default stream
    assert ag.engine.calls == [(obs.ptr, O, act.ptr, A, 8, False, out.ptr, 1, 8, 0), (obs.ptr, O, act.ptr, A, 8, True, out.ptr, 1, 8, 0)]
    assert ag.engine.host_calls == [] and ag.engine.batch_generation() == 5


def test_a_missing_actions_key_is_the_policy_form():
    ag, obs, out = mirror(), FakeDeviceArray((8, O)), FakeDeviceArray((2, 8, 1))
    ag.q_values({"observations": obs}, out=out)
    (optr, old, aptr, ald, n, target, qptr, q_ld, q_ns, stream), = ag.engine.calls
    assert aptr == 0 and (optr, old, n, target, qptr, q_ld, q_ns) == (obs.ptr, O, 8, False, out.ptr, 1, 8)


def test_views_are_kept_as_they_are():
    """row strides of the sources; `out` = a [2, 8, 1] window of a [2, 11, 3] array: rows 3 elements apart, nets 33"""
    ag = mirror()
    obs = FakeDeviceArray((8, O), strides=(4 * (O + 5), 4))
    act = FakeDeviceArray((8, A), strides=(4 * (A + 7), 4))
    out = FakeDeviceArray((2, 8, 1), strides=(4 * 33, 4 * 3, 4))
    assert ag.q_values({"observations": obs, "actions": act}, out=out) is out
    assert ag.engine.calls == [(obs.ptr, O + 5, act.ptr, A + 7, 8, False, out.ptr, 3, 33, 0)]
    assert obs.log == [] and act.log == []                                 # nothing converted


def test_out_may_hold_more_rows_than_the_call_scores():
    ag, out = mirror(), Sliceable((2, 12, 1), strides=(4 * 40, 4 * 2, 4))
    got = ag.q_values({"observations": FakeDeviceArray((8, O)), "actions": FakeDeviceArray((8, A))}, out=out)
    assert got == ("rows", (slice(None), slice(None, 8)))
    assert ag.engine.calls[0][4:] == (8, False, out.ptr, 2, 40, 0)
    # a contiguous one (no strides reported): the net stride is its row count
    ag, out = mirror(), Sliceable((2, 12, 1))
    ag.q_values({"observations": FakeDeviceArray((8, O))}, out=out)
    assert ag.engine.calls[0][4:] == (8, False, out.ptr, 1, 12, 0)
    # one row: whatever stride its row dimension reports
    ag, out = mirror(), FakeDeviceArray((2, 1, 1), strides=(4 * 7, 0, 4))
    ag.q_values({"observations": FakeDeviceArray((1, O))}, out=out)
    assert ag.engine.calls[0][4:] == (1, False, out.ptr, 1, 7, 0)


def test_conversions_happen_on_the_device():
    """not float32 -> .to(float32); an inner stride -> .contiguous(); FakeDeviceArray.cpu() raises"""
    for key, width in (("observations", O), ("actions", A)):
        for bad, log in ((FakeDeviceArray((8, width), "<f8"), [("to", "float32")]), (FakeDeviceArray((8, width), strides=(4, 32)), ["contiguous"]),
                         (FakeDeviceArray((8, width), "<f2", strides=(2, 16)), [("to", "float32")])):
            ag, out = mirror(), FakeDeviceArray((2, 8, 1))
            made = []
            for name in ("to", "contiguous"):
                def spy(self, *a, _f=getattr(FakeDeviceArray, name)):
                    made.append(_f(self, *a))
                    return made[-1]
                setattr(bad, name, spy.__get__(bad))
            td = {"observations": FakeDeviceArray((8, O)), "actions": FakeDeviceArray((8, A))}
            td[key] = bad
            ag.q_values(td, out=out)
            call, = ag.engine.calls
            ptr, ld = (call[0], call[1]) if key == "observations" else (call[2], call[3])
            assert made and made[-1].log == log and ptr == made[-1].ptr != bad.ptr and ld == width and call[4] == 8


def test_what_the_device_route_cannot_take():
    ok = dict(observations=FakeDeviceArray((8, O)), actions=FakeDeviceArray((8, A)))
    ok_out = FakeDeviceArray((2, 8, 1))
    eng = RecordingEngine()
    with pytest.raises(TypeError, match="both"):                           # mixed residency, either way round
        mirror(eng).q_values(dict(ok, actions=np.zeros((8, A), np.float32)), out=ok_out)
    with pytest.raises(TypeError, match="both"):
        mirror(eng).q_values(dict(ok, observations=torch.zeros(8, O)), out=ok_out)
    for key, width in (("observations", O), ("actions", A)):               # another GPU's memory
        with pytest.raises(TypeError, match="device"):
            mirror(eng).q_values(dict(ok, **{key: FakeDeviceArray((8, width), device_index=1)}), out=ok_out)
    off = RecordingEngine()
    off.device_inputs = False
    with pytest.raises(TypeError, match="device_inputs"):
        mirror(off).q_values(ok, out=ok_out)
    for bad in (FakeDeviceArray((2, 8, 1), device_index=1), FakeDeviceArray((2, 8, 1), "<f8"), np.zeros((2, 8, 1), np.float32)):
        with pytest.raises(TypeError, match="out"):
            mirror(eng).q_values(ok, out=bad)
    for bad in (FakeDeviceArray((2, 7, 1)), FakeDeviceArray((2, 8)), FakeDeviceArray((1, 8, 1)), FakeDeviceArray((2, 8, 2)),
                FakeDeviceArray((2, 8, 1), strides=(0, 4, 4)), FakeDeviceArray((2, 8, 1), strides=(32, 2, 4)), FakeDeviceArray((2, 8, 1), strides=(32, -4, 4))):
        with pytest.raises(ValueError, match="out"):
            mirror(eng).q_values(ok, out=bad)
    with pytest.raises(ValueError, match="expected"):                      # a wrong width
        mirror(eng).q_values(dict(ok, observations=FakeDeviceArray((8, O + 1))), out=ok_out)
    with pytest.raises(ValueError, match="rows"):                          # fields that disagree on n
        mirror(eng).q_values(dict(ok, actions=FakeDeviceArray((7, A))), out=ok_out)
    with pytest.raises(TypeError, match="out"):                            # host rows come back as numpy: no `out`
        mirror(eng).q_values({"observations": np.zeros((8, O), np.float32)}, out=ok_out)
    with pytest.raises(KeyError):
        mirror(eng).q_values({"actions": FakeDeviceArray((8, A))}, out=ok_out)
    assert eng.calls == [] and off.calls == [] and eng.host_calls == []


def test_without_torch_the_caller_brings_out(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torch", None)                        # `import torch` now raises ImportError
    with pytest.raises(TypeError, match="torch"):
        mirror().q_values({"observations": FakeDeviceArray((8, O))})
    with pytest.raises(TypeError, match="without torch the caller passes `out`"):      # a read-out that has to allocate says the same
        agent_mod._device_outputs(RecordingEngine(), 8)


def test_host_arrays_take_the_host_call_and_come_back_as_numpy():
    ag = mirror()
    obs, act = np.ones((4, O), np.float64), torch.zeros(4, A)
    got = ag.q_values({"observations": obs, "actions": act}, target=True)
    assert isinstance(got, np.ndarray) and got.shape == (2, 4, 1) and got.dtype == np.float32
    assert np.array_equal(got[:, :, 0], np.arange(8, dtype=np.float32).reshape(2, 4))
    (o_, a_, target), = ag.engine.host_calls
    assert target is True and np.array_equal(o_, obs) and np.array_equal(a_, act.numpy())
    ag.q_values({"observations": obs})
    assert ag.engine.host_calls[1][1] is None and ag.engine.calls == [] and ag.engine.batch_generation() == 5


def test_a_batch_handle_stays_current_across_a_score():
    eng = RecordingEngine()
    handle = agent_mod.BatchHandle(eng, eng.batch_generation())
    ag = mirror(eng)
    ag.q_values({"observations": FakeDeviceArray((8, O)), "actions": FakeDeviceArray((8, A))}, out=FakeDeviceArray((2, 8, 1)))
    ag.q_values({"observations": np.zeros((8, O), np.float32)})
    assert handle._is_current()
    ag._stage(handle)                                                      # ... and update_qnets(handle) would still take it


def test_null_engine_is_refused_without_a_device():
    lib = pkg.load_library()
    st = (C.c_int64 * 4)()
    buf = (C.c_float * 64)()
    assert lib.sactd3_qvalues_device(None, C.c_void_p(4096), O, C.c_void_p(8192), A, 4, _lib.Q_ONLINE, C.c_void_p(12288), 1, 4, None,
                                     _lib.SRC_ORDERED) == _lib.EINVAL
    assert lib.sactd3_qvalues(None, buf, buf, 4, _lib.Q_TARGET, buf) == _lib.EINVAL
    assert lib.sactd3_qvalues_stats(None, st) == _lib.EINVAL
    assert (_lib.Q_ONLINE, _lib.Q_TARGET) == (0, 1)
