"""CPU: the outward half of the device boundary (sactd3_read_batch_device / sactd3_rb_read_rows_device / sactd3_readout_stats,
include/sactd3.h) as far as it can be checked without a GPU -- the exported symbols and their NULL-engine behaviour, the ctypes mirror
of sactd3_device_fields_out, the output helper of the mirror (agent.py:_device_outputs) on stand-ins that carry
__cuda_array_interface__, and that a default ReplayBuffer never takes the device route.  No GPU is touched."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod
from tests.helpers import FakeDeviceArray, SlotGeneration

O, A, N = 11, 3, 8
ENGINE = SimpleNamespace(device_inputs=True, cfg=SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0, batch_size=N))
TYPESTR = {"f4": "<f4", "b1": "|b1", "i8": "<i8"}
ORDER = ("observations", "actions", "rewards", "next_observations", "dones", "index")


def fake_alloc(shape, kind):
    return FakeDeviceArray(shape, TYPESTR[kind])


def test_library_exports_the_readout_symbols_and_refuses_a_null_engine():
    lib = pkg.load_library()
    names = ("sactd3_read_batch_device", "sactd3_rb_read_rows_device", "sactd3_readout_stats")
    raw = C.CDLL(pkg.library_path())
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    f, st, idx = _lib.CDeviceFieldsOut(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
    assert lib.sactd3_read_batch_device(None, C.byref(f), None, _lib.DST_ORDERED) == _lib.EINVAL
    assert lib.sactd3_rb_read_rows_device(None, C.cast(idx, C.c_void_p), 1, 4, C.byref(f), None, 0) == _lib.EINVAL
    assert lib.sactd3_readout_stats(None, st) == _lib.EINVAL
    assert _lib.DST_ORDERED == _lib.SRC_ORDERED == 1                       # the same bit: the same two-event protocol


def test_fields_out_struct_layout():
    assert C.sizeof(_lib.CDeviceFieldsOut) == 96 and _lib.CDeviceFieldsOut.index_ld.offset == 88      # six (pointer, int64) pairs
    assert [n for n, _ in _lib.CDeviceFieldsOut._fields_][::2] == ["obs", "actions", "rewards", "next_obs", "dones", "index"]


def test_allocated_outputs_are_contiguous_and_have_the_reference_shapes():
    tensors, fields = agent_mod._device_outputs(ENGINE, N, alloc=fake_alloc)
    assert [tensors[k].shape for k in ORDER] == [(N, O), (N, A), (N, 1), (N, O), (N, 1), (N,)]
    assert [tensors[k].typestr for k in ORDER] == ["<f4", "<f4", "<f4", "<f4", "|b1", "<i8"]
    assert tensors["terminations"] is tensors["dones"] and set(tensors) == set(ORDER) | {"terminations"}
    assert fields == [(tensors[k].ptr, w) for k, w in zip(ORDER, (O, A, 1, O, 1, 1))]


def test_column_sliced_outputs_keep_their_stride():
    W = 2 * O + A + 6
    out = {"observations": FakeDeviceArray((N, O), strides=(4 * W, 4)), "actions": FakeDeviceArray((N, A), strides=(4 * W, 4)),
           "rewards": FakeDeviceArray((N, 1), strides=(4 * W, 4)), "next_observations": FakeDeviceArray((N, O), strides=(4 * W, 4)),
           "dones": FakeDeviceArray((N, 1), "|b1", strides=(3, 1)), "index": FakeDeviceArray((N,), "<i8", strides=(16,))}
    tensors, fields = agent_mod._device_outputs(ENGINE, N, out, alloc=fake_alloc)
    assert all(tensors[k] is out[k] for k in ORDER) and tensors["terminations"] is out["dones"]
    assert fields == [(out[k].ptr, ld) for k, ld in zip(ORDER, (W, W, W, W, 3, 2))]


def test_column_vectors_and_flat_vectors_are_the_same_thing():
    for shape in ((N,), (N, 1)):
        out = {"rewards": FakeDeviceArray(shape), "dones": FakeDeviceArray(shape, "|u1"), "index": FakeDeviceArray(shape, "<i8")}
        tensors, fields = agent_mod._device_outputs(ENGINE, N, out, alloc=fake_alloc)
        assert [fields[k] for k in (2, 4, 5)] == [(out["rewards"].ptr, 1), (out["dones"].ptr, 1), (out["index"].ptr, 1)]
        assert tensors["rewards"] is out["rewards"] and tensors["observations"].shape == (N, O)      # the rest is allocated
    # one row: whatever the library reports as its stride, the width will do
    tensors, fields = agent_mod._device_outputs(ENGINE, 1, {"observations": FakeDeviceArray((1, O), strides=(4, 4))}, alloc=fake_alloc)
    assert fields[0] == (tensors["observations"].ptr, O)


def test_out_views_replace_single_fields_and_terminations_names_the_flags():
    flags = FakeDeviceArray((N, 1), "|b1", strides=(3, 1))
    obs = FakeDeviceArray((N, O), strides=(4 * (O + 5), 4))
    tensors, fields = agent_mod._device_outputs(ENGINE, N, {"terminations": flags, "observations": obs}, alloc=fake_alloc)
    assert tensors["dones"] is flags and tensors["terminations"] is flags and fields[4] == (flags.ptr, 3)
    assert tensors["observations"] is obs and fields[0] == (obs.ptr, O + 5)
    assert fields[1] == (tensors["actions"].ptr, A) and tensors["actions"].shape == (N, A)
    both = agent_mod._device_outputs(ENGINE, N, {"terminations": flags, "dones": flags}, alloc=fake_alloc)[0]
    assert both["dones"] is flags
    with pytest.raises(ValueError, match="one array"):
        agent_mod._device_outputs(ENGINE, N, {"terminations": flags, "dones": FakeDeviceArray((N, 1), "|b1")}, alloc=fake_alloc)


def test_wrong_shapes_are_a_value_error():
    for key, bad in (("observations", FakeDeviceArray((N, O + 1))), ("actions", FakeDeviceArray((N,))), ("rewards", FakeDeviceArray((N, 2))),
                     ("index", FakeDeviceArray((N, 2), "<i8")), ("next_observations", FakeDeviceArray((N - 1, O))),      # too few rows
                     ("dones", FakeDeviceArray((N + 1, 1), "|b1")),                                                       # too many
                     ("actions", FakeDeviceArray((N, A), strides=(4, 4 * N))),                                            # a transposed view
                     ("observations", FakeDeviceArray((N, O), strides=(0, 4)))):                                          # an expanded row
        with pytest.raises(ValueError, match=key):
            agent_mod._device_outputs(ENGINE, N, {key: bad}, alloc=fake_alloc)
    with pytest.raises(ValueError, match="unknown output key"):
        agent_mod._device_outputs(ENGINE, N, {"obs": FakeDeviceArray((N, O))}, alloc=fake_alloc)


def test_wrong_dtypes_and_places_are_a_type_error():
    for key, bad in (("observations", FakeDeviceArray((N, O), "<f8")), ("rewards", FakeDeviceArray((N, 1), "<f2")),
                     ("dones", FakeDeviceArray((N, 1), "<f4")), ("index", FakeDeviceArray((N,), "<i4")), ("index", FakeDeviceArray((N,), "<f8")),
                     ("actions", FakeDeviceArray((N, A), "<i4")),
                     ("actions", FakeDeviceArray((N, A), device_index=1)),          # another device's memory
                     ("rewards", np.zeros((N, 1), np.float32))):                     # host memory
        with pytest.raises(TypeError, match=key):
            agent_mod._device_outputs(ENGINE, N, {key: bad}, alloc=fake_alloc)


class StubEngine(SlotGeneration):
    """the engine as the mirror's replay buffer sees it; the device read-out raises"""

    def __init__(self):
        self.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0, batch_size=N)
        self.calls = []

    def rb_sample(self):
        self.calls.append("rb_sample")
        self.slot_refilled()

    def read_batch(self):
        self.calls.append("read_batch")
        return dict(observations=np.ones((N, O), np.float32), actions=np.zeros((N, A), np.float32), rewards=np.arange(N, dtype=np.float32),
                    next_observations=np.zeros((N, O), np.float32), dones=np.zeros(N, bool), index=np.arange(N))

    def read_batch_device(self, *a, **k):
        raise AssertionError("a default replay buffer must not take the device read-out")

    rb_read_rows_device = read_batch_device


def test_default_replay_buffer_reads_back_to_numpy_and_never_calls_the_device_entry_point():
    rb, eng = pkg.ReplayBuffer(100), StubEngine()
    assert rb.device_batches is False
    rb._bind(eng)
    batch = rb.sample(N)
    assert isinstance(batch, pkg.BatchHandle) and batch._device is False
    assert isinstance(batch["observations"], np.ndarray) and batch["rewards"].shape == (N, 1) and batch["dones"].shape == (N, 1)
    assert np.array_equal(batch["terminations"], batch["dones"]) and np.array_equal(batch["index"], np.arange(N))
    assert eng.calls == ["rb_sample", "read_batch"]                        # one read-back, cached
    with pytest.raises(AssertionError, match="device read-out"):          # ... and the stub does notice a device read-out
        pkg.BatchHandle(eng, eng.batch_generation()).on_device(out={k: fake_alloc((N,) if k == "index" else (N, w), kind)
                                                                   for k, w, kind in (("observations", O, "f4"), ("actions", A, "f4"), ("rewards", 1, "f4"),
                                                                                      ("next_observations", O, "f4"), ("dones", 1, "b1"), ("index", 1, "i8"))})


def test_device_backed_handle_asks_for_one_readout_and_goes_stale_like_the_host_one():
    class Recorder(StubEngine):
        def read_batch_device(self, fields, consumer_stream=0, ordered=True):
            self.calls.append(("read_batch_device", len(fields), consumer_stream, ordered))

    eng = Recorder()
    outs = {k: fake_alloc((N,) if k == "index" else (N, w), kind) for k, w, kind in
            (("observations", O, "f4"), ("actions", A, "f4"), ("rewards", 1, "f4"), ("next_observations", O, "f4"), ("dones", 1, "b1"), ("index", 1, "i8"))}
    h = pkg.BatchHandle(eng, eng.batch_generation(), device=True)
    got = h.on_device(out=outs)
    assert got["observations"] is outs["observations"] and got["terminations"] is outs["dones"]
    assert eng.calls == [("read_batch_device", 6, 0, True)]               # one launch for all keys; not torch: the default stream
    eng.slot_refilled()                                                    # a later refill of the slot
    with pytest.raises(pkg.StaleBatchError):
        h.on_device(out=outs)
    with pytest.raises(pkg.StaleBatchError):
        h["observations"]
    assert len(eng.calls) == 1
