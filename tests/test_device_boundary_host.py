"""CPU: the routing helper of the mirror (agent.py:_device_route) on stand-ins that carry __cuda_array_interface__ -- which route
five arrays take, and what pointer / row stride the device route hands to the engine -- and the NULL-engine behaviour of the three
device-boundary entry points.  No GPU is touched: the helper only reads the interface dictionaries."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod
from tests.helpers import FakeDeviceArray, five

O, A = 11, 3
ENGINE = SimpleNamespace(device_inputs=True, cfg=SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0))


def test_contiguous_fields_go_to_the_device_as_they_are():
    xs = five()
    fields, n, keep = agent_mod._device_route(ENGINE, *xs)
    assert n == 8 and fields == [(xs[0].ptr, O), (xs[1].ptr, A), (xs[2].ptr, 1), (xs[3].ptr, O), (xs[4].ptr, 1)]
    assert all(k is x for k, x in zip(keep, xs))                 # nothing converted


def test_row_strided_fields_keep_their_stride():
    W = 2 * O + A + 6
    xs = five(obs=FakeDeviceArray((8, O), strides=(4 * W, 4)), act=FakeDeviceArray((8, A), strides=(4 * W, 4)),
              rew=FakeDeviceArray((8, 1), strides=(4 * W, 4)), done=FakeDeviceArray((8, 1), "|b1", strides=(3, 1)))
    fields, n, keep = agent_mod._device_route(ENGINE, *xs)
    assert n == 8 and [f[1] for f in fields] == [W, W, W, O, 3]
    assert [f[0] for f in fields] == [x.ptr for x in xs] and all(k is x for k, x in zip(keep, xs))


def test_column_vectors_and_flat_vectors_are_the_same_thing():
    for shape in ((8,), (8, 1)):
        xs = five(rew=FakeDeviceArray(shape), done=FakeDeviceArray(shape, "|u1"))
        fields, n, keep = agent_mod._device_route(ENGINE, *xs)
        assert n == 8 and fields[2] == (xs[2].ptr, 1) and fields[4] == (xs[4].ptr, 1)
    # a strided flat vector: the row stride is its only stride
    xs = five(rew=FakeDeviceArray((8,), strides=(20,)))
    assert agent_mod._device_route(ENGINE, *xs)[0][2] == (xs[2].ptr, 5)
    # one row: whatever the library reports as its stride, the width will do
    xs = five(n=1, obs=FakeDeviceArray((1, O), strides=(4, 4)))
    fields, n, keep = agent_mod._device_route(ENGINE, *xs)
    assert n == 1 and fields[0] == (xs[0].ptr, O)


def test_conversions_happen_on_the_device():
    xs = five(obs=FakeDeviceArray((8, O), "<f8"),                              # not float32 -> .to(float32)
              act=FakeDeviceArray((8, A), strides=(4, 32)),                    # a transposed view: inner stride != 1 -> .contiguous()
              nobs=FakeDeviceArray((8, O), strides=(0, 4)),                    # an expanded row: stride below the width -> .contiguous()
              done=FakeDeviceArray((8, 1), "<f4"))                             # float flags -> != 0
    fields, n, keep = agent_mod._device_route(ENGINE, *xs)
    assert n == 8 and [f[1] for f in fields] == [O, A, 1, O, 1]
    assert keep[0].log == [("to", "float32")] and keep[1].log == ["contiguous"] and keep[3].log == ["contiguous"] and keep[4].log == ["!= 0"]
    assert keep[2] is xs[2]
    assert [f[0] for f in fields] == [k.ptr for k in keep]                    # the converted copies are what the engine reads


def test_anything_else_takes_the_host_route():
    host = [np.zeros((8, O), np.float32), np.zeros((8, A), np.float32), np.zeros(8, np.float32), np.zeros((8, O), np.float32), np.zeros(8, bool)]
    assert agent_mod._device_route(ENGINE, *host) is None                     # numpy only
    for k in range(5):                                                         # mixed
        xs = five()
        xs[k] = host[k]
        assert agent_mod._device_route(ENGINE, *xs) is None
    assert agent_mod._device_route(ENGINE, *five(act=FakeDeviceArray((8, A), device_index=1))) is None      # another device
    off = SimpleNamespace(device_inputs=False, cfg=ENGINE.cfg)
    assert agent_mod._device_route(off, *five()) is None                      # switched off
    assert agent_mod._device_route(ENGINE, *five(n=0)) is None                # nothing to read


def test_shapes_that_fit_no_field_are_an_error():
    with pytest.raises(ValueError, match="expected"):
        agent_mod._device_route(ENGINE, *five(obs=FakeDeviceArray((8, O + 1))))
    with pytest.raises(ValueError, match="rows"):
        agent_mod._device_route(ENGINE, *five(rew=FakeDeviceArray((7,))))


def test_null_engine_is_refused_without_a_device():
    lib = pkg.load_library()
    f, st = _lib.CDeviceFields(), (C.c_int64 * 4)()
    assert lib.sactd3_rb_extend_fields_device(None, C.byref(f), 4, None, _lib.SRC_ORDERED) < 0
    assert lib.sactd3_load_batch_device(None, C.byref(f), 4, None, 0) < 0
    assert lib.sactd3_boundary_stats(None, st) < 0
    assert C.sizeof(_lib.CDeviceFields) == 80 and _lib.CDeviceFields.dones_ld.offset == 72      # five (pointer, int64) pairs
