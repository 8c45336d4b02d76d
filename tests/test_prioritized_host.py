"""CPU: everything of the prioritised route that needs no GPU -- how ReplayBuffer.sample_at, Agent.update_qnets with a "_weight" key and
Agent.td_errors hand their arrays to the engine (pointers, strides, conversions, refusals; on stand-ins that carry
__cuda_array_interface__, against a recording engine), the batch generation, the header / binding of the four entry points, their
NULL-engine behaviour, and the sampling law of loop.ProportionalSampler."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, loop
from tests.helpers import FakeDeviceArray, SlotGeneration, five

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, B = 11, 3, 8
NEW = ("sactd3_rb_sample_indices_device", "sactd3_batch_weights_device", "sactd3_td_errors_device", "sactd3_priority_stats")


class RecordingEngine(SlotGeneration):
    """what the three methods need of an engine; records what it is handed, in order"""
    device_inputs = True

    def __init__(self):
        self.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0, batch_size=B)
        self.calls = []

    def rb_sample_indices_device(self, *args):
        self.calls.append(("index",) + args)
        self.slot_refilled()

    def batch_weights_device(self, *args):
        self.calls.append(("weights",) + args)

    def td_errors_device(self, *args):
        self.calls.append(("td",) + args)

    def load_batch_device(self, fields, n, stream):
        self.calls.append(("load", n))
        self.slot_refilled()

    def update_qnets(self):
        self.calls.append(("update_qnets",))


def buffer(engine=None, **kw):
    rb = agent_mod.ReplayBuffer(64, **kw)
    rb._bind(engine or RecordingEngine())
    return rb


def mirror(engine=None):
    ag = agent_mod.Agent.__new__(agent_mod.Agent)          # the methods under test read `engine` (and the metric plumbing below) only
    ag.engine = engine or RecordingEngine()
    ag._metric_tensors = None
    return ag


def index(n=B, **kw):
    return FakeDeviceArray((n,), "<i8", **kw)


class Sliceable(FakeDeviceArray):
    def __getitem__(self, key):
        return ("rows", key)


# ------------------------------------------------------------------------------------------ the header and the binding
def test_header_declares_and_the_binding_covers_the_four_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sactd3.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for name in NEW + ("sactd3_batch_generation",):
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.sactd3_batch_generation.restype is C.c_int64
    assert "#define SACTD3_ABI_VERSION 1" in src and lib.sactd3_abi_version() == 1


def test_null_engine_is_refused_without_a_device():
    lib = pkg.load_library()
    st = (C.c_int64 * 4)()
    assert lib.sactd3_rb_sample_indices_device(None, C.c_void_p(4096), 1, C.c_void_p(8192), 1, B, None, _lib.SRC_ORDERED) == _lib.EINVAL
    assert lib.sactd3_batch_weights_device(None, C.c_void_p(8192), 1, B, None, _lib.SRC_ORDERED) == _lib.EINVAL
    assert lib.sactd3_td_errors_device(None, C.c_void_p(4096), 1, B, None, _lib.DST_ORDERED) == _lib.EINVAL
    assert lib.sactd3_priority_stats(None, st) == _lib.EINVAL
    assert lib.sactd3_batch_generation(None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------ ReplayBuffer.sample_at
def test_sample_at_hands_index_and_weights_over_where_they_are():
    """weights as [B] and as [B, 1]: the same call; no weights: address 0; not a torch array: the default stream"""
    for wshape in ((B,), (B, 1)):
        rb, idx, w = buffer(), index(), FakeDeviceArray(wshape)
        handle = rb.sample_at(idx, w)
        assert rb._engine.calls == [("index", idx.ptr, 1, w.ptr, 1, B, 0)]
        assert isinstance(handle, agent_mod.BatchHandle) and handle._is_current() and not handle._device
        assert idx.log == [] and w.log == []                                # nothing converted
    rb, idx = buffer(), index()
    rb.sample_at(idx)
    assert rb._engine.calls == [("index", idx.ptr, 1, 0, 1, B, 0)]
    assert buffer(device_batches=True).sample_at(index())._device            # the handle honours device_batches


def test_sample_at_keeps_strided_views():
    """every third element of a longer index, a column of a [B, 5] weight matrix: strides in elements, nothing copied"""
    rb = buffer()
    idx, w = index(strides=(8 * 3,)), FakeDeviceArray((B, 1), strides=(4 * 5, 4))
    rb.sample_at(idx, w)
    assert rb._engine.calls == [("index", idx.ptr, 3, w.ptr, 5, B, 0)] and idx.log == [] and w.log == []
    rb, w = buffer(), FakeDeviceArray((B,), strides=(4 * 7,))
    rb.sample_at(index(), w)
    assert rb._engine.calls[0][3:5] == (w.ptr, 7)


def test_sample_at_converts_weights_on_the_device():
    """not float32 -> .to(float32); a stride that is not whole elements -> .contiguous(); FakeDeviceArray.cpu() raises"""
    for bad, log in ((FakeDeviceArray((B,), "<f8"), [("to", "float32")]), (FakeDeviceArray((B, 1), "<f2"), [("to", "float32")]),
                     (FakeDeviceArray((B,), strides=(6,)), ["contiguous"])):
        made = []
        for name in ("to", "contiguous"):
            def spy(self, *a, _f=getattr(FakeDeviceArray, name)):
                made.append(_f(self, *a))
                return made[-1]
            setattr(bad, name, spy.__get__(bad))
        rb = buffer()
        rb.sample_at(index(), bad)
        call, = rb._engine.calls
        assert made and made[-1].log == log and call[3] == made[-1].ptr != bad.ptr and call[4] == 1


def test_sample_at_refusals():
    eng = RecordingEngine()
    for bad in (FakeDeviceArray((B,), device_index=1), np.ones(B, np.float32), torch.ones(B)):      # another GPU's memory, host arrays
        with pytest.raises(TypeError, match="device"):
            buffer(eng).sample_at(index(), bad)
    for bad in (FakeDeviceArray((B + 1,)), FakeDeviceArray((B - 1, 1))):                               # wrong row counts
        with pytest.raises(ValueError, match="expected 8 weights"):
            buffer(eng).sample_at(index(), bad)
    with pytest.raises(ValueError, match="weights"):                                                   # not a column
        buffer(eng).sample_at(index(), FakeDeviceArray((B, 2)))
    for n in (B - 1, B + 1):
        with pytest.raises(ValueError, match="expected 8 indices"):
            buffer(eng).sample_at(index(n))
    assert eng.calls == [] and eng.batch_generation() == 5                                              # nothing reached the engine
    with pytest.raises(AssertionError, match="attached"):
        agent_mod.ReplayBuffer(64).sample_at(index())


def test_sample_at_bumps_the_generation_and_older_handles_go_stale():
    eng = RecordingEngine()
    rb, ag = buffer(eng), mirror(eng)
    first = rb.sample_at(index(), FakeDeviceArray((B,)))
    assert eng.batch_generation() == 6 and first._is_current()
    second = rb.sample_at(index())
    assert eng.batch_generation() == 7 and second._is_current() and not first._is_current()
    with pytest.raises(agent_mod.StaleBatchError):
        ag.update_qnets(first)
    with pytest.raises(agent_mod.StaleBatchError):
        first["observations"]
    ag.update_qnets(second)                                                  # a sample_at handle carries its weights: nothing is staged again
    assert [c[0] for c in eng.calls] == ["index", "index", "update_qnets"]


# ------------------------------------------------------------------------------------------ Agent.update_qnets with "_weight"
def batch_of(**over):
    obs, act, rew, nobs, done = five(B)
    return dict(dict(observations=obs, actions=act, rewards=rew, next_observations=nobs, dones=done), **over)


def test_update_qnets_stages_weight_key_behind_the_batch():
    for wshape, strides, ld in (((B,), None, 1), ((B, 1), None, 1), ((B, 1), (4 * 9, 4), 9)):
        ag, w = mirror(), FakeDeviceArray(wshape, strides=strides)
        got = ag.update_qnets(batch_of(_weight=w))
        assert ag.engine.calls == [("load", B), ("weights", w.ptr, ld, B, 0), ("update_qnets",)] and list(got) == ["loss/qf_loss"]
        assert ag.engine.batch_generation() == 6                              # a caller-owned batch replaces the slot
    ag = mirror()
    ag.update_qnets(batch_of())                                              # no key: as before
    ag.update_qnets(None)
    assert ag.engine.calls == [("load", B), ("update_qnets",), ("update_qnets",)]


def test_update_qnets_asks_the_mappings_keys_not_the_mapping():
    """a TensorDict refuses `key in td` (NotImplementedError) and wants `key in td.keys()`: batches of that kind, weighted or not"""
    class KeysOnly(dict):
        def __contains__(self, key):
            raise NotImplementedError("use `key in td.keys()`")
    ag, w = mirror(), FakeDeviceArray((B,))
    ag.update_qnets(KeysOnly(batch_of(_weight=w)))
    ag.update_qnets(KeysOnly(batch_of()))
    assert ag.engine.calls == [("load", B), ("weights", w.ptr, 1, B, 0), ("update_qnets",), ("load", B), ("update_qnets",)]


def test_update_qnets_weight_conversions_and_refusals():
    ag, w = mirror(), FakeDeviceArray((B,), "<f8")
    ag.update_qnets(batch_of(_weight=w))
    assert ag.engine.calls[1][0] == "weights" and ag.engine.calls[1][1] != w.ptr and ag.engine.calls[1][2:4] == (1, B)
    with pytest.raises(TypeError, match="device"):
        mirror().update_qnets(batch_of(_weight=FakeDeviceArray((B,), device_index=1)))
    with pytest.raises(TypeError, match="device"):
        mirror().update_qnets(batch_of(_weight=np.ones(B, np.float32)))
    ag = mirror()
    with pytest.raises(ValueError, match="expected 8 weights"):
        ag.update_qnets(batch_of(_weight=FakeDeviceArray((B + 3,))))
    assert ("update_qnets",) not in ag.engine.calls                         # no update on a batch whose weights were refused


# ------------------------------------------------------------------------------------------ Agent.td_errors
def test_td_errors_addresses_out_like_q_values():
    ag, out = mirror(), FakeDeviceArray((2, B, 1))
    assert ag.td_errors(out=out) is out
    assert ag.engine.calls == [("td", out.ptr, 1, B, 0)]                     # pointer, row stride, critic stride, the default stream
    ag, out = mirror(), FakeDeviceArray((2, B, 1), strides=(4 * 33, 4 * 3, 4))   # a [2, B, 1] window of a [2, 11, 3] array
    ag.td_errors(out=out)
    assert ag.engine.calls == [("td", out.ptr, 3, 33, 0)]
    ag, out = mirror(), Sliceable((2, B + 4, 1))                             # more rows than the batch: the first B are returned
    assert ag.td_errors(out=out) == ("rows", (slice(None), slice(None, B)))
    assert ag.engine.calls == [("td", out.ptr, 1, B + 4, 0)]
    assert ag.engine.batch_generation() == 5                                  # a read-out: handles stay current


def test_td_errors_refusals():
    eng = RecordingEngine()
    for bad in (FakeDeviceArray((2, B, 1), device_index=1), FakeDeviceArray((2, B, 1), "<f8"), np.zeros((2, B, 1), np.float32)):
        with pytest.raises(TypeError, match="out"):
            mirror(eng).td_errors(out=bad)
    for bad in (FakeDeviceArray((2, B - 1, 1)), FakeDeviceArray((2, B)), FakeDeviceArray((1, B, 1)), FakeDeviceArray((2, B, 2)),
                FakeDeviceArray((2, B, 1), strides=(0, 4, 4)), FakeDeviceArray((2, B, 1), strides=(32, 2, 4))):
        with pytest.raises(ValueError, match="out"):
            mirror(eng).td_errors(out=bad)
    assert eng.calls == []


def test_td_errors_surfaces_the_engines_state_error():
    class Refusing(RecordingEngine):
        def td_errors_device(self, *args):
            raise pkg.EngineError("libsactd3_hip error -3: td_errors_device: no critic update has run on the rows now in the batch slot")
    with pytest.raises(pkg.EngineError, match="-3"):
        mirror(Refusing()).td_errors(out=FakeDeviceArray((2, B, 1)))


# ------------------------------------------------------------------------------------------ loop.ProportionalSampler
def test_train_with_a_sampler_needs_the_call_by_call_loop():
    with pytest.raises(ValueError, match="fused=False"):
        loop.train(SimpleNamespace(), None, None, fused=True, sampler=loop.ProportionalSampler(8))


def test_new_rows_enter_at_the_current_maximum_priority():
    s = loop.ProportionalSampler(6, alpha=1.0, beta=1.0, eps=0.0, device="cpu")
    s.extend(4)
    assert s.len == 4 and s.cursor == 4 and s.priorities.tolist() == [1, 1, 1, 1, 0, 0]
    s.update(torch.tensor([1, 2]), torch.tensor([[[0.5], [-3.0]], [[-0.25], [2.0]]]))       # max over critics of |td|
    assert s.priorities.tolist() == [1, 0.5, 3, 1, 0, 0] and float(s.max_priority) == 3.0
    s.extend(3)                                                              # wraps: slots 4, 5, 0
    assert s.len == 6 and s.cursor == 1 and s.priorities.tolist() == [3, 0.5, 3, 1, 3, 3]


def test_sampled_frequencies_follow_priority_to_the_alpha():
    """After update() with known TD errors, slot i is drawn with P(i) = p_i^alpha / sum_j p_j^alpha.  N = 200 000 independent draws
    (multinomial with replacement, torch seed 0): the count of slot i is Binomial(N, P(i)), standard error sqrt(N P(i) (1 - P(i))).
    Bound: 5 standard errors per slot -- a correct sampler exceeds that on one of 8 slots with probability < 8 x 5.8e-7."""
    torch.manual_seed(0)
    n, alpha, eps, draws = 8, 0.6, 1e-3, 200_000
    s = loop.ProportionalSampler(n, alpha=alpha, beta=0.4, eps=eps, device="cpu")
    s.extend(n)
    td = torch.tensor([0.1, -0.2, 0.4, -0.8, 1.6, -3.2, 6.4, 0.05])
    s.update(torch.arange(n), torch.stack([td, 0.5 * td]).reshape(2, n, 1))
    p = (td.abs().double() + eps) ** alpha
    P = (p / p.sum()).numpy()
    idx, w = s.sample(draws)
    assert idx.dtype == torch.int64 and idx.shape == (draws,) and w.shape == (draws,) and w.dtype == torch.float32
    counts = np.bincount(idx.numpy(), minlength=n)
    se = np.sqrt(draws * P * (1.0 - P))
    z = np.abs(counts - draws * P) / se
    print("P", P, "counts", counts, "z", z)
    assert (z <= 5.0).all(), z
    # the importance weights: (N P(i))^-beta, scaled so that the batch's largest is 1
    want = (n * P[idx.numpy()]) ** -0.4
    np.testing.assert_allclose(w.numpy(), want / want.max(), rtol=1e-5)
    assert float(w.max()) == 1.0 and float(w.min()) > 0.0
