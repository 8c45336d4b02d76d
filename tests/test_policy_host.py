"""CPU: everything of the policy query that needs no GPU -- the header's three declarations and the field list of sactd3_policy_io
against the ctypes binding, the NULL-engine behaviour of the three entry points, how Engine.policy_device / Engine.policy fill the
struct (against a recording library), how Agent.policy routes its rows and names its keys (on stand-ins that carry
__cuda_array_interface__), and the refusals of loop / launcher; policy_stats=0 makes no call."""
import argparse
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, engine as engine_mod, launcher, loop
from tests.helpers import FakeDeviceArray, SlotGeneration

O, A = 11, 3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sactd3.h")
NAMES = ("sactd3_policy_device", "sactd3_policy", "sactd3_policy_stats")
IO = ("actions", "eps", "mode", "mean", "log_std", "sample", "sample_logp", "action_logp", "eps_out")


# ------------------------------------------------------------------------------------------ header, binding, NULL engine
def test_header_declares_the_three_symbols_and_the_struct():
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(sactd3_engine\*", text, re.M), name
    body = re.search(r"typedef struct sactd3_policy_io \{(.*?)\} sactd3_policy_io;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const float\*|float\*|int64_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [x for f in IO for x in (f, f + "_ld")]
    assert [t for t, _ in fields] == [t for f in IO for t in ("const float*" if f in ("actions", "eps") else "float*", "int64_t")]
    assert "#define SACTD3_PI_ONLINE 0" in text and "#define SACTD3_PI_TARGET 1" in text and "#define SACTD3_ABI_VERSION 1" in text
    assert "SACTD3_STREAM_POLICY  0x400u" in open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "philox.h")).read()


def test_the_binding_covers_them():
    assert [f for f, _ in _lib.POLICY_IO_FIELDS] == list(IO)
    assert [n for n, _ in _lib.CPolicyIO._fields_] == [x for f in IO for x in (f, f + "_ld")]
    assert C.sizeof(_lib.CPolicyIO) == 9 * 16 and (_lib.PI_ONLINE, _lib.PI_TARGET) == (0, 1)
    lib = pkg.load_library()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "pi_z2" in lib.sactd3_debug_names().decode().split()


def test_null_engine_is_refused_without_a_device():
    lib = pkg.load_library()
    io, st, buf = _lib.CPolicyIO(), (C.c_int64 * 4)(), (C.c_float * 64)()
    io.mode, io.mode_ld = 4096, A
    assert lib.sactd3_policy_device(None, C.c_void_p(8192), O, 4, _lib.PI_ONLINE, C.byref(io), None, _lib.SRC_ORDERED) == _lib.EINVAL
    assert lib.sactd3_policy(None, buf, 4, _lib.PI_ONLINE, C.byref(io)) == _lib.EINVAL
    assert lib.sactd3_policy_stats(None, st) == _lib.EINVAL


# ------------------------------------------------------------------------------------------ Engine.policy* against a recording library
class RecordingLib:
    def __init__(self, fill=None):
        self.calls, self.fill = [], fill

    def _io(self, ref):
        io = ref._obj
        return {n: getattr(io, n) for n, _ in _lib.CPolicyIO._fields_}

    def sactd3_policy_device(self, h, obs, obs_ld, n, which, io, stream, flags):
        self.calls.append(("device", obs.value, obs_ld, n, which, self._io(io), stream.value, flags))
        return 0

    def sactd3_policy(self, h, obs, n, which, io):
        d = self._io(io)
        self.calls.append(("host", n, which, d))
        for k, name in enumerate(IO[2:]):                    # every wanted output gets its own value
            if d[name]:
                width = 1 if name.endswith("_logp") else A
                np.ctypeslib.as_array(C.cast(d[name], C.POINTER(C.c_float)), (n * width,))[:] = k + 1
        return 0

    def sactd3_policy_stats(self, h, out):
        out[0], out[1], out[2], out[3] = 5, 70, 2, 1
        return 0

    def sactd3_last_error(self, h):
        return b"?"


def engine(td3=False):
    eng = engine_mod.Engine.__new__(engine_mod.Engine)
    eng.lib, eng._h = RecordingLib(), C.c_void_p(1)
    eng.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0, prefer_td3_over_sac=td3)
    return eng


def test_engine_policy_device_fills_the_struct_field_by_field():
    eng = engine()
    eng.policy_device(0x1000, O + 2, 9, {"mode": (0x2000, A), "action_logp": (0x3000, 1), "actions": (0x4000, A + 1)}, stream=77)
    kind, obs, obs_ld, n, which, io, stream, flags = eng.lib.calls[0]
    assert (kind, obs, obs_ld, n, which, stream, flags) == ("device", 0x1000, O + 2, 9, _lib.PI_ONLINE, 77, _lib.SRC_ORDERED)
    want = {n: (None if not n.endswith("_ld") else 0) for n, _ in _lib.CPolicyIO._fields_}
    want.update(mode=0x2000, mode_ld=A, action_logp=0x3000, action_logp_ld=1, actions=0x4000, actions_ld=A + 1)
    assert io == want
    eng.policy_device(0x1000, O, 9, {"mode": (0x2000, A)}, target=True, ordered=False)
    assert eng.lib.calls[1][4] == _lib.PI_TARGET and eng.lib.calls[1][7] == 0 and eng.lib.calls[1][6] is None
    with pytest.raises(ValueError, match="unknown field"):
        eng.policy_device(0x1000, O, 9, {"logp": (0x2000, 1)})
    assert len(eng.lib.calls) == 2


def test_engine_policy_asks_for_the_outputs_the_arguments_imply():
    obs = np.zeros((6, O), np.float32)
    eng = engine()
    assert set(eng.policy(obs)) == {"mode", "mean", "log_std"}
    assert set(eng.policy(obs, sample=True)) == {"mode", "mean", "log_std", "sample", "sample_logp", "eps_out"}
    got = eng.policy(obs, actions=np.zeros((6, A)), eps=np.zeros((6, A)))
    assert set(got) == {"mode", "mean", "log_std", "sample", "sample_logp", "eps_out", "action_logp"}
    assert got["mode"].shape == (6, A) and got["sample_logp"].shape == (6,) and got["action_logp"].shape == (6,)
    assert all((got[name] == k + 1).all() for k, name in enumerate(IO[2:]))
    io = eng.lib.calls[-1][3]
    assert io["actions"] and io["eps"] and io["actions_ld"] == A and io["sample_logp_ld"] == 1 and eng.lib.calls[-1][1:3] == (6, _lib.PI_ONLINE)
    assert eng.lib.calls[0][3]["actions"] is None and eng.lib.calls[0][3]["eps"] is None and eng.lib.calls[0][3]["sample"] is None
    with pytest.raises(ValueError, match="rows"):
        eng.policy(obs, actions=np.zeros((5, A)))
    td3 = engine(td3=True)
    assert set(td3.policy(obs, target=True)) == {"mode"} and td3.lib.calls[0][2] == _lib.PI_TARGET
    assert eng.policy_stats() == dict(calls=5, rows=70, rows_clamped=2, rows_nan=1)


# ------------------------------------------------------------------------------------------ Agent.policy against a recording engine
class RecordingEngine(SlotGeneration):
    device_inputs = True
    policy_outputs = engine_mod.Engine.policy_outputs

    def __init__(self, td3=False):
        self.cfg = SimpleNamespace(ob_dim=O, ac_dim=A, device_id=0, prefer_td3_over_sac=td3)
        self.calls, self.host_calls = [], []

    def policy_device(self, *args):
        self.calls.append(args)

    def policy(self, obs, actions, eps, sample, target):
        self.host_calls.append((obs, actions, eps, sample, target))
        n = obs.shape[0]
        names = self.policy_outputs(bool(sample) or eps is not None, actions is not None)
        return {f: np.full((n,) if f.endswith("_logp") else (n, A), k, np.float32) for k, f in enumerate(names)}


def mirror(eng=None):
    ag = agent_mod.Agent.__new__(agent_mod.Agent)
    ag.engine = eng or RecordingEngine()
    return ag


def outs(n, *keys):
    return {k: FakeDeviceArray((n, 1 if k.endswith("log_prob") else A)) for k in keys}


def test_device_rows_go_to_the_engine_where_they_are():
    ag, obs, act = mirror(), FakeDeviceArray((8, O), strides=(4 * (O + 5), 4)), FakeDeviceArray((8, A))
    out = outs(8, "mode", "mean", "log_std", "log_prob")
    out["mode"] = FakeDeviceArray((8, A), strides=(4 * (A + 4), 4))
    got = ag.policy({"observations": obs, "actions": act}, out=out)
    assert set(got) == {"mode", "mean", "log_std", "log_prob"} and all(got[k] is out[k] for k in got)
    (optr, old, n, io, target, stream), = ag.engine.calls
    assert (optr, old, n, target, stream) == (obs.ptr, O + 5, 8, False, 0)
    assert io == {"actions": (act.ptr, A), "mode": (out["mode"].ptr, A + 4), "mean": (out["mean"].ptr, A), "log_std": (out["log_std"].ptr, A),
                  "action_logp": (out["log_prob"].ptr, 1)}
    assert ag.engine.host_calls == [] and ag.engine.batch_generation() == 5 and obs.log == []


def test_sample_and_eps_name_the_sample_keys():
    ag, obs, eps = mirror(), FakeDeviceArray((8, O)), FakeDeviceArray((8, A))
    keys = ("mode", "mean", "log_std", "sample", "sample_log_prob", "eps")
    got = ag.policy({"observations": obs}, sample=True, out=outs(8, *keys))
    assert tuple(got) == keys
    io = ag.engine.calls[0][3]
    assert set(io) == {"mode", "mean", "log_std", "sample", "sample_logp", "eps_out"}
    got = ag.policy({"observations": obs}, eps=eps, out=outs(8, *keys))           # given draws: a sample without `sample=True`
    io = ag.engine.calls[1][3]
    assert tuple(got) == keys and io["eps"] == (eps.ptr, A) and "eps_out" in io
    td3 = mirror(RecordingEngine(td3=True))
    assert tuple(td3.policy({"observations": obs}, target=True, out=outs(8, "mode"))) == ("mode",) and td3.engine.calls[0][4] is True


def test_what_the_device_route_cannot_take():
    ok = dict(observations=FakeDeviceArray((8, O)), actions=FakeDeviceArray((8, A)))
    ok_out = outs(8, "mode", "mean", "log_std", "log_prob")
    eng = RecordingEngine()
    with pytest.raises(TypeError, match="all"):                            # mixed residency
        mirror(eng).policy(dict(ok, actions=np.zeros((8, A), np.float32)), out=ok_out)
    with pytest.raises(TypeError, match="all"):
        mirror(eng).policy(ok, eps=torch.zeros(8, A), out=ok_out)
    with pytest.raises(TypeError, match="device"):
        mirror(eng).policy(dict(ok, actions=FakeDeviceArray((8, A), device_index=1)), out=ok_out)
    with pytest.raises(ValueError, match="rows"):
        mirror(eng).policy(dict(ok, actions=FakeDeviceArray((7, A))), out=ok_out)
    with pytest.raises(ValueError, match="unknown output"):                # a key this call does not fill
        mirror(eng).policy(ok, out=dict(ok_out, sample=FakeDeviceArray((8, A))))
    with pytest.raises(TypeError, match="mode"):
        mirror(eng).policy(ok, out=dict(ok_out, mode=FakeDeviceArray((8, A), "<f8")))
    with pytest.raises(ValueError, match="log_prob"):
        mirror(eng).policy(ok, out=dict(ok_out, log_prob=FakeDeviceArray((8, 2))))
    with pytest.raises(TypeError, match="out"):
        mirror(eng).policy({"observations": np.zeros((8, O), np.float32)}, out=ok_out)
    off = RecordingEngine()
    off.device_inputs = False
    with pytest.raises(TypeError, match="device_inputs"):
        mirror(off).policy(ok, out=ok_out)
    assert eng.calls == [] and eng.host_calls == [] and off.calls == []


def test_host_rows_take_the_host_call_and_come_back_as_numpy():
    ag = mirror()
    obs, act = np.ones((4, O), np.float64), torch.zeros(4, A)
    got = ag.policy({"observations": obs, "actions": act}, sample=True)
    assert list(got) == ["mode", "mean", "log_std", "sample", "sample_log_prob", "eps", "log_prob"]
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in got.values())
    assert got["mode"].shape == (4, A) and got["sample_log_prob"].shape == (4, 1) and got["log_prob"].shape == (4, 1)
    assert (got["sample_log_prob"] == 4).all() and (got["eps"] == 5).all() and (got["log_prob"] == 6).all()
    (o_, a_, e_, sample, target), = ag.engine.host_calls
    assert np.array_equal(o_, obs) and np.array_equal(a_, act.numpy()) and e_ is None and sample is True and target is False
    assert ag.engine.calls == [] and ag.engine.batch_generation() == 5


# ------------------------------------------------------------------------------------------ loop, launcher
class OfflineAgent:
    """what loop.train_offline needs of an agent; a policy query or a row read-out is an error unless allowed"""

    def __init__(self, td3=False, allow=False):
        self.engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=td3), ran=[],
                                      run_iterations=lambda i, n: self.engine.ran.append((i, n)), read_metrics=lambda: {"loss/qf_loss": 1.0})
        self.qnet_updates_so_far = self.actor_updates_so_far = 0
        self.allow, self.asked = allow, []
        self.rb = self

    def __len__(self):
        return 100

    def rows(self, index):
        assert self.allow
        index = np.asarray(index)
        assert index.dtype == np.int64 and index.min() >= 0 and index.max() < 100
        self.asked.append(index)
        return {"observations": np.zeros((len(index), O), np.float32), "actions": np.zeros((len(index), A), np.float32)}

    def policy(self, td, sample=False):
        assert self.allow and sample and set(td) == {"observations", "actions"}
        n = len(td["observations"])
        return {"log_prob": np.full((n, 1), -2.0, np.float32), "sample_log_prob": np.full((n, 1), -3.0, np.float32), "log_std": np.full((n, A), -1.0, np.float32)}


def test_policy_stats_0_makes_no_call_and_n_reads_n_rows_per_evaluation():
    cfg = SimpleNamespace(seed=3)
    ag = OfflineAgent()
    assert loop.train_offline(cfg, ag, num_updates=6, eval_every_updates=3) == {"loss/qf_loss": 1.0}
    assert loop.train_offline(cfg, ag, num_updates=6, eval_every_updates=3, policy_stats=0) == {"loss/qf_loss": 1.0}
    assert ag.asked == [] and ag.engine.ran == [(0, 3), (3, 3)] * 2
    on = OfflineAgent(allow=True)
    got = loop.train_offline(cfg, on, num_updates=6, eval_every_updates=3, policy_stats=16)
    assert got == {"loss/qf_loss": 1.0, "vitals/replay_log_prob": -2.0, "vitals/policy_entropy": 3.0, "vitals/log_std_mean": -1.0}
    assert [len(i) for i in on.asked] == [16, 16] and not np.array_equal(*on.asked) and on.engine.ran == [(0, 3), (3, 3)]
    again = OfflineAgent(allow=True)                                       # the generator is the run's own: same seed, same rows
    loop.train_offline(cfg, again, num_updates=6, eval_every_updates=3, policy_stats=16)
    assert all(np.array_equal(x, y) for x, y in zip(on.asked, again.asked))


def test_loop_and_launcher_refuse_what_has_no_sac_policy():
    cfg = SimpleNamespace(seed=0)
    td3 = OfflineAgent(td3=True)
    with pytest.raises(ValueError, match="SAC"):
        loop.train_offline(cfg, td3, num_updates=6, policy_stats=16)
    with pytest.raises(ValueError, match="SAC"):
        loop.train(cfg, None, td3, policy_stats=16)
    with pytest.raises(ValueError, match=">= 0"):
        loop.train_offline(cfg, OfflineAgent(), num_updates=6, policy_stats=-1)
    assert td3.engine.ran == [] and td3.asked == []
    assert launcher.policy_stats_plan(argparse.Namespace(algo="sac", policy_stats=64)) == 64
    assert launcher.policy_stats_plan(argparse.Namespace(algo="td3", policy_stats=0)) == 0
    with pytest.raises(ValueError, match="--algo sac"):
        launcher.policy_stats_plan(argparse.Namespace(algo="td3", policy_stats=64))
    with pytest.raises(ValueError, match=">= 0"):
        launcher.policy_stats_plan(argparse.Namespace(algo="sac", policy_stats=-1))
    with pytest.raises(ValueError, match="sac"):                           # before anything is built
        launcher.run_job("td3", "Hopper-v4", 0, 0, "unused", policy_stats=64)
    with pytest.raises(SystemExit):                                        # the parent refuses before any worker starts
        launcher.main(["--algo", "td3", "--policy_stats", "64", "--dry-run"])
