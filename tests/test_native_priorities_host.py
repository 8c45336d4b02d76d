"""CPU: what of the engine-owned priorities needs no GPU -- the numpy restatement (tests/priorities_ref.py) against torch float64, the
header / binding / NULL-engine behaviour of the new entry points, and the refusals of loop.train and ReplayBuffer."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, loop
from tests import priorities_ref as pref
from tests.helpers import SlotGeneration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sactd3_prio_enable", "sactd3_rb_sample_prioritized", "sactd3_prio_set_uniforms", "sactd3_prio_update_from_td",
       "sactd3_prio_update_device", "sactd3_prio_stats")


def test_restatement_selects_what_torch_float64_selects():
    """np.searchsorted(cumsum, m, side='right') against torch.cumsum / torch.searchsorted(right=True) in float64: random priorities
    (zeros among them), random uniforms and the edge values 0 and the largest below 1."""
    rng = np.random.default_rng(0)
    for n, length in ((2500, 2500), (5000, 2500), (1024, 1024), (1, 1)):
        leaf = rng.uniform(0.1, 1.0, n).astype(np.float32)
        leaf[rng.integers(0, n, n // 10)] = 0.0
        leaf[0] = leaf[length - 1] = 0.5
        u = np.concatenate([rng.random(300).astype(np.float32), np.float32([0.0, pref.U_MAX])])
        got = pref.select(leaf, length, u)
        c = torch.cumsum(torch.as_tensor(leaf[:length], dtype=torch.float64), 0)
        m = torch.as_tensor((u * np.float32(c[-1].item())).astype(np.float32), dtype=torch.float64)
        want = torch.searchsorted(c, m, right=True).numpy()
        assert np.array_equal(got, want)
        assert (got >= 0).all() and (got < length).all() and (leaf[got] > 0).all()      # a zero-priority slot is never drawn
    assert np.array_equal(pref.select(np.zeros(8, np.float32), 8, np.float32([0.3])), [-1])


def test_restatement_of_weights_write_back_and_uniforms():
    leaf = np.float32([1, 2, 0, 1, 4])
    w = pref.weights(leaf, 5, [0, 1, 4], 1.0)
    assert np.allclose(w, [1.0, 0.5, 0.25]) and np.array_equal(pref.weights(leaf, 5, [0, 1, 4], 0.0), [1, 1, 1])
    out = pref.write_back(leaf, [1, 3, 1], [9.0, 0.0, 4.0], 0.5)
    assert np.allclose(out, [1, 2.0, 0, 0, 4])                       # slot 1: the later position (4 -> 2) wins; 0 excludes slot 3
    assert np.allclose(pref.td_priorities([[1.0, -3.0], [-2.0, 0.5]], 0.25), [2.25, 3.25])
    assert np.allclose(pref.group_sums(np.ones(2500)), [1024, 1024, 452])
    u = pref.native_uniforms(3, 0, 64)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all() and len(set(u.tolist())) == 64
    assert not np.array_equal(u, pref.native_uniforms(3, 1, 64)) and np.array_equal(u[:40], pref.native_uniforms(3, 0, 40))
    assert abs(pref.chi2_quantile(15, 0.5) - 14.339) < 0.05 and abs(pref.chi2_quantile(15, 0.999) - 37.697) < 0.2      # (table values)
    assert 50.0 < pref.chi2_quantile(15, 1 - 1e-6) < 60.0


def test_header_declares_and_the_binding_covers_the_new_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sactd3.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name


def test_null_engine_is_an_error_code_not_a_crash():
    lib = pkg.load_library()
    out = (C.c_int64 * 4)()
    assert lib.sactd3_prio_enable(None, 0.6, 1e-6) == _lib.EINVAL
    assert lib.sactd3_rb_sample_prioritized(None, 0.4) == _lib.EINVAL
    assert lib.sactd3_prio_set_uniforms(None, None, 0) == _lib.EINVAL
    assert lib.sactd3_prio_update_from_td(None) == _lib.EINVAL
    assert lib.sactd3_prio_update_device(None, None, 1, None, 1, 1, None, 0) == _lib.EINVAL
    assert lib.sactd3_prio_stats(None, out) == _lib.EINVAL


def test_train_rejects_prioritized_with_the_fused_iteration_or_a_sampler():
    cfg = SimpleNamespace(seed=0, learning_starts=0, action_repeat=1, segment_len=1, num_envs=1, num_timesteps=0, batch_size=8)
    with pytest.raises(ValueError, match="fused=False"):
        loop.train(cfg, None, None, fused=True, prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6))
    with pytest.raises(ValueError, match="exclude"):
        loop.train(cfg, None, None, fused=False, prioritized=dict(alpha=0.6), sampler=loop.ProportionalSampler(16, device="cpu"))
    with pytest.raises(ValueError, match="unknown keys"):
        loop.train(cfg, None, None, fused=False, prioritized=dict(gamma=1.0))


class RecordingEngine(SlotGeneration):
    def __init__(self):
        self.cfg = SimpleNamespace(batch_size=8, device_id=0)
        self.calls = []

    def prio_enable(self, alpha, eps):
        self.calls.append(("enable", alpha, eps))

    def rb_sample_prioritized(self, beta):
        self.calls.append(("sample", beta))
        self.slot_refilled()

    def prio_update_from_td(self):
        self.calls.append(("from_td",))


def test_replay_buffer_wants_enable_priorities_first_and_bumps_the_generation():
    rb = agent_mod.ReplayBuffer(64)
    with pytest.raises(RuntimeError, match="enable_priorities"):
        rb.sample_prioritized(8, 0.4)
    with pytest.raises(RuntimeError, match="enable_priorities"):
        rb.update_priorities()
    with pytest.raises(ValueError):
        rb.enable_priorities(alpha=-1.0)
    rb.enable_priorities(alpha=0.7, eps=1e-3)            # before the agent exists: remembered, made when the engine is bound
    eng = RecordingEngine()
    rb._bind(eng)
    assert eng.calls == [("enable", 0.7, 1e-3)]
    h = rb.sample_prioritized(8, 0.5)
    assert eng.calls[-1] == ("sample", 0.5) and eng.batch_generation() == 6 and h._is_current()      # as sample_at does
    rb.update_priorities()
    assert eng.calls[-1] == ("from_td",)
    with pytest.raises(ValueError, match="both"):
        rb.update_priorities(index=[1, 2])
    rb2 = agent_mod.ReplayBuffer(64, device_batches=True)
    rb2._bind(eng)
    rb2.enable_priorities()
    assert eng.calls[-1] == ("enable", 0.6, 1e-6) and rb2.sample_prioritized(8, 0.4)._device
