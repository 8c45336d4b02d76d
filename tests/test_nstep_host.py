"""CPU: what of the n-step staging needs no GPU -- the numpy restatement (tests/nstep_ref.py) against a direct episode-bookkeeping loop
over rollouts of loop.SyntheticVecEnv, hand-computed returns and masks, the header / binding / NULL-engine behaviour of the new entry
points, and the refusals of ReplayBuffer and loop.train."""
import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, loop
from tests import nstep_ref as nref
from tests.helpers import SlotGeneration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sactd3_rb_sample_nstep_device", "sactd3_rb_sample_nstep", "sactd3_rb_sample_prioritized_nstep", "sactd3_nstep_info_device",
       "sactd3_nstep_stats")
# (ob_dim, ac_dim, envs, horizon, term_at)
SETTINGS = ((11, 3, 4, 50, 4.0), (17, 6, 4, 50, 4.0), (11, 3, 4, 7, 2.5), (11, 3, 3, 7, 2.5))
STEPS = (1, 2, 3, 5, 16)
ENV_STEPS = 600
GAMMA = 0.99


@functools.lru_cache(maxsize=None)
def rollout(setting):
    """600 env steps with random actions, stored as Rollout.advance stores them (a truncated env's next observation is its true final
    one) -> the five fields in append order, and per row whether its episode ended there (terminated or truncated)"""
    o, a, n, horizon, term_at = setting
    env = loop.SyntheticVecEnv(o, a, n, horizon=horizon, term_at=term_at)
    obs, _ = env.reset(seed=1)
    obs = np.asarray(obs, np.float32)
    rows = [[], [], [], [], []]
    ended, counts = [], [0, 0]
    for _ in range(ENV_STEPS):
        act = env.action_space.sample()
        arrived, rew, term, trunc, infos = env.step(act)
        arrived = np.asarray(arrived, np.float32)
        stored = arrived.copy()
        for k in np.flatnonzero(trunc):
            stored[k] = np.asarray(infos["final_observation"][k], np.float32)
        for f, v in zip(rows, (obs, np.asarray(act, np.float32), np.asarray(rew, np.float32), stored, np.asarray(term, np.float32))):
            f.append(v)
        ended.append(np.asarray(term) | np.asarray(trunc))
        counts[0] += int(np.sum(term)); counts[1] += int(np.sum(trunc))
        obs = arrived
    return tuple(np.concatenate(f) for f in rows), np.concatenate(ended), tuple(counts)


def bookkeeping_k(ended, row, steps, stride, newest_row):
    """min(steps, rows to the episode's end, rows available), walking the rows of one env in append order"""
    k = 1
    while k < steps and not ended[row] and row + stride <= newest_row:
        row += stride
        k += 1
    return k


@pytest.mark.parametrize("setting", SETTINGS)
def test_chain_length_equals_episode_bookkeeping_on_an_unwrapped_ring(setting):
    fields, ended, (terms, truncs) = rollout(setting)
    stride = setting[2]
    n = len(ended)
    assert terms + truncs > 0
    cap = n + 37
    (obs, _, rew, nobs, done), length, cursor = nref.place(fields, cap)
    assert (length, cursor) == (n, n)
    for steps in STEPS:
        got = nref.chains(obs, nobs, rew, done, np.arange(n), steps, stride, length, cursor, cap, GAMMA)
        want = [bookkeeping_k(ended, r, steps, stride, n - 1) for r in range(n)]
        assert np.array_equal(got["k"], want), (steps, np.flatnonzero(got["k"] != want)[:8])
        assert np.array_equal(got["last"], np.arange(n) + (got["k"] - 1) * stride)


@pytest.mark.parametrize("setting", SETTINGS)
def test_chain_length_equals_episode_bookkeeping_on_a_wrapped_ring(setting):
    """a capacity that is no multiple of the stride: the oldest rows are overwritten, slot = row % cap"""
    fields, ended, _ = rollout(setting)
    stride = setting[2]
    n = len(ended)
    cap = 1001
    assert n > cap and cap % stride != 0
    (obs, _, rew, nobs, done), length, cursor = nref.place(fields, cap)
    assert length == cap and cursor == n % cap
    held = np.arange(n - cap, n)                                       # the rows the ring still holds, oldest first
    for steps in STEPS:
        got = nref.chains(obs, nobs, rew, done, held % cap, steps, stride, length, cursor, cap, GAMMA)
        want = [bookkeeping_k(ended, r, steps, stride, n - 1) for r in held]
        assert np.array_equal(got["k"], want), (steps, np.flatnonzero(got["k"] != want)[:8])
        assert np.array_equal(got["last"], (held + (got["k"] - 1) * stride) % cap)


def test_hand_computed_return_and_mask_of_a_three_row_chain():
    f = np.float32
    s = np.arange(8, dtype=np.float32).reshape(4, 2)
    obs, nobs = s[:3].copy(), s[1:].copy()                             # row t+1 starts where row t arrived
    rew = f([1.0, 2.0, 4.0])
    g = f(0.5)
    for d_last in (0.0, 1.0):
        done = f([0.0, 0.0, d_last])
        k, last, R, m = nref.chain(obs, nobs, rew, done, 0, 3, 1, 3, 3, 8, g)
        assert (k, last) == (3, 2) and R == f(1.0 + 0.5 * 2.0 + 0.25 * 4.0) == f(3.0)
        assert m == (f(1.0) if d_last else f(0.75))                    # 1 - (1 - d) * 0.25; exactly 1.0 on termination
        assert nref.bits(m) == nref.bits(f(1.0) if d_last else f(0.75))
    # k = 1: the mask is d itself, whatever steps asks for (the chain is cut by the flag) and for steps == 1
    done = f([1.0, 0.0, 0.0])
    assert nref.chain(obs, nobs, rew, done, 0, 3, 1, 3, 3, 8, g) == (1, 0, f(1.0), f(1.0))
    assert nref.chain(obs, nobs, rew, f([0, 0, 0]), 0, 1, 1, 3, 3, 8, g) == (1, 0, f(1.0), f(0.0))
    # the length rule: the newest row has no successor; a refused index
    assert nref.chain(obs, nobs, rew, f([0, 0, 0]), 2, 3, 1, 3, 3, 8, g)[:2] == (1, 2)
    assert nref.chain(obs, nobs, rew, f([0, 0, 0]), 1, 3, 1, 3, 3, 8, g)[:2] == (2, 2)
    assert nref.chain(obs, nobs, rew, f([0, 0, 0]), 3, 3, 1, 3, 3, 8, g) == (0, -1, f(0.0), f(0.0))
    assert nref.chain(obs, nobs, rew, f([0, 0, 0]), -1, 3, 1, 3, 3, 8, g)[0] == 0
    # bit comparison: -0.0 against +0.0 breaks the link, equal NaN patterns keep it
    o2, n2 = obs.copy(), nobs.copy()
    n2[0, 1], o2[1, 1] = -0.0, 0.0
    assert nref.chain(o2, n2, rew, f([0, 0, 0]), 0, 3, 1, 3, 3, 8, g)[0] == 1
    n2[0, 1] = o2[1, 1] = np.nan
    assert nref.chain(o2, n2, rew, f([0, 0, 0]), 0, 3, 1, 3, 3, 8, g)[0] == 3


def test_header_declares_and_the_binding_covers_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "sactd3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert '"batch_from_index_nstep"' in text and "SACTD3_ABI_VERSION 1" in text


def test_null_engine_is_an_error_code_not_a_crash():
    lib = pkg.load_library()
    out = (C.c_int64 * 4)()
    assert lib.sactd3_rb_sample_nstep_device(None, None, 1, None, 1, 1, 3, 1, None, 0) == _lib.EINVAL
    assert lib.sactd3_rb_sample_nstep(None, 3, 1) == _lib.EINVAL
    assert lib.sactd3_rb_sample_prioritized_nstep(None, 0.4, 3, 1) == _lib.EINVAL
    assert lib.sactd3_nstep_info_device(None, None, 1, None, 1, None, 0) == _lib.EINVAL
    assert lib.sactd3_nstep_stats(None, out) == _lib.EINVAL


class RecordingEngine(SlotGeneration):
    def __init__(self):
        self.cfg = SimpleNamespace(batch_size=8, device_id=0)
        self.calls = []

    def prio_enable(self, alpha, eps):
        self.calls.append(("enable", alpha, eps))

    def rb_sample(self):
        self.calls.append(("sample",))
        self.slot_refilled()

    def rb_sample_nstep(self, steps, stride):
        self.calls.append(("sample_nstep", steps, stride))
        self.slot_refilled()

    def rb_sample_prioritized(self, beta):
        self.calls.append(("prio", beta))
        self.slot_refilled()

    def rb_sample_prioritized_nstep(self, beta, steps, stride):
        self.calls.append(("prio_nstep", beta, steps, stride))
        self.slot_refilled()


def test_replay_buffer_refuses_bad_n_step_before_it_touches_the_engine():
    rb = agent_mod.ReplayBuffer(64)                                    # not attached: touching the engine would be an AssertionError
    for call in (lambda **kw: rb.sample(8, **kw), lambda **kw: rb.sample_at([0] * 8, **kw), lambda **kw: rb.sample_prioritized(8, 0.4, **kw)):
        with pytest.raises(ValueError, match="stride"):
            call(n_step=3)
        for bad in (0, 17, -1):
            with pytest.raises(ValueError, match=r"\[1, 16\]"):
                call(n_step=bad, stride=4)
        with pytest.raises(ValueError, match="stride"):
            call(n_step=3, stride=0)
    with pytest.raises(TypeError):
        rb.sample(8, 3, 4)                                             # keyword-only
    eng = RecordingEngine()
    rb._bind(eng)
    rb.enable_priorities()
    h1 = rb.sample(8)
    assert eng.calls[-1] == ("sample",) and not h1._n_step             # n_step == 1: exactly today's call
    assert rb.sample(8, n_step=1, stride=4) is not None and eng.calls[-1] == ("sample",)
    h3 = rb.sample(8, n_step=3, stride=4)
    assert eng.calls[-1] == ("sample_nstep", 3, 4) and h3._n_step and h3._is_current() and not h1._is_current()
    assert eng.batch_generation() == 8                                  # bumped once per sampling call
    rb.sample_prioritized(8, 0.5)
    assert eng.calls[-1] == ("prio", 0.5)
    hp = rb.sample_prioritized(8, 0.5, n_step=16, stride=2)
    assert eng.calls[-1] == ("prio_nstep", 0.5, 16, 2) and hp._n_step
    with pytest.raises(agent_mod.StaleBatchError):
        h3.n_step_info()
    with pytest.raises(RuntimeError, match="n_step"):
        rb.sample(8).n_step_info()


def test_train_rejects_n_step_with_the_fused_iteration():
    cfg = SimpleNamespace(seed=0, learning_starts=0, action_repeat=1, segment_len=1, num_envs=1, num_timesteps=0, batch_size=8)
    with pytest.raises(ValueError, match="fused=False"):
        loop.train(cfg, None, None, fused=True, n_step=3)
    for bad in (0, 17):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            loop.train(cfg, None, None, fused=False, n_step=bad)
