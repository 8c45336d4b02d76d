"""CPU: the host side of the returns-to-go call (include/sactd3_returns.h) -- the header, the binding and the built library cover each
other; the keyword rule of `mc_returns` in loop.train / loop.train_offline and the launcher's flags, each asked before an agent is
touched; the sequential model against a ten-row example written out by hand."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop
from tests import returns_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other(tmp_path):
    with open(os.path.join(ROOT, "include", "sactd3_returns.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.RETURNS_SYMBOLS)
    struct = re.search(r"typedef struct sactd3_returns_io \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == [n for n, _ in _lib.CReturnsIO._fields_]
    assert int(re.search(r"SACTD3_RTG_SPAN\s+(\d+)", code).group(1)) == _lib.RTG_SPAN and _lib.ABI_VERSION == 1
    bits = dict(re.findall(r"SACTD3_RTG_([A-Z]+) = (\d+)", code))
    assert {k: int(v) for k, v in bits.items()} == dict(TERMINATED=_lib.RTG_TERMINATED, TRUNCATED=_lib.RTG_TRUNCATED, OPEN=_lib.RTG_OPEN, START=_lib.RTG_START)
    assert (rm.TERMINATED, rm.TRUNCATED, rm.OPEN, rm.START) == (_lib.RTG_TERMINATED, _lib.RTG_TRUNCATED, _lib.RTG_OPEN, _lib.RTG_START)
    assert not set(_lib.RETURNS_SYMBOLS) & set(_lib.SYMBOLS)
    probe = tmp_path / "probe.c"
    probe.write_text('#include "sactd3_returns.h"\nint main(void) { return sizeof(sactd3_returns_io) == 0; }\n')
    subprocess.run(["cc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(probe)], check=True)
    lib = P.load_library()
    assert lib.sactd3_returns_to_go_device(None, 0.99, 1, 0, 0, C.byref(_lib.CReturnsIO()), None, 0) == _lib.EINVAL
    assert lib.sactd3_returns_to_go_stats(None, (C.c_int64 * 8)()) == _lib.EINVAL


def test_the_model_against_a_hand_written_example():
    """ten rows of two interleaved envs (stride 2) in a ring of 12 slots; env 0: rows 0 2 4 | 6 8, cut by a termination at row 4;
    env 1: rows 1 3 | 5 7 9, cut by a fresh state behind row 3.  gamma = 0.5"""
    obs = np.arange(12, dtype=np.float32).reshape(12, 1)
    nobs = obs + 2
    rew = np.array([1, 10, 2, 20, 4, -8, 1, 4, 2, 2, 0, 0], np.float32)
    done = np.zeros(12, np.float32)
    done[4], nobs[3] = 1, 99
    got = rm.returns_to_go(obs, nobs, rew, done, 0.5, 2, 10, 10, 12)
    assert got["G"][:10].tolist() == [3.0, 20.0, 4.0, 20.0, 4.0, -5.5, 2.0, 5.0, 2.0, 2.0]
    assert got["U"][:10].tolist() == [7.0, 30.0, 6.0, 20.0, 4.0, -2.0, 3.0, 6.0, 2.0, 2.0]
    assert got["A"][:10].tolist() == [3.0, 20.0, 4.0, 20.0, 4.0, 10.5, 2.0, 5.0, 2.0, 2.0]
    assert got["L"][:10].tolist() == [3, 2, 2, 1, 1, 3, 2, 2, 1, 1] and got["last"][:10].tolist() == [4, 3, 4, 3, 4, 9, 8, 9, 8, 9]
    T, R, O, S = rm.TERMINATED, rm.TRUNCATED, rm.OPEN, rm.START
    assert got["ends"][:10].tolist() == [T | S, R | S, T, R, T, O | S, O | S, O, O, O]
    sub = rm.returns_to_go(obs, nobs, rew, done, 0.5, 2, 10, 10, 12, first=1, count=4)      # rows 1 .. 4: 1 -> 3 runs into the range's end, 2 -> 4
    assert sub["rows"].tolist() == [1, 2, 3, 4] and sub["G"][1:5].tolist() == [20.0, 4.0, 20.0, 4.0] and sub["ends"][1:5].tolist() == [O | S, T | S, O, T]


BAD = [(dict(stride=2), "rows"), (dict(rows=0), "rows"), (dict(rows=64, stride=0), "stride"), (dict(rows=64, tail_tol=0.0), "tail_tol"),
       (dict(rows=64, tail_tol=float("nan")), "tail_tol"), (dict(rows=64, gamma=0.9), "must be a dict")]


@pytest.mark.parametrize("spec,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(spec, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), mc_returns=spec)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, mc_returns=spec)


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    kw = launcher.train_keywords(cfg, **base, mc_returns=256, mc_stride=4)
    assert "mc_returns" not in plain and kw["mc_returns"] == dict(rows=256, stride=4) and {k: v for k, v in kw.items() if k != "mc_returns"} == plain
    for bad in (dict(mc_stride=2), dict(mc_returns=0), dict(mc_returns=256, mc_stride=0)):
        with pytest.raises(ValueError, match="mc_returns|mc_stride|stride"):
            launcher.train_keywords(cfg, **base, **bad)
