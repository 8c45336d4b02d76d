"""CPU: the host side of coloured exploration noise (include/sactd3_noise.h) -- the header, the binding and the built library cover each
other; the keyword rules of `exploration_beta` / `exploration_len` in loop.train and the launcher's flags, each asked before an agent
or an env is touched."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=8, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)
NATIVE = dict(native_rollout=True, collected_rollout=True)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other():
    with open(os.path.join(ROOT, "include", "sactd3_noise.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.NOISE_SYMBOLS)
    assert "0xB00" in header and _lib.STREAM_COLORED == 0xB00 and _lib.ABI_VERSION == 1
    P.build_library()
    raw = C.CDLL(P.library_path())
    assert all(hasattr(raw, name) for name in _lib.NOISE_SYMBOLS)
    lib = P.load_library()
    assert lib.sactd3_colored_noise_device(None, 1.0, 64, 1, 0, 0, None, 1, None, 0) == _lib.EINVAL
    assert lib.sactd3_rollout_noise_configure(None, 1.0, 64) == _lib.EINVAL and lib.sactd3_rollout_collect_colored(None, 1, None, None) == _lib.EINVAL


BAD = [(dict(exploration_beta=1.0), "needs collected_rollout"), (dict(exploration_beta=2.5, **NATIVE), "exploration_beta"),
       (dict(exploration_beta=float("nan"), **NATIVE), "exploration_beta"), (dict(exploration_beta=1.0, exploration_len=96, **NATIVE), "power of two"),
       (dict(exploration_beta=1.0, exploration_len=32, **NATIVE), "power of two"), (dict(exploration_beta=1.0, exploration_len=8192, **NATIVE), "power of two"),
       (dict(exploration_beta=1.0, exploration_len=64, segment_len=128, **NATIVE), "segment_len")]


@pytest.mark.parametrize("change,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_anything_is_touched(change, word):
    change = dict(change)
    cfg = SimpleNamespace(**{**CFG, **({"segment_len": change.pop("segment_len")} if "segment_len" in change else {})})
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), **change)


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=True,
                native_rollout=True, policy_stats=0, collected_rollout=True)
    plain = launcher.train_keywords(cfg, **base)
    assert not {"exploration_beta", "exploration_len"} & set(plain)
    kw = launcher.train_keywords(cfg, **base, exploration_beta=1.0)
    assert kw["exploration_beta"] == 1.0 and "exploration_len" not in kw
    kw = launcher.train_keywords(cfg, **base, exploration_beta=0.5, exploration_len=1024)
    assert kw["exploration_beta"] == 0.5 and kw["exploration_len"] == 1024
    assert {k: v for k, v in kw.items() if not k.startswith("exploration_")} == plain
    with pytest.raises(ValueError, match="needs collected_rollout"):
        launcher.train_keywords(cfg, **{**base, "collected_rollout": False}, exploration_beta=1.0)
    args = SimpleNamespace(prioritized=False, n_step=1, one_launch=False, updates_per_step=1, overlap_acting=False, device_env=True, native_rollout=True,
                           policy_stats=0, algo="sac", collected_rollout=True, exploration_beta=1.0, exploration_len=128)
    flags = launcher.mode_flags(args, {})
    assert flags["exploration_beta"] == 1.0 and flags["exploration_len"] == 128
    args.exploration_beta = None
    with pytest.raises(ValueError, match="needs --exploration_beta"):
        launcher.mode_flags(args, {})
