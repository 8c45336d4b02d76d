"""CPU: the host side of the candidate-scoring call (include/sactd3_action_values.h) -- the header, the binding and the built library
cover each other; the keyword rule of `ood_gap` in loop.train / loop.train_offline and the launcher's flags, each asked before an agent
is touched."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other():
    with open(os.path.join(ROOT, "include", "sactd3_action_values.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.ACTION_VALUES_SYMBOLS)
    struct = re.search(r"typedef struct sactd3_action_values_io \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == [n for n, _ in _lib.CActionValuesIO._fields_]
    assert (int(re.search(r"SACTD3_AV_POLICY\s+(\d)", code).group(1)), int(re.search(r"SACTD3_AV_UNIFORM\s+(\d)", code).group(1))) == (_lib.AV_POLICY, _lib.AV_UNIFORM)
    assert len(_lib.AV_SUMMARY) == 8 and _lib.ABI_VERSION == 1
    lib = P.load_library()
    assert lib.sactd3_action_values_device(None, None, 1, 1, 16, 0, 0, 0.2, 1.0, C.byref(_lib.CActionValuesIO()), None, 0) == _lib.EINVAL
    assert lib.sactd3_action_values_stats(None, (C.c_int64 * 8)()) == _lib.EINVAL


BAD = [(dict(candidates=16), "rows"), (dict(rows=0), "rows"), (dict(rows=64, candidates=24), "candidates"), (dict(rows=64, tau=1.0), "must be a dict")]


@pytest.mark.parametrize("spec,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(spec, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), ood_gap=spec)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, ood_gap=spec)


def test_off_makes_no_call_and_on_records_the_vitals():
    calls = []
    engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {}, run_iterations=lambda i, n: None)
    got = {"ood_gap_policy": 0.5, "ood_gap_uniform": 1.5, "value_sampled": -2.0}
    agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, ood_gap=lambda **kw: calls.append(kw) or got)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10)
    assert not calls and not any(k.startswith("vitals/ood") for k in out)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10, ood_gap=dict(rows=64, candidates=32))
    assert calls == [dict(rows=64, candidates=32)] * 2
    assert {k: out[k] for k in loop.OodGap.KEYS} == {"vitals/ood_gap_policy": 0.5, "vitals/ood_gap_uniform": 1.5, "vitals/value_sampled": -2.0}


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    kw = launcher.train_keywords(cfg, **base, ood_gap=256, ood_candidates=64)
    assert "ood_gap" not in plain and kw["ood_gap"] == dict(rows=256, candidates=64)
    assert {k: v for k, v in kw.items() if k != "ood_gap"} == plain
    for bad in (dict(ood_candidates=16), dict(ood_gap=256, ood_candidates=20)):
        with pytest.raises(ValueError, match="ood_"):
            launcher.train_keywords(cfg, **base, **bad)
