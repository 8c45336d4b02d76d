"""CPU: the host side of the feature-rank call (include/sactd3_feature_rank.h) -- the header, the binding and the built library cover
each other; the reference's summary formulas on hand-made spectra; the keyword rules of `feature_rank` in loop.train /
loop.train_offline and the launcher's flags, each asked before an agent is touched."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop
from tests import feature_rank_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other():
    with open(os.path.join(ROOT, "include", "sactd3_feature_rank.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.FEATURE_RANK_SYMBOLS)
    assert len(_lib.FEATURE_RANK_SUMMARY) == 8 and _lib.ABI_VERSION == 1
    lib = P.load_library()
    assert lib.sactd3_feature_rank_device(None, (C.c_int64 * 4)(), 1, 4, 3, 0.01, 1e-4, None, None, None, 0) == _lib.EINVAL
    assert lib.sactd3_feature_rank_stats(None, (C.c_int64 * 16)(), (C.c_float * 24)()) == _lib.EINVAL


def test_the_summary_formulas_on_hand_made_spectra():
    one = fm.summary(np.eye(1, 256)[0] * 9.0)
    assert (one["rank"], one["srank"], one["erank"], one["stable"]) == (1, 1, 1.0, 1.0)
    flat = fm.summary(np.full(256, 4.0), delta=0.01)
    assert flat["rank"] == 256 and flat["srank"] == 254 and flat["erank"] == pytest.approx(256.0) and flat["stable"] == pytest.approx(256.0)
    lam = np.zeros(256)
    lam[:3] = 1.0, 0.25, 0.5e-4                                               # the third lies under floor * lambda_1 = 1e-4
    cut = fm.summary(lam, delta=0.4, floor=1e-4)
    assert cut["rank"] == 2 and cut["srank"] == 1 and cut["sigma"][2] == 0.0 and cut["lambda_sum"] == pytest.approx(1.25005)
    assert cut["erank"] == pytest.approx(np.exp(-(2 / 3 * np.log(2 / 3) + 1 / 3 * np.log(1 / 3))))
    assert fm.summary(np.zeros(256))["rank"] == 0


BAD = [(dict(feature_rank=dict(delta=0.1)), "rows"), (dict(feature_rank=dict(rows=8192)), "rows"), (dict(feature_rank=dict(rows=64, delta=1.0)), "delta"),
       (dict(feature_rank=dict(rows=64, tau=0.1)), "must be a dict")]


@pytest.mark.parametrize("change,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(change, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), **change)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, **change)


def test_off_makes_no_call_and_on_records_the_vitals():
    calls = []
    engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {}, run_iterations=lambda i, n: None)
    got = {"srank_actor": 7, "srank_q1": 9, "srank_q2": 8, "erank_actor": 3.5, "erank_q1": 2.5, "erank_q2": 4.5, "rank_actor": 20, "rank_q1": 21, "rank_q2": 22,
           "converged_actor": 1, "converged_q1": 0, "converged_q2": 1}
    agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, feature_rank=lambda **kw: calls.append(kw) or got)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10)
    assert not calls and not any(k.startswith("vitals/srank") for k in out)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10, feature_rank=dict(rows=64, delta=0.05))
    assert calls == [dict(rows=64, delta=0.05)] * 2
    assert {k: out[k] for k in loop.FeatureRank.KEYS} == {"vitals/srank_actor": 7, "vitals/srank_critics": 8, "vitals/erank_actor": 3.5, "vitals/erank_critics": 2.5,
                                                            "vitals/feature_rank_converged": 0}


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    kw = launcher.train_keywords(cfg, **base, feature_rank=1024, feature_rank_delta=0.05)
    assert "feature_rank" not in plain and kw["feature_rank"] == dict(rows=1024, delta=0.05)
    assert {k: v for k, v in kw.items() if k != "feature_rank"} == plain
    for bad in (dict(feature_rank_delta=0.05), dict(feature_rank=5000)):
        with pytest.raises(ValueError, match="feature_rank"):
            launcher.train_keywords(cfg, **base, **bad)
