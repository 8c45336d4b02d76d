"""CPU: the host side of the dormant-neuron scan and ReDo (include/sactd3_dormant.h) -- the header, the binding and the built library
cover each other; what the calls refuse without a device; the keyword rules of `dormant` / `redo_every` in loop.train /
loop.train_offline and the launcher's flags, each asked before an agent is touched."""
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
    with open(os.path.join(ROOT, "include", "sactd3_dormant.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.DORMANT_SYMBOLS)
    enum = {k: int(v) for k, v in re.findall(r"(SACTD3_DORMANT_[A-Z]+)\s*=\s*(\d+)", code)}
    assert enum == {"SACTD3_DORMANT_ACTOR": _lib.DORMANT_ACTOR, "SACTD3_DORMANT_CRITICS": _lib.DORMANT_CRITICS}
    assert "0xA00" in header and len(_lib.DORMANT_PAIRS) == 6 and _lib.ABI_VERSION == 1
    P.build_library()
    raw = C.CDLL(P.library_path())
    assert all(hasattr(raw, name) for name in _lib.DORMANT_SYMBOLS)
    lib = P.load_library()
    assert lib.sactd3_redo.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32]


def test_a_null_handle_is_refused():
    lib = P.load_library()
    assert lib.sactd3_dormant_scan_device(None, (C.c_int64 * 4)(), 1, 4, 3, 0.025, None, None, 0) == _lib.EINVAL
    assert lib.sactd3_redo(None, 3, 0, 1) == _lib.EINVAL and lib.sactd3_dormant_stats(None, (C.c_int64 * 16)()) == _lib.EINVAL


BAD = [(dict(redo_every=50), "needs dormant"), (dict(dormant=dict(rows=64), redo_every=50, reset_every=50), "exclude"),
       (dict(dormant=dict(rows=64), redo_every=0), "redo_every"), (dict(dormant=dict(rows=64), redo_every=5, redo_what=("alpha",)), "redo_what"),
       (dict(dormant=dict(tau=0.1)), "rows"), (dict(dormant=dict(rows=64, tau=-1.0)), "tau"), (dict(dormant=dict(rows=1 << 20)), "rows")]


@pytest.mark.parametrize("change,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(change, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), **change)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, **change)


def test_train_offline_ends_its_runs_where_a_redo_is_due():
    """a stub agent: the runs end at every multiple of redo_every and at the evaluation points, one scan + recycle each, and a run that
    never resets records no vitals/resets"""
    runs, calls = [], []
    engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {},
                             run_iterations=lambda i, n: runs.append((i, n)))
    agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, recycles_so_far=0,
                            dormant=lambda **kw: calls.append(("scan", agent.qnet_updates_so_far, kw.get("what"))) or {"actor": 0.25, "critics": 0.5})
    agent.recycle_dormant = lambda what: calls.append(("redo", agent.qnet_updates_so_far, what)) or setattr(agent, "recycles_so_far", agent.recycles_so_far + 1)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=25, eval_every_updates=10, dormant=dict(rows=8), redo_every=8, redo_what=("critics",))
    assert runs == [(0, 8), (8, 2), (10, 6), (16, 4), (20, 4), (24, 1)]
    assert [c for c in calls if c[2]] == [(k, n, ("critics",)) for n in (8, 16, 24) for k in ("scan", "redo")]
    assert "vitals/resets" not in out and out["vitals/recycled"] == 3 and out["vitals/dormant_critics"] == 0.5


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    assert not {"dormant", "redo_every"} & set(plain)
    kw = launcher.train_keywords(cfg, **base, dormant=1024, dormant_tau=0.1, redo_every=500)
    assert kw["dormant"] == dict(rows=1024, tau=0.1) and kw["redo_every"] == 500
    assert {k: v for k, v in kw.items() if k not in ("dormant", "redo_every")} == plain
    with pytest.raises(ValueError, match="needs dormant"):
        launcher.train_keywords(cfg, **base, redo_every=500)
