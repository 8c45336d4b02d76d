"""CPU: what of the one-launch prioritised / n-step iteration needs no GPU -- the argument mapping of Engine.step_sampled, Agent.iteration
and loop.train(one_launch=True) onto a recording stub engine, the refusals of loop.train, the handle generation, and the header /
binding / NULL-engine behaviour of the two entry points."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as pkg
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, engine as engine_mod, loop
from tests.helpers import SlotGeneration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sactd3_step_sampled", "sactd3_step_sampled_stats")


def test_header_declares_and_the_binding_covers_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "sactd3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    # the struct on both sides of the ABI: four 32-bit words in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} sactd3_sampling;", src).group(1)
    assert re.findall(r"(int32_t|float)\s+(\w+);", body) == [("int32_t", "draw"), ("int32_t", "n_step"), ("int32_t", "stride"), ("float", "beta")]
    assert [n for n, _ in _lib.CSampling._fields_] == ["draw", "n_step", "stride", "beta"] and C.sizeof(_lib.CSampling) == 16
    assert re.search(r"SACTD3_DRAW_UNIFORM = 0, SACTD3_DRAW_PRIORITIZED = 1", src) and (_lib.DRAW_UNIFORM, _lib.DRAW_PRIORITIZED) == (0, 1)


def test_null_arguments_are_error_codes_not_crashes():
    lib = pkg.load_library()
    out = (C.c_int64 * 4)()
    sm = _lib.CSampling(_lib.DRAW_PRIORITIZED, 3, 4, 0.4)
    assert lib.sactd3_step_sampled(None, 1, C.byref(sm)) == _lib.EINVAL and lib.sactd3_step_sampled(None, 1, None) == _lib.EINVAL
    assert lib.sactd3_step_sampled_stats(None, out) == _lib.EINVAL


class RawLib:
    """stands where the ctypes library stands: records what Engine.step_sampled hands to the C ABI"""

    def __init__(self):
        self.calls = []

    def sactd3_step_sampled(self, h, do_actor, sm):
        s = sm._obj
        self.calls.append((do_actor, s.draw, s.n_step, s.stride, round(float(s.beta), 6)))
        return 0

    def sactd3_step_sampled_stats(self, h, out):
        out[0], out[1], out[2], out[3] = 9, 2, 0, 0
        return 0


def test_engine_step_sampled_fills_the_struct():
    eng = object.__new__(engine_mod.Engine)
    eng.lib, eng._h = RawLib(), 1
    eng.step_sampled(True, beta=0.5, n_step=3, stride=4)
    eng.step_sampled(False, n_step=2, stride=8)                        # beta None: the uniform draw
    eng.step_sampled(0, beta=0.0)
    assert eng.lib.calls == [(1, _lib.DRAW_PRIORITIZED, 3, 4, 0.5), (0, _lib.DRAW_UNIFORM, 2, 8, 0.0), (0, _lib.DRAW_PRIORITIZED, 1, 1, 0.0)]
    with pytest.raises(TypeError):
        eng.step_sampled(True, 0.5)                                    # keyword-only
    assert eng.step_sampled_stats() == dict(launches=9, graph_captures=2)
    eng._h = None                                                      # (nothing for __del__ to destroy)


class RecordingEngine(SlotGeneration):
    def __init__(self, delay=2):
        self.cfg = SimpleNamespace(batch_size=8, device_id=0, actor_update_delay=delay)
        self.calls = []

    def step(self, do_actor):
        self.calls.append(("step", do_actor))
        self.slot_refilled()

    def step_sampled(self, do_actor, *, beta=None, n_step=1, stride=1):
        self.calls.append(("step_sampled", do_actor, beta, n_step, stride))
        self.slot_refilled()

    def prio_enable(self, alpha, eps):
        self.calls.append(("enable", alpha, eps))

    def rb_sample_prioritized(self, beta):
        self.calls.append(("prio", beta))
        self.slot_refilled()

    def read_metrics(self):
        return {"loss/qf_loss": 0.0}


def stub_agent(delay=2):
    ag = object.__new__(agent_mod.Agent)
    ag.engine = RecordingEngine(delay)
    ag.qnet_updates_so_far = ag.actor_updates_so_far = ag.timesteps_so_far = 0
    ag.rb = agent_mod.ReplayBuffer(64)
    ag.rb._bind(ag.engine)
    return ag


def test_agent_iteration_maps_its_keywords_and_keeps_the_counters():
    ag = stub_agent()
    eng = ag.engine
    ag.iteration(0)
    ag.iteration(1)
    assert eng.calls == [("step", True), ("step", False)]             # no keyword: exactly today's call
    ag.iteration(2, beta=0.4)
    ag.iteration(3, beta=0.7, n_step=3, stride=4)
    ag.iteration(4, n_step=2, stride=8)
    assert eng.calls[2:] == [("step_sampled", False, 0.4, 1, 1), ("step_sampled", True, 0.7, 3, 4), ("step_sampled", False, None, 2, 8)]
    assert (ag.qnet_updates_so_far, ag.actor_updates_so_far) == (5, 4) and eng.batch_generation() == 10
    n = len(eng.calls)
    with pytest.raises(ValueError, match="stride"):
        ag.iteration(5, n_step=3)                                      # as ReplayBuffer.sample
    with pytest.raises(ValueError, match="stride"):
        ag.iteration(5, beta=0.4, n_step=3, stride=0)
    for bad in (0, 17):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            ag.iteration(5, n_step=bad, stride=4)
    with pytest.raises(TypeError):
        ag.iteration(5, 0.4)                                           # keyword-only
    assert len(eng.calls) == n and ag.qnet_updates_so_far == 5 and eng.batch_generation() == 10      # refused before the engine is touched


def test_an_old_batch_handle_is_stale_behind_a_prioritised_iteration():
    ag = stub_agent()
    ag.rb.enable_priorities()
    h = ag.rb.sample_prioritized(8, 0.4)
    assert h._is_current()
    ag.iteration(0, beta=0.4)
    assert not h._is_current()
    with pytest.raises(agent_mod.StaleBatchError):
        h["observations"]


def test_train_one_launch_issues_agent_iteration(monkeypatch):
    def no_env(*a, **kw):
        while True:
            yield
    monkeypatch.setattr(loop, "segment", no_env)
    cfg = SimpleNamespace(seed=0, learning_starts=8, action_repeat=1, segment_len=1, num_envs=4, num_timesteps=27, batch_size=8,
                          eval_every=10 ** 9, actor_update_delay=2)
    for kw, want in ((dict(prioritized=dict(alpha=0.7, beta=0.5, eps=1e-3)), (0.5, 1, 1)),
                     (dict(n_step=3), (None, 3, 4)),
                     (dict(prioritized=dict(beta=0.6), n_step=3), (0.6, 3, 4))):
        ag = stub_agent()
        assert loop.train(cfg, None, ag, fused=False, one_launch=True, **kw) == {"loss/qf_loss": 0.0}
        calls = ag.engine.calls
        if "prioritized" in kw:
            assert calls[0][0] == "enable" and calls[0][1] == kw["prioritized"].get("alpha", 0.6)
            calls = calls[1:]
        # iterations 0 and 1 fall before learning_starts; i = 2 .. 6 follow, the actor schedule on i itself
        assert calls == [("step_sampled", i % 3 == 0, *want) for i in range(2, 7)], (kw, calls)
        assert ag.qnet_updates_so_far == 5 and ag.actor_updates_so_far == 4


def test_train_rejects_one_launch_where_it_has_no_meaning():
    cfg = SimpleNamespace(seed=0, learning_starts=0, action_repeat=1, segment_len=1, num_envs=1, num_timesteps=0, batch_size=8)
    with pytest.raises(ValueError, match="one_launch=True needs fused=False"):
        loop.train(cfg, None, None, fused=True, one_launch=True)
    with pytest.raises(ValueError, match="one_launch=True excludes sampler"):
        loop.train(cfg, None, None, fused=False, one_launch=True, n_step=3, sampler=loop.ProportionalSampler(16, device="cpu"))
    with pytest.raises(ValueError, match="one_launch=True needs prioritized"):
        loop.train(cfg, None, None, fused=False, one_launch=True)
    with pytest.raises(ValueError, match="one_launch=True needs prioritized"):
        loop.train(cfg, None, None, fused=False, one_launch=True, n_step=1)


def test_launcher_passes_one_launch_through():
    import inspect
    from sac_td3_cudagraphs_pytorch_amd import launcher
    assert "one_launch" in inspect.signature(launcher.run_job).parameters
    src = inspect.getsource(launcher)
    assert "--one_launch" in src and "one_launch=args.one_launch" in src and "one_launch=one_launch" in src
