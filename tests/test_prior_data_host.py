"""CPU: what of learning online from prior data needs no GPU -- the slot formula of the mixed draw and the pinned cursor as numpy
models (tests/mix_ref.py), the header / binding / NULL-engine behaviour of the five entry points, the argument mapping of
Engine.step_sampled, Agent.iteration, ReplayBuffer and loop.train onto recording stubs with every new ValueError, and the launcher's
plan with and without the new flags."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as pkg
from oracle.replay_ref import sample_indices
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, engine as engine_mod, launcher, loop
from tests import mix_ref
from tests.helpers import SlotGeneration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sactd3_rb_pin", "sactd3_rb_pinned", "sactd3_rb_set_mix", "sactd3_rb_sample_mixed", "sactd3_mix_stats")


# ------------------------------------------------------------------------------------------ the slot formula
@pytest.mark.parametrize("B", [1, 40, 64, 257])
def test_mixed_indices_without_pinned_rows_are_the_uniform_sample(B):
    for seed, ctr, length in ((0, 0, 1), (7, 3, 2500), (2 ** 40 + 5, 11, 1_000_000)):
        assert np.array_equal(mix_ref.mixed_indices(seed, ctr, B, 0, 0, length), sample_indices(seed, ctr, B, length))


@pytest.mark.parametrize("B,m,P,length", [(64, 32, 37, 64), (64, 0, 37, 64), (64, 64, 37, 37), (64, 63, 37, 38), (40, 1, 1, 2),
                                          (64, 16, 2500, 2504), (64, 32, 1, 1_000_000)])
def test_mixed_indices_fall_into_their_regions(B, m, P, length):
    for ctr in range(5):
        idx = mix_ref.mixed_indices(123, ctr, B, m, P, length)
        assert idx.dtype == np.int64 and idx.shape == (B,)
        assert ((0 <= idx[:m]) & (idx[:m] < P)).all() and ((P <= idx[m:]) & (idx[m:] < length)).all()
        # one word per row, shared with the uniform stream: a row's slot depends on its own region only
        w = mix_ref.index_words(123, ctr, B)
        assert np.array_equal(idx[:m], (w[:m] * np.uint64(P)) >> np.uint64(32))
        assert np.array_equal(idx[m:] - P, (w[m:] * np.uint64(length - P)) >> np.uint64(32))
    if 0 < m < B and P > 8 and length - P > 8:
        seen = np.concatenate([mix_ref.mixed_indices(5, c, B, m, P, length) for c in range(40)])
        assert len(np.unique(seen[seen < P])) > 4 and len(np.unique(seen[seen >= P])) > 4      # (it does draw, on both sides)


def test_mixed_indices_refuse_what_the_engine_refuses():
    for args in ((8, 1, 0, 10), (8, 0, 10, 10), (8, 9, 4, 10)):
        with pytest.raises(AssertionError):
            mix_ref.mixed_indices(0, 0, *args)


# ------------------------------------------------------------------------------------------ the pinned cursor
@pytest.mark.parametrize("P", [1, 37])
@pytest.mark.parametrize("region", [1, 5, 27])
def test_pinned_ring_model(P, region):
    cap = P + region
    ring = mix_ref.PinnedRing(cap)
    ring.extend(np.arange(P))                     # the prior rows: values 0 .. P - 1
    ring.pin(P)
    assert (ring.len, ring.cursor, ring.P) == (P, P, P)
    nxt, written = 1000, []
    for _ in range(20):                           # appends of 4 rows
        rows = np.arange(nxt, nxt + 4)
        ring.extend(rows)
        written += list(rows)
        nxt += 4
        assert P <= ring.cursor < cap and ring.len == min(cap, P + len(written))
        assert np.array_equal(ring.rows[:P, 0], np.arange(P))                                  # the pinned rows are untouched
        live = min(region, len(written))
        assert sorted(ring.rows[P:P + live, 0]) == written[-live:]                             # the live region holds the newest rows
        assert ring.cursor == P + len(written) % region
        assert ring.rows[P + (len(written) - 1) % region, 0] == written[-1]                    # ... the newest one in front of the cursor
    assert ring.wraps == 80 // region
    big = np.arange(5000, 5000 + region + 13)     # more rows than the live region holds: the last `region` stay
    ring.extend(big)
    written += list(big)
    assert sorted(ring.rows[P:, 0]) == written[-region:] and np.array_equal(ring.rows[:P, 0], np.arange(P))
    assert ring.len == cap and ring.cursor == P + len(written) % region


def test_pinned_ring_model_pin_on_a_full_ring_and_unpin():
    ring = mix_ref.PinnedRing(8)
    ring.extend(np.arange(8))
    assert (ring.len, ring.cursor) == (8, 0)
    ring.pin(5)
    assert ring.cursor == 5
    ring.extend([100])
    assert list(ring.rows[:, 0]) == [0, 1, 2, 3, 4, 100, 6, 7] and ring.cursor == 6
    with pytest.raises(AssertionError):
        ring.pin(8)                               # n < cap
    with pytest.raises(AssertionError):
        mix_ref.PinnedRing(8).pin(1)              # n <= len


# ------------------------------------------------------------------------------------------ the boundary
def test_header_declares_and_the_binding_covers_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "sactd3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.sactd3_rb_pin.argtypes[1] is C.c_int64 and lib.sactd3_rb_pinned.restype is C.c_int64
    assert re.search(r"SACTD3_DRAW_UNIFORM = 0, SACTD3_DRAW_PRIORITIZED = 1, SACTD3_DRAW_MIXED = 2", src) and _lib.DRAW_MIXED == 2
    # the sampling struct is what it was
    body = re.search(r"typedef struct \{([^}]*)\} sactd3_sampling;", src).group(1)
    assert re.findall(r"(int32_t|float)\s+(\w+);", body) == [("int32_t", "draw"), ("int32_t", "n_step"), ("int32_t", "stride"), ("float", "beta")]
    assert [n for n, _ in _lib.CSampling._fields_] == ["draw", "n_step", "stride", "beta"] and C.sizeof(_lib.CSampling) == 16
    # the header says what a pinned ring cannot do yet
    assert "two-region forms are a later change" in text


def test_null_engine_is_an_error_code_not_a_crash():
    lib = pkg.load_library()
    out = (C.c_int64 * 4)()
    assert lib.sactd3_rb_pin(None, 4) == _lib.EINVAL and lib.sactd3_rb_pinned(None) == _lib.EINVAL
    assert lib.sactd3_rb_set_mix(None, 4) == _lib.EINVAL and lib.sactd3_rb_sample_mixed(None) == _lib.EINVAL
    assert lib.sactd3_mix_stats(None, out) == _lib.EINVAL
    sm = _lib.CSampling(_lib.DRAW_MIXED, 1, 1, 0.0)
    assert lib.sactd3_step_sampled(None, 1, C.byref(sm)) == _lib.EINVAL


def test_the_new_kernels_live_in_a_header_of_their_own_and_end_the_manifest():
    csrc = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
    lines = [ln.strip() for ln in open(os.path.join(csrc, "kernel_instances.inc")) if ln.startswith("template __global__ ")]
    assert [ln for ln in lines if "k_mix_draw" in ln] == lines[-2:]
    assert "k_mix_draw" in open(os.path.join(csrc, "mix_kernels.h")).read()
    for f in ("kernels.h", "prio_kernels.h", "nstep_kernels.h"):
        assert "k_mix_draw" not in open(os.path.join(csrc, f)).read(), f


# ------------------------------------------------------------------------------------------ Engine.step_sampled and friends
class RawLib:
    """stands where the ctypes library stands: records what the Engine methods hand to the C ABI"""

    def __init__(self):
        self.calls = []

    def sactd3_step_sampled(self, h, do_actor, sm):
        s = sm._obj
        self.calls.append(("step_sampled", do_actor, s.draw, s.n_step, s.stride, round(float(s.beta), 6)))
        return 0

    def sactd3_rb_set_mix(self, h, m):
        self.calls.append(("set_mix", m))
        return 0

    def sactd3_rb_pin(self, h, n):
        self.calls.append(("pin", n))
        return 0

    def sactd3_rb_pinned(self, h):
        return 37

    def sactd3_rb_sample_mixed(self, h):
        self.calls.append(("sample_mixed",))
        return 0

    def sactd3_mix_stats(self, h, out):
        out[0], out[1], out[2], out[3] = 5, 160, 160, 3
        return 0


def raw_engine():
    eng = object.__new__(engine_mod.Engine)
    eng.lib, eng._h = RawLib(), 1
    return eng


def test_engine_step_sampled_issues_set_mix_only_when_the_value_changes():
    eng = raw_engine()
    M = _lib.DRAW_MIXED
    eng.step_sampled(True, prior_rows=32)
    eng.step_sampled(False, prior_rows=32)
    eng.step_sampled(False, prior_rows=16)
    eng.step_sampled(True, prior_rows=16)
    eng.step_sampled(False, prior_rows=0)
    assert eng.lib.calls == [("set_mix", 32), ("step_sampled", 1, M, 1, 1, 0.0), ("step_sampled", 0, M, 1, 1, 0.0),
                             ("set_mix", 16), ("step_sampled", 0, M, 1, 1, 0.0), ("step_sampled", 1, M, 1, 1, 0.0),
                             ("set_mix", 0), ("step_sampled", 0, M, 1, 1, 0.0)]
    n = len(eng.lib.calls)
    eng.rb_set_mix(8)                                                  # set directly: step_sampled sees it
    eng.step_sampled(False, prior_rows=8)
    assert eng.lib.calls[n:] == [("set_mix", 8), ("step_sampled", 0, M, 1, 1, 0.0)]
    n = len(eng.lib.calls)
    with pytest.raises(ValueError, match="prior_rows"):
        eng.step_sampled(True, prior_rows=8, beta=0.4)
    with pytest.raises(ValueError, match="prior_rows"):
        eng.step_sampled(True, prior_rows=8, n_step=3, stride=4)
    assert len(eng.lib.calls) == n
    eng.step_sampled(True, beta=0.5, n_step=3, stride=4)               # the other draws are what they were
    eng.step_sampled(False, n_step=2, stride=8)
    assert eng.lib.calls[n:] == [("step_sampled", 1, _lib.DRAW_PRIORITIZED, 3, 4, 0.5), ("step_sampled", 0, _lib.DRAW_UNIFORM, 2, 8, 0.0)]
    eng._h = None


def test_engine_pin_and_stats_bindings():
    eng = raw_engine()
    eng.rb_pin(37)
    eng.rb_sample_mixed()
    assert eng.lib.calls == [("pin", 37), ("sample_mixed",)] and eng.rb_pinned() == 37
    assert eng.mix_stats() == dict(mixed_draws=5, prior_rows_drawn=160, live_rows_drawn=160, pinned_wraps=3)
    eng._h = None


# ------------------------------------------------------------------------------------------ Agent.iteration, ReplayBuffer, loop.train
class RecordingEngine(SlotGeneration):
    """today's stub signatures plus the new calls; step_sampled takes prior_rows"""

    def __init__(self, delay=2, held=40):
        self.cfg = SimpleNamespace(batch_size=8, device_id=0, actor_update_delay=delay, bc_alpha=0.0, autotune=0)
        self.calls, self.held = [], held

    def step(self, do_actor):
        self.calls.append(("step", do_actor))
        self.slot_refilled()

    def step_sampled(self, do_actor, *, beta=None, n_step=1, stride=1, prior_rows=None):
        self.calls.append(("step_sampled", do_actor, beta, n_step, stride, prior_rows))
        self.slot_refilled()

    def rb_len(self):
        return self.held

    def rb_pin(self, n):
        self.calls.append(("pin", n))

    def rb_pinned(self):
        return 12

    def rb_set_mix(self, m):
        self.calls.append(("set_mix", m))
        self._mix_rows = m

    def rb_sample_mixed(self):
        self.calls.append(("sample_mixed",))
        self.slot_refilled()

    def rb_sample(self):
        self.calls.append(("sample",))
        self.slot_refilled()

    def update_qnets(self):
        self.calls.append(("qnets",))

    def update_actor(self):
        self.calls.append(("actor",))

    def update_targ_nets(self, n):
        self.calls.append(("targ", n))

    def read_metrics(self):
        return {"loss/qf_loss": 0.0}


class OldSignatureEngine(RecordingEngine):
    """an engine stub written before this change: no prior_rows keyword"""

    def step_sampled(self, do_actor, *, beta=None, n_step=1, stride=1):
        self.calls.append(("step_sampled", do_actor, beta, n_step, stride))
        self.slot_refilled()


def stub_agent(delay=2, engine=RecordingEngine):
    ag = object.__new__(agent_mod.Agent)
    ag.engine = engine(delay)
    ag.qnet_updates_so_far = ag.actor_updates_so_far = ag.timesteps_so_far = 0
    ag.td3 = True
    ag.rb = agent_mod.ReplayBuffer(64)
    ag.rb._bind(ag.engine)
    ag._stage = lambda batch: None                                     # (a handle's slot is already staged)
    ag._results = lambda keys: {}
    return ag


def test_agent_iteration_passes_prior_rows_only_when_used():
    ag = stub_agent()
    ag.iteration(0, prior_rows=4)
    ag.iteration(1, prior_rows=0)
    assert ag.engine.calls == [("step_sampled", True, None, 1, 1, 4), ("step_sampled", False, None, 1, 1, 0)]
    assert (ag.qnet_updates_so_far, ag.actor_updates_so_far) == (2, 2)
    assert ag.engine.batch_generation() == 7                           # step_sampled itself counts the new rows, not Agent.iteration
    for kw in (dict(beta=0.4), dict(n_step=3, stride=4)):
        with pytest.raises(ValueError, match="prior_rows"):
            ag.iteration(2, prior_rows=4, **kw)
    assert len(ag.engine.calls) == 2 and ag.qnet_updates_so_far == 2
    old = stub_agent(engine=OldSignatureEngine)
    old.iteration(0)
    old.iteration(1, beta=0.4)
    old.iteration(2, n_step=2, stride=8)
    assert old.engine.calls == [("step", True), ("step_sampled", False, 0.4, 1, 1), ("step_sampled", False, None, 2, 8)]


def test_replay_buffer_pin_and_sample_mixed():
    ag = stub_agent()
    rb, eng = ag.rb, ag.engine
    rb.pin()
    rb.pin(7)
    assert eng.calls == [("pin", 40), ("pin", 7)] and rb.pinned == 12 and agent_mod.ReplayBuffer(4).pinned == 0
    h0 = rb.sample_mixed(8, 4)
    h1 = rb.sample_mixed(8, 4)
    h2 = rb.sample_mixed(8, 2)
    assert eng.calls[2:] == [("set_mix", 4), ("sample_mixed",), ("sample_mixed",), ("set_mix", 2), ("sample_mixed",)]
    assert h2._is_current() and not h1._is_current() and not h0._is_current()      # through _staged: older handles go stale
    with pytest.raises(agent_mod.StaleBatchError):
        h0["observations"]
    with pytest.raises(AssertionError):
        rb.sample_mixed(16, 4)


def test_load_dataset_pins_on_request():
    class Rb:
        capacity = 64

        def __init__(self):
            self.calls, self.held = [], 0

        def __len__(self):
            return self.held

        def extend(self, td):
            self.held += len(td["observations"])
            self.calls.append(("extend", len(td["observations"])))

        def pin(self, n=None):
            self.calls.append(("pin", n))

    data = dict(observations=np.zeros((9, 3), np.float32), actions=np.zeros((9, 2), np.float32), rewards=np.zeros(9, np.float32),
                next_observations=np.zeros((9, 3), np.float32), terminations=np.zeros(9, bool))
    a, b = SimpleNamespace(rb=Rb()), SimpleNamespace(rb=Rb())
    assert loop.load_dataset(a, data, chunk=5) == 9 and a.rb.calls == [("extend", 5), ("extend", 4)]
    assert loop.load_dataset(b, data, chunk=5, pin=True) == 9 and b.rb.calls == [("extend", 5), ("extend", 4), ("pin", None)]


def no_env(*a, **kw):
    while True:
        yield


CFG = dict(seed=0, learning_starts=8, action_repeat=1, segment_len=1, num_envs=4, num_timesteps=27, batch_size=8, eval_every=10 ** 9,
           actor_update_delay=2)


@pytest.mark.parametrize("G", [1, 2, 5])
def test_train_prior_fraction_one_launch_and_updates_per_step(monkeypatch, G):
    monkeypatch.setattr(loop, "segment", no_env)
    cfg = SimpleNamespace(**CFG)
    ag = stub_agent()
    assert loop.train(cfg, None, ag, fused=False, one_launch=True, prior_fraction=0.5, updates_per_step=G) == {"loss/qf_loss": 0.0}
    # segments 0 and 1 fall before learning_starts (i = 0, 1); 5 segments follow with G updates each, the actor schedule on i itself
    assert ag.engine.calls == [("step_sampled", i % 3 == 0, None, 1, 1, 4) for i in range(2, 2 + 5 * G)]
    assert ag.qnet_updates_so_far == 5 * G and ag.actor_updates_so_far == 2 * len([i for i in range(2, 2 + 5 * G) if i % 3 == 0])
    assert ag.timesteps_so_far == 28


@pytest.mark.parametrize("G", [1, 3])
def test_train_prior_fraction_call_by_call(monkeypatch, G):
    monkeypatch.setattr(loop, "segment", no_env)
    cfg = SimpleNamespace(**CFG)
    ag = stub_agent()
    loop.train(cfg, None, ag, fused=False, prior_fraction=0.26, updates_per_step=G)              # round(0.26 * 8) = 2
    want = [("set_mix", 2)]                                                                      # once: the value never changes
    for n, i in enumerate(range(2, 2 + 5 * G), start=1):
        want += [("sample_mixed",), ("qnets",)] + ([("actor",)] * 2 if i % 3 == 0 else []) + [("targ", n)]
    assert ag.engine.calls == want
    assert ag.qnet_updates_so_far == 5 * G


@pytest.mark.parametrize("fused", [True, False])
def test_updates_per_step_in_the_uniform_branches(monkeypatch, fused):
    monkeypatch.setattr(loop, "segment", no_env)
    cfg = SimpleNamespace(**CFG)
    base, twice = stub_agent(), stub_agent()
    loop.train(cfg, None, base, fused=fused)                                                     # G = 1 is today's loop
    loop.train(cfg, None, twice, fused=fused, updates_per_step=2)
    if fused:
        assert base.engine.calls == [("step", i % 3 == 0) for i in range(2, 7)]
        assert twice.engine.calls == [("step", i % 3 == 0) for i in range(2, 12)]
    else:
        assert [c for c in base.engine.calls if c[0] == "targ"] == [("targ", n) for n in range(1, 6)]
        assert [c for c in twice.engine.calls if c[0] == "targ"] == [("targ", n) for n in range(1, 11)]
        assert twice.engine.calls.count(("actor",)) == 2 * len([i for i in range(2, 12) if i % 3 == 0])
    assert (base.qnet_updates_so_far, twice.qnet_updates_so_far) == (5, 10)


def test_train_evaluates_once_per_segment_whatever_the_ratio(monkeypatch):
    monkeypatch.setattr(loop, "segment", no_env)
    cfg = SimpleNamespace(**{**CFG, "eval_every": 4})
    seen = []
    loop.train(cfg, None, stub_agent(), fused=True, updates_per_step=3, on_eval=lambda ag, t: seen.append((t, ag.qnet_updates_so_far)))
    assert seen == [(12, 3), (16, 6), (20, 9), (24, 12), (28, 15)]


def test_train_refuses_what_prior_data_excludes():
    cfg = SimpleNamespace(seed=0, learning_starts=0, action_repeat=1, segment_len=1, num_envs=1, num_timesteps=0, batch_size=8)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"prior_fraction must be in \[0, 1\]"):
            loop.train(cfg, None, None, fused=False, prior_fraction=bad)
    with pytest.raises(ValueError, match="prior_fraction=... needs fused=False"):
        loop.train(cfg, None, None, prior_fraction=0.5)
    with pytest.raises(ValueError, match="prior_fraction=... and sampler=... exclude"):
        loop.train(cfg, None, None, fused=False, prior_fraction=0.5, sampler=loop.ProportionalSampler(16, device="cpu"))
    with pytest.raises(ValueError, match="prior_fraction=... and prioritized=... exclude"):
        loop.train(cfg, None, None, fused=False, prior_fraction=0.5, prioritized=dict(beta=0.4))
    with pytest.raises(ValueError, match="prior_fraction=... excludes n_step > 1"):
        loop.train(cfg, None, None, fused=False, prior_fraction=0.5, n_step=3)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="updates_per_step must be >= 1"):
            loop.train(cfg, None, None, updates_per_step=bad)
    # still refused: one_launch with nothing that needs it; accepted: prior_fraction as the reason (see the tests above)
    with pytest.raises(ValueError, match="one_launch=True needs prioritized"):
        loop.train(cfg, None, None, fused=False, one_launch=True)


# ------------------------------------------------------------------------------------------ launcher
def launcher_args(**over):
    base = dict(algo="td3", offline_dataset=None, bc_alpha=None, num_updates=None, overlap_acting=False, device_env=False, prioritized=False,
                one_launch=False, n_step=1, prior_fraction=None, updates_per_step=None)
    base.update(over)
    return SimpleNamespace(**base)


def test_launcher_plan_with_and_without_the_new_flags():
    plan = launcher.offline_plan
    assert plan(launcher_args()) is None and plan(launcher_args(updates_per_step=4)) is None       # an online run: nothing to plan
    # without the flags: what it was (and arguments written before the flags existed still work)
    assert plan(launcher_args(offline_dataset="d.npz", bc_alpha=2.5, num_updates=300)) == dict(dataset="d.npz", num_updates=300, bc_alpha=2.5, plain=False)
    old = launcher_args(offline_dataset="d.npz")
    del old.prior_fraction, old.updates_per_step
    assert plan(old) == dict(dataset="d.npz", num_updates=None, bc_alpha=0.0, plain=True)
    # with them: an online run on top of the pinned dataset
    p = plan(launcher_args(offline_dataset="d.npz", prior_fraction=0.5, updates_per_step=4, one_launch=True, overlap_acting=True))
    assert p == dict(dataset="d.npz", num_updates=None, bc_alpha=0.0, plain=True, prior_fraction=0.5, updates_per_step=4)
    assert plan(launcher_args(offline_dataset="d.npz", prior_fraction=0.0))["updates_per_step"] == 1
    with pytest.raises(ValueError, match="--prior_fraction needs --offline_dataset"):
        plan(launcher_args(prior_fraction=0.5))
    for bad in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"--prior_fraction must be in \[0, 1\]"):
            plan(launcher_args(offline_dataset="d.npz", prior_fraction=bad))
    with pytest.raises(ValueError, match="--prior_fraction excludes --prioritized, --n_step, --num_updates"):
        plan(launcher_args(offline_dataset="d.npz", prior_fraction=0.5, prioritized=True, n_step=3, num_updates=10))
    with pytest.raises(ValueError, match="--updates_per_step must be >= 1"):
        plan(launcher_args(updates_per_step=0))
    with pytest.raises(ValueError, match="--updates_per_step needs an env loop"):
        plan(launcher_args(offline_dataset="d.npz", updates_per_step=4))
    with pytest.raises(ValueError, match="excludes --one_launch"):                                  # offline without a share: as before
        plan(launcher_args(offline_dataset="d.npz", one_launch=True))


def test_launcher_command_line_parses_the_new_flags(capsys):
    ok = ["--dry-run", "--num_seeds", "1", "--algo", "td3", "--offline_dataset", "d.npz", "--prior_fraction", "0.5", "--updates_per_step", "4"]
    import inspect
    sig = inspect.signature(launcher.run_job).parameters
    assert sig["prior_fraction"].default is None and sig["updates_per_step"].default == 1
    src = inspect.getsource(launcher)
    assert "--prior_fraction" in src and "--updates_per_step" in src and 'prior_fraction=plan.get("prior_fraction")' in src
    for argv, msg in ((["--prior_fraction", "0.5"], "needs --offline_dataset"), (ok[:-2] + ["--updates_per_step", "0"], "must be >= 1"),
                      (ok[:5] + ["--offline_dataset", "d.npz", "--prior_fraction", "2"], "must be in")):
        with pytest.raises(SystemExit) as ex:
            launcher.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
