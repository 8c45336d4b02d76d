"""GPU: acting on a stream of its own (sactd3_predict_begin / sactd3_predict_end, include/sactd3.h) against the serial
sactd3_predict.  Everything here is an equality: the two-stream form returns, bit for bit, what the serial call returns at the
position of `begin` in the call sequence, and the ordering policy is checked through the engine's host counters
(sactd3_acting_stats), whose values follow from the schedule of the calls, not from timing."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps, RefAgent
from tests.gpu_support import P, _lib, assert_same_state, close, close_engines, loop, make_pair, push_params, track  # noqa: F401
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu

WORKLOADS = [("sac", "hopper"), ("td3", "halfcheetah"), ("sac", "humanoid")]


def two_engines(algo, env, B, **kw):
    """two engines with the same seed and the same parameters (make_pair seeds torch before it draws them), and the oracle"""
    ref, a_eng, dims = make_pair(algo, env, B, **kw)
    _, b_eng, _ = make_pair(algo, env, B, **kw)
    return ref, a_eng, b_eng, dims


def begin_end(eng, obs, explore, after_all=False):
    eng.predict_begin(obs, explore, after_all)
    return eng.predict_end()


# ------------------------------------------------------------------------------------------ 1. same answer as predict
@pytest.mark.parametrize("algo,env", WORKLOADS)
def test_begin_end_returns_what_predict_returns(algo, env):
    ref, A, B, (o, a, bound) = two_engines(algo, env, 32)
    for n in (1, 4, 8):
        obs = torch.randn(n, o, generator=torch.Generator().manual_seed(n))
        x, y = A.predict(obs, explore=False), begin_end(B, obs, False)
        assert y.shape == (n, a) and np.array_equal(x, y), ("exploit", n)
        close(y, ref.predict(obs, explore=False), name=f"exploit n={n}")            # tolerance of test_predict
        eps = torch.randn(n, a, generator=torch.Generator().manual_seed(100 + n))
        A.set_noise(_lib.SITE_PREDICT, eps)
        B.set_noise(_lib.SITE_PREDICT, eps)
        x, y = A.predict(obs, explore=True), begin_end(B, obs, True)
        assert np.array_equal(x, y), ("explore, injected", n)
        assert np.array_equal(A.read_noise(_lib.SITE_PREDICT, n), B.read_noise(_lib.SITE_PREDICT, n))
        A.clear_noise(_lib.SITE_PREDICT)
        B.clear_noise(_lib.SITE_PREDICT)
        seen = []
        for k in range(3):                                                          # the native draw: one counter tick per call
            x, y = A.predict(obs, explore=True), begin_end(B, obs, True, after_all=(k == 1))
            assert np.array_equal(x, y) and np.isfinite(y).all(), ("explore, native", n, k)
            assert np.array_equal(A.read_noise(_lib.SITE_PREDICT, n), B.read_noise(_lib.SITE_PREDICT, n))
            seen.append(y)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # the two entry points share the counter: a serial call on B continues the stream where its begun calls left it
    obs = torch.randn(4, o, generator=torch.Generator().manual_seed(77))
    assert np.array_equal(A.predict(obs, explore=True), B.predict(obs, explore=True))


def test_begin_end_with_a_multi_block_tail():
    """40 rows with max_envs = 48: more than one block of the tail kernel, so completion is a synchronisation of the acting
    stream and the counter is advanced by a kernel of its own behind the tail"""
    o, a, bound = DIMS["hopper"]
    hps = Hps.sac(batch_size=32)
    torch.manual_seed(0)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, hps)
    A, B = [track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=256, max_envs=48, seed=7), [-bound] * a, [bound] * a))
            for _ in range(2)]
    for e in (A, B):
        push_params(e, ref)
    obs = torch.randn(40, o, generator=torch.Generator().manual_seed(3))
    y = begin_end(B, obs, False)
    assert np.array_equal(A.predict(obs, explore=False), y)
    close(y, ref.predict(obs, explore=False), name="exploit, 40 rows")
    for k in range(3):
        assert np.array_equal(A.predict(obs, explore=True), begin_end(B, obs, True)), k
        assert np.array_equal(A.read_noise(_lib.SITE_PREDICT, 40), B.read_noise(_lib.SITE_PREDICT, 40))
    assert B.acting_stats()["begun"] == 4 and B.acting_stats()["ended_by_spin"] == 0


# ------------------------------------------------------------------------------------------ 2. / 3. the loop
def acting_loop(eng, dims, n_iter, overlapped, after_all=False, rows=4, prefill=256):
    """`n_iter` iterations of: 4-row exploring predict, step(i % 3 == 0), 4-row rb_extend of the rows the actions belong to.
    overlapped: predict_begin -> step -> predict_end -> rb_extend; else predict -> step -> rb_extend.  Returns every iteration's
    actions; the rows written depend on them, so one wrong action changes everything behind it."""
    o, a, bound = dims
    eng.rb_extend(*synth_transitions(prefill, o, a, bound, seed=5))
    g = torch.Generator().manual_seed(17)
    acts = []
    for i in range(n_iter):
        obs, nobs = torch.randn(rows, o, generator=g).numpy(), torch.randn(rows, o, generator=g).numpy()
        rew, done = torch.randn(rows, generator=g).numpy(), (torch.rand(rows, generator=g) < 0.1).numpy()
        if overlapped:
            eng.predict_begin(obs, True, after_all)
            eng.step(i % 3 == 0)
            act = eng.predict_end()
        else:
            act = eng.predict(obs, True)
            eng.step(i % 3 == 0)
        eng.rb_extend(obs, act, rew, nobs, done)
        acts.append(act)
    return acts


LOOPS = [
    ("sac", "hopper", 256, 90, dict(use_graphs=True), False),
    ("sac", "hopper", 256, 90, dict(use_graphs=False), False),
    ("td3", "halfcheetah", 256, 90, dict(use_graphs=True), False),
    ("td3", "halfcheetah", 256, 90, dict(use_graphs=False), False),
    ("sac", "humanoid", 1024, 30, dict(use_graphs=True), False),
    ("sac", "hopper", 256, 90, dict(use_graphs=True, actor_update_delay=0), False),
    ("sac", "hopper", 256, 90, dict(use_graphs=True, actor_update_delay=1), False),
    ("sac", "hopper", 256, 90, dict(use_graphs=True), True),
]


@pytest.mark.parametrize("algo,env,B,n_iter,kw,after_all", LOOPS)
def test_overlapped_loop_is_the_serial_loop_bit_for_bit(algo, env, B, n_iter, kw, after_all):
    _, A, Bn, dims = two_engines(algo, env, B, **kw)
    want = acting_loop(A, dims, n_iter, overlapped=False)
    got = acting_loop(Bn, dims, n_iter, overlapped=True, after_all=after_all)
    for i, (x, y) in enumerate(zip(want, got)):
        assert np.array_equal(x, y), ("actions of iteration", i)
    assert not np.array_equal(want[0], want[-1])
    assert_same_state(A, Bn, "ring")                             # every ring row: the prefill and the rows the loop wrote
    assert A.rb_len() == Bn.rb_len() == 256 + 4 * n_iter


@pytest.mark.parametrize("after_all,want_waits", [(False, 30), (True, 90)])
def test_the_ordering_policy_engaged(after_all, want_waits):
    """actor_update_delay = 2, step(i % 3 == 0), one call in flight around every step.  A begin waits for the learner stream only
    behind a step with actor updates (iterations 1, 4, ..., 88) -- or always with after_all; the learner waits for the acting call
    only in the steps with actor updates (iterations 0, 3, ..., 87); critic-only steps add to neither count."""
    _, eng, dims = make_pair("sac", "hopper", 256)
    o = dims[0]
    begin_end(eng, np.zeros((4, o), np.float32), True)          # absorbs the parameter upload (a write of the actor)
    s0 = eng.acting_stats()
    acting_loop(eng, dims, 90, overlapped=True, after_all=after_all)
    s1 = eng.acting_stats()
    d = {k: s1[k] - s0[k] for k in s1}
    assert d["begun"] == 90
    assert d["begin_waited_for_learner"] == want_waits
    assert d["learner_waited_for_acting"] == 30
    assert 0 <= d["ended_by_spin"] <= 90


# ------------------------------------------------------------------------------------------ 4. write after read
def test_actor_writes_wait_for_the_call_in_flight():
    """predict_begin; step with actor updates and set_params(ACTOR) before predict_end: the actions are those of the parameters
    in place at `begin`, and the next call sees the new ones.  Many rounds, the two parameter sets alternating."""
    ref, A, B, (o, a, bound) = two_engines("sac", "hopper", 256)
    B.rb_extend(*synth_transitions(512, o, a, bound, seed=5))
    p0 = A.get_params(_lib.ACTOR)
    p1 = (p0 + 0.05 * np.random.default_rng(0).standard_normal(p0.shape)).astype(np.float32)
    obs = torch.randn(4, o, generator=torch.Generator().manual_seed(9)).numpy()
    want = [A.predict(obs, False)]
    A.set_params(_lib.ACTOR, p1)
    want.append(A.predict(obs, False))
    assert not np.array_equal(want[0], want[1])
    s0 = B.acting_stats()
    for k in range(40):
        B.predict_begin(obs, False)
        B.step(True)                                             # overwrites the actor ...
        B.set_params(_lib.ACTOR, (p0, p1)[(k + 1) % 2])          # ... and so does this
        assert np.array_equal(B.predict_end(), want[k % 2]), k
    assert np.array_equal(B.predict(obs, False), want[0])        # (40 rounds: p0 is in place again)
    assert np.array_equal(begin_end(B, obs, False), want[0])
    assert B.acting_stats()["learner_waited_for_acting"] - s0["learner_waited_for_acting"] >= 40


# ------------------------------------------------------------------------------------------ 5. state errors
def test_state_errors_leave_the_engine_usable():
    ref, A, B, (o, a, bound) = two_engines("sac", "hopper", 32)
    obs = torch.randn(4, o, generator=torch.Generator().manual_seed(2)).numpy()
    eps = np.zeros((4, a), np.float32)
    with pytest.raises(P.EngineError, match=r"error -3"):
        B.predict_end()                                          # nothing begun
    for bad in (np.zeros((9, o), np.float32), np.zeros((0, o), np.float32)):      # max_envs is 8
        with pytest.raises(P.EngineError, match=r"error -1"):
            B.predict_begin(bad, False)
    B.predict_begin(obs, False)
    for call in (lambda: B.predict_begin(obs, False), lambda: B.predict(obs, False), lambda: B.set_noise(_lib.SITE_PREDICT, eps),
                 lambda: B.clear_noise(_lib.SITE_PREDICT), lambda: B.clear_noise(-1), lambda: B.read_noise(_lib.SITE_PREDICT, 4)):
        with pytest.raises(P.EngineError, match=r"error -3.*in flight"):
            call()
    B.set_noise(_lib.SITE_ACTOR0, np.zeros((32, a), np.float32))  # other sites are not the acting kernels' business
    B.clear_noise(_lib.SITE_ACTOR0)
    B.sync()                                                      # drains both streams; the call is still to be collected
    assert np.array_equal(B.predict_end(), A.predict(obs, False))
    with pytest.raises(P.EngineError, match=r"error -3"):
        B.predict_end()
    assert np.array_equal(B.predict(obs, True), A.predict(obs, True))
    assert np.array_equal(begin_end(B, obs, True), A.predict(obs, True))
    B.predict_begin(obs, True)
    B.close()                                                     # with a call in flight: returns


def test_null_arguments_through_the_raw_abi():
    _, eng, (o, a, bound) = make_pair("sac", "hopper", 32)
    lib, h = eng.lib, eng._h
    obs, out, st = np.zeros((4, o), np.float32), np.zeros((4, a), np.float32), (C.c_int64 * 4)()
    fp = C.POINTER(C.c_float)
    assert lib.sactd3_predict_begin(None, obs.ctypes.data_as(fp), 4, 0, 0) == _lib.EINVAL
    assert lib.sactd3_predict_begin(h, None, 4, 0, 0) == _lib.EINVAL
    assert lib.sactd3_predict_begin(h, obs.ctypes.data_as(fp), 4, 0, 2) == _lib.EINVAL          # an unknown flag
    assert lib.sactd3_predict_end(None, out.ctypes.data_as(fp)) == _lib.EINVAL
    assert lib.sactd3_predict_end(h, None) == _lib.EINVAL
    assert lib.sactd3_acting_stats(None, st) == _lib.EINVAL and lib.sactd3_acting_stats(h, None) == _lib.EINVAL
    assert lib.sactd3_acting_stats(h, st) == 0 and list(st) == [0, 0, 0, 0]                    # none of those began anything
    assert lib.sactd3_predict_begin(h, obs.ctypes.data_as(fp), 4, 0, _lib.ACT_AFTER_ALL) == 0
    assert lib.sactd3_predict_end(h, None) == _lib.EINVAL                                      # ... and does not end the call
    assert lib.sactd3_predict_end(h, out.ctypes.data_as(fp)) == 0
    assert np.array_equal(out, eng.predict(obs, False))


# ------------------------------------------------------------------------------------------ 6. end to end
def test_train_loop_with_overlap_equals_the_serial_train_loop(tmp_path):
    """the configuration of tests/test_loop.py:test_train_loop_drives_the_engine_end_to_end, evaluator and checkpoints on, so a
    pending action meets an evaluation"""
    o, a, n = 11, 3, 4
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 400,
                             "num_timesteps": 2400, "eval_every": 800, "cudagraphs": True, "rb_capacity": 5000})
    cfg.eval_steps, cfg.measure_burnin = 2, 0
    logs = []
    for overlap in (False, True):
        env = loop.SyntheticVecEnv(o, a, n)
        env.action_space.seed(0)
        torch.manual_seed(0)
        agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                        torch.device("cuda:0"), cfg, P.ReplayBuffer(cfg.rb_capacity))
        ev = loop.Evaluator(cfg, loop.SyntheticVecEnv(o, a, 1, horizon=20), agent, loop.Tabular(tmp_path / str(overlap)),
                            ckpt_dir=tmp_path / str(overlap))
        evals = []
        m = loop.train(cfg, env, agent, fused=True, on_eval=lambda ag, ts: evals.append(ts), evaluator=ev, overlap=overlap)
        assert evals == [800, 1600, 2400] and all(np.isfinite(v) for v in m.values())
        stats = agent.engine.acting_stats()
        assert (stats["begun"] > 0) == overlap
        logs.append(dict(metrics=m, actor=track(agent.engine).get_params(_lib.ACTOR), critics=agent.engine.get_params(_lib.CRITICS),
                         counters=(agent.timesteps_so_far, agent.qnet_updates_so_far, agent.actor_updates_so_far), rb=len(agent.rb),
                         history=[(h["timestep"], h["length"], h["return"]) for h in ev.history],
                         next_action=agent.predict({"observations": np.ones((n, o), np.float32)}, explore=True)))
        agent.engine.close()
    x, y = logs
    assert x["metrics"] == y["metrics"] and x["counters"] == y["counters"] == (2404, 501, 2 * 167) and x["rb"] == y["rb"] == 2404
    assert np.array_equal(x["actor"], y["actor"]) and np.array_equal(x["critics"], y["critics"])
    assert x["history"] == y["history"] and np.array_equal(x["next_action"], y["next_action"])
