"""GPU: the batch slot's generation is the engine's (include/sactd3.h: sactd3_batch_generation).  1. the rule, call by call: it grows
with every accepted call that puts new rows into the slot and with no other; 2. a BatchHandle goes stale behind ANY such call, the
ones made on the engine directly included, and a stale handle starts no update; 3. what the reference's loop does with a handle
stays allowed, and loop.train ends where the same iterations issued on the engine without a handle end, bit for bit.
Nothing numerical: counters, refusals and equal bits."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.gpu_support import (DEV, DIMS, Hps, P, _lib, agent_mod, assert_same_state, build_engines, close_engines, cuda, engine_state,  # noqa: F401
                               extend_device, info, load_device, loop, rows, same_bits, stage, stream, td_of, track)

pytestmark = pytest.mark.gpu

O, A, BOUND = DIMS["hopper"]
B, CAP, HELD, DELAY, ENVS = 64, 256, 128, 2, 4


def filled_engine(algo):
    """hopper dims, 128 of 256 ring rows held: TD3's period graph is the plain one, SAC's the pipelined one"""
    _, (eng,), _ = build_engines(algo, DIMS["hopper"], B, cap=CAP, actor_update_delay=DELAY)
    eng.rb_extend(*[t.numpy() for t in rows(HELD, O, A, BOUND, seed=1)])
    return eng


class Walk:
    """one engine and its generation: every call goes through grows() or keeps()"""

    def __init__(self, eng):
        self.eng, self.seen = eng, [eng.batch_generation()]

    def _after(self, name, call):
        before = self.eng.batch_generation()
        call()
        self.seen.append(self.eng.batch_generation())
        return before, self.seen[-1], name

    def grows(self, name, call):
        before, after, name = self._after(name, call)
        assert after > before, (name, before, after)

    def keeps(self, name, call):
        before, after, name = self._after(name, call)
        assert after == before, (name, before, after)

    def refused(self, name, call):
        def expect_refusal():
            with pytest.raises(P.EngineError):
                call()
        self.keeps(name, expect_refusal)


# ------------------------------------------------------------------------------------------ 1. the rule, call by call
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_generation_grows_with_every_refill_and_with_nothing_else(algo):
    eng = filled_engine(algo)
    w = Walk(eng)
    batch = rows(B, O, A, BOUND, seed=2)
    few = rows(8, O, A, BOUND, seed=3)
    idx_h = np.arange(B) % HELD
    idx_d = torch.as_tensor(idx_h, device=DEV)
    ones = torch.ones(B, device=DEV)
    out, fields = agent_mod._device_outputs(eng, B)
    obs8, act8 = few[0].numpy(), few[1].numpy()
    obs8_d, act8_d = few[0].to(DEV), torch.empty(8, A, device=DEV)
    records = torch.as_tensor(eng.pack_records(*[t.numpy() for t in few])).to(DEV)

    w.grows("rb_sample", eng.rb_sample)
    w.keeps("read_batch", eng.read_batch)
    w.keeps("read_batch_device", lambda: eng.read_batch_device(fields, stream()))
    w.keeps("rb_read_rows_device", lambda: eng.rb_read_rows_device(idx_d.data_ptr(), 1, B, fields, stream()))
    w.keeps("update_qnets", eng.update_qnets)
    w.keeps("td_errors_device", lambda: td_of(eng))
    w.keeps("update_actor", eng.update_actor)
    w.keeps("update_targ_nets", lambda: eng.update_targ_nets(1))
    w.keeps("read_metrics", eng.read_metrics)
    w.keeps("batch_weights_device", lambda: eng.batch_weights_device(ones.data_ptr(), 1, B, stream()))
    w.keeps("update_qnets, weighted", eng.update_qnets)
    w.keeps("rb_extend", lambda: eng.rb_extend(*[t.numpy() for t in few]))
    w.keeps("rb_extend_fields_device", lambda: extend_device(eng, cuda(few)))
    w.keeps("rb_extend_device", lambda: (eng.rb_extend_device(records.data_ptr(), 8), eng.sync()))
    w.keeps("rb_extend_records_device", lambda: eng.rb_extend_records_device(records.data_ptr(), 8, stream()))
    w.keeps("predict", lambda: eng.predict(obs8, True))
    w.keeps("predict_device", lambda: eng.predict_device(obs8_d.data_ptr(), O, 8, True, act8_d.data_ptr(), A, stream()))
    w.keeps("q_values", lambda: eng.q_values(obs8, act8))
    w.keeps("policy", lambda: eng.policy(obs8))
    w.keeps("set_params", lambda: eng.set_params(_lib.CRITICS, eng.get_params(_lib.CRITICS)))

    w.grows("rb_sample_with_indices", lambda: eng.rb_sample_with_indices(idx_h))
    short = np.ascontiguousarray(idx_h[:B - 1], np.int64)
    w.keeps("rb_sample_with_indices, wrong count", lambda: _expect(
        eng.lib.sactd3_rb_sample_with_indices(eng._h, short.ctypes.data_as(C.POINTER(C.c_int64)), B - 1), _lib.EINVAL))
    w.grows("load_batch", lambda: eng.load_batch(*[t.numpy() for t in batch]))
    w.grows("load_batch_device", lambda: load_device(eng, cuda(batch)))
    w.grows("rb_sample_indices_device", lambda: stage(eng, idx_d))
    w.grows("rb_sample_nstep", lambda: eng.rb_sample_nstep(2, ENVS))
    w.keeps("nstep_info_device", lambda: info(eng))
    w.grows("rb_sample_nstep_device", lambda: eng.rb_sample_nstep_device(idx_d.data_ptr(), 1, 0, 1, B, 2, ENVS, stream()))
    w.keeps("rb_set_mix", lambda: eng.rb_set_mix(16))
    w.refused("rb_sample_mixed, nothing pinned", eng.rb_sample_mixed)

    w.keeps("prio_enable", eng.prio_enable)
    w.grows("rb_sample_prioritized", lambda: eng.rb_sample_prioritized(0.4))
    w.keeps("update_qnets, prioritised", eng.update_qnets)
    w.keeps("prio_update_from_td", eng.prio_update_from_td)
    w.grows("rb_sample_prioritized_nstep", lambda: eng.rb_sample_prioritized_nstep(0.4, 2, ENVS))

    w.grows("step(True)", lambda: eng.step(True))
    w.grows("step(False)", lambda: eng.step(False))
    w.grows("step_sampled", lambda: eng.step_sampled(True, n_step=2, stride=ENVS))
    w.grows("step_sampled, prioritised", lambda: eng.step_sampled(False, beta=0.4))
    w.grows("step_prefix(1)", lambda: eng.step_prefix(1))
    w.grows("step_period", eng.step_period)
    w.grows("step_periods(3)", lambda: eng.step_periods(3))
    w.grows("run_iterations(0, 7)", lambda: eng.run_iterations(0, 7))
    w.keeps("read_batch, at the end", eng.read_batch)
    assert w.seen == sorted(w.seen), w.seen                            # never back, over the whole walk

    # the mixed draw, on an engine of its own: pinned rows exclude priorities
    mixed = Walk(filled_engine(algo))
    mixed.keeps("rb_pin", lambda: mixed.eng.rb_pin(HELD // 2))
    mixed.keeps("rb_set_mix", lambda: mixed.eng.rb_set_mix(16))
    mixed.grows("rb_sample_mixed", mixed.eng.rb_sample_mixed)
    mixed.grows("step_sampled, mixed", lambda: mixed.eng.step_sampled(True, prior_rows=16))
    assert mixed.seen == sorted(mixed.seen), mixed.seen


def _expect(got, want):
    assert got == want, (got, want)


# ------------------------------------------------------------------------------------------ the mirror on the same shapes
def config(algo, **more):
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(batch_size=B, actor_update_delay=DELAY)
    return SimpleNamespace(**{**hps.__dict__, "seed": 0, "num_envs": ENVS, "action_repeat": 1, "eval_every": 10 ** 9, "cudagraphs": True,
                              "rb_capacity": CAP, **more})


def new_agent(cfg):
    torch.manual_seed(0)
    ag = P.Agent({"ob_shape": (ENVS, O), "ac_shape": (ENVS, A)}, np.full(A, -BOUND, np.float32), np.full(A, BOUND, np.float32),
                 torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
    track(ag.engine)
    return ag


def transitions(n, seed):
    obs, act, rew, nobs, done = [t.numpy() for t in rows(n, O, A, BOUND, seed=seed)]
    return {"observations": obs, "next_observations": nobs, "actions": act, "rewards": rew.reshape(-1, 1),
            "terminations": done.reshape(-1, 1), "dones": done.reshape(-1, 1)}


def filled_agent(algo):
    ag = new_agent(config(algo))
    ag.rb.extend(transitions(HELD, seed=1))
    return ag


def metrics_of(eng):
    return np.float32(list(eng.read_metrics().values()))


def assert_handle_reads_the_slot(h, eng):
    want = eng.read_batch()
    for k, v in want.items():
        assert np.array_equal(np.asarray(h[k]).reshape(v.shape), v), k


# ------------------------------------------------------------------------------------------ 2. the holes that were open
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_a_handle_goes_stale_behind_every_direct_refill(algo):
    ag = filled_agent(algo)
    eng = ag.engine
    batch = [t.numpy() for t in rows(B, O, A, BOUND, seed=2)]
    direct = {"run_iterations": lambda: eng.run_iterations(0, 3), "step": lambda: eng.step(True), "step_period": eng.step_period,
              "rb_sample": eng.rb_sample, "load_batch": lambda: eng.load_batch(*batch),
              "rb_sample_with_indices": lambda: eng.rb_sample_with_indices(np.arange(B) % HELD)}
    for name, call in direct.items():
        h = ag.rb.sample(B)
        assert h._is_current(), name
        call()
        assert not h._is_current(), name
        metrics, critics, updates = metrics_of(eng), eng.get_params(_lib.CRITICS), ag.qnet_updates_so_far
        with pytest.raises(P.StaleBatchError):
            h["observations"]
        with pytest.raises(P.StaleBatchError):
            h.on_device()
        with pytest.raises(P.StaleBatchError):
            ag.update_qnets(h)
        assert same_bits(metrics_of(eng), metrics) and same_bits(eng.get_params(_lib.CRITICS), critics), name      # no update was issued
        assert ag.qnet_updates_so_far == updates
        fresh = ag.rb.sample(B)
        assert fresh._is_current() and not h._is_current(), name
        assert_handle_reads_the_slot(fresh, eng)


# ------------------------------------------------------------------------------------------ 3. what stayed allowed still is
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_a_handle_survives_the_references_call_sequence(algo):
    """orchestrator.py:338-349 on one handle, with the calls that leave the slot's rows alone in between"""
    ag = filled_agent(algo)
    eng = ag.engine
    few = transitions(8, seed=3)
    for i in range(2):
        h = ag.rb.sample(B)
        ag.update_qnets(h)
        ag.qnet_updates_so_far += 1
        ag.q_values({"observations": few["observations"], "actions": few["actions"]})
        ag.policy({"observations": few["observations"]})
        ag.td_errors()
        ag.rb.extend(few)
        for _ in range(DELAY):
            ag.update_actor(h)
            ag.actor_updates_so_far += 1
        ag.update_targ_nets()
        assert h._is_current(), i
        assert_handle_reads_the_slot(h, eng)
    assert (ag.qnet_updates_so_far, ag.actor_updates_so_far, len(ag.rb)) == (2, 2 * DELAY, HELD + 16)


ITERS, STARTS = 10, 40
MODES = {"fused": dict(fused=True), "call_by_call": dict(fused=False), "one_launch": dict(fused=False, one_launch=True, n_step=2)}


def engine_run(cfg, env, ag, mode):
    """loop.train's control flow with the iterations issued on the engine itself: no BatchHandle is ever made"""
    eng, period = ag.engine, cfg.actor_update_delay + 1
    seg = loop.segment(env, ag, cfg.seed, cfg.segment_len, cfg.learning_starts, cfg.action_repeat)
    i = 0
    while ag.timesteps_so_far <= cfg.num_timesteps:
        next(seg)
        ag.timesteps_so_far += cfg.segment_len * cfg.num_envs
        if ag.timesteps_so_far > cfg.learning_starts:
            do_actor = i % period == 0
            if mode == "fused":
                eng.step(do_actor)
            elif mode == "one_launch":
                eng.step_sampled(do_actor, n_step=2, stride=cfg.num_envs)
            else:
                eng.rb_sample()
                eng.update_qnets()
                for _ in range(cfg.actor_update_delay if do_actor else 0):
                    eng.update_actor()
                eng.update_targ_nets(ag.qnet_updates_so_far + 1)
            ag.qnet_updates_so_far += 1
            ag.actor_updates_so_far += cfg.actor_update_delay if do_actor else 0
        i += 1


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_train_ends_where_the_engine_driven_without_handles_ends(algo, mode):
    cfg = config(algo, learning_starts=STARTS, num_timesteps=STARTS + ITERS * ENVS - 1)
    res = []
    for through_loop in (True, False):
        env = loop.SyntheticVecEnv(O, A, ENVS, horizon=7, term_at=2.5)
        env.action_space.seed(0)
        np.random.seed(0)
        ag = new_agent(cfg)
        if through_loop:
            loop.train(cfg, env, ag, **MODES[mode])
        else:
            engine_run(cfg, env, ag, mode)
        eng = ag.engine
        counters = [ag.qnet_updates_so_far, ag.actor_updates_so_far, ag.timesteps_so_far, len(ag.rb)]
        first = STARTS // ENVS                                          # the loop counts the segments in front of learning_starts too
        with_actor = [i for i in range(first, first + ITERS) if i % (DELAY + 1) == 0]
        assert counters == [ITERS, DELAY * len(with_actor), STARTS + ITERS * ENVS, STARTS + ITERS * ENVS], (through_loop, counters)
        assert eng.step_sampled_stats()["launches"] == (ITERS if mode == "one_launch" else 0)
        res.append(engine_state(eng, "ring", extra=dict(counters=np.int64(counters))))
    assert_same_state(res[0], res[1], what=f"{algo} {mode}: loop.train against the engine driven without handles")
