"""GPU: hindsight relabelling at staging (include/sactd3.h: sactd3_hindsight_configure, sactd3_rb_sample_hindsight[_device],
sactd3_hindsight_info_device, sactd3_hindsight_stats; csrc/hindsight_kernels.h) against the numpy restatement of tests/hindsight_ref.py,
bit for bit, through the C ABI and through agent.ReplayBuffer.

Shapes (o, a, B): (6, 2, 8) and (6, 2, 260) on rollouts of the host goal env (at 260 a block's span ends inside a row); (11, 3, 64) with
the achieved goal at 2..4 and the desired one at 7..9 (it straddles a 16-byte chunk); (13, 3, 32) with the desired goal at 10..12 (it
shares a chunk with the action in X and with the pad in Xn); (376, 17, 16) with three goal floats (a row spans several chunks per thread
and several blocks) -- the last three on synthetic episodic records.  Rings of 96 and 101 slots at stride 4, unwrapped and wrapped.
window in {1, 5, 64}, ratio in {0, 0.5, 1}, and injected choices among -1, 0, L - 1 and beyond L."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import hindsight_ref as hr
from tests.gpu_support import (DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, load_device, loop,  # noqa: F401
                               same_bits, stage, stream, td_of, track)

pytestmark = pytest.mark.gpu
envs = P.envs
F = np.float32
STRIDE, SENT = 4, -77
# name -> (o, a, B, achieved, desired, dim, horizon of its episodes)
CASES = {"goal-8": (6, 2, 8, 0, 4, 2, 9), "goal-260": (6, 2, 260, 0, 4, 2, 9), "straddle-64": (11, 3, 64, 2, 7, 3, 5),
         "shared-32": (13, 3, 32, 0, 10, 3, 5), "long-16": (376, 17, 16, 1, 200, 3, 5)}
RINGS = {"96-unwrapped": (96, 20), "96-wrapped": (96, 61), "101-unwrapped": (101, 25), "101-wrapped": (101, 77)}      # capacity, vector steps
WINDOWS, RATIOS = (1, 5, 64), (0.0, 0.5, 1.0)
SEED = 3                                                                  # the engines' Philox key (build_engines: seed)


@functools.lru_cache(maxsize=None)
def ring_of(case, ring):
    """rows, slot-indexed fields, geometry, episode bookkeeping, start slots and injected choices: computed once, never written"""
    o, a, B, ag, dg, G, horizon = CASES[case]
    cap, steps = RINGS[ring]
    if case.startswith("goal"):
        rows, episode = hr.host_rollout(envs.HostVecEnv("pointgoal", STRIDE, seed=5, horizon=horizon), steps)
    else:
        rows, episode = hr.synthetic_ring(o, a, STRIDE, steps, horizon, seed=o, term_every=3, achieved=ag, dim=G)
    fields, geom, held = hr.place(rows, cap)
    rng = np.random.default_rng(B + cap)
    length, cursor = geom["length"], geom["cursor"]
    newest = [(cursor - 1 - k) % cap if length == cap else length - 1 - k for k in range(STRIDE)]
    front = newest + [0, cap - 1 if length == cap else length - 1, cursor % max(length, 1), (cap - STRIDE - 1) % length, -1, length if length < cap else cap, 2 ** 40]
    idx = np.array((front + list(rng.integers(0, length, max(B - len(front), 0))))[:B], np.int64)
    if B == 8:                                                            # too few rows for the refusals: one of them, at the end
        idx[-1] = -1
    L = hr.stage(fields, geom, idx, dict(achieved=ag, desired=dg, dim=G, threshold=0.1, ratio=1.0, window=64, stride=STRIDE),
                 choice=np.zeros(B, np.int32))["L"]
    choice = np.array([(-1, 0, max(L[b] - 1, 0), L[b] + 3, 63, 2)[b % 6] for b in range(B)], np.int32)
    return dict(rows=rows, episode=episode, fields=fields, geom=geom, held=held, idx=idx, choice=choice)


def config(case, window, ratio):
    o, a, B, ag, dg, G, _ = CASES[case]
    return dict(achieved=ag, desired=dg, dim=G, threshold=0.1, ratio=ratio, window=window, stride=STRIDE)


@functools.lru_cache(maxsize=None)
def expected(case, ring, window, ratio, hctr, injected):
    r = ring_of(case, ring)
    return hr.stage(r["fields"], r["geom"], r["idx"], config(case, window, ratio), seed=SEED, hctr=hctr, choice=r["choice"] if injected else None)


def engines(case, ring, count=1, fill=True):
    o, a, B = CASES[case][:3]
    cap = RINGS[ring][0]
    ref, engs, _ = build_engines("sac", (o, a, 1.0), B, count=count, seed=SEED, cap=cap, max_envs=STRIDE)
    if fill:
        rows = ring_of(case, ring)["rows"]
        five = [rows[k] for k in ("obs", "act", "rew", "nobs")] + [rows["done"] != 0]
        for e in engs:
            for lo in range(0, len(rows["rew"]), cap - 1):
                e.rb_extend(*[f[lo:lo + cap - 1] for f in five])
            assert e.rb_len() == ring_of(case, ring)["geom"]["length"]
    return ref, engs


def stage_h(eng, idx, choice=None):
    idx = torch.as_tensor(np.asarray(idx, np.int64), device=DEV)
    ch = None if choice is None else torch.as_tensor(np.asarray(choice, np.int32), device=DEV)
    eng.rb_sample_hindsight_device(idx.data_ptr(), 1, 0 if ch is None else ch.data_ptr(), 1, idx.shape[0], stream())
    return idx, ch


def read_slot(eng, o, a):
    """batch slot 0 as hr.stage states it, the padded rows included; a sentinel on either side of the info arrays must survive"""
    B = eng.cfg.batch_size
    cx4, cn4 = -(-(o + a) // 4) * 4, -(-o // 4) * 4
    X = eng.debug_read("X").reshape(B, -1)[:, :cx4]
    Xn = eng.debug_read("Xn").reshape(B, -1)[:, :cn4]
    off = torch.full((B + 2,), SENT, dtype=torch.int32, device=DEV)
    gs = torch.full((B + 2,), SENT, dtype=torch.int32, device=DEV)
    eng.hindsight_info_device(off[1:].data_ptr(), 1, gs[1:].data_ptr(), 1, stream())
    off, gs = off.cpu().numpy(), gs.cpu().numpy()
    assert off[0] == off[-1] == gs[0] == gs[-1] == SENT
    return dict(X=X, Xn=Xn, obs=X[:, :o], act=X[:, o:o + a], nobs=Xn[:, :o], rew=eng.debug_read("rew")[:B], done=eng.debug_read("done")[:B],
                slot_idx=eng.read_batch()["index"].astype(np.int32), offset=off[1:-1], goal_slot=gs[1:-1])


ALL_KEYS = hr.KEYS + ("X", "Xn")


# ------------------------------------------------------------------------------------------ 1. slot contents, bit for bit
@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("case", list(CASES))
def test_slot_contents_are_the_restatements(case, ring):
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    _, (eng,) = engines(case, ring)
    hctr, want_stats = 0, np.zeros(3, np.int64)
    for window in WINDOWS:
        for ratio in RATIOS:                                              # the native draw at the engine's own counter
            eng.hindsight_configure(**config(case, window, ratio))
            stage_h(eng, r["idx"])
            want = expected(case, ring, window, ratio, hctr, False)
            hr.check(want, read_slot(eng, o, a), ALL_KEYS)
            hctr += 1
            want_stats += [(want["offset"] >= 0).sum(), (want["slot_idx"] < 0).sum(), ((want["offset"] >= 0) & (want["rew"] == 0)).sum()]
        eng.hindsight_configure(**config(case, window, 0.3))              # injected choices: the ratio plays no part, the counter stands
        stage_h(eng, r["idx"], r["choice"])
        want = expected(case, ring, window, 0.3, 0, True)
        hr.check(want, read_slot(eng, o, a), ALL_KEYS)
        want_stats += [(want["offset"] >= 0).sum(), (want["slot_idx"] < 0).sum(), ((want["offset"] >= 0) & (want["rew"] == 0)).sum()]
    st = eng.hindsight_stats()
    assert st == dict(native_draws=hctr, rows_relabelled=int(want_stats[0]), rows_refused=int(want_stats[1]), rows_reward_zero=int(want_stats[2]))
    assert st["rows_refused"] > 0 and st["rows_relabelled"] > 0


def test_the_cases_cover_what_they_mean_to():
    """on the CPU, from the restatement's own output for the seeds in use: every situation the kernel has a rule for occurs"""
    for case in CASES:
        B = CASES[case][2]
        seen = dict(j0=0, jlast=0, truncation=0, newest=0, wrap=0, rew0=0, rewm1=0, beyond=0, refused=0, keep=0)
        for ring in RINGS:
            r = ring_of(case, ring)
            geom, held, idx = r["geom"], r["held"], r["idx"]
            cap, length = geom["cap"], geom["length"]
            n_rows = int(held.max()) + 1
            for window in WINDOWS:
                for ratio, hctr, injected in [(q, k, False) for k, q in enumerate(RATIOS)] + [(0.3, 0, True)]:
                    w = expected(case, ring, window, ratio, hctr + 3 * WINDOWS.index(window) if not injected else 0, injected)
                    rel, L = w["offset"] >= 0, w["L"]
                    seen["j0"] += int((rel & (w["offset"] == 0) & (L > 1)).sum())
                    seen["jlast"] += int((rel & (w["offset"] == L - 1) & (L > 1)).sum())
                    seen["rew0"] += int((rel & (w["rew"] == 0)).sum())
                    seen["rewm1"] += int((rel & (w["rew"] == -1)).sum())
                    seen["refused"] += int((w["slot_idx"] < 0).sum())
                    seen["keep"] += int((~rel & (w["slot_idx"] >= 0)).sum())
                    if injected:
                        seen["beyond"] += int((r["choice"] > L - 1)[rel].sum())
                    for b in np.flatnonzero((L > 0) & (L < window)):
                        last = int(held[idx[b]]) + (L[b] - 1) * STRIDE
                        if last + STRIDE >= n_rows:
                            seen["newest"] += 1                               # cut by the ring's newest rows
                        elif r["rows"]["done"][last] == 0:
                            seen["truncation"] += 1                           # the successor exists and no flag is set: s' != s
                    seen["wrap"] += int(((idx >= 0) & (idx < length) & (idx + (L - 1) * STRIDE >= cap) & (L > 1)).sum())
        print(case, seen)
        need = [k for k in seen if not (k in ("beyond",) and B == 8)]
        assert all(seen[k] > 0 for k in need), (case, seen)


# ------------------------------------------------------------------------------------------ 2. no hindsight: k_batch_from_index's bits
@pytest.mark.parametrize("case", ["goal-260", "shared-32"])
def test_ratio_zero_and_window_one_leave_what_sample_at_leaves(case):
    ring = "101-wrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    _, (A, Bv) = engines(case, ring, count=2)
    keep = stage(Bv, torch.as_tensor(r["idx"], device=DEV))
    want = {k: Bv.debug_read(k) for k in ("X", "Xn", "rew", "done")}
    want_index = Bv.read_batch()["index"]
    for window, ratio, choice in ((1, 1.0, None), (64, 0.0, None), (64, 1.0, np.full(B, -1, np.int32))):
        A.hindsight_configure(**config(case, window, ratio))
        stage_h(A, r["idx"], choice)
        got = read_slot(A, o, a)
        if window == 1 and ratio == 1.0:                                  # every accepted row relabelled with its own arrival: reward 0, s untouched but the goal
            assert (got["offset"][got["slot_idx"] >= 0] == 0).all() and (got["rew"][got["slot_idx"] >= 0] == 0).all()
            hr.check(hr.stage(r["fields"], r["geom"], r["idx"], config(case, 1, 1.0), seed=SEED, hctr=0), got, ALL_KEYS)      # X, Xn: own arrivals as goals
            continue
        for k in ("X", "Xn", "rew", "done"):
            assert same_bits(A.debug_read(k), want[k]), (window, ratio, k)
        assert np.array_equal(A.read_batch()["index"], want_index) and (got["offset"] == -1).all() and (got["goal_slot"] == -1).all()
    del keep


# ------------------------------------------------------------------------------------------ 3. the uniform draw
def test_sample_hindsight_draws_what_sample_draws_and_ticks_once():
    case, ring = "goal-260", "96-wrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    _, (A, Bv) = engines(case, ring, count=2)
    A.hindsight_configure(**config(case, 9, 0.8))
    for call in range(3):
        A.rb_sample_hindsight()
        Bv.rb_sample()
        idx = Bv.read_batch()["index"]
        got = read_slot(A, o, a)
        assert np.array_equal(got["slot_idx"], idx.astype(np.int32)), call
        want = hr.stage(r["fields"], r["geom"], idx, config(case, 9, 0.8), seed=SEED, hctr=call)
        hr.check(want, got, ALL_KEYS)
        assert 0.6 * B < (got["offset"] >= 0).sum() < 0.95 * B
    A.rb_sample()                                                         # the counters agree: the next plain draws are the same
    Bv.rb_sample()
    assert np.array_equal(A.read_batch()["index"], Bv.read_batch()["index"]) and A.hindsight_stats()["native_draws"] == 3
    with pytest.raises(P.EngineError, match="not filled by a hindsight"):  # a plain refill: no longer a hindsight slot
        A.hindsight_info_device(torch.zeros(B, dtype=torch.int32, device=DEV).data_ptr(), 1, 0, 1, stream())


# ------------------------------------------------------------------------------------------ 4. refused rows and refused calls
def test_refused_rows_become_zero_records_and_are_counted():
    case, ring = "straddle-64", "96-unwrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    length = r["geom"]["length"]
    _, (eng,) = engines(case, ring)
    eng.hindsight_configure(**config(case, 64, 1.0))
    idx = np.array([-1, length, 2 ** 40, -2 ** 40, length + 7, 95] * 11, np.int64)[:B]      # (95: an unfilled slot of the unwrapped ring)
    idx[5::6] = np.arange(len(idx[5::6]))                                 # every sixth row is a real one
    stage_h(eng, idx)
    got = read_slot(eng, o, a)
    bad = (idx < 0) | (idx >= length)
    assert bad.sum() > 50 and (got["slot_idx"][bad] == -1).all() and (got["offset"][bad] == -1).all() and (got["goal_slot"][bad] == -1).all()
    for k in ("X", "Xn", "rew", "done"):
        assert same_bits(got[k][bad], np.zeros_like(got[k][bad])), k
    hr.check(hr.stage(r["fields"], r["geom"], idx, config(case, 64, 1.0), seed=SEED, hctr=0), got, ALL_KEYS)
    assert eng.hindsight_stats()["rows_refused"] == int(bad.sum())


def test_refused_calls_change_nothing():
    case, ring = "goal-8", "96-unwrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    _, (eng, empty) = engines(case, ring, count=2, fill=False)
    rows = r["rows"]
    eng.rb_extend(*[rows[k][:80] for k in ("obs", "act", "rew", "nobs")], rows["done"][:80] != 0)
    idx = torch.arange(B, device=DEV)
    eng.rb_sample()
    before = engine_state(eng, "slot")
    gen = eng.batch_generation()

    def refused(match, fn):
        with pytest.raises(P.EngineError, match=match):
            fn()
        assert eng.batch_generation() == gen
    refused("not configured", eng.rb_sample_hindsight)
    refused("not configured", lambda: eng.rb_sample_hindsight_device(idx.data_ptr(), 1, 0, 1, B, stream()))
    good = config(case, 9, 0.8)
    for over, match in ((dict(dim=0), "goal_dim"), (dict(dim=9), "goal_dim"), (dict(achieved=5), "outside"), (dict(desired=-1), "outside"),
                        (dict(desired=1), "overlap"), (dict(window=0), "window"), (dict(window=65), "window"), (dict(stride=0), "stride"),
                        (dict(threshold=-0.1), "threshold"), (dict(threshold=float("inf")), "threshold"), (dict(threshold=float("nan")), "threshold"),
                        (dict(ratio=-0.01), "ratio"), (dict(ratio=1.01), "ratio"), (dict(ratio=float("nan")), "ratio")):
        refused(match, lambda: eng.hindsight_configure(**dict(good, **over)))
    refused("not configured", eng.rb_sample_hindsight)                     # a refused configure configured nothing
    eng.hindsight_configure(**good)
    refused("n must equal", lambda: eng.rb_sample_hindsight_device(idx.data_ptr(), 1, 0, 1, B - 1, stream()))
    refused("idx", lambda: eng.rb_sample_hindsight_device(0, 1, 0, 1, B, stream()))
    refused("stride", lambda: eng.rb_sample_hindsight_device(idx.data_ptr(), 0, 0, 1, B, stream()))
    refused("choice", lambda: eng.rb_sample_hindsight_device(idx.data_ptr(), 1, idx.data_ptr(), 0, B, stream()))
    eng.rb_pin(10)
    refused("pinned", eng.rb_sample_hindsight)
    refused("pinned", lambda: eng.rb_sample_hindsight_device(idx.data_ptr(), 1, 0, 1, B, stream()))
    eng.rb_pin(0)
    assert_same_state(before, engine_state(eng, "slot"))
    assert eng.hindsight_stats() == dict(native_draws=0, rows_relabelled=0, rows_refused=0, rows_reward_zero=0)
    empty.hindsight_configure(**good)
    with pytest.raises(P.EngineError, match="empty"):
        empty.rb_sample_hindsight()
    eng.rb_sample_hindsight()                                             # and now it runs
    assert eng.batch_generation() == gen + 1 and eng.hindsight_stats()["native_draws"] == 1


def test_a_refused_call_leaves_the_run_ahead_chain_intact():
    """two engines run periods; one is asked, in between, for hindsight calls that are refused: the same bits afterwards"""
    case, ring = "goal-260", "96-wrapped"
    _, (A, Bv) = engines(case, ring, count=2)
    for k in range(3):
        A.step_period()
        Bv.step_period()
        with pytest.raises(P.EngineError, match="not configured"):
            A.rb_sample_hindsight()
        with pytest.raises(P.EngineError):
            A.hindsight_configure(**dict(config(case, 9, 0.8), window=0))
    assert_same_state(A, Bv, "slot", "noise")


# ------------------------------------------------------------------------------------------ 5. downstream
def test_update_qnets_on_a_hindsight_batch_equals_the_restatements_batch_loaded():
    case, ring = "goal-260", "101-wrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    _, (A, Bv) = engines(case, ring, count=2)
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for e in (A, Bv):
        e.set_noise(_lib.SITE_CRITIC, eps)
    A.hindsight_configure(**config(case, 9, 1.0))
    stage_h(A, r["idx"])
    w = expected(case, ring, 9, 1.0, 0, False)
    five = tuple(torch.as_tensor(x, device=DEV) for x in (w["obs"], w["act"], w["rew"], w["nobs"], w["done"] != 0))
    load_device(Bv, five)
    A.update_qnets()
    Bv.update_qnets()
    assert same_bits(td_of(A), td_of(Bv)) and np.isfinite(td_of(A)).all()
    assert_same_state(A, Bv, "noise")
    A.update_actor()
    Bv.update_actor()
    assert_same_state(A, Bv)


def test_the_buffers_handles_and_read_outs():
    case, ring = "goal-260", "96-wrapped"
    o, a, B = CASES[case][:3]
    r = ring_of(case, ring)
    cfg = P.launcher.job_config("sac", "PointGoal-native", SEED, num_envs=STRIDE, batch_size=B, rb_capacity=RINGS[ring][0])
    torch.manual_seed(SEED)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -1.0, F), np.full(a, 1.0, F), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=SEED)
    track(agent.engine)
    rb, rows = agent.rb, r["rows"]
    with pytest.raises(RuntimeError, match="configure_hindsight"):
        rb.sample_hindsight(B)
    for lo in range(0, len(rows["rew"]), 64):
        rb.extend({"observations": rows["obs"][lo:lo + 64], "actions": rows["act"][lo:lo + 64], "rewards": rows["rew"][lo:lo + 64].reshape(-1, 1),
                   "next_observations": rows["nobs"][lo:lo + 64], "terminations": (rows["done"][lo:lo + 64] != 0).reshape(-1, 1)})
    layout = envs.GOAL_LAYOUTS[envs.kind_of("pointgoal")]
    rb.configure_hindsight(**layout, ratio=1.0, window=9)                 # stride: the engine's max_envs = the env count
    h = rb.sample_hindsight_at(r["idx"], r["choice"])
    want = hr.stage(r["fields"], r["geom"], r["idx"], dict(layout, ratio=1.0, window=9, stride=STRIDE), choice=r["choice"])
    info = h.hindsight_info()
    assert np.array_equal(info["offset"].cpu().numpy(), want["offset"]) and np.array_equal(info["goal_index"].cpu().numpy(), want["goal_slot"])
    dev = h.on_device()
    assert same_bits(dev["observations"].cpu().numpy(), want["obs"]) and same_bits(dev["next_observations"].cpu().numpy(), want["nobs"])
    assert same_bits(dev["rewards"].cpu().numpy().reshape(-1), want["rew"])
    assert same_bits(h["observations"], want["obs"]) and same_bits(np.asarray(h["rewards"], F).reshape(-1), want["rew"])      # read_batch
    assert (want["rew"][want["offset"] >= 0] != r["fields"]["rew"][r["idx"][want["offset"] >= 0]]).any()                  # it shows relabelled rows
    agent.update_qnets(h)
    assert np.isfinite(agent.td_errors().cpu().numpy()).all()
    agent.update_actor(h)
    h2 = rb.sample_hindsight(B)                                           # the staleness rule of the batch generation
    with pytest.raises(P.StaleBatchError):
        agent.update_qnets(h)
    with pytest.raises(P.StaleBatchError):
        h.hindsight_info()
    agent.update_qnets(h2)
    plain = rb.sample(B)
    with pytest.raises(RuntimeError, match="not sampled with sample_hindsight"):
        plain.hindsight_info()
    with pytest.raises(ValueError, match="indices"):
        rb.sample_hindsight_at(r["idx"][:-1])


def run_30(seed, touch):
    cfg = P.launcher.job_config("sac", "PointGoal-native", seed, num_envs=STRIDE, learning_starts=40, batch_size=64, num_timesteps=40 + 30 * STRIDE - 1,
                                eval_every=10 ** 9, rb_capacity=512)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, F), np.full(2, 1.0, F), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    touch(agent)
    env = track(envs.NativeVecEnv("pointgoal", STRIDE, seed=seed, device=DEV))
    loop.train(cfg, env, agent, device_env=True)
    return agent


def test_an_engine_that_never_configures_hindsight_trains_as_it_did():
    """30 iterations of loop.train, fused: an engine whose library carries the feature but never uses it, against one that is asked for
    refused hindsight calls before the run -- the same bits, and nothing of the feature was allocated or counted"""
    def poke(agent):
        with pytest.raises(P.EngineError):
            agent.engine.rb_sample_hindsight()
    A, Bv = run_30(2, lambda agent: None), run_30(2, poke)
    assert A.qnet_updates_so_far == Bv.qnet_updates_so_far == 30
    assert_same_state(A.engine, Bv.engine, "slot", "noise", "ring")
    assert A.engine.hindsight_stats() == dict(native_draws=0, rows_relabelled=0, rows_refused=0, rows_reward_zero=0)


def test_train_with_hindsight_runs_the_call_sequence():
    seed = 1
    cfg = P.launcher.job_config("sac", "PointGoal-native", seed, num_envs=STRIDE, learning_starts=240, batch_size=64, num_timesteps=240 + 20 * STRIDE - 1,
                                eval_every=10 ** 9, rb_capacity=4096)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, F), np.full(2, 1.0, F), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    env = track(envs.NativeVecEnv("pointgoal", STRIDE, seed=seed, device=DEV))
    with pytest.raises(ValueError, match="needs fused=False"):
        loop.train(cfg, env, agent, device_env=True, hindsight=dict(env.goal_layout))
    assert agent.engine.hindsight_stats()["native_draws"] == 0 and agent.rb._hindsight is None      # a refused run configured nothing
    metrics = loop.train(cfg, env, agent, device_env=True, fused=False, hindsight=dict(env.goal_layout, window=env.horizon))
    st = agent.engine.hindsight_stats()
    assert agent.qnet_updates_so_far == 20 and st["native_draws"] == 20 and st["rows_refused"] == 0
    assert 0.6 * 20 * 64 < st["rows_relabelled"] < 0.95 * 20 * 64 and 0 < st["rows_reward_zero"] < st["rows_relabelled"]      # ratio 0.8
    assert all(np.isfinite(v) for v in metrics.values())


# ------------------------------------------------------------------------------------------ 6. learned end to end
def test_sac_learns_the_goal_task_with_hindsight():
    """SAC, default hyper-parameters, loop.train(device_env=True, fused=False, hindsight=...) on 4 envs of PointGoal-native for the
    recorded budget, then the greedy return over 16 envs for one horizon.  The bar is not this engine's: the oracle agent on the host twin
    with tests/hindsight_ref.py as its sampler, 3 seeds at the same budget (profiles/hindsight.json, tools/hindsight_probe.py --oracle);
    the result must be at least the worst oracle seed minus the spread (max - min) of the three -- the noise one GPU seed is subject to."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hindsight.json")) as f:
        rec = json.load(f)["learning"]
    b, seed, episodes = rec["budget"], 0, rec["episodes"]
    assert b["updates"] <= 20000 and rec["pass_at"] == rec["worst_trained"] - (rec["best_trained"] - rec["worst_trained"])
    steps = b["learning_starts"] + b["updates"] * b["num_envs"]
    mk = lambda n: P.launcher.job_config("sac", "PointGoal-native", seed, num_envs=n, learning_starts=b["learning_starts"], batch_size=b["batch_size"],
                                         num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)
    cfg, wide = mk(b["num_envs"]), mk(episodes)                           # (max_envs: the evaluation's 16 rows in one call)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, F), np.full(2, 1.0, F), torch.device(DEV), wide,
                    P.ReplayBuffer(wide.rb_capacity), seed=seed)
    track(agent.engine)
    eval_env = track(envs.NativeVecEnv("pointgoal", episodes, seed=seed + rec["eval_seed_offset"], device=DEV))
    before = envs.greedy_returns(eval_env, agent, episodes)
    env = track(envs.NativeVecEnv("pointgoal", cfg.num_envs, seed=seed, device=DEV))
    loop.train(cfg, env, agent, device_env=True, fused=False,
               hindsight=dict(env.goal_layout, ratio=rec["ratio"], window=env.horizon, stride=cfg.num_envs))
    after = envs.greedy_returns(eval_env, agent, episodes)
    st = agent.engine.hindsight_stats()
    print(f"greedy return {before['return']:.2f} -> {after['return']:.2f} after {agent.qnet_updates_so_far} updates; oracle seeds "
          f"{[r['trained'] for r in rec['seeds']]}, pass at {rec['pass_at']:.2f}; without hindsight the oracle reached "
          f"{[r['trained'] for r in rec['without_hindsight']]}")
    assert agent.qnet_updates_so_far == b["updates"] == st["native_draws"] and st["rows_refused"] == 0 and after["bad_actions"] == 0
    assert after["return"] >= rec["pass_at"], (before["return"], after["return"], rec["pass_at"])
