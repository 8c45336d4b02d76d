"""GPU: the native rollout (include/sactd3_rollout.h, csrc/env_kernels.h: k_env_step_rec, loop.NativeRollout) -- the records the env
step emits against the float64 model and its a-priori bound (tests/env_model.py), the new route against the existing one
(env.step + the glue of loop.DeviceRollout.advance + rb.extend) bit for bit, the rollout handle against loop.DeviceRollout, the
ordering of the append without a host wait, a training run either way, an engine beside it, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import env_model as em
from tests.gpu_support import (DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, loop, same_bits, track)  # noqa: F401
from tests.helpers import DIMS, synth_transitions

pytestmark = pytest.mark.gpu
envs = P.envs
KINDS = ["pendulum", "cartpole"]
BAD = (np.nan, np.inf, -np.inf)


def new_env(name, n, seed=0, horizon=None):
    return track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=horizon))


def host(x):
    return x.cpu().numpy()


def dims_of(name):
    return envs.SPECS[envs.kind_of(name)][:3]


def twin_engines(name, n, cap, B=64, algo="sac", seed=4):
    """two engines at the env's dims with the same parameters, each behind a ReplayBuffer -> [(engine, rb), (engine, rb)]"""
    _, engs, _ = build_engines(algo, dims_of(name), B, count=2, seed=seed, cap=cap, max_envs=n)
    out = []
    for e in engs:
        rb = P.ReplayBuffer(cap)
        rb._bind(e)
        out.append((e, rb))
    return out


@functools.lru_cache(maxsize=None)
def engine_layout(name):
    """(record_floats, next_obs_offset, next_obs_width) the engine reports for the env's dims: asked once per kind"""
    _, (eng,), _ = build_engines("sac", dims_of(name), 64, seed=0, cap=256, max_envs=4, push=False)
    lay = eng.rb_layout()
    eng.close()
    return lay["record_floats"], lay["next_obs_offset"], lay["next_obs_width"]


def fields(rec, layout, o, a=1):
    """a slab on the host -> its fields and its pads"""
    L, off, width = layout
    tail = off + width
    pads = np.concatenate([rec[:, o + a:off], rec[:, off + o:tail], rec[:, tail + 2:]], 1)
    return {"s": rec[:, :o], "a": rec[:, o:o + a], "next": rec[:, off:off + o], "r": rec[:, tail], "d": rec[:, tail + 1], "pads": pads}


def new_agent(name, cfg, seed):
    o, a, bound = dims_of(name)
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    return agent


def job_cfg(algo, name, seed, n, learning_starts, updates=0, batch_size=64, cap=4096, **over):
    return P.launcher.job_config(algo, name, seed, num_envs=n, learning_starts=learning_starts, batch_size=batch_size,
                                 num_timesteps=learning_starts + updates * n - 1, eval_every=10 ** 9, rb_capacity=cap, **over)


def env_books(env):
    st, books = env.state(), env.episode_stats()
    return {**{"state." + k: v for k, v in st.items()}, **{"books." + k: np.asarray(v) for k, v in books.items()}}


def same_books(x, y):
    a, b = env_books(x), env_books(y)
    return list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)


def ring_of(rb):
    return {k: host(v) for k, v in rb.rows(np.arange(len(rb))).items()} if len(rb) else {}


def same_ring(x, y):
    a, b = ring_of(x), ring_of(y)
    return len(x) == len(y) and list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------ 1. the records against the float64 model
@pytest.mark.parametrize("n", [1, 4, 257])
@pytest.mark.parametrize("name", KINDS)
def test_records_from_planted_states_against_the_float64_model(name, n):
    """One step_records per round from em.planted states (in rounds until every planted state had its step; then one round per
    action that is not a number), decoded into what em.check_step takes.  What a record does not carry is taken from where the
    step left it: `ended` from the step count behind the step (0 iff the episode ended), `truncated` = ended and not d, and the
    arrival observation of a TERMINATED env -- overwritten by the reset and stored nowhere -- from the model itself."""
    kind, seed = em.KINDS[name], 21
    o = em.OB_DIM[kind]
    env = new_env(name, n, seed=seed)
    env.reset(seed=seed)
    m = len(em.planted(kind)[1])
    rng = np.random.default_rng(n)
    rounds = [(offset, None) for offset in range(0, m if n < m else 1, n)] + [(7 + k, v) for k, v in enumerate(BAD)]
    worst, flags, counted = 0.0, np.zeros(3, int), 0
    for layout in (engine_layout(name), (28, 8, 12)):                     # the engine's own, and one with pads everywhere
        obs = torch.full((n, o + 2), -7.0, device=DEV)                    # a stride wider than the row: the rest survives
        rec = torch.full((n + 1, layout[0]), -7.0, device=DEV)            # one row more than the env has: it survives
        for offset, bad in rounds:
            phys, steps, act = em.batch(kind, n, offset, rng)
            if bad is not None:
                act[(offset * 3) % n, 0] = bad
                counted += 1
            before = {"phys": phys, "steps": steps, "episode": (np.arange(n) % 3).astype(np.uint32), "returns": rng.standard_normal(n).astype(np.float32)}
            assert em.conditioned(kind, before, act).all()                # decided on the CPU by the model alone
            env.set_state(before)
            a_dev = torch.as_tensor(act, device=DEV)
            env.step_records(a_dev, layout, rec[:n], obs)
            after = env.state()
            got_rec, got_obs = host(rec), host(obs)
            assert (got_rec[n] == np.float32(-7.0)).all() and (got_obs[:, o:] == np.float32(-7.0)).all()
            f = fields(got_rec[:n], layout, o)
            assert f["pads"].size > 0 and same_bits(f["pads"], np.zeros_like(f["pads"]))                  # every pad float: +0
            assert same_bits(f["a"], act)                                                                 # byte for byte, NaN and inf included
            assert set(np.unique(f["d"])) <= {0.0, 1.0}
            want_s, bound_s = em.observe64(kind, phys)
            assert (np.abs(f["s"].astype(np.float64) - want_s) <= bound_s).all()                          # s: the state BEFORE the step
            term = f["d"] == 1.0
            ended = after["steps"] == 0
            trunc = ended & ~term
            model = em.physics(kind, phys, act)
            final = np.where(term[:, None], np.stack([c.v for c in model["obs"]], 1).astype(np.float32), f["next"])
            assert same_bits(f["next"][~trunc], got_obs[~trunc, :o])                                      # the stored-next rule, by bits
            if trunc.any():
                assert not np.array_equal(f["next"][trunc], got_obs[trunc, :o])
            got = {"obs": got_obs[:, :o], "final_obs": final, "reward": f["r"], "terminated": term, "truncated": trunc, "ended": ended}
            worst = max(worst, em.check_step(kind, seed, env.horizon, before, act, got, after))
            flags += [int(term.sum()), int(trunc.sum()), int(ended.sum())]
            assert np.isfinite(after["phys"]).all()
    print(f"{name} n={n}: worst |err| / bound {worst:.3f}; terminated, truncated, ended {flags}")
    assert 0.0 < worst <= 1.0
    assert flags[1] >= 1 and flags[2] == flags[0] + flags[1] and (flags[0] >= 4) == (name == "cartpole")
    env.reset(seed=seed)                                                  # the counter restarts ...
    a_dev = torch.as_tensor(np.array([[BAD[i % 3]] for i in range(n)], np.float32), device=DEV)
    env.step_records(a_dev, layout, rec[:n], obs)
    assert env.episode_stats()["bad_actions"] == n and counted == 6       # ... and counts what never reaches the state


# ------------------------------------------------------------------------------------------ 2. the same bits as the existing route
def run_both_routes(name, n, cap, steps=40, pin=0, prio=False):
    """twin envs (horizon 5: truncations) from planted and random states (the cart-pole's near its limits: terminations), twin
    engines; one side env.step + the glue of DeviceRollout.advance + rb.extend, the other step_records + extend_records"""
    kind, seed = em.KINDS[name], 11
    o, a, bound = dims_of(name)
    (eA, rbA), (eB, rbB) = twin_engines(name, n, cap)
    if pin:
        pre = [t.numpy() for t in synth_transitions(pin, o, a, bound, seed=2)]
        for e, rb in ((eA, rbA), (eB, rbB)):
            e.rb_extend(*pre)
            rb.pin()
    if prio:
        rbA.enable_priorities()
        rbB.enable_priorities()
    A, Bv = new_env(name, n, seed=seed, horizon=5), new_env(name, n, seed=seed, horizon=5)
    rng = np.random.default_rng(n)
    phys, _, _ = em.batch(kind, n, 0, rng, horizon=5)
    steps0 = (np.arange(n) % 5).astype(np.int32)
    if name == "cartpole":                # two carts on their way out: beyond 2.4 on their third step, whatever the force (|x_dot| stays above 1.4)
        phys[:2], steps0[:2] = [[2.3, 2.0, 0.0, 0.0], [-2.3, -2.0, 0.0, 0.0]], 0
    start = {"phys": phys, "steps": steps0}
    layout = eB.rb_layout()
    rec = torch.zeros((n, layout["record_floats"]), device=DEV)
    obsB = torch.zeros((n, o), device=DEV)
    for env in (A, Bv):
        env.reset(seed=seed)
        env.set_state(start)
    act = torch.zeros((n, a), device=DEV)
    obsA = A.step(act)[0]                                                 # one step that is not recorded: the observations of the planted states
    Bv.step_records(act, layout, rec, obsB)
    gen = torch.Generator().manual_seed(n)
    term_seen = trunc_seen = 0
    for t in range(steps):
        act = ((torch.rand((n, a), generator=gen) * 2.4 - 1.2) * bound).to(DEV)      # the same actions for both, a little beyond the bounds
        arrived, rew, term, trunc, infos = A.step(act)
        stored = torch.where(trunc.reshape(-1, 1), infos["final_observation"], arrived)
        ended = term.reshape(-1, 1)
        rbA.extend({"observations": obsA, "next_observations": stored, "actions": act, "rewards": rew.reshape(-1, 1), "terminations": ended, "dones": ended})
        obsA = arrived
        Bv.step_records(act, layout, rec, obsB)
        rbB.extend_records(rec)
        assert same_bits(host(obsA), host(obsB)), t
        assert same_books(A, Bv), t
        assert same_ring(rbA, rbB), t
        term_seen, trunc_seen = term_seen + int(term.sum()), trunc_seen + int(trunc.sum())
    assert len(rbA) == len(rbB) == min(cap, pin + steps * n)
    assert trunc_seen >= n and (term_seen >= 1) == (name == "cartpole")      # both kinds of episode end (the pendulum never terminates)
    assert (pin + steps * n > cap) and (cap - pin) % n                     # the ring wrapped, and one slab was split across the wrap
    return eA, eB


@pytest.mark.parametrize("n,cap", [(4, 150), (257, 1899)])
@pytest.mark.parametrize("name", KINDS)
def test_step_records_and_extend_records_leave_what_the_existing_route_leaves(name, n, cap):
    eA, eB = run_both_routes(name, n, cap)
    assert_same_state(eA, eB, "ring")


def test_the_same_behind_a_pinned_prefix():
    eA, eB = run_both_routes("cartpole", 4, 150, pin=37)
    assert eA.rb_pinned() == eB.rb_pinned() == 37
    assert_same_state(eA, eB, "ring")


def test_the_same_with_priorities_enabled():
    eA, eB = run_both_routes("pendulum", 4, 150, prio=True)
    assert_same_state(eA, eB, "prio", "ring")


# ------------------------------------------------------------------------------------------ 3. the rollout handle
@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("name", KINDS)
def test_native_rollout_against_device_rollout(name, algo):
    n, seed, pairs, starts_at = 4, 6, 30, 12
    cfg = job_cfg(algo, name, seed, n, learning_starts=starts_at * n, cap=100, action_repeat=2)
    agents = [new_agent(name, cfg, seed) for _ in range(2)]
    es = [new_env(name, n, seed=seed, horizon=7) for _ in range(2)]
    old = loop.DeviceRollout(es[0], agents[0], seed, cfg.learning_starts, cfg.action_repeat)
    new = loop.NativeRollout(es[1], agents[1], seed, cfg.learning_starts, cfg.action_repeat)
    held = (new.obs.data_ptr(), new.actions.data_ptr())
    assert same_bits(host(old.obs), host(new.obs))
    for t in range(pairs):
        for ag in agents:
            ag.timesteps_so_far = t * n                                   # host state: the first pairs are random, the later ones explore
        old.choose()
        new.choose()
        assert same_bits(host(old.actions), host(new.actions)), t
        old.advance()
        new.advance()
        assert same_bits(host(old.obs), host(new.obs)), t
        assert old.steps == new.steps == t + 1
    assert (new.obs.data_ptr(), new.actions.data_ptr()) == held           # views of the bound buffers: nothing was allocated
    assert same_ring(agents[0].rb, agents[1].rb) and len(agents[1].rb) == 100
    assert same_books(es[0], es[1])
    eA, eB = agents[0].engine, agents[1].engine
    assert eA.predict_device_stats() == eB.predict_device_stats() and eB.predict_device_stats()["calls"] == (pairs - starts_at) // 2
    assert same_bits(eA.read_noise(_lib.SITE_PREDICT), eB.read_noise(_lib.SITE_PREDICT))
    assert new.stats() == dict(random_choices=starts_at // 2, policy_choices=(pairs - starts_at) // 2, steps=pairs, rows_appended=pairs * n)
    assert es[1].state()["draws"].tolist() == [starts_at // 2] * n
    assert_same_state(eA, eB, "ring")
    new.close()


# ------------------------------------------------------------------------------------------ 4. ordering without a host sync
def busy(x):
    """work queued on the torch stream in front of what follows"""
    for _ in range(12):
        x = torch.mm(x, x).clamp_(-1.0, 1.0)
    return x


@pytest.mark.parametrize("name", KINDS)
def test_the_append_is_ordered_on_the_gpu(name):
    n, seed, cap = 257, 9, 1000
    o, a, bound = dims_of(name)
    pairs = twin_engines(name, n, cap)
    seen = []
    x = torch.rand((1536, 1536), device=DEV)
    for wait, (eng, rb) in zip((False, True), pairs):
        env = new_env(name, n, seed=seed, horizon=3)
        layout = eng.rb_layout()
        rec, obs = torch.zeros((n, layout["record_floats"]), device=DEV), torch.zeros((n, o), device=DEV)
        env.reset(seed=seed)
        act = env.action_space.sample()
        settle = (lambda: (torch.cuda.synchronize(), eng.sync())) if wait else (lambda: None)
        settle()
        out = []
        for k in range(3):                                                # the third step rewrites the slab while the second append may still read it
            if not wait:
                busy(x)
            env.step_records(act, layout, rec, obs)
            settle()
            rb.extend_records(rec)
            settle()
            out.append(rb.rows(np.arange((k + 1) * n)))                   # read out at once: it sees the new rows
            settle()
        seen.append([{k: host(v) for k, v in rows.items()} for rows in out] + [env_books(env)])
    for got, want in zip(*seen):
        assert list(got) == list(want) and all(same_bits(got[k], want[k]) for k in got)
    first, last = seen[0][0], seen[0][2]
    assert all(same_bits(first[k], last[k][:n]) for k in first)             # the first slab's rows are still what they were
    assert not same_bits(last["observations"][:n], last["observations"][n:2 * n])


@pytest.mark.parametrize("name", KINDS)
def test_rollout_calls_back_to_back_equal_calls_with_a_wait_after_each(name):
    n, seed = 4, 5
    cfg = job_cfg("sac", name, seed, n, learning_starts=3 * n, cap=256)
    agents = [new_agent(name, cfg, seed) for _ in range(2)]
    x = torch.rand((1536, 1536), device=DEV)
    ros = [loop.NativeRollout(new_env(name, n, seed=seed, horizon=4), ag, seed, cfg.learning_starts, 1) for ag in agents]
    for wait, ro, ag in zip((False, True), ros, agents):
        for t in range(8):
            ag.timesteps_so_far = t * n
            if not wait:
                busy(x)
            ro.choose()
            if wait:
                torch.cuda.synchronize(), ag.engine.sync()
            ro.advance()
            if wait:
                torch.cuda.synchronize(), ag.engine.sync()
    assert same_ring(agents[0].rb, agents[1].rb) and len(agents[0].rb) == 8 * n
    assert same_bits(host(ros[0].obs), host(ros[1].obs)) and same_bits(host(ros[0].actions), host(ros[1].actions))
    assert same_books(ros[0].env, ros[1].env)
    for ro in ros:
        ro.close()


# ------------------------------------------------------------------------------------------ 5. training
@pytest.mark.parametrize("one_stream", [False, True])
@pytest.mark.parametrize("algo,name", [("sac", "pendulum"), ("td3", "cartpole")])
def test_training_through_the_native_rollout_is_training_through_the_device_rollout(algo, name, one_stream):
    """one_stream: the engine's own stream is torch's current stream around loop.train, so the env's kernels and the engine's share a
    stream (the configuration profiles/native_rollout.json measures as train_on_engine_stream): the same bits either way"""
    n, seed, updates = 4, 3, 60
    cfg = job_cfg(algo, name, seed, n, learning_starts=300, updates=updates, batch_size=256, cap=1 << 12)
    agents, es = [], []
    for native in (True, False):
        agent, env = new_agent(name, cfg, seed), new_env(name, n, seed=seed, horizon=25)
        if one_stream:
            with torch.cuda.stream(torch.cuda.ExternalStream(agent.engine.device_handles()[0])):
                loop.train(cfg, env, agent, device_env=True, native_rollout=native)
            agent.engine.sync()
        else:
            loop.train(cfg, env, agent, device_env=True, native_rollout=native)
        agents.append(agent)
        es.append(env)
    assert agents[0].qnet_updates_so_far == agents[1].qnet_updates_so_far == updates
    assert agents[0].engine.predict_device_stats() == agents[1].engine.predict_device_stats()
    assert same_ring(agents[0].rb, agents[1].rb) and same_books(es[0], es[1])
    assert_same_state(agents[0].engine, agents[1].engine, "slot", "noise", "ring")


# ------------------------------------------------------------------------------------------ 6. an engine beside it
def test_an_engine_trains_the_same_bits_with_a_rollout_bound_to_another_engine():
    N = 12
    _, (A, B), (o, a, bound) = build_engines("sac", DIMS["hopper"], 64, count=2, seed=4, cap=2048)
    data = synth_transitions(1024, o, a, bound, seed=6)
    for e in (A, B):
        e.rb_extend(*[t.numpy() for t in data])
    cfg = job_cfg("sac", "cartpole", 1, 4, learning_starts=8, cap=512)
    agent = new_agent("cartpole", cfg, 1)
    ro = loop.NativeRollout(new_env("cartpole", 4, seed=1), agent, 1, cfg.learning_starts, 1)
    for i in range(N):
        A.step(i % 3 == 0)
        B.step(i % 3 == 0)
        for _ in range(3):
            agent.timesteps_so_far += 4
            ro.choose()
            ro.advance()                                                  # on torch's stream and the other engine's, while B's iteration runs
    torch.cuda.synchronize()
    assert_same_state(A, B, "slot", "noise")
    assert ro.stats()["steps"] == 3 * N and len(agent.rb) == 3 * N * 4
    ro.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing():
    n, seed = 4, 2
    (eng, rb), (other, _) = twin_engines("pendulum", n, 128)
    _, (cart,), _ = build_engines("sac", dims_of("cartpole"), 64, seed=0, cap=128, max_envs=n, push=False)
    env, wide = new_env("pendulum", n, seed=seed), new_env("pendulum", n + 4, seed=seed)
    lib = eng.lib
    layout = eng.rb_layout()
    L = (layout["record_floats"], layout["next_obs_offset"], layout["next_obs_width"])
    rec = torch.zeros((n + 1, L[0]), device=DEV)
    obs, act = torch.zeros((n, 3), device=DEV), torch.zeros((n, 1), device=DEV)
    env.reset(seed=seed)
    env.step_records(act, layout, rec[:n], obs)
    rb.extend_records(rec[:n])
    torch.cuda.synchronize()
    eng.sync()
    before = (env_books(env), ring_of(rb), len(rb), host(rec), host(obs), eng.boundary_stats())      # (the counters last: a read-out counts too)
    room = np.zeros(n * L[0] + 4, np.float32)
    host_rec = room[(-room.ctypes.data % 16) // 4:][:n * L[0]].reshape(n, L[0])      # 16-byte aligned, on the host

    def env_step(layout3, rec_ptr):
        lay = _lib.CRecordLayout(*layout3)
        return lib.sactd3_rollout_env_step(env._h, act.data_ptr(), 1, C.byref(lay), C.c_void_p(rec_ptr), obs.data_ptr(), 3, None)

    def create(engine, e, rec_ptr=None):
        buf = _lib.CRolloutBuffers(obs.data_ptr(), 3, act.data_ptr(), 1, rec.data_ptr() if rec_ptr is None else rec_ptr)
        h = C.c_void_p()
        rc = lib.sactd3_rollout_create(engine._h, e._h, C.byref(buf), None, C.byref(h))
        assert not h.value
        return rc, lib.sactd3_rollout_last_error(None).decode()

    def extend(ptr, flags=_lib.SRC_ORDERED, count=n):
        return lib.sactd3_rb_extend_records_device(eng._h, C.c_void_p(ptr), count, None, flags), lib.sactd3_last_error(eng._h).decode()

    def env_text():
        return lib.sactd3_env_last_error(env._h).decode()

    rc, text = create(cart, env)                                          # mismatched dims
    assert rc == _lib.EINVAL and "ob_dim" in text
    rc, text = create(eng, wide)                                          # num_envs > max_envs
    assert rc == _lib.EINVAL and "max_envs" in text
    rc, text = create(eng, env, rec.data_ptr() + 4)                       # a misaligned slab, to all three entry points
    assert rc == _lib.EINVAL and "aligned" in text
    assert env_step(L, rec.data_ptr() + 4) == _lib.EINVAL and "aligned" in env_text()
    rc, text = extend(rec.data_ptr() + 4)
    assert rc == _lib.EINVAL and "aligned" in text
    for bad in ((L[0] + 2, L[1], L[2]), (L[0], L[1] + 2, L[2]), (L[0] + 4, L[1], L[2] + 1)):      # a layout that is not a multiple of 4
        assert env_step(bad, rec.data_ptr()) == _lib.EINVAL and "multiples of 4" in env_text()
    for bad, word in (((L[0], 0, L[2]), "next_off"), ((L[0], L[1], 0), "next_width"), ((L[1] + L[2], L[1], L[2]), "record_len")):
        assert env_step(bad, rec.data_ptr()) == _lib.EINVAL and word in env_text()
    assert env_step(L, host_rec.ctypes.data) == _lib.EINVAL and "device memory" in env_text()      # a host pointer for `records`
    rc, text = extend(host_rec.ctypes.data)
    assert rc == _lib.EINVAL and "device memory" in text
    rc, text = create(eng, env, host_rec.ctypes.data)
    assert rc == _lib.EINVAL and "device memory" in text
    rc, text = extend(rec.data_ptr(), flags=2)                            # an unknown flag
    assert rc == _lib.EINVAL and "unknown flag" in text
    rc, text = extend(rec.data_ptr(), count=-1)
    assert rc == _lib.EINVAL
    assert extend(rec.data_ptr(), count=0)[0] == 0                        # a no-op: no launch, no events
    with pytest.raises(TypeError):
        rb.extend_records(host_rec)
    with pytest.raises(ValueError):
        rb.extend_records(rec[:n, :L[0] - 4])
    torch.cuda.synchronize()
    eng.sync()
    counters = eng.boundary_stats()                                       # no refused call inserted an event or counted a row
    after = (env_books(env), ring_of(rb), len(rb), host(rec), host(obs), counters)
    for x, y in zip(before[:2], after[:2]):
        assert list(x) == list(y) and all(same_bits(x[k], y[k]) for k in x)
    assert before[2] == after[2] == n and same_bits(before[3], after[3]) and same_bits(before[4], after[4]) and before[5] == after[5]
    # and the handle still works after all of them
    rc, _ = create(other, env, rec.data_ptr() + 4)
    assert rc == _lib.EINVAL
    ro_env = new_env("pendulum", n, seed=seed)
    cfg = job_cfg("sac", "pendulum", seed, n, learning_starts=10 ** 6, cap=128)
    ro = loop.NativeRollout(ro_env, new_agent("pendulum", cfg, seed), seed, cfg.learning_starts, 1)
    assert lib.sactd3_rollout_choose(ro._h, 9) == _lib.EINVAL and b"mode" in lib.sactd3_rollout_last_error(ro._h)
    assert lib.sactd3_rollout_choose(ro._h, _lib.ROLLOUT_REPEAT) == 0 and ro.stats()["random_choices"] == 0
    ro.choose()
    ro.advance()
    assert ro.stats() == dict(random_choices=1, policy_choices=0, steps=1, rows_appended=n)
    ro.close()
