"""Every native noise stream of the engine against the float64 Philox model of tests/noise_model.py: the VALUE of every element
of every noise buffer, inside a bound fixed before any run (the exhaustively measured error of the device's log / sin / cos units:
profiles/libm_ulp.json, tests/bounds.py: NOISE), and the SCHEDULE -- which (counter, site code) each draw of a call sequence uses
(noise_model.Schedule).  No element is left out and nothing of the bound comes from the engine.

Who produces the draws (csrc/engine.hip: enqueue_trunk, set_noise; csrc/kernels.h: noise_body, k_actor_tail*): wherever the trunk launch
in front of a tail is one of the k_nt forms or the 32 x 32-tiled one, a few extra blocks of it (noise_body: philox_normal4, one
Philox block per thread, 1024 elements per block) fill the site's buffer and the tail loads it (eps_ready).  Only the 64 x 64-tiled
trunk (B >= 1024 with at least 3/4 of the chip's CUs in tiles: a single actor pass from B = 3072 on) carries no extra blocks: there
the tail draws for itself (philox_normal, gen = !eps_ready) and writes the buffer.  So every case below but the B = 3072 engine of
test_both_producers_make_the_same_bits goes through noise_body -- B = 17 its ragged last block, B x a > 1024 its second block -- and
that test holds the two producers to the same bits at the same (seed, counter, code)."""
import numpy as np
import pytest
import torch

from tests import bounds, noise_model as nm
from tests.gpu_support import (DEV, MAXN, P, _lib, assert_same_state, build_engines, close_engines, engine_state, same_bits,  # noqa: F401
                               stream, track, trajectories)
from tests.helpers import DIMS, observe, synth_transitions

pytestmark = pytest.mark.gpu

SEED = 21
RING = 300
SITES = nm.TRAIN_SITES
assert (_lib.SITE_CRITIC, _lib.SITE_ACTOR0, _lib.SITE_ACTOR1, _lib.SITE_ALPHA0, _lib.SITE_ALPHA1, _lib.SITE_PREDICT) == tuple(range(6))

#        name -> (algo, env, B, fields)
CASES = {"sac-hopper-17": ("sac", "hopper", 17, {}),
         "sac-humanoid-61": ("sac", "humanoid", 61, {}),
         "sac-o3a32-257": ("sac", "o3a32", 257, {}),
         "td3-halfcheetah-256-smoothing": ("td3", "halfcheetah", 256, {"targ_actor_smoothing": True}),
         "td3-halfcheetah-256-plain": ("td3", "halfcheetah", 256, {"targ_actor_smoothing": False}),
         "sac-humanoid-1024": ("sac", "humanoid", 1024, {}),
         "sac-hopper-256-fixed-alpha-delay1": ("sac", "hopper", 256, {"autotune": False, "actor_update_delay": 1}),
         "sac-hopper-256-fixed-alpha-delay3": ("sac", "hopper", 256, {"autotune": False, "actor_update_delay": 3})}


def engines(case, count=1, use_graphs=True, rows=RING, max_envs=8, seed=SEED):
    algo, env, B, fields = CASES[case]
    _, engs, (o, a, bound) = build_engines(algo, DIMS[env], B, count=count, seed=seed, cap=1024, max_envs=max_envs, use_graphs=use_graphs, **fields)
    data = [t.numpy() for t in synth_transitions(rows, o, a, bound, seed=7)]
    for eng in engs:
        eng.rb_extend(*data)
    return engs


def schedule_of(eng):
    c = eng.cfg
    return nm.Schedule(sac=not c.prefer_td3_over_sac, autotune=bool(c.autotune), smoothing=bool(c.targ_actor_smoothing), delay=c.actor_update_delay)


def check_sites(name, what, eng, sched, first, sites=SITES):
    """every element of every training site: inside the bound of the draw the schedule names; a site nothing was drawn into still holds
    what it held when the engine was made (`first`)"""
    for site in sites:
        got = eng.read_noise(site)
        held = sched.holds[site]
        if held is None:
            assert same_bits(got, first[site]), f"{what}: site {site} was written although the schedule draws nothing there"
            continue
        r = nm.check(f"{what}: site {site}", got, eng.cfg.seed, *held, around=6)
        observe(name, f"site {site}: worst |err| / bound", r)


def first_reads(eng):
    return {s: eng.read_noise(s) for s in SITES}


# ------------------------------------------------------------------------------------------ (a) values and schedule, single iterations
@pytest.mark.parametrize("path", ["api", "step"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_values_and_schedule_of_single_iterations(case, path):
    """Two periods of the actor schedule and one iteration more (7 at delay 2), as the API sequence or as step(do_actor), with graphs and
    with use_graphs = 0; after EVERY call every element of the five training sites.  The API path's update_actor has no place in an
    iteration: it always draws into ACTOR0 / ALPHA0 (Schedule.actor(j, api=True))."""
    name = "test_values_and_schedule_of_single_iterations"
    for eng in engines(case, count=2, use_graphs=(True, False)):
        sched, first = schedule_of(eng), first_reads(eng)
        delay = eng.cfg.actor_update_delay
        form = f"{case} {path} graphs={int(eng.cfg.use_graphs)}"
        for i in range(2 * (delay + 1) + 1):
            do_actor = i % (delay + 1) == 0
            if path == "step":
                eng.step(do_actor)
                sched.iteration(do_actor)
                check_sites(name, f"{form} iteration {i}", eng, sched, first)
                continue
            eng.rb_sample()
            eng.update_qnets()
            sched.critic()
            check_sites(name, f"{form} iteration {i} update_qnets", eng, sched, first)
            for j in range(delay if do_actor else 0):
                eng.update_actor()
                sched.actor(j, api=True)
                check_sites(name, f"{form} iteration {i} update_actor {j}", eng, sched, first)
            eng.update_targ_nets(i + 1)
            check_sites(name, f"{form} iteration {i} update_targ_nets", eng, sched, first)
        if eng.cfg.prefer_td3_over_sac and not eng.cfg.targ_actor_smoothing:
            # nothing reads noise_ctr in this configuration, so its ticks are unobservable (and harmless); the acting stream is its own
            assert same_bits(eng.read_noise(_lib.SITE_CRITIC), first[_lib.SITE_CRITIC])
        obs = np.zeros((3, eng.cfg.ob_dim), np.float32)
        eng.predict(obs, True)
        observe(name, "predict behind training: worst |err| / bound", nm.check(f"{form}: predict", eng.read_noise(_lib.SITE_PREDICT, 3), SEED, 0, 48))


# ------------------------------------------------------------------------------------------ (b) the run-ahead forms
def is_pipelined(eng):
    """csrc/engine.hip: period_is_pipelined, restated for SAC (TD3's actor updates draw nothing, so its form leaves the same labels):
    delay 1 or 2, autotune, an opening trunk that reads ring rows itself -- observations of at most 64 floats below B = 1024, wider
    ones from B = 1024 up to where the 64 x 64-tiled trunk takes over (3/4 of the MI355X's 256 CUs in tiles of two nets: B = 1536)"""
    c = eng.cfg
    o, B = c.ob_dim, c.batch_size
    gathers = (o <= 64 and B < 1024) or (o > 64 and B >= 1024 and ((B + 63) // 64) * 4 * 2 < 192)
    return (not c.prefer_td3_over_sac) and bool(c.autotune) and c.actor_update_delay in (1, 2) and gathers


RUN_AHEAD = [("sac-hopper-17", "period"), ("sac-hopper-17", "prefix1"), ("sac-hopper-17", "prefix2"), ("sac-hopper-17", "periods3"),
             ("sac-humanoid-61", "period"), ("sac-humanoid-61", "periods3"), ("sac-o3a32-257", "period"), ("sac-o3a32-257", "periods3"),
             ("sac-humanoid-1024", "period"), ("sac-hopper-256-fixed-alpha-delay1", "periods3"), ("sac-hopper-256-fixed-alpha-delay3", "period"),
             ("td3-halfcheetah-256-smoothing", "period"), ("td3-halfcheetah-256-smoothing", "periods3")]


@pytest.mark.parametrize("case,form", RUN_AHEAD, ids=[f"{c}-{f}" for c, f in RUN_AHEAD])
def test_run_ahead_forms_leave_the_labels_of_the_schedule_and_continue(case, form):
    """step_period, step_prefix(m), step_periods(3) (one run graph of two periods and a single period): behind each call every site
    buffer is ONE draw of its own code -- nm.label finds exactly one counter among those used so far and a few ahead -- and that
    counter is the one Schedule names for "what read_noise shows behind this call"; then a single step(1) and a step(0) draw at the
    counters that follow, which a lost or doubled tick of a deferred temperature step would shift."""
    name = "test_run_ahead_forms_leave_the_labels_of_the_schedule_and_continue"
    for eng in engines(case, count=2, use_graphs=(True, False)):
        run_ahead_labels(name, eng, f"{case} graphs={int(eng.cfg.use_graphs)}", form)


def run_ahead_labels(name, eng, case, form):
    sched, first = schedule_of(eng), first_reads(eng)
    pipe = is_pipelined(eng)

    def labels(what):
        for site in SITES:
            held = sched.holds[site]
            got = eng.read_noise(site)
            if held is None:
                assert same_bits(got, first[site]), (what, site)
                continue
            found = nm.label(got, SEED, nm.SITE_CODE[site], range(0, sched.ctr + 4))
            assert found == held[0], f"{what}: site {site} is (ctr {found}, code {held[1]}) = {nm.describe(got, SEED, range(0, sched.ctr + 4))}, expected (ctr {held[0]}, code {held[1]})"
            observe(name, f"site {site}: worst |err| / bound", nm.ratio(got, SEED, *held))

    eng.step(True)                      # not at counter 0: one iteration first
    sched.iteration(True)
    for rep in range(2):                # twice: the second call starts from what the first left (a chained opening pair, where there is one)
        if form == "period":
            eng.step_period()
            sched.period(pipe)
        elif form == "periods3":
            eng.step_periods(3)
            for _ in range(3):
                sched.period(pipe)
        else:
            m = int(form[-1])
            eng.step_prefix(m)
            sched.prefix(m)
        labels(f"{case} {form} call {rep}")
    for do_actor in (True, False):
        eng.step(do_actor)
        sched.iteration(do_actor)
        labels(f"{case} {form}: step({int(do_actor)}) behind")


SAMPLED = ["prioritised", "nstep", "mixed"]


@pytest.mark.parametrize("draw", SAMPLED)
def test_step_sampled_draws_on_the_schedule_of_step(draw):
    """step_sampled in its prioritised, n-step and mixed draws: the counters and codes of step(do_actor) over 4 iterations, with every
    actor update drawing into ACTOR0 / ALPHA0 -- the call is the API sequence launch for launch (csrc/engine.hip: enqueue_step_sampled)"""
    name = "test_step_sampled_draws_on_the_schedule_of_step"
    algo, env, B, fields = CASES["sac-hopper-17"]
    _, (eng,), (o, a, bound) = build_engines(algo, DIMS[env], B, seed=SEED, cap=1024)
    if draw == "nstep":
        eng.rb_extend(*trajectories(o, a, RING, 3))
    else:
        eng.rb_extend(*[t.numpy() for t in synth_transitions(RING, o, a, bound, seed=7)])
    if draw == "prioritised":
        eng.prio_enable(0.6, 1e-6)
    if draw == "mixed":
        eng.rb_pin(RING)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(40, o, a, bound, seed=8)])
    kw = {"prioritised": dict(beta=0.4), "nstep": dict(n_step=3, stride=4), "mixed": dict(prior_rows=B // 2)}[draw]
    sched, first = schedule_of(eng), first_reads(eng)
    for i in range(4):
        eng.step_sampled(i % 3 == 0, **kw)
        sched.iteration(i % 3 == 0, api=True)
        check_sites(name, f"{draw} iteration {i}", eng, sched, first)
    eng.step(True)                      # ... and the fused iteration behind it goes on where the counters stand
    sched.iteration(True)
    check_sites(name, f"{draw}: step(1) behind", eng, sched, first)


# ------------------------------------------------------------------------------------------ (c) what is read back is what was consumed
TWINS = ["sac-hopper-17", "sac-humanoid-61", "sac-o3a32-257", "td3-halfcheetah-256-smoothing"]


def inject_from(T, E, sched):
    for site in SITES:
        if sched.holds[site] is not None:
            T.set_noise(site, E.read_noise(site))


@pytest.mark.parametrize("path", ["api", "step"])
@pytest.mark.parametrize("case", TWINS)
def test_read_back_noise_is_what_the_update_consumed(case, path):
    """E runs natively; its twin T (seed, ring and batch the same) gets E's read-back arrays injected at every site and runs the same
    call: parameters, targets, temperature, Adam state, metrics and TD errors bit for bit -- so read_noise hands back exactly the
    numbers the tails consumed, whichever kernel produced them."""
    E, T = engines(case, count=2)
    sched = schedule_of(E)
    if path == "step":
        for i, do_actor in enumerate((True, False)):
            E.step(do_actor)
            sched.iteration(do_actor)
            inject_from(T, E, sched)
            T.step(do_actor)
            assert_same_state(engine_state(E, "td", "index"), engine_state(T, "td", "index"), what=f"{case} step {i}")
        return
    for eng in (E, T):
        eng.rb_sample()
    E.update_qnets()
    sched.critic()
    inject_from(T, E, sched)
    T.update_qnets()
    assert_same_state(engine_state(E, "td", "index"), engine_state(T, "td", "index"), what=f"{case} update_qnets")
    for j in range(E.cfg.actor_update_delay):
        E.update_actor()
        sched.actor(j, api=True)
        inject_from(T, E, sched)
        T.update_actor()
        assert_same_state(engine_state(E, "td"), engine_state(T, "td"), what=f"{case} update_actor {j}")
    for eng in (E, T):
        eng.update_targ_nets(1)
    assert_same_state(engine_state(E, "td"), engine_state(T, "td"), what=f"{case} update_targ_nets")


# ------------------------------------------------------------------------------------------ (d) acting
def act(eng, how, obs, explore):
    n = obs.shape[0]
    if how == "predict":
        return eng.predict(obs, explore)
    if how == "begin_end":
        eng.predict_begin(obs, explore)
        return eng.predict_end()
    x = torch.as_tensor(obs, device=DEV)
    out = torch.empty(n, eng.cfg.ac_dim, device=DEV)
    eng.predict_device(x.data_ptr(), x.stride(0), n, explore, out.data_ptr(), out.stride(0), stream(), True)
    eng.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", ["sac-hopper-17", "td3-halfcheetah-256-smoothing", "sac-humanoid-61"])
def test_acting_draws_code_48_at_the_running_count_of_exploring_calls(case):
    """n = 1, 4, 5 (a single-block tail, which ticks predict_ctr itself) and max_envs rows (several blocks: launch_tick), through predict,
    predict_begin/_end and predict_device: read_noise(SITE_PREDICT, n) is (number of exploring calls so far, 48); a non-exploring call
    draws and ticks nothing; training in between moves neither predict_ctr nor the predict buffer, acting does not move noise_ctr.
    TD3: the exploring action is mode + eps (scale actor_noise_std) -- the engine's tail does not clip it -- in float64 from the
    read-back eps and predict(explore=False) of the same rows: the fp32 result rounds scale std once, its product with eps once and
    the sum once, |err| <= SAFETY (2u |eps scale std| + u |action|)."""
    name = "test_acting_draws_code_48_at_the_running_count_of_exploring_calls"
    (eng,) = engines(case, max_envs=MAXN)
    sched, first = schedule_of(eng), first_reads(eng)
    o, a, bound = DIMS[CASES[case][1]]
    allobs = synth_transitions(MAXN, o, a, bound, seed=13)[0].numpy()
    calls = [("predict", 1, True), ("predict", 4, False), ("begin_end", 4, True), ("device", 5, True), ("predict", MAXN, True),
             ("device", MAXN, False), ("begin_end", MAXN, True), ("device", MAXN, True), ("predict", 5, True), ("begin_end", 1, True)]
    last_n = 0
    for k, (how, n, explore) in enumerate(calls):
        obs = allobs[:n]
        before = eng.read_noise(_lib.SITE_PREDICT, MAXN)
        got = act(eng, how, obs, explore)
        sched.predict(explore)
        if not explore:
            assert same_bits(eng.read_noise(_lib.SITE_PREDICT, MAXN), before), (k, "a non-exploring call wrote the predict buffer")
        else:
            last_n = n
            eps = eng.read_noise(_lib.SITE_PREDICT, n)
            observe(name, "worst |err| / bound", nm.check(f"{case} call {k} ({how}, n = {n})", eps, SEED, *sched.holds[_lib.SITE_PREDICT], around=6))
            if eng.cfg.prefer_td3_over_sac:
                mode = bounds.f64(eng.predict(obs, False))
                k_ = bounds.f64(np.float32(bound)) * bounds.f32c(eng.cfg.actor_noise_std)      # scale = (max - min) / 2 = bound
                want = mode + bounds.f64(eps) * k_
                tol = bounds.SAFETY * (2.0 * bounds.U * np.abs(bounds.f64(eps) * k_) + bounds.U * np.abs(want))
                observe(name, "TD3 exploring action: worst |err| / bound", bounds.check(f"{case} call {k}: action", got, want, tol))
        if k in (2, 6):      # training in between
            eng.step(True)
            sched.iteration(True)
            check_sites(name, f"{case}: step behind acting call {k}", eng, sched, first)
            assert nm.label(eng.read_noise(_lib.SITE_PREDICT, last_n), SEED, 48, range(0, 12)) == sched.holds[_lib.SITE_PREDICT][0]
    assert sched.predict_ctr == 8


# ------------------------------------------------------------------------------------------ (e) both producers
def test_both_producers_make_the_same_bits():
    """(seed, counter 0, code 0), SAC Hopper: at B = 256 the draw is made by noise_body riding the opening trunk (philox_normal4), at
    B = 3072 by the tail itself (philox_normal; the 64 x 64-tiled trunk carries no extra blocks).  Element e = row * 3 + j does not
    depend on B: the first 768 elements are the same bits, and both buffers lie inside the model's bound."""
    name = "test_both_producers_make_the_same_bits"
    bufs = {}
    for B in (256, 3072):
        _, (eng,), (o, a, bound) = build_engines("sac", DIMS["hopper"], B, seed=SEED, cap=4096)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(RING, o, a, bound, seed=7)])
        eng.step(True)
        for site, ctr in ((_lib.SITE_CRITIC, 0), (_lib.SITE_ACTOR0, 1), (_lib.SITE_ALPHA0, 1), (_lib.SITE_ACTOR1, 2), (_lib.SITE_ALPHA1, 2)):
            bufs[B, site] = eng.read_noise(site)
            observe(name, f"B = {B}: worst |err| / bound", nm.check(f"B = {B} site {site}", bufs[B, site], SEED, ctr, nm.SITE_CODE[site]))
        eng.close()
    for site in SITES:
        assert same_bits(bufs[256, site], bufs[3072, site][:256]), f"site {site}: the two producers differ in bits"


# ------------------------------------------------------------------------------------------ the synthetic ring fill
@pytest.mark.parametrize("env", ["hopper", "humanoid"])
def test_synthetic_fill_matches_its_model(env):
    """300 rows of k_rb_fill through the ring read-out (rb_sample_with_indices + read_batch: a record of many chunks), per-dimension
    asymmetric action bounds: normals inside the bound of the library's measured figures, actions inside the hull of the fused and
    unfused fp32 forms, rewards nrm[0] of the last chunk, dones exactly the model's"""
    name = "test_synthetic_fill_matches_its_model"
    o, a, _ = DIMS[env]
    B, rows, fill_seed = 100, 300, 5
    rng = np.random.default_rng(3)
    lo = (-rng.uniform(0.2, 2.0, a)).astype(np.float32)
    hi = rng.uniform(0.1, 3.0, a).astype(np.float32)
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=512, max_envs=4, seed=1), lo, hi))
    eng.rb_fill_synthetic(rows, fill_seed)
    assert eng.rb_len() == rows
    m = nm.fill_model(fill_seed, rows, o, a, lo, hi)
    got = {}
    for lo_row in range(0, rows, B):
        eng.rb_sample_with_indices(np.arange(lo_row, lo_row + B))
        for k, v in eng.read_batch().items():
            got.setdefault(k, []).append(v)
    got = {k: np.concatenate(v) for k, v in got.items()}
    assert np.array_equal(got["index"], np.arange(rows))
    for k, key in (("obs", "observations"), ("nobs", "next_observations"), ("rew", "rewards")):
        want, tol = m[k]
        observe(name, f"{env} {k}: worst |err| / bound", bounds.check(f"{env} {k}", got[key], want, tol))
    observe(name, f"{env} actions: worst place in the hull", bounds.check_interval(f"{env} actions", got["actions"], *m["act"]))
    assert 0 < m["done"].sum() < rows                    # (both outcomes occur among the 300 rows: 2 dones at either shape)
    assert np.array_equal(got["dones"].reshape(-1).astype(bool), m["done"])
