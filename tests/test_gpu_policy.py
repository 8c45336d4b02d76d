"""GPU: querying the policy on caller-supplied rows (sactd3_policy_device / sactd3_policy, include/sactd3.h; csrc/policy_kernels.h).
Every output against float64 intervals derived from the engine's own trunk rows (tests/policy_checks.py; the checker itself is checked
on the CPU by tests/test_policy_bounds.py) and against the oracle's actor at the suite's forward-pass tolerance; everything else is an
equality: the mode is the exploit action the scoring route's policy form computes, a row's outputs are the same bits whatever rows are
asked with it, views change nothing, the native draws follow their own Philox stream, and training and acting cannot tell whether a
call was made.

Shapes (tests/gpu_support.py: SHAPES / shape_engines): SAC Hopper (a = 3: the narrow head form), SAC Humanoid (o = 376, a = 17: the MFMA
form, a second element per lane, wide observations), SAC Hopper without LayerNorm, TD3 HalfCheetah.  Row counts 1, 67 and 1041 = a
chunk of 1024 rows and one of 17."""
import copy
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import noise_model
from tests import policy_checks as pc
from tests import tail_checks as tc
from tests.gpu_support import (DEV, NROWS, SENTINEL, SHAPES, P, _lib, assert_same_state, close, close_engines, data, loop, make_engine,  # noqa: F401
                               same_bits, score, shape_engines, stream, track)
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = ["sac-hopper", "sac-humanoid", "sac-hopper-noln", "td3-halfcheetah"]
ROWS = (1, 67, NROWS)
LOGP = ("sample_logp", "action_logp")


def ask(eng, obs, actions=None, eps=None, sample=False, target=False, want=None, ordered=True):
    """policy_device on CUDA tensors -> {output: host array}; `want`: the outputs (default: all that the arguments imply)"""
    n, a = obs.shape[0], eng.cfg.ac_dim
    want = want or eng.policy_outputs(bool(sample) or eps is not None, actions is not None)
    out = {k: torch.full((n,) if k in LOGP else (n, a), SENTINEL, device=DEV) for k in want}
    fields = {k: (v.data_ptr(), 1 if k in LOGP else a) for k, v in out.items()}
    for k, x in (("actions", actions), ("eps", eps)):
        if x is not None:
            fields[k] = (x.data_ptr(), max(x.stride(0), a))
    eng.policy_device(obs.data_ptr(), max(obs.stride(0), obs.shape[1]), n, fields, target, stream(), ordered)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(x, y):
    return set(x) == set(y) and all(same_bits(x[k], y[k]) for k in x)


def dev(x):
    return torch.as_tensor(np.asarray(x, F32), device=DEV)


@functools.lru_cache(maxsize=None)
def draws(shape, n=NROWS):
    a = SHAPES[shape][1][1]
    return torch.randn(n, a, generator=torch.Generator().manual_seed(41))


# ------------------------------------------------------------------------------------------ 1. intervals
@pytest.mark.parametrize("degenerate", [False, True], ids=["benign", "degenerate"])
@pytest.mark.parametrize("shape", ALL)
def test_every_output_lies_in_its_float64_interval(shape, degenerate):
    """nets, observations and draws of tail_checks.make_case (head-bias offsets that saturate both squashes, per-dimension asymmetric
    bounds, rows of exact-zero and of +-4 draws), 1, 67 and 1041 rows: every output of the LAST chunk against the intervals derived
    from debug_read("pi_z2") -- the rows that chunk's head kernel read.  Given actions: rows 0 .. 4 the edges (at the upper bounds, at
    the lower, hi + 1, one +inf, one NaN component), every other row from 5 on the policy's own sample for the same draws, the rest
    drawn uniformly inside the bounds (tail_checks.make_case)."""
    algo, (o, a, _), ln = SHAPES[shape]
    c = tc.make_case(algo, o, a, NROWS, ln, 2000 + ALL.index(shape), degenerate_nets=degenerate)
    eng = make_engine(dict(c, B=64))
    with pytest.raises(P.EngineError, match="no policy query"):
        eng.debug_read("pi_z2")
    obs, eps = dev(c["obs"]), dev(c["eps_a"])
    if not c["sac"]:
        for target, params in ((False, c["actor"]), (True, c["actor_t"])):
            for n in ROWS:
                got = ask(eng, obs[:n], target=target)
                z2 = eng.debug_read("pi_z2").reshape(-1, 256)
                lo = n - z2.shape[0]
                assert z2.shape[0] == (n - 1) % 1024 + 1
                pc.check_policy_outputs(f"policy_intervals[{shape}]", z2, params, c, {"mode": got["mode"][lo:]})
        return
    own = ask(eng, obs, eps=eps, want=("sample",))["sample"]
    g = c["act"].copy()
    g[5::2] = own[5::2]
    g[0], g[1], g[2] = c["hi"], c["lo"], c["hi"] + F32(1)
    g[3, a - 1], g[4, 0] = np.inf, np.nan
    gd = dev(g)
    for n in ROWS:
        got = ask(eng, obs[:n], gd[:n], eps[:n])
        assert set(got) == {"mode", "mean", "log_std", "sample", "sample_logp", "eps_out", "action_logp"}
        assert same_bits(got["eps_out"], c["eps_a"][:n])
        z2 = eng.debug_read("pi_z2").reshape(-1, 256)
        lo = n - z2.shape[0]
        assert z2.shape[0] == (n - 1) % 1024 + 1
        io = {k: got[k][lo:] for k in ("mode", "mean", "log_std", "sample", "sample_logp", "action_logp")}
        seen = pc.check_policy_outputs(f"policy_intervals[{shape}-{'degenerate' if degenerate else 'benign'}]", z2, c["actor"], c,
                                       dict(io, eps=c["eps_a"][lo:n], actions=g[lo:n]))
        assert set(seen) == set(io)
        print(shape, degenerate, n, {k: round(v, 4) for k, v in seen.items()})
    if degenerate:          # (the 1041 rows) tanh(raw) == +-1 <=> log_std is exactly 2 or -5; y == +-1 <=> sample == bi +- sc
        assert np.isin(got["log_std"], (F32(2), F32(-5))).any(), "tanh(raw log-std) did not saturate"
        assert ((got["sample"] == c["bias"] + c["scale"]) | (got["sample"] == c["bias"] - c["scale"])).any(), "y did not saturate"


# ------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("shape", ALL)
def test_mode_and_sample_match_the_oracles_actor(shape):
    """the oracle's actor on the same rows, injected draws: rtol 1e-5 + atol 1e-5, what
    tests/test_gpu_qvalues.py::test_scores_match_the_oracles_twin_critics applies to a forward pass at these shapes and this data"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs_h = data(shape)[0]
    obs = obs_h.to(DEV)
    if SHAPES[shape][0] == "td3":
        for target, net in ((False, ref.actor), (True, ref.actor_target)):
            with torch.no_grad():
                want = net(obs_h).numpy()
            for n in ROWS:
                got = ask(eng, obs[:n], target=target)["mode"]
                print(shape, target, n, "max |d mode|", float(np.abs(got - want[:n]).max()))
                close(got, want[:n], rtol=1e-5, atol=1e-5, name=f"{shape} mode target={target} n={n}")
        return
    eps_h = draws(shape)
    with torch.no_grad():
        want = ref.actor.get_action(obs_h, eps_h)
        w64 = copy.deepcopy(ref.actor).double().get_action(obs_h.double(), eps_h.double())["log_prob"].numpy().reshape(-1)
    # Which rows the float32 oracle can arbitrate sample_log_prob on, decided by the oracle alone: with the suite's perturbed nets the
    # policy's std reaches ~7, y = tanh(mean + e std) comes within 3e-8 of +-1, and log(sc (1 - y^2) + 1e-6) then loses every digit
    # of 1 - y^2 in float32 -- the oracle's float32 log-prob is up to 0.058 away from its own float64 value (hopper: 174 of the 1041
    # rows beyond 1e-5 + 1e-5 |v|).  A reference that misses the tolerance itself settles nothing at that tolerance, so the log-prob
    # is compared on the rows where the float32 oracle is within a QUARTER of the tolerance of its float64 self (the engine evaluates
    # the same float32 formula with another tanhf, so its error is of the oracle's size: up to three times it still meets the
    # tolerance).  Those must be more than half of the rows; the others are held, every one, by the float64 intervals of test 1.  mode and sample are
    # compared on every row.
    w32 = want["log_prob"].numpy().reshape(-1)
    fit = np.abs(w32.astype(np.float64) - w64) <= 0.25 * (1e-5 + 1e-5 * np.abs(w64))
    print(shape, "rows the float32 oracle arbitrates:", int(fit.sum()), "of", fit.size)
    assert fit.mean() > 0.5                                          # (70 % at Humanoid, 77 % at Hopper, all without LayerNorm)
    for n in ROWS:
        got = ask(eng, obs[:n], eps=eps_h[:n].to(DEV))
        for key, wkey in (("mode", "mode"), ("sample", "sample")):
            w = want[wkey].numpy()[:n]
            print(shape, n, key, "max |d|", float(np.abs(got[key] - w).max()))
            close(got[key], w, rtol=1e-5, atol=1e-5, name=f"{shape} {key} n={n}")
        rows = np.flatnonzero(fit[:n])
        if rows.size:
            print(shape, n, "sample_logp", rows.size, "rows, max |d|", float(np.abs(got["sample_logp"][rows] - w32[rows]).max()))
            close(got["sample_logp"][rows], w32[rows], rtol=1e-5, atol=1e-5, name=f"{shape} sample_logp n={n}")


# ------------------------------------------------------------------------------------------ 3. bit-for-bit ties to existing paths
@pytest.mark.parametrize("shape", ALL)
def test_bit_for_bit_ties(shape):
    """q_values(obs, actions=mode) == q_values(obs), the scoring route's policy form (online critics); sample with eps = 0 == mode; a
    row's outputs are the same bits alone, inside 67 rows and inside 1041 rows; the host call gives the device call's bits"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    sac = SHAPES[shape][0] == "sac"
    obs_h, act_h = data(shape)
    obs, act = obs_h.to(DEV), act_h.to(DEV)
    eps = draws(shape).to(DEV) if sac else None
    kw = dict(actions=act, eps=eps) if sac else {}
    cut = lambda d, lo, hi: {k: (None if v is None else v[lo:hi]) for k, v in d.items()}
    full = ask(eng, obs, **kw)
    assert all(np.isfinite(v).all() for v in full.values())
    assert same_bits(score(eng, obs, dev(full["mode"])), score(eng, obs))
    mid = ask(eng, obs[:67], **cut(kw, 0, 67))
    assert same(mid, {k: v[:67] for k, v in full.items()})
    for i in (0, 5, 16, 66, 1023, 1024, 1040):
        one = ask(eng, obs[i:i + 1], **cut(kw, i, i + 1))
        assert same(one, {k: v[i:i + 1] for k, v in full.items()}), i
    if sac:
        zero = ask(eng, obs[:67], eps=torch.zeros(67, a, device=DEV))
        assert same_bits(zero["sample"], zero["mode"]) and same_bits(zero["mode"], full["mode"][:67])
        host = eng.policy(obs_h.numpy(), actions=act_h.numpy(), eps=draws(shape).numpy())
    else:
        host = eng.policy(obs_h.numpy())
    assert same(host, full)


# ------------------------------------------------------------------------------------------ 4. native draws
def test_native_draws_follow_their_own_philox_stream_and_move_no_other_counter():
    """eps_out of two consecutive native calls lies, element by element, inside the a-priori bound of the float64 Philox model of the
    noise tests (tests/noise_model.py) with stream 0x400 and the counter at 0, then 1; a call with `eps` given leaves the counter alone (the next native call draws with 2);
    the host call draws from the same stream.  A twin engine that asks nothing has the same noise buffers at every site and returns
    the same exploring action."""
    ref, (R, N), (o, a, bound) = shape_engines("sac-humanoid", count=2)
    obs_h = data("sac-humanoid")[0]
    obs = obs_h.to(DEV)
    # every element inside the a-priori bound of the float64 model (tests/noise_model.py) at stream word 0x400
    on_stream = lambda got, ctr: noise_model.check(f"policy draw {ctr}", got, 3, ctr, noise_model.STREAM_POLICY)
    for ctr, n in ((0, NROWS), (1, 67)):
        got = ask(R, obs[:n], sample=True)
        assert got["eps_out"].shape == (n, a)
        on_stream(got["eps_out"], ctr)
        again = ask(R, obs[:n], eps=dev(got["eps_out"]))                     # its sample is the sample of those draws; no tick
        assert same_bits(again["sample"], got["sample"]) and same_bits(again["sample_logp"], got["sample_logp"])
    got = R.policy(obs_h[:67].numpy(), sample=True)
    assert got["eps_out"].shape == (67, a)
    on_stream(got["eps_out"], 2)
    got = ask(R, obs[:5], want=("sample_logp",))                             # (sample_logp alone draws too)
    assert np.isfinite(got["sample_logp"]).all()
    on_stream(ask(R, obs[:5], want=("eps_out", "sample"))["eps_out"], 4)
    ask(R, obs[:5])                                                          # no sample wanted: no tick
    on_stream(ask(R, obs[:5], sample=True)["eps_out"], 5)
    for eng in (R, N):
        eng.rb_extend(*[t.numpy() for t in synth_transitions(300, o, a, bound, seed=31)])
        eng.run_iterations(0, 3)
        if eng is R:
            ask(R, obs[:67], sample=True)
    x, y = R.predict(obs_h[:4].numpy(), True), N.predict(obs_h[:4].numpy(), True)
    assert np.array_equal(x, y)
    for site in range(6):
        assert np.array_equal(R.read_noise(site), N.read_noise(site)), site
    assert N.policy_stats() == dict(calls=0, rows=0, rows_clamped=0, rows_nan=0) and R.policy_stats()["calls"] == 10


# ------------------------------------------------------------------------------------------ 5. edge actions
@pytest.mark.parametrize("shape", ["sac-hopper", "sac-humanoid"])
def test_edge_actions_clamp_count_and_stay_in_their_row(shape):
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs = data(shape)[0][:12].to(DEV)
    g = data(shape)[1][:12].numpy().copy()
    base = ask(eng, obs, dev(g), want=("action_logp", "mode"))
    assert np.isfinite(base["action_logp"]).all() and eng.policy_stats()["rows_clamped"] == 0
    e = g.copy()
    e[1], e[2] = bound, -bound                    # exactly at the bounds: |v| == 1 > M
    e[3, 0], e[4, 0] = bound + 1, bound + 100     # beyond: identical bits
    e[6, a - 1] = np.inf                          # clamps, counted as clamped
    e[8, 1] = np.nan                              # NaN for that row only, counted
    e[9, 0], e[9, 2] = np.nan, -np.inf            # one row, both counters, once each
    got = ask(eng, obs, dev(e), want=("action_logp", "mode"))
    lp = got["action_logp"]
    st = eng.policy_stats()
    assert (st["rows_clamped"], st["rows_nan"]) == (6, 2) and st["calls"] == 2 and st["rows"] == 24
    clamped, nan = pc.row_flags(e, np.full(a, bound, F32), np.zeros(a, F32))
    assert clamped.sum() == 6 and nan.sum() == 2
    assert np.isnan(lp[[8, 9]]).all() and np.isfinite(np.delete(lp, [8, 9])).all()
    assert same_bits(got["mode"], base["mode"])
    untouched = [0, 5, 7, 10, 11]
    assert same_bits(lp[untouched], base["action_logp"][untouched])
    f = e.copy()
    f[4, 0] = bound + 1
    assert same_bits(ask(eng, obs[4:5], dev(f[4:5]), want=("action_logp",))["action_logp"], lp[4:5])
    f = g.copy()
    f[3, 0] = bound                               # ... and beyond the bound is the bound
    assert same_bits(ask(eng, obs[3:4], dev(f[3:4]), want=("action_logp",))["action_logp"], lp[3:4])


# ------------------------------------------------------------------------------------------ 6. views
@pytest.mark.parametrize("shape", ["sac-hopper", "sac-humanoid", "td3-halfcheetah"])
def test_views_in_and_out_from_another_stream(shape):
    """obs / actions / eps = strided, 4-byte-aligned views; outputs = windows at odd offsets of sentinel-filled tensors, a subset of
    them NULL; issued from another torch stream with SACTD3_SRC_ORDERED: the bits of the contiguous call, nothing outside the windows
    touched, the sources unchanged"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    sac = SHAPES[shape][0] == "sac"
    ag = P.Agent.__new__(P.Agent)
    ag.engine = eng
    obs_h, act_h = data(shape)
    side = torch.cuda.Stream()
    for n in (1, 67):
        obs, act, eps = obs_h[:n].to(DEV), act_h[:n].to(DEV), draws(shape)[:n].to(DEV)
        want = ask(eng, obs, act, eps) if sac else ask(eng, obs)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            big = torch.full((n, o + 5), float("nan"), device=DEV)
            big[:, 1:1 + o] = obs
            wide = torch.full((n, 2 * a + 7), float("nan"), device=DEV)
            wide[:, 3:3 + a] = act
            wide[:, a + 4:2 * a + 4] = eps
            big0, wide0 = big.clone(), wide.clone()
            keys = ("mode", "log_std", "sample", "log_prob") if sac else ("mode",)         # mean, sample_log_prob, eps: not wanted
            bases = {k: torch.full((n + 2, (1 if k == "log_prob" else a) + 4), SENTINEL, device=DEV) for k in keys}
            views = {k: b[1:1 + n, 3:3 + (1 if k == "log_prob" else a)] for k, b in bases.items()}
            fields = {f: (views[k].data_ptr(), views[k].stride(0)) for k, f in (("mode", "mode"), ("log_std", "log_std"), ("sample", "sample"),
                                                                                 ("log_prob", "action_logp")) if k in views}
            if sac:
                fields["actions"], fields["eps"] = (wide[:, 3:].data_ptr(), wide.stride(0)), (wide[:, a + 4:].data_ptr(), wide.stride(0))
            eng.policy_device(big[:, 1:].data_ptr(), big.stride(0), n, fields, False, side.cuda_stream)
            host = {k: b.cpu().numpy() for k, b in bases.items()}
            assert torch.equal(big.view(torch.int32), big0.view(torch.int32)) and torch.equal(wide.view(torch.int32), wide0.view(torch.int32))
        for k, f in (("mode", "mode"), ("log_std", "log_std"), ("sample", "sample"), ("log_prob", "action_logp")):
            if k not in host:
                continue
            w = 1 if k == "log_prob" else a
            assert same_bits(host[k][1:1 + n, 3:3 + w].reshape(want[f].shape), want[f]), (n, k)
            host[k][1:1 + n, 3:3 + w] = F32(SENTINEL)
            assert same_bits(host[k], np.full_like(host[k], SENTINEL)), (n, k)
        # Agent.policy: the same views through the mirror, `out` given for some keys and made for the others
        td = {"observations": big[:, 1:1 + o], "actions": wide[:, 3:3 + a]} if sac else {"observations": big[:, 1:1 + o]}
        res = ag.policy(td, eps=wide[:, a + 4:2 * a + 4] if sac else None, out={"mode": views["mode"]})
        assert res["mode"].data_ptr() == views["mode"].data_ptr()
        names = dict(mode="mode", mean="mean", log_std="log_std", sample="sample", sample_log_prob="sample_logp", eps="eps_out", log_prob="action_logp")
        assert set(res) == {k for k, f in names.items() if f in want}
        for k, v in res.items():
            assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (n, 1 if k.endswith("log_prob") else a)
            assert same_bits(v.cpu().numpy().reshape(want[names[k]].shape), want[names[k]]), (n, k)
        res = ag.policy({"observations": obs_h[:n].numpy(), **({"actions": act_h[:n]} if sac else {})}, eps=draws(shape)[:n].numpy() if sac else None)
        assert all(isinstance(v, np.ndarray) for v in res.values())
        assert all(same_bits(v.reshape(want[names[k]].shape), want[names[k]]) for k, v in res.items())
    with pytest.raises(TypeError):
        ag.policy({"observations": obs_h[:4].to(DEV), "actions": act_h[:4].numpy()})


# ------------------------------------------------------------------------------------------ 7. invisible to training
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-td3_2"])
def test_asking_between_chained_periods_changes_nothing(shape):
    """two engines, one asks (native and injected draws, given actions; 67 rows) between rb_extend and the periods, between two
    back-to-back periods, around single steps and inside predict_begin / predict_end: same parameters, Adam state, metrics, sampled
    indices, TD errors, actions, graphs and every counter but the feature's own"""
    _, (R, N), (o, a, bound) = shape_engines(shape, count=2, cap=1000)
    sac = SHAPES[shape][0] == "sac"
    obs, act = [t[:67].to(DEV) for t in data(shape)]
    eps = draws("sac-hopper")[:67].to(DEV)
    res = []
    for eng, asks in ((R, True), (N, False)):
        eng.rb_extend(*[t.numpy() for t in synth_transitions(600, o, a, bound, seed=31)])
        it, samples = 0, []

        def read():
            if asks and sac:
                for got in (ask(eng, obs, act, sample=True), ask(eng, obs, act, eps), ask(eng, obs)):
                    assert all(np.isfinite(v).all() for v in got.values())
            elif asks:
                assert np.isfinite(ask(eng, obs)["mode"]).all() and np.isfinite(ask(eng, obs, target=True)["mode"]).all()
        for k in range(3):                                           # rb_extend every period
            eng.rb_extend(*[t.numpy() for t in synth_transitions(8, o, a, bound, seed=70 + k)])
            read()
            it = eng.run_iterations(it, 3)
            read()
            samples.append(eng.read_batch()["index"])
        it = eng.run_iterations(it, 3)
        read()
        it = eng.run_iterations(it, 3)
        samples.append(eng.read_batch()["index"])
        for do_actor in (False, True):                               # single steps
            read()
            eng.step(do_actor)
            samples.append(eng.read_batch()["index"])
        read()
        td = torch.empty(2, 64, device=DEV)
        eng.td_errors_device(td.data_ptr(), 1, 64, stream())
        acts = []
        for n in (4, 17):                                            # allowed while an acting call is in flight, and invisible to it
            ob = data(shape)[0][100:100 + n].numpy()
            eng.predict_begin(ob, True)
            read()
            acts.append(eng.predict_end())
            acts.append(eng.read_noise(_lib.SITE_PREDICT, n))
        res.append((samples, [eng.graph_kernel_count(w) for w in range(8)], td.cpu().numpy(), acts))
    (sr, gr, tr, ar), (sn, gn, tn, an) = res
    assert_same_state(R, N)
    assert all(np.array_equal(x, y) for x, y in zip(sr, sn)) and len(sr) == 6
    assert gr == gn and sum(gr) > 0 and same_bits(tr, tn)
    assert all(np.array_equal(x, y) for x, y in zip(ar, an))
    for name in ("qvalues_stats", "boundary_stats", "readout_stats", "predict_device_stats", "priority_stats", "step_periods_stats", "mix_stats"):
        if name == "boundary_stats":                                 # (its fourth counter counts ordered calls of every route: the feature's too)
            x, y = getattr(R, name)(), getattr(N, name)()
            assert list(x.values())[:3] == list(y.values())[:3], name
        else:
            assert getattr(R, name)() == getattr(N, name)(), name
    ra, na = R.acting_stats(), N.acting_stats()                       # (how a call's wait ended is timing, not schedule)
    assert all(ra[k] == na[k] for k in ("begun", "begin_waited_for_learner", "learner_waited_for_acting")) and ra["begun"] == 2
    calls = 12 * (3 if sac else 2)
    assert R.policy_stats() == dict(calls=calls, rows=calls * 67, rows_clamped=0, rows_nan=0)
    assert N.policy_stats() == dict(calls=0, rows=0, rows_clamped=0, rows_nan=0)


# ------------------------------------------------------------------------------------------ 8. follows the parameters
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah"])
def test_outputs_follow_the_parameters(shape):
    """after update_actor the outputs change; after set_params(ACTOR, old) they are the old bits; TD3's target form follows ACTOR_TARGET"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    sac = SHAPES[shape][0] == "sac"
    obs, act = [t[:67].to(DEV) for t in data(shape)]
    kw = dict(actions=act, eps=draws(shape)[:67].to(DEV)) if sac else {}
    before = ask(eng, obs, **kw)
    tb = None if sac else ask(eng, obs, target=True)
    old = eng.get_params(_lib.ACTOR)
    eng.load_batch(*[t.numpy() for t in synth_transitions(64, o, a, bound, seed=11)])
    eng.update_qnets()
    eng.update_actor()
    after = ask(eng, obs, **kw)
    for k in before:
        if k != "eps_out":
            assert not np.array_equal(before[k], after[k]), k
    if not sac:
        t0 = ask(eng, obs, target=True)
        assert same_bits(t0["mode"], tb["mode"])                         # the target actor has not moved
        eng.set_params(_lib.ACTOR_TARGET, eng.get_params(_lib.ACTOR))
        assert same_bits(ask(eng, obs, target=True)["mode"], after["mode"])
    eng.set_params(_lib.ACTOR, old)
    assert same(ask(eng, obs, **kw), before)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing_and_leave_the_engine_usable():
    lib, ORD, vp = None, _lib.SRC_ORDERED, C.c_void_p
    for shape in ("sac-hopper", "td3-halfcheetah"):
        ref, (eng,), (o, a, bound) = shape_engines(shape)
        sac = SHAPES[shape][0] == "sac"
        lib, h = eng.lib, eng._h
        obs, act = [t[:8].to(DEV) for t in data(shape)]
        eps = draws(shape)[:8].to(DEV)
        names = [f for f, _ in _lib.POLICY_IO_FIELDS]
        outs = {f: torch.full((8, 1 if f.endswith("_logp") else a), SENTINEL, device=DEV) for f in names[2:]}
        host = np.zeros((8, max(o, a)), F32)
        pinned = torch.zeros(8, max(o, a)).pin_memory()

        def io(**over):
            """the valid struct of the shape with fields replaced: name=(pointer, stride) or None"""
            base = {"mode": (outs["mode"].data_ptr(), a)}
            if sac:
                base.update({f: (outs[f].data_ptr(), 1 if f.endswith("_logp") else a) for f in names[2:]})
                base.update(actions=(act.data_ptr(), a), eps=(eps.data_ptr(), a))
            base.update(over)
            s = _lib.CPolicyIO()
            for f, v in base.items():
                if v is not None:
                    setattr(s, f, v[0] or None)
                    setattr(s, f + "_ld", v[1])
            return s

        call = lambda s, obs_p=obs.data_ptr(), ld=o, n=8, which=0, flags=ORD: lib.sactd3_policy_device(h, vp(obs_p), ld, n, which, C.byref(s) if s is not None else None, None, flags)
        assert call(io()) == 0                                               # (the valid call, so that what follows isolates one fault each)
        eng.sync()
        good = {f: v.cpu().numpy().copy() for f, v in outs.items()}
        for v in outs.values():
            v.fill_(SENTINEL)
        torch.cuda.synchronize()
        snap = [eng.get_params(w) for w in (_lib.ACTOR, _lib.CRITICS)]
        bad = [call(io(), obs_p=0), call(None), call(io(), n=0), call(io(), n=-3), call(io(), ld=o - 1), call(io(), flags=2), call(io(), flags=ORD | 4),
               call(io(), which=2), call(io(), which=-1), call(io(), obs_p=host.ctypes.data), call(io(), obs_p=pinned.data_ptr()),
               call(io(mode=(host.ctypes.data, a))), call(io(mode=(pinned.data_ptr(), a))), call(io(mode=(outs["mode"].data_ptr(), a - 1)))]
        if sac:
            none = {f: None for f in names[2:]}
            bad += [call(io(**none)),                                                                       # no output
                    call(io(), which=_lib.PI_TARGET),                                                       # SAC has no target actor
                    call(io(actions=None)),                                                                 # action_logp without actions
                    call(io(**dict(none, mode=(outs["mode"].data_ptr(), a)))),                              # eps without a sample
                    call(io(**dict(none, mode=(outs["mode"].data_ptr(), a), eps=None, eps_out=(outs["eps_out"].data_ptr(), a)))),
                    call(io(actions=(act.data_ptr(), a - 1))), call(io(eps=(eps.data_ptr(), a - 1))),
                    call(io(sample_logp=(outs["sample_logp"].data_ptr(), 0))), call(io(action_logp=(outs["action_logp"].data_ptr(), 0))),
                    call(io(actions=(host.ctypes.data, a))), call(io(eps=(pinned.data_ptr(), a))), call(io(log_std=(host.ctypes.data, a)))]
        else:
            bad += [call(io(mode=None))]
            bad += [call(io(**{f: (act.data_ptr() if f in ("actions", "eps") else outs[f].data_ptr(), a if not f.endswith("_logp") else 1)}))
                    for f in names if f != "mode"]                                                          # every SAC-only field
        assert bad and all(rc == _lib.EINVAL for rc in bad), bad
        fp = C.POINTER(C.c_float)
        hs = io(**{f: None for f in names})
        hs.mode, hs.mode_ld = host.ctypes.data, a
        assert lib.sactd3_policy(h, None, 8, 0, C.byref(hs)) == _lib.EINVAL
        assert lib.sactd3_policy(h, host.ctypes.data_as(fp), 0, 0, C.byref(hs)) == _lib.EINVAL
        assert lib.sactd3_policy(h, host.ctypes.data_as(fp), 8, 2, C.byref(hs)) == _lib.EINVAL
        assert lib.sactd3_policy(h, host.ctypes.data_as(fp), 8, 0, None) == _lib.EINVAL
        with pytest.raises(P.EngineError, match="stride"):
            eng.policy_device(obs.data_ptr(), o - 1, 8, {"mode": (outs["mode"].data_ptr(), a)})
        st = (C.c_int64 * 4)()
        assert lib.sactd3_policy_stats(h, None) == _lib.EINVAL
        assert lib.sactd3_policy_stats(h, st) == 0 and list(st) == [1, 8, 0, 0]          # none of those launched or counted anything
        eng.sync()
        assert all((v == SENTINEL).all() for v in outs.values())
        assert all(np.array_equal(x, eng.get_params(w)) for x, w in zip(snap, (_lib.ACTOR, _lib.CRITICS)))
        assert call(io()) == 0                                               # ... and the engine is as usable as before: the same bits
        eng.sync()
        for f, v in outs.items():
            if f in good and (sac or f == "mode"):
                assert same_bits(v.cpu().numpy(), good[f]), f
        eng.rb_fill_synthetic(300)                                           # ... and runs a normal iteration
        eng.run_iterations(0, 3)
        assert all(np.isfinite(v) for v in eng.read_metrics().values())
        eng.close()


# ------------------------------------------------------------------------------------------ 10. the loop
def test_the_loop_records_the_policys_vitals_and_trains_the_same_bits(tmp_path):
    o, a, n = 11, 3, 4
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 800, "eval_every": 200, "cudagraphs": True, "rb_capacity": 2000, "eval_steps": 1, "measure_burnin": 0})
    runs = []
    for stats in (64, 0):
        env = loop.SyntheticVecEnv(o, a, n)
        env.action_space.seed(0)
        torch.manual_seed(0)
        agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, F32), np.full(a, 1.0, F32), torch.device(DEV), cfg,
                        P.ReplayBuffer(cfg.rb_capacity))
        tab = loop.Tabular(tmp_path / str(stats))
        ev = loop.Evaluator(cfg, loop.SyntheticVecEnv(o, a, 1, horizon=20), agent, tab)
        m = loop.train(cfg, env, agent, evaluator=ev, policy_stats=stats)
        tab.close()
        eng = track(agent.engine)
        runs.append((m, [eng.get_params(w) for w in range(5)], [eng.get_adam_state(w) for w in (_lib.ACTOR, _lib.CRITICS, _lib.LOG_ALPHA)],
                     (agent.qnet_updates_so_far, agent.actor_updates_so_far, agent.timesteps_so_far), eng.policy_stats(),
                     (tmp_path / str(stats) / "progress.csv").read_text().splitlines()[0]))
        eng.close()
    (m1, p1, s1, c1, st1, head1), (m0, p0, s0, c0, st0, head0) = runs
    assert set(m1) - set(m0) == set(loop.PolicyStats.KEYS) and all(np.isfinite(m1[k]) for k in loop.PolicyStats.KEYS)
    assert m1["vitals/policy_entropy"] != 0 and -5.0 <= m1["vitals/log_std_mean"] <= 2.0
    assert {k: v for k, v in m1.items() if k in m0} == m0 and c1 == c0
    assert all(np.array_equal(x, y) for x, y in zip(p1, p0))
    assert all(t1 == t0 and np.array_equal(a1, a0) and np.array_equal(b1, b0) for (a1, b1, t1), (a0, b0, t0) in zip(s1, s0))
    assert st1["calls"] == 3 and st1["rows"] == 3 * 64 and st1["rows_nan"] == 0 and st0["calls"] == 0
    assert all(k in head1.split(",") for k in loop.PolicyStats.KEYS) and not any(k in head0.split(",") for k in loop.PolicyStats.KEYS)
