"""GPU: scoring caller-supplied state-action pairs (sactd3_qvalues_device / sactd3_qvalues, include/sactd3.h).  Against the oracle's
twin critics at the suite's Q-value tolerance; everything else is an equality: a row's values are the same bits whatever rows are
scored with it, the policy form is its own composition, views change nothing, and training cannot tell whether a call was made.

Engines come from shape_engines() of tests/gpu_support.py (B = 64, a 2048-row ring, the oracle's perturbed parameters); the rows are
its data(): synth_transitions(1041, seed 5).  Shapes: SAC Hopper (K = o + a = 14: fused first layer), TD3 HalfCheetah (K = 23), SAC
Humanoid (K = 393: k_nt_wide + the unfused layer 2), SAC Hopper without LayerNorm, and K = 64 / 65, the two sides of the fused first
layer's limit.  Row counts 1, 5, 16, 17, 67: one row, a partial tile, a whole one, a whole one and a row, several blocks; 1041 crosses
the 1024-row chunk and ends in a partial tile."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import RefAgent
from tests.gpu_support import (DEV, MAXN, NROWS, SENTINEL, P, _lib, assert_same_state, close, close_engines, data, same_bits, score,  # noqa: F401
                               shape_engines, stream)
from tests.helpers import observe, synth_transitions

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 16, 17, 67)


def oracle_q(ref, obs, act, target):
    """[2, n] float32; act None: the policy form"""
    with torch.no_grad():
        if act is None:
            act = torch.as_tensor(ref.predict(obs, explore=False))
        return RefAgent._twin(ref.qnets_target if target else ref.qnets, obs, act).squeeze(-1).numpy()


# ------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah", "sac-humanoid", "sac-hopper-noln", "sac-k64", "sac-k65"])
def test_scores_match_the_oracles_twin_critics(shape):
    """RefAgent._twin on the same rows, online and target, explicit actions and pi(s) = ref.predict(explore=False): rtol 1e-5 +
    atol 1e-5, what the suite applies to debug_read("q") / "q_target" / "q_pi" at these shapes and this data distribution (the float32
    oracle sits within 7 % of that of its float64 self on exactly these inputs: 1.0e-6 at |Q| <= 3.3)."""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs, act = data(shape)
    obs_d, act_d = obs.to(DEV), act.to(DEV)
    for target in (False, True):
        want = {False: oracle_q(ref, obs[:max(ROWS)], act[:max(ROWS)], target), True: oracle_q(ref, obs[:max(ROWS)], None, target)}
        for policy in (False, True):
            for n in ROWS:
                got = score(eng, obs_d[:n], None if policy else act_d[:n], target)
                assert got.shape == (2, n) and np.isfinite(got).all()
                w = want[policy][:, :n]
                observe(f"qvalues_against_oracle[{shape}]", f"{'target' if target else 'online'} {'policy' if policy else 'explicit'}: max |dq| / (1e-5 + 1e-5 |q|)",
                        float((np.abs(got - w) / (1e-5 + 1e-5 * np.abs(w))).max()))
                print(shape, "target" if target else "online", "policy" if policy else "explicit", n, "max |dq|", float(np.abs(got - w).max()))
                close(got, w, rtol=1e-5, atol=1e-5, name=f"{shape} target={target} policy={policy} n={n}")
    assert eng.qvalues_stats() == dict(calls=20, rows=4 * sum(ROWS), ordered_calls=20, policy_calls=10)


# ------------------------------------------------------------------------------------------ 2. a row's bits do not depend on its company
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah", "sac-humanoid", "sac-hopper-noln", "sac-k65"])
def test_a_rows_values_do_not_depend_on_the_rows_scored_with_it(shape):
    """row i alone, inside 67 rows and inside 1041 rows (two chunks: 1024 rows in the launch shape of many tiles, then 17): the same
    bits, explicit and policy actions, online and target"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs, act = [t.to(DEV) for t in data(shape)]
    for policy in (False, True):
        for target in (False, True):
            full = score(eng, obs, None if policy else act, target)
            mid = score(eng, obs[:67], None if policy else act[:67], target)
            assert full.shape == (2, NROWS) and np.isfinite(full).all()
            assert same_bits(full[:, :67], mid), (policy, target)
            for i in (0, 5, 16, 66, 1023, 1024, 1040):
                one = score(eng, obs[i:i + 1], None if policy else act[i:i + 1], target)
                assert same_bits(one, full[:, i:i + 1]), (policy, target, i)
            tail = score(eng, obs[1000:], None if policy else act[1000:], target)      # 41 rows, another position in the chunk
            assert same_bits(tail, full[:, 1000:]), (policy, target)


def test_a_call_of_batch_size_rows_takes_no_large_batch_form():
    """Humanoid, B = 1024: the trunk's 64 x 64 / 32 x 32 forms belong to M == B >= 1024 -- 1024 scored rows must not take them:
    the same bits as the same rows scored 16 at a time, explicit and policy actions"""
    ref, (eng,), (o, a, bound) = shape_engines("sac-humanoid", B=1024)
    obs, act = [t.to(DEV)[:1024] for t in data("sac-humanoid")]
    for policy in (False, True):
        full = score(eng, obs, None if policy else act)
        parts = [score(eng, obs[lo:lo + 16], None if policy else act[lo:lo + 16]) for lo in range(0, 1024, 16)]
        assert same_bits(full, np.concatenate(parts, axis=1)), policy
    want = oracle_q(ref, data("sac-humanoid")[0][:1024], data("sac-humanoid")[1][:1024], False)
    close(score(eng, obs, act), want, rtol=1e-5, atol=1e-5, name="humanoid B=1024")


# ------------------------------------------------------------------------------------------ 3. the policy form is its composition
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah", "sac-humanoid"])
def test_policy_form_equals_scoring_the_exploit_action(shape):
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs = data(shape)[0].to(DEV)
    for n in (1, 5, 17, 67, MAXN):
        pi = torch.empty(n, a, device=DEV)
        eng.predict_device(obs[:n].data_ptr(), o, n, False, pi.data_ptr(), a, stream())
        for target in (False, True):
            assert same_bits(score(eng, obs[:n], None, target), score(eng, obs[:n], pi, target)), (n, target)


# ------------------------------------------------------------------------------------------ 4. views, and the host call
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah", "sac-humanoid"])
def test_views_in_and_out_and_the_host_call(shape):
    """obs = big[:, 1:1+o], actions = wide[:, 3:3+a] (rows 4-byte aligned only, strides above the widths), out = a [2, n + 2, 1] view
    at an odd offset of a sentinel-filled tensor: the bits of the contiguous call, nothing outside [2, n] touched, sources unchanged;
    Engine.q_values and Agent.q_values on host arrays give the same bits as numpy"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    ag = P.Agent.__new__(P.Agent)                                    # the mirror's method on an engine of this test
    ag.engine = eng
    obs_h, act_h = data(shape)
    for n in (1, 5, 67):
        obs, act = obs_h[:n].to(DEV), act_h[:n].to(DEV)
        big = torch.full((n, o + 5), float("nan"), device=DEV)
        big[:, 1:1 + o] = obs
        wide = torch.full((n, a + 6), float("nan"), device=DEV)
        wide[:, 3:3 + a] = act
        big0, wide0 = big.clone(), wide.clone()
        for target in (False, True):
            for policy in (False, True):
                want = score(eng, obs, None if policy else act, target)
                base = torch.full((2, n + 3, 3), SENTINEL, device=DEV)
                view = base[:, 1:, 1:2]
                td = {"observations": big[:, 1:1 + o]} if policy else {"observations": big[:, 1:1 + o], "actions": wide[:, 3:3 + a]}
                gen = eng.batch_generation()
                got = ag.q_values(td, target=target, out=view)
                assert eng.batch_generation() == gen
                assert tuple(got.shape) == (2, n, 1) and got.data_ptr() == view.data_ptr()
                host = base.cpu().numpy()
                assert same_bits(host[:, 1:1 + n, 1], want), (n, target, policy)
                host[:, 1:1 + n, 1] = np.float32(SENTINEL)
                assert same_bits(host, np.full_like(host, SENTINEL)), (n, target, policy)
                # `out` made by the call; float64 / inner-stride sources are converted on the device
                td2 = {"observations": obs.double()} if policy else {"observations": obs.double(), "actions": act.t().contiguous().t()}
                res = ag.q_values(td2, target=target)
                assert res.dtype == torch.float32 and res.is_cuda and tuple(res.shape) == (2, n, 1) and same_bits(res.cpu().numpy()[:, :, 0], want)
                # host arrays: numpy, the same bits
                host_q = eng.q_values(obs_h[:n].numpy(), None if policy else act_h[:n].numpy(), target)
                assert isinstance(host_q, np.ndarray) and same_bits(host_q, want), (n, target, policy)
                td3 = {"observations": obs_h[:n].numpy()} if policy else {"observations": obs_h[:n], "actions": act_h[:n].numpy()}
                res = ag.q_values(td3, target=target)
                assert isinstance(res, np.ndarray) and res.shape == (2, n, 1) and same_bits(res[:, :, 0], want)
        assert torch.equal(big.view(torch.int32), big0.view(torch.int32)) and torch.equal(wide.view(torch.int32), wide0.view(torch.int32))
    with pytest.raises(TypeError):                                   # one field on the host, one on the device
        ag.q_values({"observations": obs_h[:4].to(DEV), "actions": act_h[:4].numpy()})
    # more rows than a chunk through the host call: the bits of the device call
    assert same_bits(eng.q_values(obs_h.numpy(), act_h.numpy()), score(eng, obs_h.to(DEV), act_h.to(DEV)))


# ------------------------------------------------------------------------------------------ 5. invisible to training
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-td3_2"])
def test_scoring_between_chained_periods_changes_nothing(shape):
    """two engines, one scores (online, target, policy form; 67 rows) between rb_extend and the periods and between two back-to-back
    periods -- the second starts from the opening pair the first precomputed, if the chain holds: same parameters, Adam state, metrics,
    sampled indices and graphs; the counters count what was called.  Then a score inside predict_begin / predict_end: the action and
    the exploration draw of the twin that did not score."""
    _, (R, N), (o, a, bound) = shape_engines(shape, count=2, cap=1000)
    obs, act = [t[:67].to(DEV) for t in data(shape)]
    res = []
    for eng, scores in ((R, True), (N, False)):
        eng.rb_extend(*[t.numpy() for t in synth_transitions(600, o, a, bound, seed=31)])
        it, samples = 0, []

        def read():
            if scores:
                for q in (score(eng, obs, act), score(eng, obs, act, True), score(eng, obs)):
                    assert np.isfinite(q).all()
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
        res.append((samples, [eng.graph_kernel_count(w) for w in range(8)]))
    (sr, gr), (sn, gn) = res
    assert_same_state(R, N)
    assert all(np.array_equal(x, y) for x, y in zip(sr, sn)) and len(sr) == 4
    assert gr == gn and sum(gr) > 0
    assert R.qvalues_stats() == dict(calls=21, rows=21 * 67, ordered_calls=21, policy_calls=7)
    assert N.qvalues_stats() == dict(calls=0, rows=0, ordered_calls=0, policy_calls=0)
    # allowed while an acting call is in flight, and invisible to it
    for n in (4, 17):
        ob = data(shape)[0][100:100 + n].numpy()
        R.predict_begin(ob, True)
        for q in (score(R, obs, act), score(R, obs, act, True), score(R, obs)):
            assert np.isfinite(q).all()
        got = R.predict_end()
        N.predict_begin(ob, True)
        assert np.array_equal(got, N.predict_end())
        assert np.array_equal(R.read_noise(_lib.SITE_PREDICT, n), N.read_noise(_lib.SITE_PREDICT, n))
    ra, na = R.acting_stats(), N.acting_stats()                       # (how a call's wait ended is timing, not schedule)
    assert all(ra[k] == na[k] for k in ("begun", "begin_waited_for_learner", "learner_waited_for_acting")) and ra["begun"] == 2


# ------------------------------------------------------------------------------------------ 6. follows the parameters
@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah"])
def test_scores_follow_the_parameters(shape):
    """one critic update + Polyak step with an injected draw, on the engine and on the oracle: the online and the target scores of
    fixed rows both change, and meet the oracle's new ones at the tolerance of test 1"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    obs_h, act_h = [t[:67] for t in data(shape)]
    obs, act = obs_h.to(DEV), act_h.to(DEV)
    before = [score(eng, obs, act), score(eng, obs, act, True), score(eng, obs)]
    batch = synth_transitions(64, o, a, bound, seed=11)
    eps = torch.randn(64, a, generator=torch.Generator().manual_seed(12))
    ref.update_qnets(ref.to_batch(*batch), eps)
    ref.qnet_updates_so_far += 1
    ref.update_targ_nets()
    eng.load_batch(*[t.numpy() for t in batch])
    eng.set_noise(_lib.SITE_CRITIC, eps)
    eng.update_qnets()
    eng.update_targ_nets(1)
    after = [score(eng, obs, act), score(eng, obs, act, True), score(eng, obs)]
    want = [oracle_q(ref, obs_h, act_h, False), oracle_q(ref, obs_h, act_h, True), oracle_q(ref, obs_h, None, False)]
    for name, b, x, w in zip(("online", "target", "policy"), before, after, want):
        assert not np.array_equal(b, x), name
        observe(f"qvalues_follow_the_parameters[{shape}]", f"{name}: max |dq| / (1e-5 + 1e-5 |q|)", float((np.abs(x - w) / (1e-5 + 1e-5 * np.abs(w))).max()))
        print(shape, name, "max |dq|", float(np.abs(x - w).max()), "moved by", float(np.abs(x - b).max()))
        close(x, w, rtol=1e-5, atol=1e-5, name=f"{shape} {name} after the update")


@pytest.mark.parametrize("shape", ["sac-hopper", "td3-halfcheetah", "sac-humanoid"])
def test_a_scored_row_has_the_bits_the_critic_update_computes(shape):
    """the batch's (s, a) rows scored with the online critics, then update_qnets on that batch: debug_read("q") -- the Q-values the
    update computed from the same parameters, in the B < 1024 kernels' K split -- holds the same bits"""
    ref, (eng,), (o, a, bound) = shape_engines(shape)
    batch = synth_transitions(64, o, a, bound, seed=11)
    eng.load_batch(*[t.numpy() for t in batch])
    got = score(eng, batch[0].to(DEV), batch[1].to(DEV))
    eng.update_qnets()
    assert same_bits(got, eng.debug_read("q").reshape(2, 64))


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_leave_the_engine_usable():
    ref, (eng,), (o, a, bound) = shape_engines("sac-hopper")
    lib, h, ORD, vp = eng.lib, eng._h, _lib.SRC_ORDERED, C.c_void_p
    obs, act = [t[:8].to(DEV) for t in data("sac-hopper")]
    out = torch.full((2, 8), SENTINEL, device=DEV)
    host_o, host_a, host_q = np.zeros((8, o), np.float32), np.zeros((8, a), np.float32), np.zeros((2, 8), np.float32)
    pinned = torch.zeros(8, o).pin_memory()
    po, pa, pq = vp(obs.data_ptr()), vp(act.data_ptr()), vp(out.data_ptr())
    call = lambda *args: lib.sactd3_qvalues_device(h, *args)
    assert call(po, o, pa, a, 8, 0, pq, 1, 8, None, ORD) == 0                                # (the valid call, so that what follows isolates one fault each)
    eng.sync()
    good = out.cpu().numpy().copy()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert call(None, o, pa, a, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL                    # NULL obs / q
    assert call(po, o, pa, a, 8, 0, None, 1, 8, None, ORD) == _lib.EINVAL
    assert call(vp(host_o.ctypes.data), o, pa, a, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL  # host pointers: pageable, pinned
    assert call(vp(pinned.data_ptr()), o, pa, a, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL
    assert call(po, o, vp(host_a.ctypes.data), a, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL
    assert call(po, o, pa, a, 8, 0, vp(host_q.ctypes.data), 1, 8, None, ORD) == _lib.EINVAL
    assert b"device memory" in lib.sactd3_last_error(h)
    assert call(po, o - 1, pa, a, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL                  # strides below the widths
    assert call(po, o, pa, a - 1, 8, 0, pq, 1, 8, None, ORD) == _lib.EINVAL
    assert call(po, o, pa, a, 8, 0, pq, 0, 8, None, ORD) == _lib.EINVAL
    assert call(po, o, pa, a, 8, 0, pq, 1, 0, None, ORD) == _lib.EINVAL
    assert call(po, o, pa, a, 0, 0, pq, 1, 8, None, ORD) == _lib.EINVAL                      # n = 0
    assert call(po, o, pa, a, 8, 2, pq, 1, 8, None, ORD) == _lib.EINVAL                      # which = 2
    assert call(po, o, pa, a, 8, -1, pq, 1, 8, None, ORD) == _lib.EINVAL
    assert call(po, o, pa, a, 8, 0, pq, 1, 8, None, 2) == _lib.EINVAL                        # an unknown flag
    fp = C.POINTER(C.c_float)
    assert lib.sactd3_qvalues(h, host_o.ctypes.data_as(fp), host_a.ctypes.data_as(fp), 0, 0, host_q.ctypes.data_as(fp)) == _lib.EINVAL
    assert lib.sactd3_qvalues(h, host_o.ctypes.data_as(fp), host_a.ctypes.data_as(fp), 8, 2, host_q.ctypes.data_as(fp)) == _lib.EINVAL
    assert lib.sactd3_qvalues(h, None, None, 8, 0, host_q.ctypes.data_as(fp)) == _lib.EINVAL
    with pytest.raises(P.EngineError, match="which|n >= 1|stride|flag|device memory|null"):
        eng.q_values_device(obs.data_ptr(), o - 1, act.data_ptr(), a, 8, False, out.data_ptr(), 1, 8)
    st = (C.c_int64 * 4)()
    assert lib.sactd3_qvalues_stats(h, None) == _lib.EINVAL
    assert lib.sactd3_qvalues_stats(h, st) == 0 and list(st) == [1, 8, 1, 0]                 # none of those launched anything
    eng.sync()
    assert (out == SENTINEL).all()
    assert call(po, o, pa, a, 8, 0, pq, 1, 8, None, ORD) == 0                                # ... and the engine is as usable as before
    eng.sync()
    assert same_bits(out.cpu().numpy(), good)
