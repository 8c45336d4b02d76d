"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP engine, called through the C ABI, against the
oracle (oracle/sac_td3_ref.py = autograd restatement of the reference; oracle/manual_grads.py = the same maths
in the engine's kernel decomposition, used to localise a faulty kernel).

Tolerances: fp32 with a different summation order than torch.  Losses / Q-values / targets: rtol 1e-5 + atol 1e-5
(north_star).  Gradients: atol scaled by the tensor's max (reductions over B).  Post-Adam parameters: see
tests/helpers.py:assert_params_close.
"""
import numpy as np
import pytest
import torch

from oracle import replay_ref
from oracle.sac_td3_ref import Hps, RefAgent
from tests import noise_model
from tests.gpu_stage_checks import check_update_actor_intermediates, check_update_qnets_intermediates
from tests.gpu_support import (P, _lib, actor_layout, close, close_engines, crit_layout, flat_actor, flat_critics, gclose, logp_close,  # noqa: F401
                               make_pair, push_params, schema, track)
from tests.helpers import (DIMS, PINNED_CPU_ENV, assert_params_close, in_pinned_cpu_process, observe, randomize_ln,
                           synth_transitions)

pytestmark = pytest.mark.gpu


def scalars_close(test, it, got, want, tol):
    """every reported scalar of one iteration: |engine - oracle| <= tol (1 + |oracle|)  (= rtol tol + atol tol); the observed
    worst value is recorded per (test, iteration) so that `tol` can be kept near what is measured"""
    for k, v in want.items():
        d = abs(got[k] - v) / (1.0 + abs(v))
        observe(test, f"iter {it} scalars", d)
        assert d <= tol, f"{test} iter {it} {k}: engine {got[k]!r} oracle {v!r} normalised delta {d:.3e} > {tol:.1e}"


# ------------------------------------------------------------------------------------------ replay buffer

def test_params_roundtrip():
    ref, eng, _ = make_pair("sac", "hopper", 32)
    for which, want in ((_lib.ACTOR, flat_actor(ref, ref.actor)), (_lib.CRITICS_TARGET, flat_critics(ref, ref.qnets_target))):
        assert np.array_equal(eng.get_params(which), want)
    m = np.random.default_rng(0).standard_normal(eng.param_count(_lib.CRITICS)).astype(np.float32)
    eng.set_adam_state(_lib.CRITICS, m, m * m, 7)
    m2, v2, st = eng.get_adam_state(_lib.CRITICS)
    assert np.array_equal(m, m2) and np.array_equal(m * m, v2) and st == 7


@pytest.mark.parametrize("env", ["hopper", "halfcheetah", "humanoid"])
def test_replay_extend_gather_bit_exact(env):
    o, a, bound = DIMS[env]
    B, cap = 64, 1000
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=cap, max_envs=8), [-bound] * a, [bound] * a))
    ring = replay_ref.RingRef(cap, o, a)
    rng = np.random.default_rng(1)
    obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(1300, o, a, bound, seed=2)]
    done[::7] = True
    assert eng.rb_len() == 0
    pos = 0
    for n in (1, 4, 4, 8, 300, 683, 300):  # ragged pushes that wrap the ring once
        sl = slice(pos, pos + n)
        eng.rb_extend(obs[sl], act[sl], rew[sl], nobs[sl], done[sl])
        ring.extend(obs[sl], act[sl], rew[sl], nobs[sl], done[sl])
        pos += n
        assert eng.rb_len() == ring.len
        idx = rng.integers(0, ring.len, B)
        idx[0], idx[-1] = 0, ring.len - 1
        eng.rb_sample_with_indices(idx)
        got, want = eng.read_batch(), ring.gather(idx)
        for k in want:
            assert np.array_equal(got[k], want[k]), (env, n, k)
    with pytest.raises(P.EngineError):
        eng.rb_sample_with_indices(np.full(B, ring.len))  # out of range is refused, not read


def test_empty_buffer_refuses_sampling():
    eng = track(P.Engine(P.Config(ob_dim=11, ac_dim=3, batch_size=16, rb_capacity=64), [-1] * 3, [1] * 3))
    with pytest.raises(P.EngineError):
        eng.rb_sample()
    with pytest.raises(P.EngineError):
        eng.step(False)


def test_native_index_stream_matches_philox_oracle():
    o, a, bound = DIMS["hopper"]
    B, seed = 256, 1234567890123
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=5000, seed=seed), [-1] * a, [1] * a))
    obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(3000, o, a, bound, seed=3)]
    eng.rb_extend(obs, act, rew, nobs, done)
    for draw in range(3):
        eng.rb_sample()
        got = eng.read_batch()
        want_idx = replay_ref.sample_indices(seed, draw, B, 3000)
        assert np.array_equal(got["index"], want_idx)
        assert np.array_equal(got["observations"], obs[want_idx]) and np.array_equal(got["rewards"], rew[want_idx])
        assert np.array_equal(got["actions"], act[want_idx]) and np.array_equal(got["dones"], done[want_idx])
        assert np.array_equal(got["next_observations"], nobs[want_idx])


def test_gather_with_several_chunks_per_thread():
    """Above 2^20 16-byte chunks per batch k_gather gives every thread GATHER_CPT chunks of a contiguous span (the shape of the
    bandwidth sweep): B = 4096 rows of a 600-wide observation = 1.2 M chunks.  Bit-exact against the host copy of the rows."""
    o, a, B, seed = 600, 4, 4096, 99
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=8192, seed=seed), [-1] * a, [1] * a))
    obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(6000, o, a, 1.0, seed=8)]
    eng.rb_extend(obs, act, rew, nobs, done)
    for draw in range(2):
        eng.rb_sample()
        got = eng.read_batch()
        idx = replay_ref.sample_indices(seed, draw, B, 6000)
        assert np.array_equal(got["index"], idx)
        assert np.array_equal(got["observations"], obs[idx]) and np.array_equal(got["next_observations"], nobs[idx])
        assert np.array_equal(got["actions"], act[idx]) and np.array_equal(got["rewards"], rew[idx]) and np.array_equal(got["dones"], done[idx])


def test_full_size_ring_properties():
    """BASELINE config 4 at full size (Humanoid-v4 records, 1 000 000 rows = 3.1 GB of HBM, B = 1024), where the ring cannot
    be mirrored on the host: size-independent properties instead.  (i) the native index stream is the Philox oracle's,
    in range; (ii) sampling is idempotent: gathering the SAME indices again (injected) returns bit-identical rows, and a
    row drawn twice inside one batch is identical both times; (iii) rows written by rb_extend at the wrap-around edge of
    a full ring come back bit-exact and the length saturates at the capacity."""
    o, a, bound = DIMS["humanoid"]
    B, cap, seed = 1024, 1_000_000, 77
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=cap, seed=seed), [-bound] * a, [bound] * a))
    eng.rb_fill_synthetic(cap - 3, seed=5)
    assert eng.rb_len() == cap - 3
    obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(8, o, a, bound, seed=6)]
    eng.rb_extend(obs, act, rew, nobs, done)             # rows cap-3 .. cap-1, then wraps onto rows 0 .. 4
    assert eng.rb_len() == cap
    eng.rb_sample()
    first = eng.read_batch()
    want_idx = replay_ref.sample_indices(seed, 0, B, cap)
    assert np.array_equal(first["index"], want_idx) and first["index"].min() >= 0 and first["index"].max() < cap
    eng.rb_sample_with_indices(first["index"])
    again = eng.read_batch()
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    probe = np.concatenate([np.arange(cap - 3, cap), np.arange(0, 5), np.full(B - 8, cap - 1)])
    eng.rb_sample_with_indices(probe)
    got = eng.read_batch()
    assert np.array_equal(got["observations"][:8], obs) and np.array_equal(got["next_observations"][:8], nobs)
    assert np.array_equal(got["actions"][:8], act) and np.array_equal(got["rewards"][:8], rew) and np.array_equal(got["dones"][:8], done)
    assert np.array_equal(got["observations"][8:], np.broadcast_to(obs[2], (B - 8, o)))      # the same row, 1016 times over


def test_synthetic_fill_statistics():
    o, a, bound = DIMS["humanoid"]
    B = 1024
    eng = track(P.Engine(P.Config(ob_dim=o, ac_dim=a, batch_size=B, rb_capacity=20000), [-bound] * a, [bound] * a))
    eng.rb_fill_synthetic(20000, seed=9)
    assert eng.rb_len() == 20000
    eng.rb_sample()
    b = eng.read_batch()
    assert abs(b["observations"].mean()) < 0.01 and abs(b["observations"].std() - 1) < 0.01
    assert abs(b["next_observations"].std() - 1) < 0.01 and abs(b["rewards"].std() - 1) < 0.1
    assert b["actions"].min() >= -bound and b["actions"].max() <= bound and abs(b["actions"].mean()) < 0.01
    assert 0 <= b["dones"].mean() < 0.05


# ------------------------------------------------------------------------------------------ single updates

# the last four run the large-batch kernel forms (B >= 1024, csrc/engine.hip BIG_BATCH): k_nt64 / k_nt64_ln (4-, 2- and 1-net
# launches), k_nn64, k_critic_tail<16>, k_ln_bwd<16> (+ the fused dQ/da slice product), k_tn64 + k_adam_red, k_actor_tail(2),
# k_actor_head_bwd -- every intermediate and every per-key gradient against oracle/manual_grads.py, like the small-batch forms
CASES = [("sac", "hopper", 256, True), ("sac", "hopper", 40, False), ("td3", "halfcheetah", 256, True),
         ("sac", "humanoid", 96, True), ("sac", "humanoid", 1024, True), ("td3", "humanoid", 1024, True),
         ("sac", "hopper", 1024, True), ("sac", "humanoid", 1024, False),
         # more than one 256-row slab below B = 1024: the fused row + GEMM launches with a ragged last row block, and k_tn's folded
         # LayerNorm backward across two slabs (the second one partly masked)
         ("sac", "hopper", 300, True), ("td3", "halfcheetah", 512, True),
         # the other shapes of the dQ/da partials (helpers.DIMS)
         ("sac", "sac4", 128, True), ("td3", "td3_2", 64, True), ("td3", "td3_7", 256, False)]


@pytest.mark.parametrize("algo,env,B,ln", CASES)
def test_update_qnets_intermediates(algo, env, B, ln):
    check_update_qnets_intermediates(algo, env, B, ln)


@pytest.mark.parametrize("algo,env,B,ln", CASES)
def test_update_actor_intermediates(algo, env, B, ln):
    check_update_actor_intermediates(algo, env, B, ln)


def _fixture_views(fx, prefix, key, got):
    """[(label, got view, stored view, elements summed)] of one gradient against its entry in tests/golden/nets_bwd_*.npz"""
    name = f"{prefix}/{key}"
    got = np.asarray(got, np.float32)
    if name in fx.files:
        return [(name, got, fx[name], 1)]
    return [(name + "/rows8", got[::8], fx[name + "/rows8"], 1), (name + "/rowsum", got.astype(np.float64).sum(1), fx[name + "/rowsum"], got.shape[1]),
            (name + "/colsum", got.astype(np.float64).sum(0), fx[name + "/colsum"], got.shape[0])]


def _grads_match_fixture(fx, prefix, got_dict, what):
    """per key: gclose's bound (rtol 2e-4, atol 2e-6 + 1e-5 max|g|) widened by 8x the fp32 noise floor the fixture measured for that
    key with the reference's own modules (`noise/...` = max |fp32 - fp64| of torch's gradient: make_golden.bwd_functionals)"""
    for k, g in got_dict.items():
        views = _fixture_views(fx, prefix, k, g)
        gmax = max(float(np.abs(v[2]).max()) for v in views if v[3] == 1)
        floor = 8.0 * float(fx[f"noise/{prefix}/{k}"])
        observe("kernels_reproduce_the_reference_nets_backward", f"{prefix}/{k}: fp32 noise floor / max|g|", float(fx[f"noise/{prefix}/{k}"]) / max(gmax, 1e-30))
        for label, got, want, n in views:
            if n == 1:
                observe("kernels_reproduce_the_reference_nets_backward", f"{label}: max |hip - reference| / max|g|", float(np.abs(got - want).max()) / max(gmax, 1e-30))
                close(got, want, rtol=2e-4, atol=2e-6 + 1e-5 * gmax + floor, name=f"{what} {label}")
            else:   # float64 sums of n elements, each within the bound above
                np.testing.assert_allclose(got, want, rtol=2e-4, atol=n * (2e-6 + 1e-5 * gmax + floor), err_msg=f"{what} {label}")


@pytest.mark.parametrize("env", ["hopper", "halfcheetah", "humanoid"])
def test_kernels_reproduce_the_reference_nets_backward(env, tmp_path):
    """HIP kernels against autograd through the REFERENCE's own network classes (hashed in tests/golden/nets_bwd_*.npz, written by
    tests/golden/make_golden.py from /root/reference/agents/nets.py; the oracle reproduces them bit for bit on the CPU,
    tests/test_golden.py).  Same parameters (seeds 11 / 13 / 14 / 16), same inputs (seed 321), same rsample noise (seed 12), at the
    BASELINE batch sizes (Hopper / HalfCheetah 256, Humanoid 1024: the large-batch kernel forms).
      critic loss  sum_i mse(Q_i(s, a), y)  (agents/agent.py:230-233): dones = 1 makes the Bellman target the reward, rewards = y
                   -> k_nt / k_nt64(_ln) -> k_critic_tail -> k_nn(64) -> k_ln_bwd -> k_tn / k_tn64 + k_adam_red, every gradient per key;
      actor loss   (alpha logp - min Q).mean() (:272-281) and TD3's (-Q1).mean(): k_actor_tail(_s) -> critic trunk -> k_actorq_tail ->
                   k_nn -> k_ln_bwd (+dQ/da) -> k_actor_head_bwd(_s) -> k_nn -> k_ln_bwd -> k_tn, action / logp / Q / dL/da / every gradient."""
    import importlib.util
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    from oracle.sac_td3_ref import DetPolicy, QNet, SquashedGaussPolicy
    o, a, bound = DIMS[env]
    B = mg.BWD_B[env]
    # the reference's numbers: recomputed by the oracle's classes with the pinned CPU numerics (tests/helpers.py), and written only
    # if every array hashes to its entry of tests/golden/nets_bwd_<env>.npz (tests/test_golden.py: the oracle reproduces them)
    path = tmp_path / f"nets_bwd_{env}.npz"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(here, "golden", "make_golden.py"), "--oracle-bwd", env, str(path)]
    out = subprocess.run(cmd, env=dict(os.environ, **PINNED_CPU_ENV), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fx = np.load(path)
    ob, ac, y, eps, digest = mg.bwd_inputs(env)
    assert np.array_equal(digest, fx["digest"]) and np.array_equal(eps.numpy(), fx["eps"])      # the regenerated inputs ARE the fixture's
    mn, mx = torch.full((a,), -bound), torch.full((a,), bound)
    torch.manual_seed(11); actor = SquashedGaussPolicy(o, a, mn, mx, True)
    torch.manual_seed(13); q1 = QNet(o, a, True)
    torch.manual_seed(14); pi = DetPolicy(o, a, mn, mx, 0.1, True)
    torch.manual_seed(16); q2 = QNet(o, a, True)
    flat_q = np.concatenate([schema.dict_to_flat(q.state_dict(), o + a, 1, True) for q in (q1, q2)])
    ones = torch.ones(B, dtype=torch.bool)
    H, ldc, a4 = 256, (o + a + 3) // 4 * 4, (a + 3) // 4 * 4
    for algo, net, nh in (("sac", actor, 2 * a), ("td3", pi, a)):
        hps = (Hps.td3 if algo == "td3" else Hps.sac)(batch_size=B, alpha_init=mg.BWD_ALPHA)
        eng = track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=B, max_envs=4, seed=0), [-bound] * a, [bound] * a))
        flat_a = schema.dict_to_flat({k: v for k, v in net.state_dict().items() if k.startswith(("fc_stack", "head"))}, o, nh, True)
        for which, flat in ((_lib.ACTOR, flat_a), (_lib.ACTOR_TARGET, flat_a), (_lib.CRITICS, flat_q), (_lib.CRITICS_TARGET, flat_q)):
            eng.set_params(which, flat)
        eng.load_batch(ob, ac, y, ob, ones)
        if algo == "sac":      # the critic loss (same kernels in both modes: once)
            eng.set_noise(_lib.SITE_CRITIC, eps)
            eng.update_qnets()
            close(eng.debug_read("targ_q"), y, 0, 0, "Bellman target == y (dones = 1)")
            close(eng.debug_read("q").reshape(2, B), fx["qloss/q"], name="Q(s, a) of the reference's Critic")
            close(eng.read_metrics()["loss/qf_loss"], fx["qloss/loss"], name="twin MSE")
            got = eng.debug_read("grad_critics").reshape(2, -1)
            for i in range(2):
                _grads_match_fixture(fx, f"qloss/critic{i}", schema.flat_to_dict(got[i], o + a, 1, True), "critic loss")
            eng.set_params(_lib.CRITICS, flat_q)          # (the Adam step moved them; the actor loss takes the fixture's critics)
            eng.set_noise(_lib.SITE_ACTOR0, eps); eng.set_noise(_lib.SITE_ALPHA0, eps)
        eng.update_actor()
        pre = f"aloss/{algo}"
        close(eng.debug_read("Xp").reshape(B, ldc)[:, o:o + a], fx[pre + "/a_pi"], name=f"{algo} pi(s)")
        nq = 2 if algo == "sac" else 1
        dA = eng.debug_read("dA").reshape(2, B, a4)[:nq, :, :a].sum(0)
        gclose(dA, fx[pre + "/d_action"], name=f"{algo} dLoss/dAction")
        if algo == "sac":
            logp_close(eng.debug_read("logp_pi"), fx[pre + "/logp"], fx[pre + "/a_pi"], bound, 0.0, "log pi(a|s)")
            close(eng.debug_read("q_pi").reshape(2, B), fx[pre + "/q_pi"], name="Q_i(s, pi(s))")
        close(eng.read_metrics()["loss/actor_loss"], fx[pre + "/loss"], name=f"{algo} actor loss")
        _grads_match_fixture(fx, pre, schema.flat_to_dict(eng.debug_read("grad_actor"), o, nh, True), f"{algo} actor loss")
        eng.close()


def test_clip_norm_and_polyak():
    ref, eng, (o, a, bound) = make_pair("sac", "hopper", 64, clip_norm=0.05)
    obs, act, rew, nobs, done = synth_transitions(64, o, a, bound, seed=8)
    e = torch.randn(64, a)
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_ACTOR0, e); eng.set_noise(_lib.SITE_ALPHA0, e)
    eng.update_actor()
    ref.update_actor(ref.to_batch(obs, act, rew, nobs, done), e, e)
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, 1, "clipped actor step", layout=actor_layout(ref))
    before = eng.get_params(_lib.CRITICS_TARGET)
    ref.qnet_updates_so_far = 1
    ref.update_targ_nets(); eng.update_targ_nets(1)
    after = eng.get_params(_lib.CRITICS_TARGET)
    assert not np.array_equal(before, after)
    close(after, flat_critics(ref, ref.qnets_target), rtol=1e-6, atol=1e-7, name="Polyak")


def test_crit_targ_update_freq_gate():
    ref, eng, _ = make_pair("sac", "hopper", 16, crit_targ_update_freq=2)
    t0 = eng.get_params(_lib.CRITICS_TARGET)
    eng.update_targ_nets(1)
    assert np.array_equal(eng.get_params(_lib.CRITICS_TARGET), t0)   # 1 % 2 != 0: no update (agent.py:323-324)
    eng.update_targ_nets(2)
    assert not np.array_equal(eng.get_params(_lib.CRITICS_TARGET), t0)


# ------------------------------------------------------------------------------------------ trajectories

# Trajectory comparisons (7-9 iterations from a common start, the drift of two fp32 Adam implementations included).  Every bound is
# set from what the tests observe on the GPU (tests/helpers.py:observe -> gpurun_out/parity_observed.json), at most ~2x above it:
#   scalars    |engine - oracle| <= tol (1 + |oracle|): 1e-5 (north_star) on the first iteration, 2e-5 FLAT afterwards
#              (observed: <= 2.2e-7 on the API-path trajectories, <= 8.0e-6 over the 7 fused iterations at the BASELINE shapes);
#   parameters per state_dict key: <= TRAJ_BAD of a matrix's elements and <= TRAJ_VEC_BAD elements of a vector beyond atol 2e-5 +
#              rtol 1e-5 (observed: 0 everywhere except Humanoid's 256 x 393 first critic layer after 7 iterations, 2.5e-2 / 1), and no
#              element further than TRAJ_CAP x lr from the oracle's (observed: <= 0.24 lr)
TRAJ_BAD, TRAJ_BAD_WIDE, TRAJ_VEC_BAD, TRAJ_CAP = 2e-3, 5e-2, 2, 0.5


def TRAJ_TOL(i):
    return 1e-5 if i == 0 else 2e-5


def push_adam(eng, ref):
    """the oracle's torch.optim.Adam states (exp_avg, exp_avg_sq, step) into the engine's optimisers, state_dict order."""
    def flat(modules, opt, in_dim, nh, key):
        out = []
        for m in modules:
            sd = {n: opt.state[p_][key] for n, p_ in m.named_parameters()}
            out.append(schema.dict_to_flat(sd, in_dim, nh, ref.hps.layer_norm))
        return np.concatenate(out)
    def step_of(opt):
        return int(round(float(next(iter(opt.state.values()))["step"]))) if opt.state else 0
    nh = ref.ac_dim if ref.hps.prefer_td3_over_sac else 2 * ref.ac_dim
    if ref.q_optimizer.state:
        eng.set_adam_state(_lib.CRITICS, flat(ref.qnets, ref.q_optimizer, ref.ob_dim + ref.ac_dim, 1, "exp_avg"),
                           flat(ref.qnets, ref.q_optimizer, ref.ob_dim + ref.ac_dim, 1, "exp_avg_sq"), step_of(ref.q_optimizer))
    if ref.actor_optimizer.state:
        eng.set_adam_state(_lib.ACTOR, flat([ref.actor], ref.actor_optimizer, ref.ob_dim, nh, "exp_avg"),
                           flat([ref.actor], ref.actor_optimizer, ref.ob_dim, nh, "exp_avg_sq"), step_of(ref.actor_optimizer))
    opt = getattr(ref, "alpha_optimizer", None)
    if opt is not None and opt.state:
        st = opt.state[ref.log_alpha]
        eng.set_adam_state(_lib.LOG_ALPHA, np.array([float(st["exp_avg"])], np.float32), np.array([float(st["exp_avg_sq"])], np.float32), step_of(opt))


def run_iterations(ref, eng, dims, n_iter, B, data_seed=11, before=None):
    o, a, bound = dims
    obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(2000, o, a, bound, seed=data_seed)]
    eng.rb_extend(obs, act, rew, nobs, done)
    g = torch.Generator().manual_seed(12)
    rng = np.random.default_rng(13)
    delay = ref.hps.actor_update_delay
    logs = []
    for i in range(n_iter):
        idx = rng.integers(0, 2000, B)
        noise = {"critic": torch.randn(B, a, generator=g), "actor": [torch.randn(B, a, generator=g) for _ in range(delay)],
                 "alpha": [torch.randn(B, a, generator=g) for _ in range(delay)]}
        b = ref.to_batch(obs[idx], act[idx], rew[idx], nobs[idx], done[idx])
        if before is not None:
            before(i)
        want = {k: float(v) for k, v in ref.iteration(b, i, noise).items()}
        do_actor = i % (delay + 1) == 0
        eng.set_noise(_lib.SITE_CRITIC, noise["critic"])
        eng.rb_sample_with_indices(idx)
        eng.update_qnets()
        if do_actor:
            for j in range(delay):
                eng.set_noise(_lib.SITE_ACTOR0, noise["actor"][j]); eng.set_noise(_lib.SITE_ALPHA0, noise["alpha"][j])
                eng.update_actor()
        eng.update_targ_nets(i + 1)
        got = eng.read_metrics()
        logs.append((want, got))
    return logs


@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah")])
def test_trajectory_api_path(algo, env):
    """orchestrator.py:337-352 driven call by call for 9 iterations with injected indices and noise."""
    B = 128
    ref, eng, dims = make_pair(algo, env, B)
    logs = run_iterations(ref, eng, dims, 9, B)
    rec = f"trajectory_api_path[{algo}-{env}]"
    for i, (want, got) in enumerate(logs):
        # error growth through the (chaotic) optimisation: north_star's 1e-5 on the first iteration, at most one more 1e-5 per iteration
        scalars_close(rec, i, got, want, TRAJ_TOL(i))
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, 9, "critics", max_bad_frac=TRAJ_BAD,
                        layout=crit_layout(ref), vec_bad=TRAJ_VEC_BAD, record=rec, max_lr_steps=TRAJ_CAP)
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, 6, "actor", max_bad_frac=TRAJ_BAD,
                        layout=actor_layout(ref), vec_bad=TRAJ_VEC_BAD, record=rec, max_lr_steps=TRAJ_CAP)
    assert_params_close(eng.get_params(_lib.CRITICS_TARGET), flat_critics(ref, ref.qnets_target), ref.hps.qnets_lr, 9, "critic targets",
                        layout=crit_layout(ref), record=rec, max_lr_steps=TRAJ_CAP)


RESYNC_TOL = 3e-5   # flat: |engine - oracle| <= RESYNC_TOL (1 + |oracle|) on every iteration (fp32 noise floor of the critic loss, see the docstring)


@pytest.mark.parametrize("algo,env,B", [("sac", "hopper", 256), ("td3", "halfcheetah", 256), ("sac", "humanoid", 128), ("sac", "humanoid", 1024)])
def test_every_iteration_from_the_oracles_own_state(algo, env, B):
    """The trajectory tests above widen their tolerance with the iteration number because two fp32 implementations of Adam drift
    apart (tests/helpers.py).  Here the drift is taken out: before EVERY iteration the engine is given the oracle's parameters,
    targets, temperature and Adam states, so each of the 9 iterations (3 with actor updates) is an independent one-iteration
    comparison from an evolved state -- and the tolerance is FLAT.  Its value is the fp32 noise floor of the critic loss (a mean of
    squared differences of O(1-10) numbers): evaluated from the same state, the oracle itself in float32 differs from the oracle in
    float64 by 0.9e-5 .. 1.3e-5 relative (measured on the CPU with the first iterations of this very trajectory), and two float32
    implementations by up to twice that; 26 of the 27 iterations compared here agree to <= 5e-6, one to 2.4e-5.
    orchestrator.py:337-352."""
    ref, eng, dims = make_pair(algo, env, B)
    def resync(i):
        push_params(eng, ref)
        push_adam(eng, ref)
    logs = run_iterations(ref, eng, dims, 9, B, before=resync)
    for i, (want, got) in enumerate(logs):
        scalars_close(f"every_iteration_from_the_oracles_own_state[{algo}-{env}-{B}]", i, got, want, RESYNC_TOL)


@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah")])
def test_graph_replay_equals_eager_launches(algo, env):
    """the captured hipGraphs and the plain launch sequence are the same kernels: bit-identical state."""
    B = 64
    outs = []
    for use_graphs in (True, False):
        ref, eng, (o, a, bound) = make_pair(algo, env, B, use_graphs=use_graphs)
        obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(500, o, a, bound, seed=21)]
        eng.rb_extend(obs, act, rew, nobs, done)
        for i in range(6):
            eng.rb_sample()
            eng.update_qnets()
            if i % 3 == 0:
                eng.update_actor(); eng.update_actor()
            eng.update_targ_nets(i + 1)
        outs.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET),
                     eng.read_metrics(), eng.graph_kernel_count(0)))
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(x, y)
    assert outs[0][3] == outs[1][3]
    assert outs[0][4] > 0 and outs[1][4] == 0


@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah")])
def test_period_and_cut_short_period_launch_sequences_equal_their_graphs(algo, env):
    """use_graphs = 0 issues the very launch sequences the period / cut-short-period / opening graphs are captured from (chained
    opening pairs included): 11 iterations through run_iterations -- singles, whole periods, a cut-short period -- are bit-identical
    with and without hipGraphs."""
    outs = []
    for use_graphs in (True, False):
        ref, eng, (o, a, bound) = make_pair(algo, env, 64, use_graphs=use_graphs, seed=3)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(700, o, a, bound, seed=22)])
        assert eng.run_iterations(1, 10) == 11 and eng.run_iterations(11, 4) == 15     # 1, 2 | 3-5 | 6-8 | 9, 10 cut short ; 11 | 12-14
        outs.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET), eng.get_params(_lib.ACTOR_TARGET),
                     eng.get_params(_lib.LOG_ALPHA), eng.read_batch()["index"], np.array(list(eng.read_metrics().values())), eng.graph_kernel_count(4)))
    for x, y in zip(outs[0][:7], outs[1][:7]):
        assert np.array_equal(x, y)
    assert outs[0][7] > 0 and outs[1][7] == 0


BASELINE_SHAPES = [("sac", "hopper", 256, 100_000), ("td3", "halfcheetah", 256, 100_000), ("sac", "humanoid", 1024, 65_536)]


@pytest.mark.parametrize("algo,env,B,cap", BASELINE_SHAPES)
def test_fused_step_against_oracle_at_baseline_shapes(algo, env, B, cap, request):
    """The TIMED path (sactd3_step: one hipGraph per iteration, native Philox sampling and noise) against the oracle at
    BASELINE.json's shapes -- configs 2 / 3 / 4: SAC Hopper B=256, TD3 HalfCheetah B=256, SAC Humanoid B=1024 with a
    65 536-row ring.  After every fused iteration the batch indices the engine drew and the normals it used at every
    noise site are read back and the oracle's `iteration` (orchestrator.py:337-352) is driven with exactly those, in the
    reference's draw order critic -> [actor -> alpha] x delay (agents/agent.py:205,254,298).  This exercises what only
    the fused form runs: the ring-indirect first layer, the gather blocks riding in the first trunk launch, the dual-draw
    actor tail, the temperature step riding in the next trunk launch, and at B >= 1024 the k_gather + k_nt64 route.
    Tolerance: losses / alpha rtol 1e-5 + atol 1e-5 on the first iteration (north_star), widening with the iteration
    number as in test_trajectory_api_path; parameters: tests/helpers.py:assert_params_close.  The oracle's initial parameters
    and iterations are computed with the pinned CPU numerics (tests/helpers.py), so that they do not change with the host."""
    if not in_pinned_cpu_process(request):
        return
    ref, eng, (o, a, bound) = make_pair(algo, env, B, seed=5, rb_capacity=cap)
    n = min(cap, 65_536)
    rows = [t.numpy() for t in synth_transitions(n, o, a, bound, seed=61)]
    rows[4][::9] = True
    for lo in range(0, n, 8192):
        eng.rb_extend(*[r[lo:lo + 8192] for r in rows])
    assert eng.rb_len() == n
    delay, n_iter = ref.hps.actor_update_delay, 7
    rec = f"fused_step_against_oracle_at_baseline_shapes[{algo}-{env}-{B}]"
    sites_a, sites_l = (_lib.SITE_ACTOR0, _lib.SITE_ACTOR1), (_lib.SITE_ALPHA0, _lib.SITE_ALPHA1)
    for i in range(n_iter):
        do_actor = i % (delay + 1) == 0
        eng.step(do_actor)
        got_b = eng.read_batch()
        idx = got_b["index"]
        assert idx.min() >= 0 and idx.max() < n
        for k, r in zip(("observations", "actions", "rewards", "next_observations", "dones"), rows):
            assert np.array_equal(got_b[k], r[idx]), (i, k)                       # the gather itself: bit-exact
        noise = {"critic": torch.from_numpy(eng.read_noise(_lib.SITE_CRITIC))}
        if do_actor and algo == "sac":
            noise["actor"] = [torch.from_numpy(eng.read_noise(sites_a[j])) for j in range(delay)]
            noise["alpha"] = [torch.from_numpy(eng.read_noise(sites_l[j])) for j in range(delay)]
        b = ref.to_batch(*[r[idx] for r in rows])
        want = {k: float(v) for k, v in ref.iteration(b, i, noise).items()}
        got = eng.read_metrics()
        scalars_close(rec, i, got, want, TRAJ_TOL(i))
        if i == 0:   # the gradients the fused launches left behind (critics; the SECOND actor update), per key, against autograd
            # (critics only: the actor arena holds the SECOND update's gradients, taken from parameters that are already one
            #  sign-like fp32 Adam step apart, tests/helpers.py; the actor's gradients are compared per key by the intermediates tests)
            got_c = eng.debug_read("grad_critics").reshape(2, -1)
            for qi in range(2):
                gd = schema.flat_to_dict(got_c[qi], o + a, 1, True)
                for (k, _), gr in zip(ref.qnets[qi].named_parameters(), ref.trace["q_grads"][qi * len(gd):(qi + 1) * len(gd)]):
                    gclose(gd[k], gr, name=f"fused step: critic{qi} grad {k}")
    n_act = delay * len([i for i in range(n_iter) if i % (delay + 1) == 0])
    bad = TRAJ_BAD_WIDE if env == "humanoid" else TRAJ_BAD
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, n_iter, "critics", max_bad_frac=bad,
                        layout=crit_layout(ref), vec_bad=TRAJ_VEC_BAD, record=rec, max_lr_steps=TRAJ_CAP)
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, n_act, "actor", max_bad_frac=TRAJ_BAD,
                        layout=actor_layout(ref), vec_bad=TRAJ_VEC_BAD, record=rec, max_lr_steps=TRAJ_CAP)
    assert_params_close(eng.get_params(_lib.CRITICS_TARGET), flat_critics(ref, ref.qnets_target), ref.hps.qnets_lr, n_iter, "critic targets",
                        layout=crit_layout(ref), record=rec, max_lr_steps=TRAJ_CAP)
    if algo == "td3":
        assert_params_close(eng.get_params(_lib.ACTOR_TARGET), flat_actor(ref, ref.actor_target), ref.hps.actor_lr, n_act, "actor target",
                            layout=actor_layout(ref), record=rec, max_lr_steps=TRAJ_CAP)
    else:
        close(eng.get_params(_lib.LOG_ALPHA)[0], ref.log_alpha, rtol=1e-5, atol=1e-6, name="log_alpha")
    _, _, tq = eng.get_adam_state(_lib.CRITICS)
    _, _, ta = eng.get_adam_state(_lib.ACTOR)
    assert tq == n_iter and ta == n_act                                          # counters of orchestrator.py:342,349


@pytest.mark.parametrize("algo,env,B", [("sac", "hopper", 64), ("td3", "halfcheetah", 64), ("sac", "humanoid", 64),
                                        ("sac", "hopper", 256), ("td3", "halfcheetah", 256), ("sac", "humanoid", 1024),
                                        ("td3", "humanoid", 1024), ("sac", "hopper", 1024),     # (wide / narrow observations at large batch)
                                        # past the 2-net tiling switch; past the 1-net switch; ragged at the top of the scope
                                        ("sac", "humanoid", 1473), ("sac", "hopper", 3009), ("td3", "halfcheetah", 4095)])
def test_fused_step_equals_api_sequence(algo, env, B):
    """sactd3_step (one graph per iteration) == rb_sample + update_qnets + 2x update_actor + update_targ_nets, bit for
    bit, at a small batch and at BASELINE.json's batch sizes (where other kernel instances are chosen)."""
    res = []
    for fused in (True, False):
        ref, eng, (o, a, bound) = make_pair(algo, env, B, seed=3)
        obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(3000, o, a, bound, seed=22)]
        eng.rb_extend(obs, act, rew, nobs, done)
        for i in range(7):
            if fused:
                eng.step(i % 3 == 0)
            else:
                eng.rb_sample()
                eng.update_qnets()
                if i % 3 == 0:
                    eng.update_actor(); eng.update_actor()
                eng.update_targ_nets(i + 1)
        res.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET),
                    eng.get_params(_lib.ACTOR_TARGET), eng.read_batch()["index"]))
    # same Philox streams (index: sample counter; noise: site codes 16+j / 32+j and the noise counter), same kernels
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)


# (algo, env, B, actor_update_delay, (first iteration, number of iterations))
PERIOD_CASES = [(algo, env, B, 2, (1, 10)) for algo, env, B in [
    ("sac", "hopper", 256), ("td3", "halfcheetah", 256), ("sac", "humanoid", 1024), ("sac", "hopper", 64),
    ("td3", "humanoid", 1024), ("sac", "sac4", 128), ("td3", "td3_7", 300), ("td3", "td3_2", 64),
    ("sac", "humanoid", 1473), ("sac", "hopper", 3009), ("td3", "halfcheetah", 4095)]]
# delay 1: the pipelined period with ONE critic-only iteration run ahead; delay 3: the period as four iterations back to back with
# deferred temperature steps (csrc/engine.hip period_is_pipelined); the smallest batch, where every launch is more than one block
PERIOD_CASES += [(algo, env, 64, delay, (1, 10)) for delay in (1, 3) for algo, env in (("sac", "hopper"), ("td3", "halfcheetah"))]
# a period, then step_prefix(1) on the opening pair that period left in the OTHER batch slot (the cut-short period graph of variant 1)
PERIOD_CASES += [(algo, env, 64, 2, (0, 4)) for algo, env in (("sac", "hopper"), ("td3", "halfcheetah"))]


def _period_case_id(case):
    algo, env, B, delay, span = case
    return f"{algo}-{env}-{B}" + (f"-delay{delay}" if delay != 2 else "") + (f"-from{span[0]}x{span[1]}" if span != (1, 10) else "")


@pytest.mark.parametrize("algo,env,B,delay,span", [pytest.param(*c, id=_period_case_id(c)) for c in PERIOD_CASES])
def test_period_graph_equals_single_iterations(algo, env, B, delay, span):
    """sactd3_step_period (delay + 1 iterations of the schedule of orchestrator.py:345-349 in ONE graph: actor updates in the first,
    then `delay` critic-only ones) == as many sactd3_step calls, bit for bit; Engine.run_iterations mixes both forms around period
    boundaries; with crit_targ_update_freq != 1 (SAC) the period form is refused and run_iterations falls back."""
    i0, n_iter = span
    hp = {} if delay == 2 else {"actor_update_delay": delay}
    res = []
    for mode in ("period", "single"):
        ref, eng, (o, a, bound) = make_pair(algo, env, B, seed=4, **hp)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(3000, o, a, bound, seed=23)])
        if mode == "period":
            # delay 2 from 1: iterations 1, 2 singly, periods 3-5 and 6-8, then 9, 10 as a cut-short period
            assert eng.run_iterations(i0, n_iter) == i0 + n_iter
        if mode == "period" and delay == 2 and span == (1, 10):
            eng.instantiate_graphs()                        # (the single iteration with actor updates was not needed so far: count its nodes)
            # SAC (pipelined, chained periods -- csrc/engine.hip BatchSlot / chain_ready): the period's last temperature step rides in the
            # next iteration's first launch (one node fewer); the critic-only iterations' sampling + next-action passes (trunk launch(es)
            # + tail: 2 nodes at narrow observations, 3 at wide ones) run ahead in the first iteration's last actor-trunk / tail launches,
            # and so does the opening pair of the NEXT period -- so a period graph holds no opening nodes at all; a 2- / 3-node opening
            # graph runs only when no precomputed pair is there (the first period, or after any state change in between)
            # TD3: the same, through the target actors of the NEXT Polyak updates (written ahead by the last actor update's Adam epilogue);
            # it has no temperature pair to ride in, so the run-ahead is a trunk + tail pair of its own at the end of the first iteration
            c0, c1 = eng.graph_kernel_count(2), eng.graph_kernel_count(3)
            o_ = DIMS[env][0]
            if not ((o_ <= 64 and B < 1024) or (o_ > 64 and 1024 <= B < 1473)):
                # csrc/engine.hip period_is_pipelined: only where the opening trunk gathers the replay rows itself (narrow observations
                # below B = 1024, wide ones from 1024 to 1472).  Elsewhere the period graph is the three single iterations back to back,
                # less (SAC) the last temperature step where the next iteration's opening trunk can carry it (opening_trunk_carries_alpha:
                # below B = 1473)
                assert eng.graph_kernel_count(4) == c1 + 2 * c0 - (1 if algo == "sac" and B < 1473 else 0)
            else:
                opening = 3 if env == "humanoid" else 2
                if algo == "sac":
                    assert eng.graph_kernel_count(4) == c1 - 1 + 2 * (c0 - opening) - opening and eng.graph_kernel_count(5) == opening
                else:
                    assert eng.graph_kernel_count(4) == c1 + 2 * (c0 - opening) and eng.graph_kernel_count(5) == opening
                # step_prefix(1): the iteration with the actor updates on a precomputed opening pair; step_prefix(2): + one critic-only
                # iteration whose opening pair ran ahead (SAC: in the temperature pair, whose step is deferred; TD3: a trunk + tail pair of its own)
                assert eng.graph_kernel_count(6) == c1 - opening
                assert eng.graph_kernel_count(7) == c1 - opening + (c0 - opening) + (-1 if algo == "sac" else opening)
        if mode == "single":
            for i in range(i0, i0 + n_iter):
                eng.step(i % (delay + 1) == 0)
        res.append([eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET), eng.get_params(_lib.ACTOR_TARGET),
                    eng.get_params(_lib.LOG_ALPHA), eng.get_adam_state(_lib.CRITICS)[2], eng.get_adam_state(_lib.ACTOR)[2]])
        # the batch the last iteration trained on and its critic-site draws: behind step_prefix(1) on the other slot (the (0, 4) spans)
        # that is slot 3, not slot 0
        res[-1] += [eng.read_batch()["index"], eng.read_noise(_lib.SITE_CRITIC)]
        if span != (1, 10):
            res[-1].append(np.array(list(eng.read_metrics().values())))
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    n_act = delay * len([i for i in range(i0, i0 + n_iter) if i % (delay + 1) == 0])
    assert res[0][5] == n_iter and res[0][6] == n_act      # counters of orchestrator.py:342,349 (10 and 6 at delay 2 from 1)
    if algo == "sac":
        ref, eng, (o, a, bound) = make_pair(algo, env, 32, crit_targ_update_freq=2)
        eng.rb_fill_synthetic(500)
        with pytest.raises(P.EngineError):
            eng.step_period()
        assert eng.run_iterations(0, 7) == 7 and eng.get_adam_state(_lib.CRITICS)[2] == 7


@pytest.mark.parametrize("algo,env,B", [("sac", "hopper", 256), ("sac", "humanoid", 1024), ("sac", "halfcheetah", 64), ("td3", "halfcheetah", 256),
                                        ("td3", "humanoid", 1024), ("td3", "hopper", 64)])
def test_chained_periods_with_state_changes_in_between_equal_single_iterations(algo, env, B):
    """A SAC period graph leaves the NEXT period's opening pair (sample, gather, next-action pass, first policy pass) precomputed;
    that is only valid while nothing it depends on changes.  Interleave periods with everything a caller may do between two of them
    -- new rows in the ring (rb.extend, orchestrator.py:100-113), acting (predict), a parameter write, single iterations, an API-path
    update -- and require the result to be bit-identical to the same sequence issued as single iterations (sactd3_step)."""
    res = []
    for mode in ("period", "single"):
        ref, eng, (o, a, bound) = make_pair(algo, env, B, seed=6)
        rows = [t.numpy() for t in synth_transitions(3000, o, a, bound, seed=29)]
        eng.rb_extend(*[r[:2000] for r in rows])
        it = [0]

        def run(n):
            if mode == "period":
                it[0] = eng.run_iterations(it[0], n)
            else:
                for _ in range(n):
                    eng.step(it[0] % 3 == 0)
                    it[0] += 1
        run(6)                                                  # two periods back to back: the second starts from the precomputed pair
        eng.rb_extend(*[r[2000:2600] for r in rows])           # the ring grows: the next sample is drawn from 2600 rows
        run(3)
        acted = eng.predict(rows[0][:4], True)                  # acting in between reads the actor only
        run(3)
        eng.set_params(_lib.ACTOR, eng.get_params(_lib.ACTOR))  # a parameter write (same values)
        run(4)                                                  # a period, then a single iteration ...
        run(5)                                                  # ... two more singles, then a period
        eng.rb_sample(); eng.update_qnets(); eng.update_targ_nets(22)    # an API-path update on a fresh sample
        it[0] += 1                                              # (counts as iteration 21: not a multiple of 3)
        run(2)                                                  # singles 22, 23 (whole periods only start at multiples of 3)
        run(6)                                                  # periods 24-26, 27-29
        run(2)                                                  # 30, 31: the first two iterations of a period in one launch (step_prefix(2)) on the chained opening pair
        run(1)                                                  # 32: a single critic-only iteration
        run(1)                                                  # 33: step_prefix(1) behind a single iteration (opening graph first)
        res.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET), eng.get_params(_lib.ACTOR_TARGET),
                    eng.get_params(_lib.LOG_ALPHA), eng.read_batch()["index"], eng.read_noise(_lib.SITE_CRITIC), acted,
                    eng.get_adam_state(_lib.CRITICS)[2], eng.get_adam_state(_lib.ACTOR)[2], np.array(list(eng.read_metrics().values()))))
        if mode == "period":
            assert eng.graph_kernel_count(5) > 0                # the opening graph exists: the chained form was in use
            assert eng.graph_kernel_count(6) > 0 and eng.graph_kernel_count(7) > eng.graph_kernel_count(6)     # ... and both cut-short periods
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    assert res[0][8] == 34 and res[0][9] == 22


def test_graphs_can_be_instantiated_ahead_of_the_first_step():
    """sactd3_instantiate_graphs captures the step / period graphs without launching or changing anything: the node counts are
    there before any iteration ran, and the iterations that follow are bit-identical to those of an engine that captured lazily."""
    res = []
    for ahead in (True, False):
        ref, eng, (o, a, bound) = make_pair("sac", "hopper", 64, seed=9)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(500, o, a, bound, seed=2)])
        if ahead:
            before = (eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS))
            eng.instantiate_graphs()
            assert eng.graph_kernel_count(2) == 5 and eng.graph_kernel_count(3) == 18 and eng.graph_kernel_count(4) == 21
            assert np.array_equal(before[0], eng.get_params(_lib.ACTOR)) and np.array_equal(before[1], eng.get_params(_lib.CRITICS))
        eng.run_iterations(0, 7)
        res.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.LOG_ALPHA), eng.read_batch()["index"]))
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    # delay 1: the pipelined period with one iteration run ahead; delay 3: the period that is not pipelined.  The entry points find the
    # graphs instantiate_graphs made -- none is captured again under another id: every public id (0..8, 10, 16..19) the lazily capturing
    # twin has used holds the same node count ahead, and the iterations capture no further run graph (2 where pipelined, else 0)
    for delay, run_graphs in ((1, 2), (3, 0)):
        res, counts = [], []
        for ahead in (True, False):
            ref, eng, (o, a, bound) = make_pair("sac", "hopper", 64, seed=9, actor_update_delay=delay)
            eng.rb_extend(*[t.numpy() for t in synth_transitions(300, o, a, bound, seed=2)])
            if ahead:
                eng.instantiate_graphs()
                assert eng.step_periods_stats()["run_graphs_captured"] == run_graphs
            eng.run_iterations(0, 12)
            if ahead:
                assert eng.step_periods_stats()["run_graphs_captured"] == run_graphs
            counts.append({i: eng.graph_kernel_count(i) for i in (*range(9), 10, *range(16, 20))})
            res.append((eng.get_params(_lib.ACTOR), eng.get_params(_lib.CRITICS), eng.get_params(_lib.LOG_ALPHA), eng.read_batch()["index"]))
        used = {i: n for i, n in counts[1].items() if n}
        assert used and {i: counts[0][i] for i in used} == used, (delay, counts)
        for x, y in zip(*res):
            assert np.array_equal(x, y), delay
    # a gated target update (crit_targ_update_freq = 2): both variants of the step graphs are captured, no period graph
    res = []
    for ahead in (True, False):
        ref, eng, (o, a, bound) = make_pair("sac", "hopper", 32, seed=9, crit_targ_update_freq=2)
        eng.rb_fill_synthetic(300)
        if ahead:
            eng.instantiate_graphs()
            assert eng.graph_kernel_count(2) > 0 and eng.graph_kernel_count(3) > 0 and eng.graph_kernel_count(4) == 0
        eng.run_iterations(0, 6)
        res.append((eng.get_params(_lib.CRITICS), eng.get_params(_lib.CRITICS_TARGET), eng.get_params(_lib.ACTOR)))
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def test_native_noise_stream_matches_philox_oracle():
    ref, eng, (o, a, bound) = make_pair("sac", "hopper", 256, seed=77)
    obs, act, rew, nobs, done = synth_transitions(256, o, a, bound, seed=1)
    eng.load_batch(obs, act, rew, nobs, done)
    eng.update_qnets()
    got = eng.read_noise(_lib.SITE_CRITIC)
    # every element inside the a-priori bound of the float64 model (tests/noise_model.py: measured unit errors, nothing observed here)
    observe("test_native_noise_stream_matches_philox_oracle", "worst |err| / bound", noise_model.check("counter 0", got, 77, 0, 0))
    eng.update_qnets()   # the graph bumped the device-side counter itself: fresh draws
    got2 = eng.read_noise(_lib.SITE_CRITIC)
    observe("test_native_noise_stream_matches_philox_oracle", "worst |err| / bound", noise_model.check("counter 1", got2, 77, 1, 0))
    assert not np.allclose(got, got2)


@pytest.mark.parametrize("algo,env", [("sac", "hopper"), ("td3", "halfcheetah"), ("sac", "humanoid")])
def test_predict(algo, env):
    ref, eng, (o, a, bound) = make_pair(algo, env, 32)
    for n in (1, 4, 8):
        obs = torch.randn(n, o, generator=torch.Generator().manual_seed(n))
        close(eng.predict(obs, explore=False), ref.predict(obs, explore=False), name="exploit")
        eps = torch.randn(n, a, generator=torch.Generator().manual_seed(100 + n))
        eng.set_noise(_lib.SITE_PREDICT, eps)
        close(eng.predict(obs, explore=True), ref.predict(obs, explore=True, eps=eps), name="explore (injected)")
        eng.clear_noise(_lib.SITE_PREDICT)
        x, y = eng.predict(obs, explore=True), eng.predict(obs, explore=True)
        assert not np.array_equal(x, y) and np.isfinite(x).all()
    with pytest.raises(P.EngineError):
        eng.predict(torch.zeros(9, o), explore=False)


@pytest.mark.parametrize("use_graphs", [True, False])
def test_predict_returns_only_finished_actions(use_graphs):
    """sactd3_predict waits for its kernels through a pinned host word the acting tail publishes after its last store (no
    stream synchronisation for single-block tails).  Alternate two observation sets, with updates and replay writes keeping
    the stream busy in between: every call must return ITS observations' actions -- a premature return would hand back the
    previous call's (the staging buffer still holds them).  agents/agent.py:172-181."""
    o, a, bound = DIMS["hopper"]
    hps = Hps.sac(batch_size=64)
    torch.manual_seed(0)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, hps)
    eng = track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=4096, seed=3, use_graphs=use_graphs), [-bound] * a, [bound] * a))
    push_params(eng, ref)
    eng.rb_fill_synthetic(1000)
    g = torch.Generator().manual_seed(5)
    obs = [torch.randn(4, o, generator=g).numpy(), torch.randn(4, o, generator=g).numpy(), torch.randn(1, o, generator=g).numpy()]
    want = [eng.predict(x, False).copy() for x in obs]
    eng.sync()
    assert not np.allclose(want[0], want[1])
    rows = [np.zeros((4, o), np.float32), np.zeros((4, a), np.float32), np.zeros(4, np.float32), np.zeros((4, o), np.float32), np.zeros(4, bool)]
    for i in range(6000):
        k = i % 3
        got = eng.predict(obs[k], False)
        assert np.array_equal(got, want[k]), (i, k)
    # with the learner running: the parameters move, so compare the two calls of a pair issued back to back on the same observations
    for i in range(600):
        eng.rb_extend(*rows)
        eng.step(i % 3 == 0)
        x = eng.predict(obs[i % 2], False)
        y = eng.predict(obs[i % 2], False)
        assert np.array_equal(x, y) and np.isfinite(x).all(), i
        z = eng.predict(obs[1 - i % 2], False)
        assert not np.array_equal(x, z), i


def test_predict_many_envs_is_reproducible():
    """predict for more rows than one 16-row block (a large vector env): exploitation matches the oracle and the native
    exploration stream is a function of (seed, call number, row) only -- two engines with the same seed agree call by
    call, whichever block of the kernel a row lands in."""
    o, a, bound = DIMS["hopper"]
    hps = Hps.sac(batch_size=32)
    torch.manual_seed(0)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, hps)
    engs = [track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=256, max_envs=48, seed=7), [-bound] * a, [bound] * a)) for _ in range(2)]
    for e in engs:
        push_params(e, ref)
    obs = torch.randn(40, o, generator=torch.Generator().manual_seed(3))
    close(engs[0].predict(obs, explore=False), ref.predict(obs, explore=False), name="exploit, 40 rows")
    seq = [[e.predict(obs, explore=True) for _ in range(3)] for e in engs]
    for x, y in zip(*seq):
        assert np.array_equal(x, y)
    assert not np.array_equal(seq[0][0], seq[0][1]) and not np.array_equal(seq[0][1], seq[0][2])
    eps = torch.randn(40, a, generator=torch.Generator().manual_seed(4))
    engs[0].set_noise(_lib.SITE_PREDICT, eps)
    close(engs[0].predict(obs, explore=True), ref.predict(obs, explore=True, eps=eps), name="explore (injected), 40 rows")


def test_agent_mirror_drives_like_the_reference():
    """The Python `Agent`/`ReplayBuffer` mirror, used the way orchestrator.py:317-352 uses the reference's."""
    from types import SimpleNamespace
    o, a, bound = DIMS["hopper"]
    hps = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "cudagraphs": True, "rb_capacity": 1000, "seed": 0})
    rb = P.ReplayBuffer(hps.rb_capacity)
    torch.manual_seed(0)
    agent = P.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32),
                    torch.device("cuda:0"), hps, rb)
    torch.manual_seed(0)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, Hps.sac(batch_size=64))
    assert np.array_equal(agent.engine.get_params(_lib.ACTOR), flat_actor(ref, ref.actor))  # same init as the reference
    obs, act, rew, nobs, done = synth_transitions(400, o, a, bound, seed=2)
    for t in range(0, 400, 4):
        sl = slice(t, t + 4)
        agent.rb.extend({"observations": obs[sl], "next_observations": nobs[sl], "actions": act[sl],
                         "rewards": rew[sl].reshape(-1, 1), "terminations": done[sl].reshape(-1, 1), "dones": done[sl].reshape(-1, 1)})
    assert len(agent.rb) == 400
    tlog = {}
    for i in range(6):
        ac = agent.predict({"observations": obs[:4]}, explore=True)
        assert ac.shape == (4, a) and ac.dtype == np.float32
        batch = agent.rb.sample(hps.batch_size)
        tlog.update(agent.update_qnets(batch)); agent.qnet_updates_so_far += 1
        if i % (hps.actor_update_delay + 1) == 0:
            for _ in range(hps.actor_update_delay):
                tlog.update(agent.update_actor(batch)); agent.actor_updates_so_far += 1
        agent.update_targ_nets()
    vals = {k: float(v) for k, v in tlog.items()}
    assert set(vals) == {"loss/qf_loss", "loss/actor_loss", "loss/alpha_loss", "vitals/alpha"}
    assert all(np.isfinite(v) for v in vals.values())
    assert batch["observations"].shape == (64, o) and batch["dones"].shape == (64, 1)


def test_engine_graphs_do_not_follow_the_reference_loops_cudagraphs_key():
    """INTEGRATION.md runs the reference loop with `cudagraphs: false` (so that orchestrator.py:313-315 does not wrap the
    ctypes-backed methods in CudaGraphModule); the engine's own hipGraphs stay on, and can be switched off explicitly."""
    from types import SimpleNamespace
    o, a, bound = DIMS["hopper"]
    mk = lambda **kw: P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device("cuda:0"),
                              SimpleNamespace(**{**Hps.sac(batch_size=32).__dict__, "cudagraphs": False, "rb_capacity": 256, "seed": 0}),
                              P.ReplayBuffer(256), **kw)
    for kw, want in ((dict(), True), (dict(use_graphs=True), True), (dict(use_graphs=False), False)):
        ag = mk(**kw)
        ag.engine.rb_fill_synthetic(200)
        ag.iteration(0)
        ag.update_qnets(ag.rb.sample(32))
        ag.engine.sync()
        assert (ag.engine.graph_kernel_count(0) > 0) == want and (ag.engine.graph_kernel_count(3) > 0) == want


def test_calls_run_on_the_engines_device_whatever_the_current_device_is():
    """every ABI entry point selects the engine's device itself (a caller thread that changed its current device, or a
    fresh thread, must not break a call): drive an engine from a second Python thread."""
    import threading
    ref, eng, (o, a, bound) = make_pair("sac", "hopper", 32)
    eng.rb_fill_synthetic(500)
    res = {}

    def work():
        try:
            for i in range(4):
                eng.step(i % 3 == 0)
            res["m"] = eng.read_metrics()
            res["act"] = eng.predict(np.zeros((2, o), np.float32), explore=False)
        except Exception as ex:            # noqa: BLE001
            res["err"] = ex
    th = threading.Thread(target=work)
    th.start(); th.join()
    assert "err" not in res, res.get("err")
    assert all(np.isfinite(v) for v in res["m"].values()) and res["act"].shape == (2, a)


def test_time_nodes_lists_the_iteration_graphs():
    """sactd3_time_nodes walks the same enqueue sequence the graphs are captured from: node counts agree with the
    instantiated graphs (5 / 18 at Hopper shapes: two launches open the iteration -- sample, gather, next-action pass and the
    first actor update's policy pass --, three make the critic update, four an actor update, two each temperature draw, one the
    last temperature step) and every node has a kernel-instance name, a grid and a time."""
    ref, eng, (o, a, bound) = make_pair("sac", "hopper", 256)
    eng.rb_fill_synthetic(2000)
    for i in range(3):
        eng.step(i % 3 == 0)
    eng.sync()
    n0, n1 = eng.graph_kernel_count(2), eng.graph_kernel_count(3)
    g0, g1 = eng.time_nodes(False, 5), eng.time_nodes(True, 5)
    assert (len(g0), len(g1)) == (n0, n1) == (5, 18)
    for n in g0 + g1:
        assert n["name"].startswith("k_") and ":" in n["name"] and n["threads"] > 0 and 0.0 < n["us"] < 1e4
    assert sum(n["flops"] for n in g0) > 0.3e9      # (critic update of SURVEY 8d: A + 8C per sample at B = 256)
    eng.step(False)                                 # the engine still runs afterwards
    assert all(np.isfinite(v) for v in eng.read_metrics().values())


def test_update_results_are_zero_dim_device_tensors():
    """agents/agent.py:238-242,305-311 return 0-dim DEVICE tensors that orchestrator.py:341,348 put into `tlog` and :383 reads
    at evaluation time.  The mirror returns 0-dim float32 CUDA tensors that alias the engine's metrics slots (no copy, no host
    sync when returned); read later they hold the latest values; `metrics="lazy"` keeps the torch-free handles."""
    from types import SimpleNamespace
    o, a, bound = DIMS["hopper"]
    mk = lambda **kw: P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device("cuda:0"),
                              SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "rb_capacity": 512, "seed": 0}), P.ReplayBuffer(512), **kw)
    ag = mk()
    ag.engine.rb_fill_synthetic(400)
    tlog = {}
    for i in range(3):
        batch = ag.rb.sample(64)
        tlog.update(ag.update_qnets(batch))
        tlog.update(ag.update_actor(batch))
        ag.qnet_updates_so_far += 1
        ag.update_targ_nets()
    assert set(tlog) == {"loss/qf_loss", "loss/actor_loss", "loss/alpha_loss", "vitals/alpha"}
    for k, v in tlog.items():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and v.dtype == torch.float32, k
    got = {k: v.item() for k, v in tlog.items()}                     # what tlog.to_dict() materialises at eval time
    assert got == ag.engine.read_metrics()
    stacked = torch.stack(list(tlog.values()))                       # usable as ordinary tensors (e.g. by a TensorDict)
    assert stacked.shape == (4,) and torch.isfinite(stacked).all()
    lazy = mk(metrics="lazy")
    lazy.engine.rb_fill_synthetic(400)
    r = lazy.update_qnets(lazy.rb.sample(64))
    assert isinstance(r["loss/qf_loss"], P.agent.LazyMetric) and np.isfinite(float(r["loss/qf_loss"]))


# ------------------------------------------------------------------------------------------ config corners

# one iteration = a critic step and TWO actor steps on top of each other: north_star's 1e-5 (observed <= 2.7e-6 over all corners and odd shapes)
CORNER_TOL = 1e-5


@pytest.mark.parametrize("algo,env,B,hp", [
    ("sac", "hopper", 256, dict(autotune=False)),                       # fixed temperature (agents/agent.py:313-318)
    ("sac", "hopper", 256, dict(bcq_style_targ_mix=True)),              # soft-min target mix with SAC
    ("td3", "halfcheetah", 256, dict(targ_actor_smoothing=False)),      # agents/agent.py:201-202
    ("td3", "halfcheetah", 256, dict(bcq_style_targ_mix=False)),        # hard min (TD3 paper)
    ("sac", "humanoid", 1024, dict()),                                  # BASELINE config 4 shape (wide first layer, B=1024)
    ("td3", "humanoid", 1024, dict()),                                  # the same launches with the target actor in the opening group
    ("sac", "humanoid", 1024, dict(ln=False)),                          # k_nt64_ln's ReLU-only prologue
    ("sac", "hopper", 4096, dict()),                                    # largest batch of the scope (batch <= 4096)
    ("sac", "hopper", 1, dict()),                                       # degenerate batch
    # the same four options in the large-batch kernel forms (k_critic_tail<16>, k_actor_tail(2), k_tn64 + k_adam_red)
    ("sac", "hopper", 1024, dict(autotune=False)),
    ("sac", "hopper", 1024, dict(bcq_style_targ_mix=True)),
    ("td3", "halfcheetah", 1024, dict(targ_actor_smoothing=False)),
    ("td3", "halfcheetah", 1024, dict(bcq_style_targ_mix=False)),
])
def test_one_iteration_config_corners(algo, env, B, hp):
    """one whole iteration (critic update, two actor updates on top of each other, Polyak) from the oracle's state, call by call"""
    ref, eng, (o, a, bound) = make_pair(algo, env, B, **hp)
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=31)
    g = torch.Generator().manual_seed(32)
    noise = {"critic": torch.randn(B, a, generator=g), "actor": [torch.randn(B, a, generator=g) for _ in range(2)],
             "alpha": [torch.randn(B, a, generator=g) for _ in range(2)]}
    want = {k: float(v) for k, v in ref.iteration(ref.to_batch(obs, act, rew, nobs, done), 0, noise).items()}
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_CRITIC, noise["critic"])
    eng.update_qnets()
    for j in range(2):
        eng.set_noise(_lib.SITE_ACTOR0, noise["actor"][j]); eng.set_noise(_lib.SITE_ALPHA0, noise["alpha"][j])
        eng.update_actor()
    eng.update_targ_nets(1)
    got = eng.read_metrics()
    rec = f"one_iteration_config_corners[{algo}-{env}-{B}-{sorted(hp.items())}]"
    scalars_close(rec, 0, got, want, CORNER_TOL)
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, 1, "critics", layout=crit_layout(ref), record=rec)
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, 2, "actor", max_bad_frac=1e-3,
                        layout=actor_layout(ref), vec_bad=1, record=rec)
    close(eng.get_params(_lib.CRITICS_TARGET), flat_critics(ref, ref.qnets_target), rtol=1e-5, atol=1e-5, name="targets")
    if algo == "td3":
        close(eng.get_params(_lib.ACTOR_TARGET), flat_actor(ref, ref.actor_target), rtol=1e-5, atol=1e-5, name="actor target")


def test_actor_update_delay_other_than_two():
    """actor_update_delay = 1 and 3 through the fused step: counters / schedule of orchestrator.py:345-349."""
    for delay in (1, 3):
        ref, eng, (o, a, bound) = make_pair("sac", "hopper", 64, actor_update_delay=delay)
        obs, act, rew, nobs, done = [t.numpy() for t in synth_transitions(300, o, a, bound, seed=41)]
        eng.rb_extend(obs, act, rew, nobs, done)
        for i in range(2 * (delay + 1)):
            eng.step(i % (delay + 1) == 0)
        _, _, ta = eng.get_adam_state(_lib.ACTOR)
        _, _, tq = eng.get_adam_state(_lib.CRITICS)
        assert tq == 2 * (delay + 1) and ta == 2 * delay
        assert all(np.isfinite(v) for v in eng.read_metrics().values())


@pytest.mark.parametrize("algo,o,a,B", [("sac", 64, 1, 48), ("sac", 65, 16, 33), ("sac", 3, 32, 64), ("td3", 48, 17, 80),
                                         ("sac", 20, 5, 16), ("td3", 1, 1, 17)])
def test_one_iteration_odd_dimensions(algo, o, a, B):
    """Edges of the kernels' shape handling: fused first layer up to 64 inputs (1, 2 or 4 k-chunks) vs the wide path
    from 65, head widths up to 64 outputs (4 MFMA column tiles), batch sizes that are not multiples of 16."""
    bound = 0.7
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(batch_size=B)
    torch.manual_seed(1)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, hps)
    randomize_ln(ref)
    eng = track(P.Engine(P.Config.from_hps(hps, o, a, rb_capacity=512, max_envs=4, seed=1), [-bound] * a, [bound] * a))
    push_params(eng, ref)
    obs, act, rew, nobs, done = synth_transitions(B, o, a, bound, seed=51)
    g = torch.Generator().manual_seed(52)
    noise = {"critic": torch.randn(B, a, generator=g), "actor": [torch.randn(B, a, generator=g) for _ in range(2)],
             "alpha": [torch.randn(B, a, generator=g) for _ in range(2)]}
    want = {k: float(v) for k, v in ref.iteration(ref.to_batch(obs, act, rew, nobs, done), 0, noise).items()}
    eng.load_batch(obs, act, rew, nobs, done)
    eng.set_noise(_lib.SITE_CRITIC, noise["critic"])
    eng.update_qnets()
    for j in range(2):
        eng.set_noise(_lib.SITE_ACTOR0, noise["actor"][j]); eng.set_noise(_lib.SITE_ALPHA0, noise["alpha"][j])
        eng.update_actor()
    eng.update_targ_nets(1)
    got = eng.read_metrics()
    rec = f"one_iteration_odd_dimensions[{algo}-{o}-{a}-{B}]"
    scalars_close(rec, 0, got, want, CORNER_TOL)
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, 1, "critics", max_bad_frac=1e-3,
                        layout=crit_layout(ref), vec_bad=1, record=rec)
    assert_params_close(eng.get_params(_lib.ACTOR), flat_actor(ref, ref.actor), ref.hps.actor_lr, 2, "actor", max_bad_frac=1e-3,
                        layout=actor_layout(ref), vec_bad=1, record=rec)
    x = torch.randn(3, o, generator=g)
    close(eng.predict(x, explore=False), ref.predict(x, explore=False), name="predict")
    # and the fused iteration runs on these shapes too
    o_, a_, r_, n_, d_ = [t.numpy() for t in synth_transitions(300, o, a, bound, seed=53)]
    eng.rb_extend(o_, a_, r_, n_, d_)
    for i in range(4):
        eng.step(i % 3 == 0)
    assert all(np.isfinite(v) for v in eng.read_metrics().values())


def test_error_paths_return_codes_not_crashes():
    """The C ABI reports bad calls through error codes / messages (include/sactd3.h conventions)."""
    import ctypes as C
    lib = P.load_library()
    cc = P.Config(ob_dim=11, ac_dim=3, batch_size=32, rb_capacity=128).to_c()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    h = C.c_void_p()
    for field, bad in (("abi_version", 99), ("ob_dim", 0), ("ac_dim", 33), ("batch_size", 0), ("device_id", 64), ("crit_targ_update_freq", 0)):
        c2 = P.Config(ob_dim=11, ac_dim=3, batch_size=32, rb_capacity=128).to_c()
        setattr(c2, field, bad)
        assert lib.sactd3_create(C.byref(c2), lo, hi, C.byref(h)) < 0 and not h.value, field
        assert lib.sactd3_last_error(None)
    assert lib.sactd3_create(C.byref(cc), None, hi, C.byref(h)) < 0
    eng = track(P.Engine(P.Config(ob_dim=11, ac_dim=3, batch_size=32, rb_capacity=128), [-1] * 3, [1] * 3))
    with pytest.raises(ValueError):
        eng.set_params(_lib.ACTOR, np.zeros(5, np.float32))                 # wrong length caught before the call
    assert lib.sactd3_get_params(eng._h, 17, (C.c_float * 4)()) < 0          # unknown parameter set
    with pytest.raises(P.EngineError):
        eng.load_batch(np.zeros((8, 11)), np.zeros((8, 3)), np.zeros(8), np.zeros((8, 11)), np.zeros(8))   # n != batch_size
    with pytest.raises(P.EngineError):
        eng.set_noise(_lib.SITE_CRITIC, np.zeros((64, 3), np.float32))        # more rows than a batch
    with pytest.raises(P.EngineError):
        eng.debug_read("no_such_buffer")
    with pytest.raises(P.EngineError):
        eng.rb_fill_synthetic(129)                                           # beyond capacity
    assert lib.sactd3_graph_kernel_count(eng._h, 9) < 0 and lib.sactd3_sync(None) < 0
    assert lib.sactd3_step_prefix(eng._h, 0) < 0 and lib.sactd3_step_prefix(eng._h, 3) < 0 and lib.sactd3_step_prefix(None, 1) < 0   # 1 <= m <= delay
    # the engine is still usable afterwards
    eng.rb_fill_synthetic(100)
    eng.step(True)
    assert all(np.isfinite(v) for v in eng.read_metrics().values())
