"""GPU: training on caller-chosen ring rows with loss weights, and the TD errors back (sactd3_rb_sample_indices_device,
sactd3_batch_weights_device, sactd3_td_errors_device, the weighted form of sactd3_update_qnets; include/sactd3.h).  Against the oracle
at the tolerances the suite applies to the unweighted critic update; everything else is an equality of bits against a twin engine.

Engines are shape_engines() of tests/gpu_support.py (the oracle's perturbed parameters), with a 2048-row ring of
synth_transitions (every 5th row done) and the critic site's noise injected.  Shapes: SAC Hopper at B = 64; at B = 40 (ends in a
partial 16-row tile: the clamped rows meet the weight); TD3 HalfCheetah at B = 64; SAC Hopper without LayerNorm at B = 64; SAC Hopper at
B = 1024 (k_critic_tail_w<16> instead of k_ctail_nn_w<2>)."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests.gpu_support import (DEV, SENTINEL, SHAPES, P, _lib, assert_same_bits, assert_same_state, close, close_engines, crit_layout, cuda,  # noqa: F401
                               flat_critics, gclose, load_device, loop, same_bits, schema, shape_engines, slot, stage, stream, td_of, track)
from tests.helpers import assert_params_close, observe, synth_transitions

pytestmark = pytest.mark.gpu

RING = 2048
# name -> (shape of gpu_support.SHAPES, batch size)
CASES = {"sac-hopper-64": ("sac-hopper", 64), "sac-hopper-40": ("sac-hopper", 40), "td3-halfcheetah-64": ("td3-halfcheetah", 64),
         "sac-hopper-noln-64": ("sac-hopper-noln", 64), "sac-hopper-1024": ("sac-hopper", 1024)}
ALL = list(CASES)


@functools.lru_cache(maxsize=None)
def ring_rows(shape):
    """the 2048 transitions every engine's ring holds: computed once per shape, never written"""
    _, (o, a, bound), _ = SHAPES[shape]
    obs, act, rew, nobs, done = synth_transitions(RING, o, a, bound, seed=9)
    done = done.clone()
    done[::5] = True
    return obs, act, rew, nobs, done


def build(case, count):
    """the oracle and `count` twin engines: same parameters, same ring, same injected critic noise"""
    shape, B = CASES[case]
    ref, engs, (o, a, bound) = shape_engines(shape, count, B=B, cap=RING)
    eps = torch.randn(B, a, generator=torch.Generator().manual_seed(4))
    for eng in engs:
        eng.rb_extend(*[t.numpy() for t in ring_rows(shape)])
        eng.set_noise(_lib.SITE_CRITIC, eps)
    return ref, engs, (o, a, bound), B, eps


def indices(B, seed=0):
    """ring slots with the ring's first and last rows (at both ends of the batch) and repeats"""
    idx = np.random.default_rng(seed).integers(0, RING, B)
    idx[0], idx[1], idx[2], idx[-1] = 0, RING - 1, idx[3], RING - 1
    return idx.astype(np.int64)


def weights_u02(B, seed=1):
    """U(0, 2) with exact zeros, rows 0 and B - 1 among them"""
    w = torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 2.0
    w[::7] = 0.0
    w[B - 1] = 0.0
    return w


def attach(eng, w):
    w = w.to(DEV) if not w.is_cuda else w
    eng.batch_weights_device(w.data_ptr(), max(w.stride(0), 1), w.shape[0], stream())
    return w


def critic_update_state(eng):
    """what a critic update leaves: gradients, the tail's stores, the loss, parameters, Adam state"""
    m, v, t = eng.get_adam_state(_lib.CRITICS)
    return dict(grad=eng.debug_read("grad_critics"), dz2=eng.debug_read("c_dz2"), q=eng.debug_read("q"), y=eng.debug_read("targ_q"),
                loss=np.float32(eng.read_metrics()["loss/qf_loss"]), params=eng.get_params(_lib.CRITICS), m=m, v=v, t=np.float32(t))


# ------------------------------------------------------------------------------------------ 1. staging equals the host route
@pytest.mark.parametrize("case", ALL)
def test_index_staging_leaves_what_the_host_route_leaves(case):
    """sactd3_rb_sample_indices_device against sactd3_rb_sample_with_indices on a twin: X, Xn, rew, done and the slot's indices, bit
    for bit -- contiguous indices, then (over the first batch) a strided view with strided weights; repeated slots, the ring's first
    and last rows.  No tick of the sample counter: both engines then draw the same native sample."""
    _, (D, H), _, B, _ = build(case, 2)
    idx = indices(B)
    stage(D, idx)
    H.rb_sample_with_indices(idx)
    assert_same_bits(slot(D), slot(H), what="contiguous")
    assert np.array_equal(slot(D)["index"], idx)
    idx2 = indices(B, seed=5)[::-1].copy()
    wide = torch.full((B, 3), 7, dtype=torch.int64, device=DEV)
    wide[:, 1] = torch.as_tensor(idx2, device=DEV)
    wwide = torch.full((B, 5), 3.0, device=DEV)
    keep = stage(D, wide[:, 1], wwide[:, 2])
    H.rb_sample_with_indices(idx2)
    assert_same_bits(slot(D), slot(H), what="strided")
    assert D.priority_stats() == dict(index_stagings=2, weight_stagings=0, td_readouts=0, rows_refused=0)
    D.rb_sample()
    H.rb_sample()
    assert_same_bits(slot(D), slot(H), what="native sample behind the stagings")
    del keep


# ------------------------------------------------------------------------------------------ 2. weights of 1 change nothing
@pytest.mark.parametrize("case", ALL)
def test_unit_weights_equal_the_plain_update(case):
    """staging + the weighted update_qnets against rb_sample_with_indices + the plain one: gradients, dz2, q, the Bellman target, the
    loss, the critics and their Adam state, bit for bit -- with explicit ones, then (a second step) with w == NULL"""
    _, (D, H), _, B, _ = build(case, 2)
    for step, w in enumerate((torch.ones(B), None)):
        idx = indices(B, seed=step)
        keep = stage(D, idx, w)
        H.rb_sample_with_indices(idx)
        D.update_qnets()
        H.update_qnets()
        assert_same_bits(critic_update_state(D), critic_update_state(H), what=f"step {step}")
        del keep
    assert D.graph_kernel_count(8) == H.graph_kernel_count(0) > 0 and H.graph_kernel_count(8) == 0 and D.graph_kernel_count(0) == 0
    assert_same_state(D, H)


# ------------------------------------------------------------------------------------------ 3. powers of two scale exactly
@pytest.mark.parametrize("case", ALL)
def test_power_of_two_weights_scale_gradients_and_loss_exactly(case):
    """w == 2 and w == 0.5 against w == 1: every gradient and the loss are the unit-weight values times the weight as float32 bit
    patterns (a power of two commutes with every rounding of the sums); q and the Bellman target do not move"""
    _, engs, _, B, _ = build(case, 3)
    idx = indices(B)
    got = []
    for eng, scale in zip(engs, (1.0, 2.0, 0.5)):
        keep = stage(eng, idx, torch.full((B,), scale))
        eng.update_qnets()
        got.append(critic_update_state(eng))
        del keep
    one = got[0]
    assert np.abs(one["grad"]).max() > 0 and one["loss"] > 0
    for g, scale in zip(got[1:], (2.0, 0.5)):
        s = np.float32(scale)
        assert same_bits(g["grad"], one["grad"] * s), scale
        assert same_bits(g["dz2"], one["dz2"] * s), scale
        assert same_bits(np.asarray(g["loss"]), np.asarray(one["loss"] * s)), (scale, g["loss"], one["loss"])
        assert_same_bits(g, one, ("q", "y"), what=scale)


# ------------------------------------------------------------------------------------------ 4. a row of weight 0 is invisible
@pytest.mark.parametrize("case", ALL)
def test_a_row_of_weight_zero_is_invisible(case):
    """two engines hold the same caller-owned device batch but for the rewards and done flags of the weight-0 rows (rows 0 and B - 1
    among them), weights attached with sactd3_batch_weights_device: gradients, loss, parameters and Adam state have equal bits"""
    shape, _ = CASES[case]
    _, (D, T), _, B, _ = build(case, 2)
    rows = [t[indices(B)] for t in ring_rows(shape)]
    w = weights_u02(B)
    zero = w == 0
    assert zero[0] and zero[B - 1] and 2 < int(zero.sum()) < B // 2
    other = [t.clone() for t in rows]
    other[2][zero] = other[2][zero] * -3.0 + 1000.0
    other[4][zero] = ~other[4][zero]
    for eng, five in ((D, rows), (T, other)):
        load_device(eng, cuda(five))
        keep = attach(eng, w)
        eng.update_qnets()
        del keep
    x, y = critic_update_state(D), critic_update_state(T)
    assert_same_bits(x, y, ("grad", "loss", "params", "m", "v", "t"))
    assert not same_bits(x["y"], y["y"])                                      # the rows did differ
    assert D.priority_stats()["weight_stagings"] == 1


# ------------------------------------------------------------------------------------------ 5. against the oracle
def oracle_weighted_update(ref, b, eps, w):
    """RefAgent.update_qnets (oracle/sac_td3_ref.py) with loss = sum_k (w (q_k - y)^2).mean(): y computed as it computes it, on its
    own nets and optimiser -> (loss, per-net gradient dictionaries)"""
    h = ref.hps
    ref.q_optimizer.zero_grad()
    with torch.no_grad():
        if h.prefer_td3_over_sac:
            pi_next = ref.actor_target(b.next_observations)
            if h.targ_actor_smoothing:
                n_ = (eps * h.td3_std).clamp(-h.td3_c, h.td3_c)
                a_next = torch.max(torch.min(pi_next + n_, ref.max_ac), ref.min_ac)
            else:
                a_next = pi_next
            logp_next = None
        else:
            a_next, logp_next, _ = ref.actor.get_action(b.next_observations, eps).values()
        q_t = ref._twin(ref.qnets_target, b.next_observations, a_next)
        q_min = q_t.min(0).values
        q_prime = 0.75 * q_min + 0.25 * q_t.max(0).values if h.bcq_style_targ_mix else q_min
        if not h.prefer_td3_over_sac:
            q_prime = q_prime - ref.alpha * logp_next
        targ_q = b.rewards.flatten() + (1.0 - b.dones.flatten().float()) * h.gamma * q_prime.view(-1)
    q = ref._twin(ref.qnets, b.observations, b.actions)
    loss = sum((w * (q[i].view(-1) - targ_q) ** 2).mean() for i in range(2))
    loss.backward()
    grads = [{k: p.grad.clone() for k, p in net.named_parameters()} for net in ref.qnets]
    ref.q_optimizer.step()
    return loss.detach(), grads, q.detach().squeeze(-1), targ_q


@pytest.mark.parametrize("case", ALL)
def test_weighted_update_against_the_oracle(case):
    """weights ~ U(0, 2) with exact zeros: gradients per state_dict key (gclose), the loss (close) and the critics after Adam
    (assert_params_close) at the tolerances check_update_qnets_intermediates applies to the unweighted update at these shapes -- the
    weight scales every gradient term linearly, so the relative error is that of the unweighted update."""
    shape, _ = CASES[case]
    ref, (eng,), (o, a, bound), B, eps = build(case, 1)
    ln = ref.hps.layer_norm
    idx, w = indices(B), weights_u02(B)
    obs, act, rew, nobs, done = [t[idx] for t in ring_rows(shape)]
    keep = stage(eng, idx, w)
    eng.update_qnets()
    loss, grads, q, targ_q = oracle_weighted_update(ref, ref.to_batch(obs, act, rew, nobs, done), eps, w)
    close(eng.debug_read("q").reshape(2, B), q, name="online Q")
    got_g = eng.debug_read("grad_critics").reshape(2, -1)
    for i in range(2):
        gd = schema.flat_to_dict(got_g[i], o + a, 1, ln)
        for k, _ in schema.net_keys(o + a, 1, ln):
            want = grads[i][k].numpy()
            ratio = float(np.abs(gd[k].reshape(want.shape) - want).max() / (2e-6 + 1e-5 * np.abs(want).max() + 2e-4 * np.abs(want).max()))
            observe(f"weighted_update_against_oracle[{case}]", f"critic{i} grad {k}: max |dg| / gclose bound at max |g|", ratio)
            gclose(gd[k], want, name=f"critic{i} grad {k}")
    got_loss = eng.read_metrics()["loss/qf_loss"]
    observe(f"weighted_update_against_oracle[{case}]", "|dloss| / (1e-5 + 1e-5 |loss|)", abs(got_loss - float(loss)) / (1e-5 + 1e-5 * abs(float(loss))))
    print(case, "loss", got_loss, float(loss))
    close(got_loss, loss, name="qf_loss")
    assert_params_close(eng.get_params(_lib.CRITICS), flat_critics(ref, ref.qnets), ref.hps.qnets_lr, 1, "critics after Adam",
                        layout=crit_layout(ref), record=f"weighted_update_against_oracle[{case}]")
    del keep


# ------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("case", ALL)
def test_bad_indices_and_bad_weights_are_neutralised_and_counted(case):
    """indices -1, len(rb) and 2^40 among valid ones: zero records with slot index -1 and weight 0, counted; the update's bits equal
    a twin's whose batch has valid rows there at weight 0.  Then weights NaN, -1 and inf (through both staging calls): staged as 0
    and counted.  Every bad value is one the kernels are specified to neutralise; the engine stays usable."""
    _, (D, T), _, B, _ = build(case, 2)
    good, w = indices(B, seed=2), weights_u02(B, seed=3) + 0.25
    bad_rows = [0, 5, B - 1]
    bad = good.copy()
    bad[bad_rows] = (-1, RING, 2 ** 40)
    w_twin = w.clone()
    w_twin[bad_rows] = 0.0
    keep = stage(D, bad, w), stage(T, good, w_twin)
    s = slot(D)
    assert (s["index"][bad_rows] == -1).all() and np.array_equal(np.delete(s["index"], bad_rows), np.delete(good, bad_rows))
    ldc = s["X"].size // B
    for k, width in (("X", ldc), ("Xn", ldc), ("rew", 1), ("done", 1)):
        assert not s[k].reshape(B, width)[bad_rows].any(), k
        assert same_bits(np.delete(s[k].reshape(B, width), bad_rows, 0), np.delete(slot(T)[k].reshape(B, width), bad_rows, 0)), k
    assert D.priority_stats()["rows_refused"] == 3 and T.priority_stats()["rows_refused"] == 0
    D.update_qnets()
    T.update_qnets()
    x, y = critic_update_state(D), critic_update_state(T)
    assert np.isfinite(x["grad"]).all() and np.isfinite(x["params"]).all() and np.isfinite(x["loss"])
    assert_same_bits(x, y, ("grad", "loss", "params", "m", "v", "t"), what="bad indices")
    # bad weights, first with the rows, then attached to the slot as it is
    w_bad = w.clone()
    w_bad[[1, 2, 3]] = torch.tensor([float("nan"), -1.0, float("inf")])
    w_twin = w.clone()
    w_twin[[1, 2, 3]] = 0.0
    for via in ("rows", "slot"):
        if via == "rows":
            keep = stage(D, good, w_bad), stage(T, good, w_twin)
        else:
            keep = attach(D, w_bad), attach(T, w_twin)
        D.update_qnets()
        T.update_qnets()
        x, y = critic_update_state(D), critic_update_state(T)
        assert np.isfinite(x["grad"]).all() and np.isfinite(x["params"]).all() and np.isfinite(x["loss"]), via
        assert_same_bits(x, y, ("grad", "loss", "params", "m", "v", "t"), what=via)
    assert D.priority_stats() == dict(index_stagings=2, weight_stagings=1, td_readouts=0, rows_refused=9)
    assert T.priority_stats()["rows_refused"] == 0
    # a row with a bad index AND a bad weight counts once; a refused row stays at weight 0 when weights are attached later
    both = good.copy()
    both[1] = -7
    keep = stage(D, both, w_bad)
    assert D.priority_stats()["rows_refused"] == 12
    w_twin = w.clone()
    w_twin[1] = 0.0
    keep = keep, attach(D, w), stage(T, good, w_twin)
    D.update_qnets()
    T.update_qnets()
    assert_same_bits(critic_update_state(D), critic_update_state(T), ("grad", "loss", "params"), what="refused row, weights attached later")
    # the engine stays usable
    D.rb_sample()
    D.update_qnets()
    assert np.isfinite(D.read_metrics()["loss/qf_loss"])
    del keep


def test_bad_arguments_are_refused_and_leave_the_engine_usable():
    _, (D,), _, B, _ = build("sac-hopper-64", 1)
    idx, w, td = torch.as_tensor(indices(B), device=DEV), torch.ones(B, device=DEV), torch.empty(2, B, device=DEV)
    host = np.zeros(4 * B, np.float32)
    lib, h = D.lib, D._h
    vp = lambda t: C.c_void_p(t.data_ptr())
    E = _lib.EINVAL
    assert lib.sactd3_rb_sample_indices_device(h, vp(idx), 1, vp(w), 1, B - 1, None, 1) == E          # n != batch_size
    assert lib.sactd3_rb_sample_indices_device(h, vp(idx), 0, vp(w), 1, B, None, 1) == E              # strides below 1
    assert lib.sactd3_rb_sample_indices_device(h, vp(idx), 1, vp(w), 0, B, None, 1) == E
    assert lib.sactd3_rb_sample_indices_device(h, vp(idx), 1, vp(w), 1, B, None, 2) == E              # an unknown flag
    assert lib.sactd3_rb_sample_indices_device(h, None, 1, vp(w), 1, B, None, 1) == E
    assert lib.sactd3_rb_sample_indices_device(h, C.c_void_p(host.ctypes.data), 1, vp(w), 1, B, None, 1) == E      # host memory
    assert lib.sactd3_rb_sample_indices_device(h, vp(idx), 1, C.c_void_p(host.ctypes.data), 1, B, None, 1) == E
    assert lib.sactd3_batch_weights_device(h, vp(w), 1, B + 1, None, 1) == E
    assert lib.sactd3_batch_weights_device(h, vp(w), 0, B, None, 1) == E
    assert lib.sactd3_batch_weights_device(h, vp(w), 1, B, None, 4) == E
    assert lib.sactd3_batch_weights_device(h, C.c_void_p(host.ctypes.data), 1, B, None, 1) == E
    assert lib.sactd3_td_errors_device(h, None, 1, B, None, 1) == E
    assert lib.sactd3_td_errors_device(h, vp(td), 0, B, None, 1) == E
    assert lib.sactd3_td_errors_device(h, vp(td), 1, 0, None, 1) == E
    assert lib.sactd3_td_errors_device(h, vp(td), 1, B, None, 2) == E
    assert lib.sactd3_td_errors_device(h, C.c_void_p(host.ctypes.data), 1, B, None, 1) == E
    assert lib.sactd3_priority_stats(h, None) == E
    assert D.priority_stats() == dict(index_stagings=0, weight_stagings=0, td_readouts=0, rows_refused=0)
    empty = track(P.Engine(D.cfg, [-1.0] * D.cfg.ac_dim, [1.0] * D.cfg.ac_dim))
    with pytest.raises(P.EngineError, match="-3.*empty"):
        stage(empty, idx, w)
    stage(D, idx, w)                                                         # ... and the engine takes a good call
    D.update_qnets()
    assert np.isfinite(td_of(D)).all()


# ------------------------------------------------------------------------------------------ 7. TD errors
def check_td(eng, what):
    """td_errors == debug_read("q") - debug_read("targ_q") as float32 bits; and the rows are the reported slot's: where a row is
    done, y is its reward exactly, so q - td gives the reward read_batch() reports back (to the rounding of the two subtractions)"""
    B = eng.cfg.batch_size
    td = td_of(eng)
    q, y = eng.debug_read("q").reshape(2, B), eng.debug_read("targ_q")
    assert same_bits(td, q - y[None, :]), what
    batch = eng.read_batch()
    done = batch["dones"].reshape(-1)
    assert done.sum() >= 1, what
    rec = (q - td)[:, done]
    assert np.abs(rec - batch["rewards"].reshape(-1)[done][None, :]).max() <= 1e-5 * (1.0 + np.abs(q).max() + np.abs(td).max()), what
    return td


@pytest.mark.parametrize("case", ALL)
def test_td_errors_are_the_last_critic_updates(case):
    """after update_qnets (plain and weighted), step(True), step_period() and step_prefix(1); SACTD3_ESTATE before any update and
    after a refill of the slot; strided `out` views; a twin that never asks ends in the same state, the period behind a read-out
    between two periods included (the precomputed opening pair stays valid)"""
    _, (D, T), _, B, _ = build(case, 2)
    with pytest.raises(P.EngineError, match="-3"):
        td_of(D)
    idx = indices(B)
    for eng in (D, T):
        eng.rb_sample_with_indices(idx)
        eng.update_qnets()
    check_td(D, "update_qnets")
    # a [2, B, 1] window of a larger array: rows 2 elements apart, critics 2 (B + 3); nothing else is written
    big = torch.full((2, B + 3, 2), SENTINEL, device=DEV)
    D.td_errors_device(big[:, 1:, 1:].data_ptr(), 2, 2 * (B + 3), stream())
    host = big.cpu().numpy()
    assert same_bits(host[:, 1:B + 1, 1], td_of(D)) and (host[:, :, 0] == np.float32(SENTINEL)).all() and (host[:, 0] == np.float32(SENTINEL)).all()
    assert (host[:, B + 1:] == np.float32(SENTINEL)).all()
    for eng in (D, T):
        eng.rb_sample()
    with pytest.raises(P.EngineError, match="-3"):                            # a refill since the update
        td_of(D)
    w = weights_u02(B) + 0.5
    keep = [stage(eng, idx, w) for eng in (D, T)]
    with pytest.raises(P.EngineError, match="-3"):
        td_of(D)
    for eng in (D, T):
        eng.update_qnets()
    check_td(D, "weighted update_qnets")
    for name, call in (("step", lambda e: e.step(True)), ("step_period", lambda e: e.step_period()), ("step_period again", lambda e: e.step_period()),
                       ("step_prefix", lambda e: e.step_prefix(1)), ("step(False)", lambda e: e.step(False))):
        call(D)
        call(T)
        check_td(D, name)
        assert np.array_equal(D.read_batch()["index"], T.read_batch()["index"]), name
    assert_same_state(D, T)
    assert D.priority_stats()["td_readouts"] >= 8 and T.priority_stats()["td_readouts"] == 0
    del keep


# ------------------------------------------------------------------------------------------ 8. lifetime of the weights
@pytest.mark.parametrize("refill", ["rb_sample", "load_batch_device", "step", "drop"])
def test_weights_do_not_outlive_their_batch(refill):
    """after rb_sample, load_batch_device, step, and batch_weights_device(NULL), update_qnets is the plain one again: bit-equal to a
    twin that never staged weights"""
    case = "sac-hopper-64"
    shape, _ = CASES[case]
    _, (D, T), _, B, _ = build(case, 2)
    idx = indices(B)
    keep = stage(D, idx, weights_u02(B))
    if refill == "rb_sample":
        D.rb_sample()
        T.rb_sample()
    elif refill == "load_batch_device":
        five = cuda([t[idx] for t in ring_rows(shape)])
        load_device(D, five)
        load_device(T, five)
    elif refill == "step":
        D.step(False)
        T.step(False)
    else:
        D.batch_weights_device(0, 1, B, stream())
        T.rb_sample_with_indices(idx)
    D.update_qnets()
    T.update_qnets()
    assert_same_bits(critic_update_state(D), critic_update_state(T), what=refill)
    assert_same_bits(slot(D), slot(T), what=refill)
    assert D.graph_kernel_count(8) == 0 and D.graph_kernel_count(0) > 0      # the weighted graph was never needed
    del keep


def test_actor_update_is_never_weighted():
    """update_actor behind a weighted critic update equals a twin's behind a plain one on the same rows, once the twin has been given
    the same critics: same actor gradients, parameters, metrics; and the two critic graphs have the same number of nodes"""
    _, (D, T), _, B, _ = build("sac-hopper-64", 2)
    idx = indices(B)
    keep = stage(D, idx, weights_u02(B))
    T.rb_sample_with_indices(idx)
    D.update_qnets()
    T.update_qnets()
    assert not np.array_equal(D.get_params(_lib.CRITICS), T.get_params(_lib.CRITICS))
    T.set_params(_lib.CRITICS, D.get_params(_lib.CRITICS))
    D.update_actor()
    T.update_actor()
    assert same_bits(D.debug_read("grad_actor"), T.debug_read("grad_actor"))
    for which in (_lib.ACTOR, _lib.LOG_ALPHA):
        assert same_bits(D.get_params(which), T.get_params(which)), which
    x, y = D.read_metrics(), T.read_metrics()
    assert all(x[k] == y[k] for k in ("loss/actor_loss", "loss/alpha_loss", "vitals/alpha"))
    D.rb_sample()
    D.update_qnets()
    assert D.graph_kernel_count(8) == D.graph_kernel_count(0) > 0
    del keep


# ------------------------------------------------------------------------------------------ 9. the loop
def test_train_with_a_proportional_sampler_stays_on_the_device():
    """loop.train(fused=False, sampler=ProportionalSampler) on SyntheticDeviceVecEnv, 40 iterations past learning_starts: finite losses;
    the priorities of the last sampled slots are |td| (max over critics) + eps of the TD errors the engine reports; every device call
    of the run was a stream-ordered one and nothing was read back through the host."""
    o, a, n, iters = 11, 3, 4, 40
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=64).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 200,
                             "num_timesteps": 200 + iters * n - 1, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 1000})
    env = loop.SyntheticDeviceVecEnv(o, a, n, horizon=7, term_at=2.5, device=DEV)
    env.action_space.seed(0)
    torch.manual_seed(0)
    agent = P.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                    torch.device(DEV), cfg, P.ReplayBuffer(cfg.rb_capacity))
    sampler = loop.ProportionalSampler(cfg.rb_capacity, alpha=0.6, beta=0.4, eps=1e-6, device=DEV)
    seen = []
    update = sampler.update

    def spy(index, td):
        seen.append((index, td.clone()))                                     # (device tensors: looked at after the run)
        update(index, td)
    sampler.update = spy
    with pytest.raises(ValueError, match="fused=False"):
        loop.train(cfg, env, agent, fused=True, device_env=True, sampler=sampler)
    metrics = loop.train(cfg, env, agent, fused=False, device_env=True, sampler=sampler)
    eng = track(agent.engine)
    assert all(np.isfinite(v) for v in metrics.values()), metrics
    assert len(seen) == agent.qnet_updates_so_far >= iters and sampler.len == eng.rb_len() == len(agent.rb)
    ps, bs, pd, ro = eng.priority_stats(), eng.boundary_stats(), eng.predict_device_stats(), eng.readout_stats()
    assert ps == dict(index_stagings=len(seen), weight_stagings=0, td_readouts=len(seen), rows_refused=0)
    assert bs["ordered_calls"] == bs["device_extends"] + pd["calls"] + ps["index_stagings"] + ps["td_readouts"] and pd["ordered_calls"] == pd["calls"]
    assert bs["device_batches"] == 0 and ro["batch_readouts"] == 0 and ro["row_readouts"] == 0
    for index, td in seen:
        assert index.dtype == torch.int64 and td.shape == (2, 64, 1) and bool(torch.isfinite(td).all())
        assert int(index.min()) >= 0 and int(index.max()) < sampler.len
    # the last update's rows: the engine's own q - y, and the slots it trained on
    B = 64
    td_host = eng.debug_read("q").reshape(2, B) - eng.debug_read("targ_q")[None, :]
    index, td = seen[-1]
    assert same_bits(td.cpu().numpy().reshape(2, B), td_host) and np.array_equal(index.cpu().numpy(), eng.read_batch()["index"])
    want = np.abs(td_host).max(0) + np.float32(1e-6)
    ih = index.cpu().numpy()
    slots, counts = np.unique(ih, return_counts=True)
    once = np.isin(ih, slots[counts == 1])                                   # (a slot drawn twice keeps one of its two rows' values)
    assert once.sum() > B // 2 and same_bits(sampler.priorities[index].cpu().numpy()[once], want[once])
    pri = sampler.priorities[:sampler.len].cpu().numpy()
    assert (pri > 0).all() and np.isfinite(pri).all() and float(sampler.max_priority) >= pri.max() > 0
