"""CPU: the checker of the GPU-resident environments (tests/env_model.py) checks itself, without a GPU.  An fp32 numpy emulation of
the kernel in its own operation order passes the bound on the planted states; each defect a step kernel can have is refused; the
planted states are conditioned (none within its bound of a threshold) although some lie exactly ON one."""
import numpy as np
import pytest

from tests import bounds, env_model as em

SEED, N = 11, 257
# the task whose planted states show the defect (the cart-pole's reward is a constant and it has no clip and no angle to normalise;
# the pendulum has no threshold, never terminates and takes its torque unscaled)
DEFECT_TASK = {"reward_from_next_state": em.PENDULUM, "no_speed_clip": em.PENDULUM, "angle_not_normalised": em.PENDULUM,
               "ge_at_threshold": em.CARTPOLE, "final_obs_after_reset": None, "truncated_with_terminated": em.CARTPOLE,
               "reset_ignores_episode": None, "force_not_scaled": em.CARTPOLE}


def inputs(kind, n=N, offset=0, seed=0):
    rng = np.random.default_rng(seed)
    phys, steps, act = em.batch(kind, n, offset, rng)
    before = {"phys": phys, "steps": steps, "episode": (np.arange(n) % 3).astype(np.uint32),
              "returns": rng.standard_normal(n).astype(np.float32), "draws": np.zeros(n, np.uint32)}
    return before, act


@pytest.mark.parametrize("kind", [em.PENDULUM, em.CARTPOLE])
def test_the_fp32_emulation_passes_on_the_planted_states(kind):
    before, act = inputs(kind)
    assert em.conditioned(kind, before, act).all()                       # decided by the model alone
    got, after = em.emulate32(kind, SEED, em.HORIZON, before, act)
    worst = em.check_step(kind, SEED, em.HORIZON, before, act, got, after)
    assert 0.0 < worst <= 1.0
    # the planted states do what they were planted for
    m = len(em.planted(kind)[1])
    if kind == em.PENDULUM:
        assert got["truncated"][:m].sum() == 1 and not got["terminated"].any()
        th, w = before["phys"][:m, 0], after["phys"][:m, 1]
        assert (np.abs(after["phys"][:2, 0] - th[:2]) > 6.0).all()     # theta wrapped, both ways
        assert w[2] == 8.0 and w[3] == -8.0                            # the clip held
    else:
        assert list(got["terminated"][:8]) == [False, True, False, True, False, True, False, True]
        assert got["truncated"][:m].sum() == 1 and not (got["truncated"] & got["terminated"]).any()
        assert after["phys"][0, 0] == em.X_LIMIT and after["phys"][4, 2] == em.THETA_LIMIT      # exactly on the thresholds, and not beyond


@pytest.mark.parametrize("defect", em.DEFECTS)
def test_each_defect_is_refused(defect):
    kinds = (em.PENDULUM, em.CARTPOLE) if DEFECT_TASK[defect] is None else (DEFECT_TASK[defect],)
    for kind in kinds:
        before, act = inputs(kind)
        got, after = em.emulate32(kind, SEED, em.HORIZON, before, act, defect)
        with pytest.raises(bounds.Violation):
            em.check_step(kind, SEED, em.HORIZON, before, act, got, after)


def test_eight_defects():
    assert len(em.DEFECTS) == len(set(em.DEFECTS)) == 8 and set(DEFECT_TASK) == set(em.DEFECTS)


@pytest.mark.parametrize("kind", [em.PENDULUM, em.CARTPOLE])
@pytest.mark.parametrize("n", [1, 4])
def test_small_batches_cover_every_planted_state_in_rounds(kind, n):
    m = len(em.planted(kind)[1])
    seen = set()
    for offset in range(0, m, n):
        before, act = inputs(kind, n, offset)
        assert em.conditioned(kind, before, act).all()
        got, after = em.emulate32(kind, SEED, em.HORIZON, before, act)
        em.check_step(kind, SEED, em.HORIZON, before, act, got, after)
        seen |= {(offset + k) % m for k in range(min(n, m))}
    assert seen == set(range(m))


def test_a_state_within_its_bound_of_a_threshold_is_not_conditioned():
    """x' = x + 0.02 x_dot lands within a rounding of 2.4: the model cannot decide the flag and says so; with x_dot = 0 the same x' is
    exact and it can"""
    phys = np.array([[2.39, 0.5, 0.0, 0.0], [2.4, 0.0, 0.0, 0.0]], np.float32)
    phys[0, 0] = np.float32(2.4) - np.float32(0.02) * np.float32(0.5)
    before = {"phys": phys, "steps": np.zeros(2, np.int32), "episode": np.zeros(2, np.uint32), "returns": np.zeros(2, np.float32)}
    assert list(em.conditioned(em.CARTPOLE, before, np.zeros((2, 1), np.float32))) == [False, True]
    # the pendulum's cost squares angnorm(theta): at +-pi the wrap is ambiguous, a little inside it is not
    phys = np.array([[em.PI_F, 0, 0, 0], [em.PI_F - np.float32(1e-4), 0, 0, 0]], np.float32)
    assert list(em.conditioned(em.PENDULUM, dict(before, phys=phys), np.zeros((2, 1), np.float32))) == [False, True]


def test_the_bound_is_built_from_roundings_and_the_measured_library_error():
    """one exact operation adds nothing; one inexact one adds U |r|; a sine adds the recorded figure and nothing else"""
    x = em.V(np.array([2.4]).astype(np.float32)) + (em.V.of(0.02) * em.V(np.zeros(1)))
    assert x.e[0] == 0.0 and x.v[0] == float(np.float32(2.4))
    y = em.V(np.array([1.0])) + em.V(np.array([2.0 ** -30]))
    assert y.e[0] == pytest.approx(em.U * y.v[0])
    assert em.V(np.array([0.5])).sin().e[0] == em.SINF_ABS and em.V(np.array([0.5])).cos().e[0] == em.COSF_ABS
    import json
    import os
    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "libm_trig.json")))
    assert (em.SINF_ABS, em.COSF_ABS) == (rec["sinf_abs"], rec["cosf_abs"])      # as measured, no factor on top
    assert 2.0 ** -26 < em.SINF_ABS < 2.0 ** -22 and 2.0 ** -26 < em.COSF_ABS < 2.0 ** -22      # a float32 library function's, not a placeholder


def test_reset_draws_are_a_function_of_seed_env_and_episode():
    a = em.first_states(em.CARTPOLE, 5, np.arange(8), np.zeros(8))
    b = em.first_states(em.CARTPOLE, 5, np.arange(3, 8), np.zeros(5))
    assert np.array_equal(a[3:], b)                                         # env i whatever num_envs is
    assert not np.array_equal(a, em.first_states(em.CARTPOLE, 5, np.arange(8), np.ones(8)))
    assert not np.array_equal(a, em.first_states(em.CARTPOLE, 6, np.arange(8), np.zeros(8)))
    assert (np.abs(a) <= 0.05).all()
    p = em.first_states(em.PENDULUM, 5, np.arange(4096), np.zeros(4096))
    assert (np.abs(p[:, 0]) <= float(em.PI_F)).all() and (np.abs(p[:, 1]) <= 1.0).all() and not p[:, 2:].any()
    assert p[:, 0].min() < -3.0 and p[:, 0].max() > 3.0
    assert em.STREAM_ENV not in (0x000, 0x100, 0x200, 0x300, 0x400)          # csrc/philox.h: the engine's stream codes
