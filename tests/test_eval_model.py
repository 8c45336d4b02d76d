"""The checker of the one-launch evaluation rollout (tests/eval_model.py) on the CPU: it accepts a numpy-float32 emulation of the whole
rollout on the env's host twin, and refuses every planted defect.  No GPU, no library."""
import numpy as np
import pytest

from tests import bounds, eval_model as M

pytest.importorskip("sac_td3_cudagraphs_pytorch_amd")
from sac_td3_cudagraphs_pytorch_amd import envs  # noqa: E402

HORIZON, T = 4, 7          # an auto-reset and the end of the call's episode inside a handful of steps
GAMMA, LOG_ALPHA, SEED, CTR, ENV_SEED = 0.9, -1.2, 11, 3, 5


def _case(kind, sac, ln, sample, rng_seed=0, w1_scale=1.0, head_scale=1.0):
    o, a = envs.SPECS[envs.kind_of(kind)][:2]
    p = M.random_params(np.random.default_rng(rng_seed), o, 2 * a if sac else a, ln, w1_scale, head_scale)
    return dict(kind=kind, p=p, kw=dict(ln=ln, sac=sac, sample=sample, soft=sample, gamma=GAMMA, log_alpha=LOG_ALPHA, seed=SEED, ctr=CTR))


def _run(c, n=5, defect=None, state=None, steps=T):
    rec, scale, bias = M.emulate32(c["kind"], n, steps, HORIZON, c["p"], env_seed=ENV_SEED, defect=defect, state=state, **c["kw"])
    return M.check_rollout(rec, c["p"], scale=scale, bias=bias, **c["kw"]), rec


@pytest.mark.parametrize("kind", ["pendulum", "cartpole", "pointgoal"])
@pytest.mark.parametrize("sac,sample", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("ln", [True, False])
def test_the_checker_accepts_the_float32_emulation(kind, sac, sample, ln):
    worst, rec = _run(_case(kind, sac, ln, sample), n=17)
    assert 0.0 <= worst <= 1.0
    assert rec["live"][:HORIZON].all() and (rec["ep_length"] == HORIZON).all()      # nothing terminates in four steps: the time limit ends them
    assert not rec["live"][HORIZON:].any() and not rec["rtg"][HORIZON:].any()
    if sample:
        assert np.abs(rec["logp"]).min() > 0 and rec["eps"].std() > 0.5


def test_saturated_heads_and_single_steps_pass():
    assert _run(_case("pendulum", True, True, True, head_scale=50.0))[0] <= 1.0
    worst, rec = _run(_case("pointgoal", True, True, True), n=1, steps=1)
    assert worst <= 1.0 and (rec["ep_length"] == 0).all() and not rec["rtg"].any() and rec["live"].all()      # still open: no return


def test_termination_beats_truncation():
    """the cart-pole one step from its angle limit, three steps into a four-step horizon: it terminates at the call's first step"""
    n = 5
    phys = np.tile(np.array([0.0, 0.0, 0.2094, 2.0], np.float32), (n, 1))
    state = {"phys": phys, "steps": np.full(n, 2, np.int32)}
    worst, rec = _run(_case("cartpole", False, True, False), n=n, state=state)
    assert worst <= 1.0
    assert (rec["ep_length"] == 1).all() and rec["ep_terminated"].all() and (rec["live"].sum(0) == 1).all()
    assert np.array_equal(rec["g0"], rec["reward"][0]) and np.array_equal(rec["ep_return"], rec["reward"][0])


# w1_scale 0.001: the layer-1 pre-activations have a variance below the LayerNorm's epsilon, so that dropping it moves every row by far more
# than any rounding; gamma < 1, alpha > 0, rewards and log-probs away from zero, scale 2 (the pendulum): every other defect shows the same way
@pytest.mark.parametrize("defect", M.DEFECTS)
def test_the_checker_refuses_every_planted_defect(defect):
    c = _case("pendulum", True, True, True, w1_scale=0.001)
    assert _run(c)[0] <= 1.0                                   # the same inputs pass without the defect
    with pytest.raises(bounds.Violation):
        _run(c, defect=defect)


def test_there_are_at_least_seven_defects_and_each_is_reached():
    assert len(M.DEFECTS) >= 7 and len(set(M.DEFECTS)) == len(M.DEFECTS)
    c = _case("pendulum", True, True, True, w1_scale=0.001)
    base = M.emulate32(c["kind"], 5, T, HORIZON, c["p"], env_seed=ENV_SEED, **c["kw"])[0]
    for d in M.DEFECTS:
        got = M.emulate32(c["kind"], 5, T, HORIZON, c["p"], env_seed=ENV_SEED, defect=d, **c["kw"])[0]
        assert any(not np.array_equal(got[k], base[k]) for k in ("actions", "rtg", "live")), d


def test_the_draws_are_the_streams_own():
    """element i ac_dim + j of (ctr, t, 0x800, element >> 2): another counter, step or stream is refused; the float32 draws are inside the bound"""
    z, b = M.normals64(SEED, CTR, 3, 5, 2)
    e = M.normals32(SEED, CTR, 3, 5, 2)
    assert bounds.check("eps", e, z, b) <= 1.0
    for other in (M.normals32(SEED, CTR + 1, 3, 5, 2), M.normals32(SEED + 1, CTR, 3, 5, 2), e[::-1].copy()):
        with pytest.raises(bounds.Violation):
            bounds.check("eps", other, z, b)
    assert abs(float(M.normals32(SEED, CTR, 64, 64, 2).mean())) < 0.05 and abs(float(M.normals32(SEED, CTR, 64, 64, 2).std()) - 1.0) < 0.05


def test_returns_model_by_hand():
    r = np.array([[1.0], [2.0], [4.0], [8.0]], np.float32)
    lp = np.array([[0.0], [1.0], [2.0], [3.0]], np.float32)
    ended = np.array([[False], [False], [True], [False]])
    m = M.returns32(r, lp, ended, ended, 0.5, 0.5, True)
    # G2 = 4; G1 = 2 + 0.5 (4 - 0.5 * 2) = 3.5; G0 = 1 + 0.5 (3.5 - 0.5 * 1) = 2.5
    assert m["rtg"][:, 0].tolist() == [2.5, 3.5, 4.0, 0.0] and m["live"][:, 0].tolist() == [1, 1, 1, 0]
    assert m["ep_return"][0] == 7.0 and m["ep_length"][0] == 3 and m["ep_terminated"][0] == 1 and m["g0"][0] == 2.5
    hard = M.returns32(r, lp, ended, ~ended, 0.5, 0.5, False)
    assert hard["rtg"][:, 0].tolist() == [3.0, 4.0, 4.0, 0.0] and hard["ep_terminated"][0] == 0
    still = M.returns32(r, lp, np.zeros((4, 1), bool), np.zeros((4, 1), bool), 0.5, 0.5, False)
    assert not still["rtg"].any() and still["live"].all() and still["ep_length"][0] == 0 and still["ep_return"][0] == 15.0
