"""The checker of the collected rollout segment (tests/collect_model.py) on the CPU: it accepts a numpy-float32 emulation of the whole call
on the env's host twin, in every mode, and refuses every planted defect.  No GPU, no library."""
import numpy as np
import pytest

from tests import bounds, collect_model as M, eval_model

pytest.importorskip("sac_td3_cudagraphs_pytorch_amd")
from sac_td3_cudagraphs_pytorch_amd import envs  # noqa: E402

HORIZON, T = 5, 12         # every env crosses two resets
SEED, CTR, ENV_SEED, NOISE = 11, 3, 5, 0.1


def _params(kind, sac, ln, head_scale=1.0):
    o, a = envs.SPECS[envs.kind_of(kind)][:2]
    return eval_model.random_params(np.random.default_rng(0), o, 2 * a if sac else a, ln, 1.0, head_scale)


def _run(kind, mode, sac=True, ln=True, n=5, steps=T, defect=None, head_scale=1.0, state=None):
    return M.check_emulation(kind, n, steps, HORIZON, _params(kind, sac, ln, head_scale), mode=mode, sac=sac, ln=ln, noise_std=NOISE,
                             seed=SEED, ctr=CTR, env_seed=ENV_SEED, state=state, defect=defect)


@pytest.mark.parametrize("kind", ["pendulum", "cartpole", "pointgoal"])
@pytest.mark.parametrize("mode", [M.RANDOM, M.EXPLORE, M.EXPLOIT], ids=["random", "explore", "exploit"])
@pytest.mark.parametrize("sac", [True, False], ids=["sac", "td3"])
@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
def test_the_checker_accepts_the_float32_emulation(kind, mode, sac, ln):
    n = 17
    worst, got = _run(kind, mode, sac, ln, n=n)
    assert 0.0 <= worst <= 1.0 and (worst > 0.0) == (mode != M.RANDOM)
    o, a = envs.SPECS[envs.kind_of(kind)][:2]
    layout = M.layout_for(o, a)
    f = M.fields(got["slab"], layout, o, a)
    assert not f["pads"].any() and f["pads"].size > 0
    # the time limit ended two episodes of every env (a cart-pole may also have dropped its pole); a truncation sets no flag
    assert (got["state"]["episode"] >= 2).all()
    if kind != "cartpole":
        assert not f["d"].any() and (got["state"]["episode"] == 2).all() and (got["state"]["steps"] == T - 2 * HORIZON).all()
    assert (got["state"]["draws"] == (T if mode == M.RANDOM else 0)).all()
    assert (np.abs(got["eps"]).max() > 0) == (mode == M.EXPLORE)


def test_single_steps_single_envs_and_saturated_heads_pass():
    assert _run("pointgoal", M.EXPLORE, n=1, steps=1)[0] <= 1.0
    assert _run("pendulum", M.RANDOM, n=1, steps=1)[0] == 0.0
    worst, got = _run("pendulum", M.EXPLORE, sac=False, head_scale=50.0)
    a = M.fields(got["slab"], M.layout_for(3, 1), 3, 1)["a"]
    assert worst <= 1.0 and (np.abs(a) > 2.0).any()                 # TD3's exploring action leaves the bounds: it is stored as chosen


def test_a_call_goes_on_from_the_state_it_is_given():
    n = 5
    state = {"steps": np.full(n, 3, np.int32), "draws": np.arange(n).astype(np.uint32), "episode": np.full(n, 4, np.uint32)}
    worst, got = _run("cartpole", M.RANDOM, n=n, state=state)
    assert worst == 0.0 and (got["state"]["draws"] == np.arange(n) + T).all() and (got["state"]["episode"] >= 6).all()


# which call shows which defect: the draws' defects need an exploring call, the scale's TD3 and a bound that is not 1 (the pendulum's 2),
# the clamp's an action beyond the bounds (saturated heads plus noise), the counter's the random mode; the record's show in any
CASES = {"stream_code": dict(mode=M.EXPLORE), "no_t": dict(mode=M.EXPLORE), "env_major": dict(mode=M.EXPLOIT),
         "next_not_arrival": dict(mode=M.EXPLOIT), "d_on_truncation": dict(mode=M.EXPLOIT), "noise_no_scale": dict(mode=M.EXPLORE, sac=False),
         "clamped_action": dict(mode=M.EXPLORE, sac=False, head_scale=50.0), "draws_stuck": dict(mode=M.RANDOM)}


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_the_checker_refuses_every_planted_defect(defect):
    kw = CASES[defect]
    assert _run("pendulum", **kw)[0] <= 1.0                          # the same call passes without the defect
    with pytest.raises(bounds.Violation):
        _run("pendulum", defect=defect, **kw)


def test_there_are_at_least_eight_defects_and_each_is_reached():
    assert len(M.DEFECTS) >= 8 and len(set(M.DEFECTS)) == len(M.DEFECTS) and set(CASES) == set(M.DEFECTS)
    for d in M.DEFECTS:
        kw = dict(CASES[d])
        sac, hs = kw.pop("sac", True), kw.pop("head_scale", 1.0)
        args = dict(mode=kw["mode"], sac=sac, ln=True, noise_std=NOISE, seed=SEED, ctr=CTR, env_seed=ENV_SEED)
        base = M.emulate32("pendulum", 5, T, HORIZON, _params("pendulum", sac, True, hs), **args)[0]
        got = M.emulate32("pendulum", 5, T, HORIZON, _params("pendulum", sac, True, hs), defect=d, **args)[0]
        assert any(not np.array_equal(got[k], base[k]) for k in ("slab", "eps")) or not np.array_equal(got["state"]["draws"], base["state"]["draws"]), d


def test_the_draws_are_the_streams_own():
    """element i ac_dim + j of (ctr, t, 0x900, element >> 2): another counter, key, step or stream is refused"""
    z, b = M.normals64(SEED, CTR, 3, 5, 2)
    e = M.normals32(SEED, CTR, 3, 5, 2)
    assert bounds.check("eps", e, z, b) <= 1.0
    others = (M.normals32(SEED, CTR + 1, 3, 5, 2), M.normals32(SEED + 1, CTR, 3, 5, 2), e[::-1].copy(), M.normals32(SEED, CTR, 3, 5, 2, stream=0x800),
              M.normals32(SEED, CTR, 3, 5, 2, with_t=False), eval_model.normals32(SEED, CTR, 3, 5, 2))
    for other in others:
        with pytest.raises(bounds.Violation):
            bounds.check("eps", other, z, b)
    big = M.normals32(SEED, CTR, 64, 64, 2)
    assert abs(float(big.mean())) < 0.05 and abs(float(big.std()) - 1.0) < 0.05


def test_the_layout_is_the_engines():
    assert [M.layout_for(o, a) for o, a in ((3, 1), (4, 1), (6, 2), (11, 3))] == [(16, 4, 4), (16, 8, 4), (32, 8, 8), (32, 16, 12)]
