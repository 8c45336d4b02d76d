"""GPU: the goal env (include/sactd3_env.h: SACTD3_ENV_POINTGOAL; csrc/env_kernels.h) against the float64 model and its bound and the
float32 restatement bit for bit (tests/goal_env_model.py), its records against `pack_records` of the plain step, and one native
rollout against the device rollout."""
import numpy as np
import pytest
import torch

from tests import goal_env_model as gm
from tests.gpu_support import DEV, P, assert_same_state, loop, same_bits, track

pytestmark = pytest.mark.gpu
envs = P.envs
F = np.float32


def new_env(n, seed=0, horizon=None):
    return track(envs.NativeVecEnv("pointgoal", n, seed=seed, device=DEV, horizon=horizon))


def host(x):
    return x.cpu().numpy()


def got_of(res):
    obs, rew, term, trunc, infos = res
    return {"obs": host(obs), "final_obs": host(infos["final_observation"]), "reward": host(rew), "terminated": host(term),
            "truncated": host(trunc), "ended": host(infos["_final_observation"])}


def new_agent(cfg, seed):
    torch.manual_seed(seed)
    agent = P.Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, F), np.full(2, 1.0, F), torch.device(DEV), cfg,
                    P.ReplayBuffer(cfg.rb_capacity), seed=seed)
    track(agent.engine)
    return agent


def test_spec_and_goal_layout():
    env = new_env(3, seed=1)
    assert (env.o, env.a, env.horizon, env.bound) == (6, 2, 50, 1.0) and env.goal_layout == gm.LAYOUT
    assert new_env(3, horizon=9).horizon == 9
    obs = host(env.reset(seed=1)[0])
    assert same_bits(obs, np.concatenate([gm.first_states(1, np.arange(3), np.zeros(3)), gm.goals(1, np.arange(3), np.zeros(3))], 1))


def test_planted_states_wall_threshold_and_horizon():
    seed = 21
    phys, steps, ep, act = gm.planted(seed)
    n = len(steps)
    env = new_env(n, seed=seed)
    env.reset(seed=seed)
    before = {"phys": phys, "steps": steps, "episode": ep, "returns": np.linspace(-3, 0, n).astype(F)}
    assert gm.conditioned(seed, before, act).all()
    env.set_state(before)
    got = got_of(env.step(torch.as_tensor(act, device=DEV)))
    worst = gm.check_step(seed, env.horizon, before, act, got, env.state(), exact=True)
    fin = got["final_obs"]
    assert fin[0, 0] == 1.0 and fin[1, 1] == -1.0 and tuple(fin[7, :2]) == (1.0, 1.0) and fin[8, 0] == -1.0
    assert list(got["reward"][[2, 3, 4, 10]]) == [0.0, -1.0, 0.0, -1.0]       # d2 == thr^2: on the goal; one ulp beyond: off it
    assert list(np.flatnonzero(got["truncated"])) == [5] and not got["terminated"].any() and 0.0 < worst <= 1.0
    # the host twin from the same state: the same bits
    twin = envs.HostVecEnv("pointgoal", n, seed=seed)
    twin.set_state(before)
    obs, rew, term, trunc, infos = twin.step(act)
    assert same_bits(obs, got["obs"]) and same_bits(rew, got["reward"]) and same_bits(twin.state()["phys"], env.state()["phys"])


def test_200_rolled_steps_against_the_model_and_the_host_twin():
    seed, n, T = 5, 5, 200
    env, twin = new_env(n, seed=seed), envs.HostVecEnv("pointgoal", n, seed=seed)
    env.reset(seed=seed)
    twin.reset(seed=seed)
    worst, ends, on_goal = 0.0, 0, 0
    for t in range(T):
        before = env.state()
        act = env.action_space.sample()
        a = host(act)
        assert same_bits(a, gm.random_actions(seed, np.arange(n), before["draws"]))
        if t % 3 == 0:
            a = (a * F(1.3)).astype(F)                                        # beyond the bounds: clamped
            act = torch.as_tensor(a, device=DEV)
        assert gm.conditioned(seed, before, a).all(), t
        got = got_of(env.step(act))
        worst = max(worst, gm.check_step(seed, env.horizon, before, a, got, env.state(), exact=True))
        twin.action_space.sample()
        obs, rew = twin.step(a)[:2]
        assert same_bits(obs, got["obs"]) and same_bits(rew, got["reward"]), t
        ends, on_goal = ends + int(got["ended"].sum()), on_goal + int((got["reward"] == 0).sum())
    st, ht = env.episode_stats(), twin.episode_stats()
    print(f"worst |err| / bound over {T} steps {worst:.3f}; {on_goal} steps on a goal")
    assert 0.0 < worst <= 1.0 and ends == 4 * n == st["episodes"] and st["bad_actions"] == 0
    assert all(same_bits(np.asarray(st[k]), np.asarray(ht[k])) for k in ("last_return", "first_return", "last_length", "first_length"))
    assert all(same_bits(env.state()[k], twin.state()[k]) for k in ("phys", "steps", "episode", "returns", "draws"))


def test_a_nan_in_one_component_only():
    n, seed = 4, 3
    env = new_env(n, seed=seed)
    env.reset(seed=seed)
    act = np.array([[np.nan, 0.5], [0.5, np.inf], [np.nan, -np.inf], [3.4028235e38, -0.25]], F)
    before = env.state()
    got = got_of(env.step(torch.as_tensor(act, device=DEV)))
    gm.check_step(seed, env.horizon, before, act, got, env.state(), exact=True)
    assert env.episode_stats()["bad_actions"] == 3 and np.isfinite(env.state()["phys"]).all()
    assert same_bits(env.state()["phys"][:, 2:4], (F(0.2) * np.array([[0, 0.5], [0.5, 0], [0, 0], [1.0, -0.25]], F)).astype(F))


@pytest.mark.parametrize("n", [4, 257])
def test_records_are_pack_records_of_the_plain_step(n):
    seed, H = 11, 5
    A, B = new_env(n, seed=seed, horizon=H), new_env(n, seed=seed, horizon=H)
    obsA = A.reset(seed=seed)[0]
    B.reset(seed=seed)
    gen = torch.Generator().manual_seed(n)
    for layout in ((20, 8, 8), (32, 12, 12)):                              # the tightest for (6, 2), and one with pads everywhere
        rec = torch.full((n + 1, layout[0]), -7.0, device=DEV)
        obsB = torch.full((n, 8), -7.0, device=DEV)
        trunc_seen = 0
        for t in range(2 * H + 1):
            act = (torch.rand((n, 2), generator=gen) * 2.4 - 1.2)
            if t == 2:
                act[0, 1], act[1 % n, 0] = float("nan"), float("inf")
            act = act.to(DEV)
            arrived, rew, term, trunc, infos = A.step(act)
            stored = torch.where(trunc.reshape(-1, 1), infos["final_observation"], arrived)
            want = envs.pack_records(layout, host(obsA), host(act), host(rew), host(stored), host(term))
            B.step_records(act, layout, rec[:n], obsB)
            got = host(rec)
            assert same_bits(got[:n], want), t                                # s, a (NaN bits included), s' stored, r, d and every pad
            assert (got[n] == F(-7.0)).all() and (host(obsB)[:, 6:] == F(-7.0)).all() and same_bits(host(obsB)[:, :6], host(arrived))
            obsA = arrived
            trunc_seen += int(trunc.sum())
        assert trunc_seen == 2 * n
        assert all(same_bits(A.state()[k], B.state()[k]) for k in ("phys", "steps", "episode", "returns", "draws"))
    assert A.episode_stats()["bad_actions"] == B.episode_stats()["bad_actions"] == 2 * 2      # two envs per layout: one bad component each


def test_native_rollout_against_device_rollout():
    n, seed, pairs, starts_at = 4, 6, 30, 12
    cfg = P.launcher.job_config("sac", "PointGoal-native", seed, num_envs=n, learning_starts=starts_at * n, batch_size=64,
                                num_timesteps=10 ** 6, eval_every=10 ** 9, rb_capacity=100)
    agents = [new_agent(cfg, seed) for _ in range(2)]
    es = [new_env(n, seed=seed, horizon=7) for _ in range(2)]
    old = loop.DeviceRollout(es[0], agents[0], seed, cfg.learning_starts, 1)
    new = loop.NativeRollout(es[1], agents[1], seed, cfg.learning_starts, 1)
    for t in range(pairs):
        for ag in agents:
            ag.timesteps_so_far = t * n
        old.choose()
        new.choose()
        assert same_bits(host(old.actions), host(new.actions)), t
        old.advance()
        new.advance()
        assert same_bits(host(old.obs), host(new.obs)), t
    ra, rb = (({k: host(v) for k, v in ag.rb.rows(np.arange(len(ag.rb))).items()}) for ag in agents)
    assert len(agents[1].rb) == 100 and list(ra) == list(rb) and all(same_bits(ra[k], rb[k]) for k in ra)
    assert all(same_bits(es[0].state()[k], es[1].state()[k]) for k in ("phys", "steps", "episode", "returns", "draws"))
    sa, sb = es[0].episode_stats(), es[1].episode_stats()
    assert all(same_bits(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa) and sa["episodes"] == n * (pairs // 7)
    assert new.stats()["rows_appended"] == pairs * n
    assert_same_state(agents[0].engine, agents[1].engine, "ring")
    new.close()
