"""loop.Rollout / segment / train with overlap=True (the action that opens a segment is begun before the caller gets control and
collected when the env is stepped) against the restated reference generator, without a GPU; the launcher's switch for it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.rollout_ref import ListBuffer, segment_ref
from sac_td3_cudagraphs_pytorch_amd import loop


class SerialAgent:
    """the stand-in of tests/test_loop.py: predict() is a fixed function of the observation and of the call number"""

    def __init__(self, a):
        self.rb, self.timesteps_so_far, self.a, self.calls = ListBuffer(), 0, a, 0

    def predict(self, td, *, explore):
        self.calls += 1
        ob = np.asarray(td["observations"], np.float32)
        return np.tanh(ob[:, : self.a] * 0.7 + 0.1 * self.calls).astype(np.float32)


class OverlapAgent(SerialAgent):
    """... with the two halves: the action is a function of what predict_begin() saw; every call is logged"""

    def __init__(self, a):
        super().__init__(a)
        self.log, self.held = [], None

    def predict(self, td, *, explore):
        raise AssertionError("an overlapped rollout acts through predict_begin / predict_end only")

    def predict_begin(self, td, *, explore):
        assert explore is True and self.held is None, "one call in flight at most"
        self.held = SerialAgent.predict(self, td, explore=explore)
        self.log.append(("begin", self.timesteps_so_far, len(self.rb)))

    def predict_end(self):
        assert self.held is not None, "predict_end without predict_begin"
        out, self.held = self.held, None
        self.log.append(("end", self.timesteps_so_far, len(self.rb)))
        return out


@pytest.mark.parametrize("segment_len,action_repeat", [(1, 1), (3, 1), (2, 2)])
def test_overlapped_segment_writes_the_same_rows_as_the_restated_reference(segment_len, action_repeat):
    o, a, n, learning_starts, yields = 5, 2, 4, 40, 40
    runs = []
    for overlapped in (True, False):
        env = loop.SyntheticVecEnv(o, a, n, horizon=7, term_at=2.5)
        env.action_space.seed(3)
        agent = OverlapAgent(a) if overlapped else SerialAgent(a)
        if overlapped:
            gen = loop.segment(env, agent, seed=11, segment_len=segment_len, learning_starts=learning_starts, action_repeat=action_repeat,
                               overlap=True)
        else:
            gen = segment_ref(env, agent, seed=11, segment_len=segment_len, learning_starts=learning_starts, action_repeat=action_repeat)
        in_flight_at_yield = 0
        for _ in range(yields):
            next(gen)
            in_flight_at_yield += overlapped and agent.held is not None
            agent.timesteps_so_far += segment_len * n
        runs.append((agent, in_flight_at_yield))
    (got_agent, in_flight), (want_agent, _) = runs
    got, want = got_agent.rb.rows, want_agent.rb.rows
    assert len(got) == len(want) > 100
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            assert g[k].dtype == w[k].dtype and np.array_equal(g[k], w[k]), k
    log = got_agent.log
    # begins and ends alternate strictly, one end per begin but for the call that is in flight when the test stops
    assert [kind for kind, _, _ in log] == (["begin", "end"] * len(log))[:len(log)] and log[-1][0] == "begin"
    # as many policy actions as the serial reference computed, none of them in the random phase
    assert got_agent.calls == want_agent.calls > 0
    assert all(ts >= learning_starts for _, ts, _ in log)
    # no begin on a repeated action: the rows written when a call begins are a multiple of action_repeat env steps
    assert all((rows // n) % action_repeat == 0 for kind, _, rows in log if kind == "begin")
    # the caller had control with an action in flight (that is the overlap) at every yield of the policy phase whose segment
    # opens with a fresh action
    assert in_flight > 0
    if action_repeat == 1:
        assert in_flight == sum(1 for k in range(yields) if k * segment_len * n >= learning_starts)


def test_overlap_needs_an_agent_with_the_two_halves():
    env = loop.SyntheticVecEnv(3, 1, 2)
    gen = loop.segment(env, SerialAgent(1), seed=0, segment_len=1, learning_starts=0, action_repeat=1, overlap=True)
    with pytest.raises(TypeError, match="predict_begin"):
        next(gen)
    with pytest.raises(TypeError, match="predict_begin"):
        loop.Rollout(env, SerialAgent(1), 0, 0, 1, overlap=True)
    loop.Rollout(env, SerialAgent(1), 0, 0, 1)                         # the default asks for nothing new


class _Engine:
    def read_metrics(self):
        return {"ok": 1.0}


class TrainAgent(OverlapAgent):
    """... plus what loop.train touches; predict() (the evaluator's call) refuses to run under a pending action"""

    def __init__(self, a):
        super().__init__(a)
        self.engine, self.iterations, self.best_eval_ep_ret, self.evals = _Engine(), [], -np.inf, 0

    def predict(self, td, *, explore):
        assert self.held is None, "something acted with the agent while an action was pending"
        self.evals += 1
        return np.zeros((len(td["observations"]), self.a), np.float32)

    def iteration(self, i):
        self.iterations.append((i, self.held is not None))

    def save(self, path, sfx=None):
        pass


def test_train_resolves_a_pending_action_before_an_evaluation_and_at_the_end():
    from types import SimpleNamespace
    o, a, n = 4, 2, 2
    cfg = SimpleNamespace(seed=1, segment_len=1, learning_starts=20, action_repeat=1, num_timesteps=60, num_envs=n, eval_every=10,
                          eval_steps=1, batch_size=8, actor_update_delay=2)
    agent = TrainAgent(a)
    env = loop.SyntheticVecEnv(o, a, n, horizon=9)
    env.action_space.seed(0)
    ev = loop.Evaluator(cfg, loop.SyntheticVecEnv(o, a, 1, horizon=5), agent)
    seen = []
    out = loop.train(cfg, env, agent, evaluator=ev, on_eval=lambda ag, ts: seen.append((ts, ag.held is None)), overlap=True)
    assert out == {"ok": 1.0} and agent.held is None                    # nothing left in flight behind the loop
    assert agent.evals > 0 and seen and all(idle for _, idle in seen)
    assert agent.iterations and all(in_flight for _, in_flight in agent.iterations)   # every update was issued under a begun action
    # same rows as the serial loop with the same policy function
    ref = SerialAgent(a)
    ref.engine, ref.iteration, ref.best_eval_ep_ret = _Engine(), (lambda i: None), -np.inf
    env2 = loop.SyntheticVecEnv(o, a, n, horizon=9)
    env2.action_space.seed(0)
    loop.train(cfg, env2, ref)
    # (the evaluator's greedy calls went through predict() in the overlapped run and are not counted by `calls` there)
    assert len(agent.rb.rows) == len(ref.rb.rows) > 0
    for g, w in zip(agent.rb.rows, ref.rb.rows):
        for k in w:
            assert np.array_equal(g[k], w[k]), k


def test_launcher_dry_run_accepts_overlap_acting(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--env_bundle", "debug", "--num_seeds", "2",
                          "--gpus", "2", "--dry-run", "--overlap_acting", "--out", str(tmp_path)], cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    sweep = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("SWEEP ")][0][6:])
    assert sweep["jobs"] == sweep["expected_jobs"] > 0
    from sac_td3_cudagraphs_pytorch_amd import launcher
    import inspect
    assert "overlap_acting" in inspect.signature(launcher.run_job).parameters
