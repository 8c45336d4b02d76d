"""CPU: every mode of loop.train against a table recorded at the commit in front of `update_plan` (tests/golden/train_modes.json).

A case is one set of keywords of loop.train.  It runs on a recording agent -- every method train and the rollouts call on the agent, its
ring and its engine appends [name, arguments, keywords] to ONE list, and the agent keeps the three counters -- with a recording sampler, a
stub env with or without `step_records`, and `loop.segment` replaced by an endless generator (the rollouts are constructed, never stepped).
`loop.NativeRollout` needs a GPU to construct, so a stand-in that records its construction takes its place.  The outcome is
    ["raises", type name, message, calls made before]   or   ["runs", calls, [timesteps, qnet updates, actor updates], on_eval points]

  grid A  update modes: fused x sampler x prioritized x n_step x one_launch x prior_fraction x updates_per_step          1152 cases
  grid B  rollout modes: three update modes of grid A x overlap x device_env x native_rollout x env with / without records   48 cases

The file holds the distinct outcomes once and one index per case.  `python -m tests.test_train_modes FILE` writes it; it needs only
loop.train, so it runs in a checkout of any commit."""
import contextlib
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from sac_td3_cudagraphs_pytorch_amd import launcher, loop

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_modes.json")
CFG = dict(seed=0, learning_starts=8, action_repeat=1, segment_len=1, num_envs=4, num_timesteps=27, batch_size=8, actor_update_delay=2,
           eval_every=12)
UPDATE_KEYS = ("fused", "sampler", "prioritized", "n_step", "one_launch", "prior_fraction", "updates_per_step")
GRID_A = [dict(zip(UPDATE_KEYS, v)) for v in itertools.product(
    (True, False), (None, "stub"), (None, {}, {"beta": 0.6}, {"gamma": 1}), (0, 1, 3, 17), (True, False), (None, -0.1, 0.5), (0, 1, 2))]
DEFAULT_MODE = dict(fused=True, sampler=None, prioritized=None, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1)
MODES_B = (DEFAULT_MODE,                                                      # the fused one
           dict(DEFAULT_MODE, fused=False, prioritized={"beta": 0.6}),        # the prioritized call-by-call one
           dict(DEFAULT_MODE, fused=False, one_launch=True))                  # one that is refused
ROLLOUT_KEYS = ("overlap", "device_env", "native_rollout", "records_env")
GRID_B = [dict(mode, **dict(zip(ROLLOUT_KEYS, v))) for mode in MODES_B for v in itertools.product((False, True), repeat=4)]

# train() used to enable the priorities BEFORE it looked at the rollout keywords; now every refusal comes first.  These cases of grid B
# -- the prioritized mode with a rollout that is refused -- were recorded with an `rb.enable_priorities` call in front of the exception
# and run without it now.  Nothing else about them differs, and no case of grid A is among them.
REFUSED_BEFORE_PRIORITIES = (18, 19, 22, 26, 27, 28, 29, 30, 31)


def plain(x):
    """arguments as JSON holds them; an object that is no plain value by its type's name"""
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    return x if x is None or isinstance(x, (bool, int, float, str)) else f"<{type(x).__name__}>"


class Recorder:
    """any method: appends [prefix + name, arguments, keywords] to `calls`; what a draw returns names the call that made it"""
    RETURNS = {"sampler.sample": lambda k: (f"index@{k}", f"weights@{k}"), "td_errors": lambda k: f"td@{k}",
               "update_qnets": lambda k: {}, "update_actor": lambda k: {}, "engine.read_metrics": lambda k: {"calls": k}}

    def __init__(self, calls, prefix=""):
        self._calls, self._prefix = calls, prefix

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        full = self._prefix + name

        def call(*a, **kw):
            self._calls.append([full, plain(a), plain(kw)])
            k = len(self._calls)
            return self.RETURNS[full](k) if full in self.RETURNS else (f"batch@{k}" if full.startswith("rb.sample") else None)
        return call


class Agent(Recorder):
    def __init__(self, calls):
        super().__init__(calls)
        self.rb, self.engine = Recorder(calls, "rb."), Recorder(calls, "engine.")
        self.timesteps_so_far = self.qnet_updates_so_far = self.actor_updates_so_far = 0


class Env:
    def __init__(self, calls):
        self.calls = calls

    def reset(self, seed=None):
        self.calls.append(["env.reset", [], {"seed": seed}])
        return np.zeros((CFG["num_envs"], 3), np.float32), {}


class RecordsEnv(Env):
    def step_records(self):
        raise AssertionError("the rollout is never stepped")


class NativeStandIn:
    """stands where loop.NativeRollout stands (that one allocates on the GPU): records that it was constructed, and with what"""

    def __init__(self, env, agent, *args):
        env.calls.append(["NativeRollout", plain(args), {}])

    def resolve(self):
        pass


def endless_segment(env, agent, *args, **kw):
    agent.engine._calls.append(["segment", plain(args), {k: type(v).__name__ if k == "rollout" else plain(v) for k, v in kw.items()}])
    while True:
        yield


@contextlib.contextmanager
def no_env_loop():
    kept = loop.segment, loop.NativeRollout
    loop.segment, loop.NativeRollout = endless_segment, NativeStandIn
    try:
        yield
    finally:
        loop.segment, loop.NativeRollout = kept


def update_keywords(case, calls):
    kw = {k: case[k] for k in UPDATE_KEYS}
    kw["sampler"] = Recorder(calls, "sampler.") if case["sampler"] else None
    kw["prioritized"] = None if case["prioritized"] is None else dict(case["prioritized"])
    return kw


def outcome(case):
    """one case through loop.train (inside `no_env_loop()`)"""
    calls, evals = [], []
    agent = Agent(calls)
    env = (RecordsEnv if case.get("records_env") else Env)(calls)
    kw = update_keywords(case, calls)
    kw.update({k: case[k] for k in ROLLOUT_KEYS[:3] if k in case})
    try:
        loop.train(SimpleNamespace(**CFG), env, agent, on_eval=lambda ag, t: evals.append([t, ag.qnet_updates_so_far, ag.actor_updates_so_far]),
                   **kw)
    except Exception as ex:   # noqa: BLE001 -- the refusal IS the outcome
        return ["raises", type(ex).__name__, str(ex), calls]
    return ["runs", calls, [agent.timesteps_so_far, agent.qnet_updates_so_far, agent.actor_updates_so_far], evals]


def record(path):
    distinct, index = [], {}
    with no_env_loop():
        for grid in (GRID_A, GRID_B):
            for case in grid:
                text = json.dumps(outcome(case), sort_keys=True, separators=(",", ":"))
                if text not in distinct:
                    distinct.append(text)
                index.setdefault("grid_a" if grid is GRID_A else "grid_b", []).append(distinct.index(text))
    with open(path, "w") as f:
        f.write('{"config":' + json.dumps(CFG, separators=(",", ":")) + ',\n"grid_a":' + json.dumps(index["grid_a"], separators=(",", ":")) +
                ',\n"grid_b":' + json.dumps(index["grid_b"], separators=(",", ":")) + ',\n"outcomes":[\n' + ",\n".join(distinct) + "\n]}\n")
    return len(distinct)


def recorded():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["config"] == CFG and len(doc["grid_a"]) == len(GRID_A) == 1152 and len(doc["grid_b"]) == len(GRID_B) == 48
    return [doc["outcomes"][k] for k in doc["grid_a"]], [doc["outcomes"][k] for k in doc["grid_b"]]


def same(got, want):
    return json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)


def test_every_update_mode_reproduces_its_recorded_outcome():
    want, _ = recorded()
    with no_env_loop():
        wrong = [(n, case) for n, case in enumerate(GRID_A) if not same(outcome(case), want[n])]
    assert not wrong, (len(wrong), wrong[:3])
    assert {w[0] for w in want} == {"raises", "runs"}


def test_every_rollout_mode_reproduces_its_recorded_outcome():
    _, want = recorded()
    for n in REFUSED_BEFORE_PRIORITIES:                                # recorded with the call, expected without it
        assert want[n][0] == "raises" and [c[0] for c in want[n][3]] == ["rb.enable_priorities"], n
        want[n] = want[n][:3] + [[]]
    with no_env_loop():
        wrong = [(n, case) for n, case in enumerate(GRID_B) if not same(outcome(case), want[n])]
    assert not wrong, (len(wrong), wrong[:3])


def test_the_known_differences_are_the_refused_rollouts_of_the_prioritized_mode():
    want_a, want_b = recorded()
    assert sorted(REFUSED_BEFORE_PRIORITIES) == [n for n, case in enumerate(GRID_B) if case["prioritized"] is not None and want_b[n][0] == "raises"]
    rollout_refusals = {w[2] for n, w in enumerate(want_b) if n in REFUSED_BEFORE_PRIORITIES}
    assert all(("native_rollout" in m or "device_env" in m) for m in rollout_refusals), rollout_refusals
    # ... and only they: no other refusal anywhere was recorded behind a call
    assert all(w[3] == [] for w in want_a if w[0] == "raises")
    assert all(w[3] == [] for n, w in enumerate(want_b) if w[0] == "raises" and n not in REFUSED_BEFORE_PRIORITIES)


def test_update_plan_alone_refuses_exactly_what_train_refuses():
    want, _ = recorded()
    cfg = SimpleNamespace(**CFG)
    for n, case in enumerate(GRID_A):
        try:
            plan = loop.update_plan(cfg, **update_keywords(case, []))
            got = ["runs", int(plan.updates_per_step)]
        except Exception as ex:   # noqa: BLE001
            got = ["raises", type(ex).__name__, str(ex)]
        assert got[0] == want[n][0] and (got[0] == "runs" or got == want[n][:3]), (n, case, got, want[n][:3])
        if got[0] == "runs":
            assert got[1] == case["updates_per_step"] and callable(plan.update)
            assert (plan.priorities is not None) == (case["prioritized"] is not None)


def test_update_plan_touches_no_agent_and_needs_no_torch():
    """the launcher's parent process asks it: a config of two numbers, nothing else, and no import behind the module's own"""
    before = set(sys.modules)
    plan = loop.update_plan(SimpleNamespace(batch_size=256, num_envs=4), fused=False, sampler=None, prioritized=dict(alpha=0.7), n_step=3,
                            one_launch=True, prior_fraction=None, updates_per_step=2)
    assert plan.priorities == dict(alpha=0.7, eps=1e-6) and plan.updates_per_step == 2
    assert set(sys.modules) == before
    calls = []
    plan.update(Agent(calls), 5, {})
    assert calls == [["iteration", [5], dict(beta=0.4, n_step=3, stride=4)]]


def test_the_launcher_maps_its_flags_once_and_asks_the_plan_before_a_worker_starts(capsys):
    import inspect
    facts = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                 native_rollout=False, policy_stats=0)
    plain_run = dict(fused=True, prioritized=None, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap=False,
                     device_env=False, native_rollout=False, policy_stats=0)
    def kw(**facts):
        return launcher.train_keywords(SimpleNamespace(batch_size=8, num_envs=4), **facts)
    assert kw(**facts) == plain_run
    assert kw(**dict(facts, prioritized=True, device_env=True, native_rollout=True, policy_stats=64)) == \
        dict(plain_run, fused=False, prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6), device_env=True, native_rollout=True, policy_stats=64)
    assert kw(**dict(facts, n_step=3, one_launch=True, overlap_acting=True)) == dict(plain_run, fused=False, n_step=3, one_launch=True, overlap=True)
    assert kw(**dict(facts, prior_fraction=1, updates_per_step=4)) == dict(plain_run, fused=False, prior_fraction=1.0, updates_per_step=4)
    with pytest.raises(ValueError, match="one_launch=True needs fused=False"):      # it asks loop.update_plan on the way
        kw(**dict(facts, one_launch=True))
    args = SimpleNamespace(algo="sac", updates_per_step=None, **{k: v for k, v in facts.items() if k not in ("prior_fraction", "updates_per_step")})
    assert launcher.mode_flags(args, {}) == facts and launcher.mode_flags(args, dict(prior_fraction=0.5))["prior_fraction"] == 0.5
    assert inspect.getsource(launcher.run_job).count("loop.train(") == 1
    for argv, msg in ((["--one_launch"], "one_launch=True needs fused=False"), (["--n_step", "17"], "n_step must be in [1, 16]"),
                      (["--one_launch", "--n_step", "0"], "one_launch=True needs prioritized")):
        with pytest.raises(SystemExit) as ex:
            launcher.main(["--dry-run", "--num_seeds", "1"] + argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err


if __name__ == "__main__":
    print(record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN), "distinct outcomes")
