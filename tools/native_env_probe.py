#!/usr/bin/env python3
"""Measurements around the GPU-resident vector envs (envs.py, include/sactd3_env.h) -> profiles/native_env.json.  Nothing in the record
is a pass / fail bar of this tool; tests/test_gpu_native_env.py takes the learning tests' budget and bar from its "learning" entry.

    python tools/native_env_probe.py --oracle          # CPU, minutes: the oracle agent (oracle/sac_td3_ref.py) on envs.HostVecEnv, 3 seeds
                                                       # per task at the learning tests' budget -> "learning" (budget, per-seed returns, bar)
    python tools/native_env_probe.py                   # GPU: alternating child processes, 5 runs each, median and range ->
                                                       #   "train": loop.train(device_env=True) iterations/s on NativeVecEnv against
                                                       #            loop.SyntheticDeviceVecEnv at the same (o, a, num_envs), the same build
                                                       #   "step":  one vector step -- the launch alone (fixed buffers) and NativeVecEnv.step
                                                       #   "eval":  envs.greedy_returns on the GPU against loop.evaluate on the host twin
    python tools/native_env_probe.py --bench TREE      # GPU: this checkout's bench.py against the bench.py of another, built checkout
                                                       # (the parent commit's), alternating, 5 runs each -> "bench"
Each mode rewrites its own entries of the record and leaves the others."""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "native_env.json")
RUNS = 5
SEEDS = (0, 1, 2)
EPISODES = 16
# the learning tests' budget: SAC, default hyper-parameters, 4 envs, one iteration per vector step
LEARNING = {"pendulum": dict(num_envs=4, learning_starts=1000, updates=3500, batch_size=256),
            "cartpole": dict(num_envs=4, learning_starts=1000, updates=2000, batch_size=256)}


def learning_cfg(kind, seed, budget=None):
    """the SimpleNamespace loop.train and Agent take: launcher.DEFAULTS["sac"] with the budget's entries; no evaluation inside the run"""
    from sac_td3_cudagraphs_pytorch_amd import launcher
    b = dict(budget or LEARNING[kind])
    steps = b["learning_starts"] + b["updates"] * b["num_envs"]
    return launcher.job_config("sac", kind, seed, num_envs=b["num_envs"], learning_starts=b["learning_starts"], batch_size=b["batch_size"],
                               num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)


def merge(entries):
    rec = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rec = json.load(f)
    rec.update(entries)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "runs": len(xs)}


# ---------------------------------------------------------------------------------------------------- the oracle on the host twin
class OracleAgent:
    """oracle/sac_td3_ref.py:RefAgent behind the surface loop.train and envs.greedy_returns use: a numpy ring, uniform draws"""

    def __init__(self, kind, cfg, seed):
        import torch
        from oracle.sac_td3_ref import Hps, RefAgent
        from sac_td3_cudagraphs_pytorch_amd import envs
        o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
        torch.manual_seed(seed)
        self.ref = RefAgent(o, a, [-bound] * a, [bound] * a, Hps.sac(batch_size=cfg.batch_size))
        self.ref.keep_trace = False
        self.rng = np.random.default_rng(seed)
        self.B, self.rows, self.cursor, self.cap = cfg.batch_size, 0, 0, cfg.rb_capacity
        self.cols = {"observations": np.zeros((self.cap, o), np.float32), "actions": np.zeros((self.cap, a), np.float32),
                     "rewards": np.zeros((self.cap, 1), np.float32), "next_observations": np.zeros((self.cap, o), np.float32),
                     "dones": np.zeros((self.cap, 1), bool)}
        self.rb = self
        self.timesteps_so_far = self.qnet_updates_so_far = self.actor_updates_so_far = 0
        self.engine = SimpleNamespace(read_metrics=lambda: {}, cfg=SimpleNamespace(max_envs=1 << 20))

    def extend(self, td):
        n = len(td["rewards"])
        at = (self.cursor + np.arange(n)) % self.cap
        for k, col in self.cols.items():
            col[at] = np.asarray(td[k]).reshape(n, -1)
        self.cursor, self.rows = (self.cursor + n) % self.cap, min(self.cap, self.rows + n)

    def predict(self, td, *, explore):
        return self.ref.predict(td["observations"], explore=explore)

    def iteration(self, i):
        at = self.rng.integers(0, self.rows, self.B)
        c = self.cols
        self.ref.iteration(self.ref.to_batch(c["observations"][at], c["actions"][at], c["rewards"][at], c["next_observations"][at], c["dones"][at]), i)
        self.qnet_updates_so_far += 1


def oracle_run(kind, seed):
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    cfg = learning_cfg(kind, seed)
    agent = OracleAgent(kind, cfg, seed)
    eval_env = envs.HostVecEnv(kind, EPISODES, seed=seed + 1000)
    before = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    t0 = time.time()
    loop.train(cfg, envs.HostVecEnv(kind, cfg.num_envs, seed=seed), agent)
    after = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    return {"seed": seed, "untrained": float(before), "trained": float(after), "updates": agent.qnet_updates_so_far, "seconds": time.time() - t0}


def oracle_mode():
    out = {"what": "oracle.sac_td3_ref.RefAgent (SAC, default hyper-parameters) trained by loop.train on envs.HostVecEnv; greedy return by "
                   f"envs.greedy_returns over {EPISODES} envs for one horizon, before and after.  bar = midpoint between the worst trained and "
                   "the best untrained seed; a task keeps its learning test only if every seed clears the bar by a quarter of that gap",
           "episodes": EPISODES, "eval_seed_offset": 1000, "tasks": {}}
    for kind in LEARNING:
        runs = [oracle_run(kind, s) for s in SEEDS]
        worst, best = min(r["trained"] for r in runs), max(r["untrained"] for r in runs)
        gap = worst - best
        out["tasks"][kind] = {"budget": LEARNING[kind], "seeds": runs, "worst_trained": worst, "best_untrained": best,
                              "bar": 0.5 * (worst + best), "margin_needed": 0.25 * gap,
                              "test_kept": bool(gap > 0 and all(r["trained"] - 0.5 * (worst + best) >= 0.25 * gap for r in runs))}
        print(kind, json.dumps(out["tasks"][kind]), flush=True)
    merge({"learning": out})


# ---------------------------------------------------------------------------------------------------- GPU children: one measurement each
def child_train(kind, which):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs, loop
    cfg = learning_cfg(kind, 0, dict(num_envs=4, learning_starts=1000, updates=3000, batch_size=256))
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    dev = torch.device("cuda", 0)
    env = envs.NativeVecEnv(kind, cfg.num_envs, seed=0, device=dev) if which == "native" else \
        loop.SyntheticDeviceVecEnv(o, a, cfg.num_envs, horizon=200, term_at=6.0, bound=bound, device=dev)
    torch.manual_seed(0)
    agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), dev, cfg,
                  ReplayBuffer(cfg.rb_capacity), seed=0)
    warm = learning_cfg(kind, 0, dict(num_envs=4, learning_starts=1000, updates=200, batch_size=256))
    loop.train(warm, env, agent, device_env=True)          # graphs instantiated, allocator warm; the counters go on from here
    agent.engine.sync()
    u0, t0 = agent.qnet_updates_so_far, time.perf_counter()
    cfg.num_timesteps += agent.timesteps_so_far
    loop.train(cfg, env, agent, device_env=True)
    agent.engine.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"iterations_per_s": (agent.qnet_updates_so_far - u0) / dt, "iterations": agent.qnet_updates_so_far - u0}


def child_step(kind, n):
    import ctypes as C
    import torch
    from sac_td3_cudagraphs_pytorch_amd import _lib, envs
    env = envs.NativeVecEnv(kind, n, seed=0)
    obs, _ = env.reset()
    act = env.action_space.sample()
    out = _lib.CEnvOut(obs.data_ptr(), obs.stride(0), None, 0, None, 0, None, 0, None, 0, None, 0)
    st = env._stream()
    reps = 2000
    res = {}
    for name, body in (("launch_only", lambda: env._call("sactd3_env_step", act.data_ptr(), act.stride(0), C.byref(out), st)),
                       ("env_step", lambda: env.step(act))):
        for _ in range(200):
            body()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            body()
        e1.record()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        res[name] = {"device_us_per_step": 1e3 * e0.elapsed_time(e1) / reps, "host_issue_us_per_step": 1e6 * host / reps}
    return res


def child_eval(kind, which):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs, loop
    cfg = learning_cfg(kind, 0)
    cfg.num_envs = EPISODES                                  # (max_envs of the engine: one predict call per step)
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), dev, cfg,
                  ReplayBuffer(1024), seed=0)
    if which == "native":
        env = envs.NativeVecEnv(kind, EPISODES, seed=5, device=dev)
        envs.greedy_returns(env, agent, EPISODES)
        t0 = time.perf_counter()
        got = envs.greedy_returns(env, agent, EPISODES)
    else:
        ev = SimpleNamespace(seed=5, num_episodes=EPISODES)
        env = envs.HostVecEnv(kind, 1, seed=5)
        loop.evaluate(SimpleNamespace(seed=5, num_episodes=2), env, agent)
        t0 = time.perf_counter()
        got = loop.evaluate(ev, env, agent)
    return {"seconds": time.perf_counter() - t0, "episodes": EPISODES, "return": float(got["return"])}


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "200"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


CHILDREN = {"train": child_train, "step": child_step, "eval": child_eval}


def run_child(*argv, timeout=300):
    """a fresh process per measurement; -> its JSON.  A child that fails ends the whole probe: nothing more is started on the GPU."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *map(str, argv)], capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def gpu_mode(runs):
    rec = {"train": {}, "step": {}, "eval": {}}
    for kind in LEARNING:
        got = {"native": [], "synthetic": []}
        for _ in range(runs):
            for which in got:                                # alternating: native, synthetic, native, ...
                got[which].append(run_child("train", kind, which)["iterations_per_s"])
        rec["train"][kind] = {"what": "loop.train(device_env=True), SAC, 4 envs, B 256, 3000 iterations behind a 200-iteration warm-up: iterations/s",
                              **{k: spread(v) for k, v in got.items()}}
        print("train", kind, json.dumps(rec["train"][kind]), flush=True)
        ev = {"native": [], "host": []}
        for _ in range(runs):
            for which in ev:
                ev[which].append(run_child("eval", kind, which)["seconds"])
        rec["eval"][kind] = {"what": f"{EPISODES} greedy episodes: envs.greedy_returns on the GPU (one host wait) against loop.evaluate on a "
                                     "one-env HostVecEnv (a predict round trip per step): seconds", **{k: spread(v) for k, v in ev.items()}}
        print("eval", kind, json.dumps(rec["eval"][kind]), flush=True)
        for n in (4, 4096):
            runs_n = [run_child("step", kind, n) for _ in range(runs)]
            rec["step"][f"{kind}-{n}"] = {f"{name}.{fig}": spread([r[name][fig] for r in runs_n]) for name in ("launch_only", "env_step")
                                          for fig in ("device_us_per_step", "host_issue_us_per_step")}
            print("step", kind, n, json.dumps(rec["step"][f"{kind}-{n}"]), flush=True)
    merge(rec)


def bench_mode(other, runs):
    got = {"this": [], "other": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["other"].append(child_bench(other))
    keys = [k for k in ("value", "ms_per_step") if k in got["this"][0]]
    merge({"bench": {"what": "bench.py --gpus 1 --steps 2000 --warmup 200 of this checkout and of the parent commit's, alternating processes",
                     **{side: {k: spread([r[k] for r in rs]) for k in keys} for side, rs in got.items()}}})
    print(json.dumps({side: {k: spread([r[k] for r in rs])["median"] for k in keys} for side, rs in got.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.child:
        kind_args = [int(x) if x.isdigit() else x for x in args.child[1:]]
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](*kind_args)), flush=True)
    elif args.oracle:
        oracle_mode()
    elif args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs)
    else:
        gpu_mode(args.runs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
