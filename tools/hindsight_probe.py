#!/usr/bin/env python3
"""The learning record of hindsight replay -> profiles/hindsight.json.  Nothing in the record is a pass / fail bar of this tool;
tests/test_gpu_hindsight.py takes its learning test's budget and the oracle's figures from the "learning" entry.

    python tools/hindsight_probe.py --oracle     # CPU, minutes: the oracle agent (oracle/sac_td3_ref.py) on envs.HostVecEnv("pointgoal") with
                                                 # tests/hindsight_ref.py as its sampler, 3 seeds in parallel child processes at the learning
                                                 # test's budget, and one run at the same budget without hindsight -> "learning"

    python tools/hindsight_probe.py              # GPU: alternating child processes, 5 runs each, median and range ->
                                                 #   "stage": time per staging call at the PointGoal shape, B = 256 -- the hindsight kernel at
                                                 #            window 1, 16 and 50 against k_batch_from_index and the n-step kernel (3 steps)
                                                 #   "loop":  loop.train(device_env=True, fused=False) iterations/s with and without hindsight
                                                 #   "gpu_learning": the learning test's run with and without hindsight (recorded, not asserted)

    python tools/hindsight_probe.py --one-launch [--parent-library PATH]
                                                 # GPU -> profiles/hindsight_one_launch.json (a file of its own: hindsight.json stays):
                                                 #   "loop":  the hindsight loop of the shape above, iterations/s, as one graph launch per
                                                 #            iteration (one_launch=True), call by call with this build and, with PATH (a
                                                 #            libsactd3_hip.so built from the parent commit), call by call with that build --
                                                 #            alternating child processes, 5 runs each, median and range, and the ratios
    python tools/hindsight_probe.py --kernel-stats STATS.csv
                                                 # -> "kernel_us" of the same file: the per-launch device time of the two kernels the graph
                                                 #    adds, read from the kernel statistics of a profiled run of the one-launch loop,
                                                 #      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
                                                 #          python tools/hindsight_probe.py --child loop 1 1
Each mode rewrites its own entries of its record and leaves the others."""
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
OUT = os.path.join(ROOT, "profiles", "hindsight.json")
ONE_LAUNCH_OUT = os.path.join(ROOT, "profiles", "hindsight_one_launch.json")
SEEDS = (0, 1, 2)
EPISODES = 16
KIND = "pointgoal"
# the learning test's budget: SAC, default hyper-parameters, 4 envs, one iteration per vector step (the cap is 20 000 updates)
BUDGET = dict(num_envs=4, learning_starts=1000, updates=4000, batch_size=256)
RATIO = 0.8


def learning_cfg(seed, budget=None):
    from sac_td3_cudagraphs_pytorch_amd import launcher
    b = dict(budget or BUDGET)
    steps = b["learning_starts"] + b["updates"] * b["num_envs"]
    return launcher.job_config("sac", "PointGoal-native", seed, num_envs=b["num_envs"], learning_starts=b["learning_starts"],
                               batch_size=b["batch_size"], num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)


class OracleAgent:
    """oracle/sac_td3_ref.py:RefAgent behind the surface loop.train and envs.greedy_returns use: a numpy ring indexed by slot, uniform
    start rows, and -- with `hindsight` -- tests/hindsight_ref.stage as the sampler (the rule the engine's kernel is held to)"""

    def __init__(self, cfg, seed, hindsight):
        import torch
        from oracle.sac_td3_ref import Hps, RefAgent
        from sac_td3_cudagraphs_pytorch_amd import envs
        kind = envs.kind_of(KIND)
        o, a, bound, horizon = envs.SPECS[kind][:4]
        torch.manual_seed(seed)
        self.ref = RefAgent(o, a, [-bound] * a, [bound] * a, Hps.sac(batch_size=cfg.batch_size))
        self.ref.keep_trace = False
        self.rng = np.random.default_rng(seed)
        self.seed, self.draws = seed, 0
        self.hs = dict(envs.GOAL_LAYOUTS[kind], ratio=RATIO, window=horizon, stride=cfg.num_envs) if hindsight else None
        self.B, self.rows, self.cursor, self.cap = cfg.batch_size, 0, 0, cfg.rb_capacity
        self.cols = {"observations": np.zeros((self.cap, o), np.float32), "actions": np.zeros((self.cap, a), np.float32),
                     "rewards": np.zeros((self.cap, 1), np.float32), "next_observations": np.zeros((self.cap, o), np.float32),
                     "dones": np.zeros((self.cap, 1), bool)}
        self.rb = self
        self.timesteps_so_far = self.qnet_updates_so_far = self.actor_updates_so_far = 0
        self.relabelled = 0
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
        from tests import hindsight_ref as hr
        at = self.rng.integers(0, self.rows, self.B)
        c = self.cols
        if self.hs is None:
            batch = (c["observations"][at], c["actions"][at], c["rewards"][at], c["next_observations"][at], c["dones"][at])
        else:
            fields = dict(obs=c["observations"], act=c["actions"], nobs=c["next_observations"], rew=c["rewards"].reshape(-1),
                          done=c["dones"].reshape(-1).astype(np.float32))
            got = hr.stage(fields, dict(length=self.rows, cursor=self.cursor, cap=self.cap), at, self.hs, seed=self.seed, hctr=self.draws)
            self.draws += 1
            self.relabelled += int((got["offset"] >= 0).sum())
            batch = (got["obs"], got["act"], got["rew"].reshape(-1, 1), got["nobs"], (got["done"] != 0).reshape(-1, 1))
        self.ref.iteration(self.ref.to_batch(*batch), i)
        self.qnet_updates_so_far += 1


def oracle_run(seed, hindsight):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    torch.set_num_threads(1)                              # (four children side by side: one thread each, no oversubscription)
    cfg = learning_cfg(seed)
    agent = OracleAgent(cfg, seed, hindsight)
    eval_env = envs.HostVecEnv(KIND, EPISODES, seed=seed + 1000)
    before = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    t0 = time.time()
    loop.train(cfg, envs.HostVecEnv(KIND, cfg.num_envs, seed=seed), agent)
    after = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    return {"seed": seed, "hindsight": bool(hindsight), "untrained": float(before), "trained": float(after), "updates": agent.qnet_updates_so_far,
            "rows_relabelled": agent.relabelled, "seconds": time.time() - t0}


def oracle_mode():
    jobs = [(s, 1) for s in SEEDS] + [(SEEDS[0], 0)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--oracle-child", str(s), str(h)], stdout=subprocess.PIPE, text=True, env=env,
                              cwd=ROOT) for s, h in jobs]
    runs = []
    for p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise SystemExit(f"an oracle child failed ({p.returncode})")
        runs.append(json.loads(out.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]), flush=True)
    with_h, without = [r for r in runs if r["hindsight"]], [r for r in runs if not r["hindsight"]]
    worst, best = min(r["trained"] for r in with_h), max(r["trained"] for r in with_h)
    rec = {"what": "oracle.sac_td3_ref.RefAgent (SAC, default hyper-parameters) trained by loop.train on envs.HostVecEnv('pointgoal') with "
                   f"tests/hindsight_ref.stage as its sampler (ratio {RATIO}, window = the horizon); greedy return by envs.greedy_returns over "
                   f"{EPISODES} envs for one horizon (-n: n steps off the goal), before and after.  The GPU test passes at or above "
                   "worst_trained - spread, spread = max - min of the three seeds; the run without hindsight is recorded, not asserted",
           "episodes": EPISODES, "eval_seed_offset": 1000, "budget": BUDGET, "ratio": RATIO, "seeds": with_h, "worst_trained": worst,
           "best_trained": best, "spread": best - worst, "pass_at": worst - (best - worst), "without_hindsight": without,
           "oracle_learned": bool(worst > max(r["untrained"] for r in with_h) + 5.0)}
    merge({"learning": rec})


def merge(entries):
    full = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            full = json.load(f)
    full.update(entries)
    with open(OUT, "w") as f:
        json.dump(full, f, indent=1)
        f.write("\n")


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "runs": len(xs)}


# ---------------------------------------------------------------------------------------------------- GPU children: one measurement each
RUNS = 5
STAGE_CALLS = 2000
STAGE_KINDS = ("index", "nstep3", "hindsight1", "hindsight16", "hindsight50")


def gpu_agent(cfg, seed, max_envs=None):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer
    wide = cfg if max_envs is None else SimpleNamespace(**dict(vars(cfg), num_envs=max_envs))      # (max_envs: the evaluation's rows in one call)
    torch.manual_seed(seed)
    return Agent({"ob_shape": (6,), "ac_shape": (2,)}, np.full(2, -1.0, np.float32), np.full(2, 1.0, np.float32), torch.device("cuda", 0), wide,
                 ReplayBuffer(wide.rb_capacity), seed=seed)


def hindsight_kw(env, n):
    return dict(env.goal_layout, ratio=RATIO, window=env.horizon, stride=n)


def child_stage(which):
    """seconds per staging call: STAGE_CALLS calls issued back to back on a ring of 8000 rows of the goal env, one wait at the end
    (host issue and device time together: the calls are launch-bound)"""
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    cfg = learning_cfg(0, dict(num_envs=4, learning_starts=8000, updates=0, batch_size=256))
    agent = gpu_agent(cfg, 0)
    env = envs.NativeVecEnv(KIND, 4, seed=0, device=torch.device("cuda", 0))
    ro = loop.DeviceRollout(env, agent, 0, cfg.learning_starts, 1)
    for _ in range(2000):
        ro.choose()
        ro.advance()
    rb, eng = agent.rb, agent.engine
    idx = torch.randint(0, len(rb), (256,), device="cuda")
    if which.startswith("hindsight"):
        rb.configure_hindsight(**dict(hindsight_kw(env, 4), window=int(which[len("hindsight"):])))
        call = lambda: rb.sample_hindsight_at(idx)
    elif which == "nstep3":
        call = lambda: rb.sample_at(idx, n_step=3, stride=4)
    else:
        call = lambda: rb.sample_at(idx)
    for _ in range(200):
        call()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(STAGE_CALLS):
        call()
    eng.sync()
    return (time.perf_counter() - t0) / STAGE_CALLS


def child_loop(hindsight, one_launch=False):
    """iterations per second of loop.train(device_env=True, fused=False) on the goal env, behind a warm-up run"""
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    budget = dict(num_envs=4, learning_starts=1000, updates=3000, batch_size=256)
    cfg, warm = learning_cfg(0, budget), learning_cfg(0, dict(budget, updates=200))
    agent = gpu_agent(cfg, 0)
    env = envs.NativeVecEnv(KIND, 4, seed=0, device=torch.device("cuda", 0))
    kw = dict(hindsight=hindsight_kw(env, 4), one_launch=bool(one_launch)) if hindsight else {}
    loop.train(warm, env, agent, device_env=True, fused=False, **kw)
    agent.engine.sync()
    done = agent.qnet_updates_so_far
    t0 = time.perf_counter()
    loop.train(cfg, env, agent, device_env=True, fused=False, **kw)
    agent.engine.sync()
    return (agent.qnet_updates_so_far - done) / (time.perf_counter() - t0)


def child_learn(seed, hindsight):
    """the learning test's run (tests/test_gpu_hindsight.py), with or without hindsight"""
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    cfg = learning_cfg(seed)
    agent = gpu_agent(cfg, seed, max_envs=EPISODES)
    dev = torch.device("cuda", 0)
    eval_env = envs.NativeVecEnv(KIND, EPISODES, seed=seed + 1000, device=dev)
    before = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    env = envs.NativeVecEnv(KIND, cfg.num_envs, seed=seed, device=dev)
    loop.train(cfg, env, agent, device_env=True, fused=False, **(dict(hindsight=hindsight_kw(env, cfg.num_envs)) if hindsight else {}))
    after = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    return {"seed": seed, "hindsight": bool(hindsight), "untrained": float(before), "trained": float(after), "updates": agent.qnet_updates_so_far}


def kernel_stats_mode(path):
    """the rows of a rocprofv3 kernel-statistics file that name a hindsight kernel or the draw it replaces -> the "kernel_us" entry"""
    import csv
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "hindsight" in r["Name"] or "k_mix_draw" in r["Name"]]
    rec = {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                          "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
           for r in rows}
    rec["what"] = ("device time per launch from the kernel statistics of a profiled one-launch hindsight loop (PointGoal-native, 4 envs, B = 256, "
                   "window 50, the ring growing from 1000 rows): every launch of the run, warm-up included")
    global OUT
    OUT = ONE_LAUNCH_OUT
    merge({"kernel_us": rec})
    print(json.dumps({"kernel_us": rec}), flush=True)


def run_child(*argv, library=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    if library:                                                           # (another build of the library: _lib.library_path)
        env["SACTD3_LIBRARY"] = os.path.abspath(library)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in argv], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def gpu_mode():
    stage = {k: [] for k in STAGE_KINDS}
    loops = {"plain": [], "hindsight": []}
    for _ in range(RUNS):                                                 # alternating: every kind once per round
        for k in STAGE_KINDS:
            stage[k].append(run_child("stage", k))
        loops["plain"].append(run_child("loop", 0))
        loops["hindsight"].append(run_child("loop", 1))
    learn = [run_child("learn", s, h) for s in SEEDS for h in (1, 0)]
    merge({"stage": {"what": f"microseconds per staging call, {STAGE_CALLS} calls back to back and one wait (host issue + device), PointGoal shape, "
                             "B = 256, ring of 8000 rows: rb.sample_at (k_batch_from_index), n_step = 3, and sample_hindsight_at at window 1, 16, 50",
                     **{k: spread([1e6 * x for x in v]) for k, v in stage.items()}},
           "loop": {"what": "iterations/s of loop.train(device_env=True, fused=False) on PointGoal-native, 4 envs, B = 256, 3000 updates behind a warm-up",
                    **{k: spread(v) for k, v in loops.items()}},
           "gpu_learning": {"what": "the learning test's run on the GPU, budget as in `learning`; recorded, not asserted", "runs": learn}})
    print(json.dumps({"stage": {k: spread([1e6 * x for x in v]) for k, v in stage.items()}, "loop": {k: spread(v) for k, v in loops.items()},
                      "gpu_learning": learn}), flush=True)


def one_launch_mode(parent_library):
    kinds = {"one_launch": ("loop", 1, 1), "call_by_call": ("loop", 1, 0)}
    loops = {k: [] for k in list(kinds) + (["call_by_call_parent"] if parent_library else [])}
    for _ in range(RUNS):                                                 # alternating: every kind once per round
        for k, argv in kinds.items():
            loops[k].append(run_child(*argv))
        if parent_library:
            loops["call_by_call_parent"].append(run_child("loop", 1, 0, library=parent_library))
    rec = {k: spread(v) for k, v in loops.items()}
    base = rec.get("call_by_call_parent", rec["call_by_call"])
    rec["what"] = ("iterations/s of loop.train(device_env=True, fused=False, hindsight=...) on PointGoal-native, 4 envs, B = 256, 3000 updates behind "
                   "a warm-up: one_launch=True, call by call with this build, call by call with the parent commit's build")
    rec["ratio_to_parent_median"] = rec["one_launch"]["median"] / base["median"]
    rec["parent_spread"] = (base["max"] - base["min"]) / base["median"]
    rec["one_launch_median_clears_parent_best"] = bool(rec["one_launch"]["median"] > base["max"])
    out = {"loop": rec}
    global OUT
    OUT = ONE_LAUNCH_OUT
    merge(out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-child", nargs=2, type=int, metavar=("SEED", "HINDSIGHT"))
    ap.add_argument("--child", nargs="+", metavar="WHAT")
    ap.add_argument("--one-launch", action="store_true")
    ap.add_argument("--parent-library", default=None, metavar="PATH")
    ap.add_argument("--kernel-stats", default=None, metavar="STATS.csv")
    args = ap.parse_args()
    if args.oracle_child:
        print(json.dumps(oracle_run(args.oracle_child[0], bool(args.oracle_child[1]))), flush=True)
    elif args.child:
        what, rest = args.child[0], args.child[1:]
        if what == "loop":
            got = child_loop(bool(int(rest[0])), bool(int(rest[1])) if len(rest) > 1 else False)
        else:
            got = child_stage(rest[0]) if what == "stage" else child_learn(int(rest[0]), bool(int(rest[1])))
        print(json.dumps(got), flush=True)
    elif args.oracle:
        oracle_mode()
    elif args.one_launch:
        one_launch_mode(args.parent_library)
    elif args.kernel_stats:
        kernel_stats_mode(args.kernel_stats)
    else:
        gpu_mode()
