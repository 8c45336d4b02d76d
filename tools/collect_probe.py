#!/usr/bin/env python3
"""Measurements around the collected rollout segment (loop.NativeRollout.collect, loop.train(collected_rollout=True),
include/sactd3_rollout_collect.h) -> profiles/collect.json, by the method of tools/rollout_cycle_probe.py: one fresh process per
measurement, the sides alternating, 5 runs each, median / min / max.  Nothing in the record is a pass / fail bar of this tool;
tests/test_gpu_collect.py takes its learning test's budget and bar from the "learning" entry.  "faster" is said of a configuration
only where the new median lies beyond the parent's BEST run.

    python tools/collect_probe.py --oracle          # CPU, minutes: the oracle agent (oracle/sac_td3_ref.py) on envs.HostVecEnv("pendulum")
                                                    # under the collect-then-update schedule -- a segment of segment_len steps chosen with
                                                    # the parameters in front of it, then updates_per_step updates -- 3 seeds -> "learning":
                                                    # budget, per-seed greedy returns, bar = worst seed - (best seed - worst seed)
    python tools/collect_probe.py --parent TREE     # GPU.  TREE: a built checkout of the parent commit
        "step"   (--only step)  device time and host issue time per ENV STEP, microseconds: collect(T) for T in 1, 8, 64 at 4 and 4096 envs,
                 the three tasks, RANDOM and EXPLORE, against T x (choose, advance) on the parent's build
        "train"  (--only train)  loop.train iterations/s, SAC, 4 envs, B 256, segment_len 8, updates_per_step 8: this build with
                 collected_rollout=True against the parent's native_rollout=True run with the same keywords
        "train_on_engine_stream"  (--only engine_stream)  the same with the ENGINE's stream as torch's current stream around loop.train
    python tools/collect_probe.py --bench TREE      # GPU: this checkout's bench.py against TREE's, alternating, 3 runs a build -> "bench"
Each mode rewrites its own entries of the record and leaves the others."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "collect.json")
RUNS = 5
KINDS = ("pendulum", "cartpole", "pointgoal")
STEP_TS = (1, 8, 64)
STEP_NS = (4, 4096)
STEP_REPS = {1: 600, 8: 100, 64: 16}          # calls per timed run: about a thousand env steps each
MODES = {"random": 0, "explore": 1}           # SACTD3_ROLLOUT_RANDOM / _EXPLORE
SEEDS = (0, 1, 2)
EPISODES = 16
# the learning test's budget: SAC, default hyper-parameters, the 3 500 updates of the pendulum test of tests/test_gpu_native_env.py
LEARNING = dict(kind="pendulum", num_envs=4, learning_starts=1000, updates=3500, batch_size=256, segment_len=4, updates_per_step=4)


def merge(entries):
    rec = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rec = json.load(f)
    for k, v in entries.items():
        rec[k] = {**rec.get(k, {}), **v} if isinstance(v, dict) and isinstance(rec.get(k), dict) else v
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "runs": len(xs)}


def train_cfg(kind, seed, num_envs, updates, learning_starts=1000, batch_size=256, segment_len=1, updates_per_step=1, cap=1 << 15):
    """the config of a run of `updates` updates behind `learning_starts` steps: updates / updates_per_step bodies of segment_len vector steps"""
    from sac_td3_cudagraphs_pytorch_amd import launcher
    steps = learning_starts + (updates // updates_per_step) * segment_len * num_envs
    return launcher.job_config("sac", kind, seed, num_envs=num_envs, learning_starts=learning_starts, batch_size=batch_size,
                               num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=cap, segment_len=segment_len)


def new_agent(kind, cfg):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    torch.manual_seed(0)
    return Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device("cuda", 0), cfg,
                 ReplayBuffer(cfg.rb_capacity), seed=0)


# ---------------------------------------------------------------------------------------------------- the oracle under the schedule
def oracle_run(seed):
    """collect-then-update on the host: every segment's actions come from the parameters in front of it (the random draw while
    timesteps_so_far < learning_starts), then updates_per_step updates -- the loop body of loop.train(collected_rollout=True)"""
    from native_env_probe import OracleAgent
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    b = LEARNING
    cfg = train_cfg(b["kind"], seed, b["num_envs"], b["updates"], b["learning_starts"], b["batch_size"], b["segment_len"], b["updates_per_step"])
    agent = OracleAgent(b["kind"], cfg, seed)
    eval_env = envs.HostVecEnv(b["kind"], EPISODES, seed=seed + 1000)
    before = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    t0 = time.time()
    ro = loop.Rollout(envs.HostVecEnv(b["kind"], cfg.num_envs, seed=seed), agent, seed, cfg.learning_starts, 1)
    i = 0
    while agent.timesteps_so_far <= cfg.num_timesteps:
        for _ in range(cfg.segment_len):                   # (timesteps_so_far stands still inside a segment: one mode per segment)
            ro.choose()
            ro.advance()
        agent.timesteps_so_far += cfg.segment_len * cfg.num_envs
        if agent.timesteps_so_far <= cfg.learning_starts:
            i += 1
            continue
        for _ in range(b["updates_per_step"]):
            agent.iteration(i)
            i += 1
    after = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    return {"seed": seed, "untrained": float(before), "trained": float(after), "updates": agent.qnet_updates_so_far, "seconds": time.time() - t0}


def oracle_mode():
    # (two threads a child: three children with a thread per core each only get in each other's way)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="2", MKL_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--oracle-child", str(s)], stdout=subprocess.PIPE, text=True, env=env)
             for s in SEEDS]
    runs = []
    for p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise SystemExit(out[-2000:])
        runs.append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    worst, best = min(r["trained"] for r in runs), max(r["trained"] for r in runs)
    out = {"what": "oracle.sac_td3_ref.RefAgent (SAC, default hyper-parameters) on envs.HostVecEnv under the collect-then-update schedule; greedy "
                   f"return by envs.greedy_returns over {EPISODES} envs for one horizon, before and after.  bar = worst_trained - spread, spread "
                   "= max - min of the three seeds' trained returns",
           "episodes": EPISODES, "eval_seed_offset": 1000, "budget": LEARNING, "seeds": runs, "worst_trained": worst, "best_trained": best,
           "spread": best - worst, "bar": worst - (best - worst), "best_untrained": max(r["untrained"] for r in runs)}
    merge({"learning": out})
    print(json.dumps(out), flush=True)


# ---------------------------------------------------------------------------------------------------- GPU children: one measurement each
def child_step(kind, n, side):
    """side "collect": collect(T, mode); side "calls": T x (choose(mode), advance) -- the only one a parent tree has.  Per (mode, T):
    device time between two events on the rollout's stream and host issue time, both per env step, behind a warm-up and a wait"""
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    dev = torch.device("cuda", 0)
    cfg = train_cfg(kind, 0, n, 0, learning_starts=0, cap=max(1 << 15, 64 * n))
    agent = new_agent(kind, cfg)
    env = envs.NativeVecEnv(kind, n, seed=0, device=dev)
    ro = loop.NativeRollout(env, agent, 0, 0, 1)
    lib, h = ro._lib, ro._h
    settle = lambda: (torch.cuda.synchronize(), agent.engine.sync())
    res = {}
    for mode_name, mode in MODES.items():
        for T in STEP_TS:
            if side == "collect":
                def call():
                    ro.collect(T, mode)
            else:
                def call():
                    for _ in range(T):
                        rc = lib.sactd3_rollout_choose(h, mode) or lib.sactd3_rollout_advance(h)
                        if rc:
                            raise SystemExit(f"rollout call failed ({rc})")
            reps = STEP_REPS[T]
            for _ in range(max(2, reps // 10)):
                call()
            settle()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            host = time.perf_counter() - t0
            settle()
            res[f"{mode_name}_T{T}"] = {"device_us": 1e3 * e0.elapsed_time(e1) / (reps * T), "host_us": 1e6 * host / (reps * T)}
    ro.close()
    return res


def child_train(kind, which, stream="torch"):
    """which: "collected" (collected_rollout=True) or "native" (the call sequence; the only one a parent tree has); stream "engine":
    torch's current stream is the engine's own while the loop runs"""
    import contextlib
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    more = dict(native_rollout=True, updates_per_step=8, **(dict(collected_rollout=True) if which == "collected" else {}))
    cfg = train_cfg(kind, 0, 4, 4000, segment_len=8, updates_per_step=8)
    env = envs.NativeVecEnv(kind, cfg.num_envs, seed=0, device=torch.device("cuda", 0))
    agent = new_agent(kind, cfg)
    on = torch.cuda.stream(torch.cuda.ExternalStream(agent.engine.device_handles()[0])) if stream == "engine" else contextlib.nullcontext()
    with on:
        loop.train(train_cfg(kind, 0, 4, 400, segment_len=8, updates_per_step=8), env, agent, device_env=True, **more)      # graphs, allocator
        agent.engine.sync()
        u0, t0 = agent.qnet_updates_so_far, time.perf_counter()
        cfg.num_timesteps += agent.timesteps_so_far
        loop.train(cfg, env, agent, device_env=True, **more)
        agent.engine.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"iterations_per_s": (agent.qnet_updates_so_far - u0) / dt, "iterations": agent.qnet_updates_so_far - u0}


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "3000", "--warmup", "300"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


CHILDREN = {"step": child_step, "train": child_train}


def run_child(tree, *argv, timeout=300):
    """a fresh process per measurement, importing the package of `tree`; -> its JSON.  A child that fails ends the whole probe:
    nothing more is started on the GPU."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", *map(str, argv)], capture_output=True, text=True,
                         timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} in {tree} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def step_group(parent, runs):
    what = ("microseconds per ENV STEP (one step of all n envs), device time between two events on the rollout's stream and host issue time: "
            "collect = NativeRollout.collect(T, mode) of this build, parent_calls = T x (choose(mode), advance) of the parent commit's build; "
            "collect_below_parent_min: the collected median lies below the parent's best run")
    for kind in KINDS:
        for n in STEP_NS:
            got = {"collect": [], "parent_calls": []}
            for _ in range(runs):                                          # alternating
                got["collect"].append(run_child(ROOT, "step", kind, n, "collect"))
                got["parent_calls"].append(run_child(parent, "step", kind, n, "calls"))
            entry = {}
            for case in got["collect"][0]:
                row = {side: {k: spread([r[case][k] for r in rs]) for k in ("device_us", "host_us")} for side, rs in got.items()}
                row["collect_below_parent_min"] = {k: bool(row["collect"][k]["median"] < row["parent_calls"][k]["min"]) for k in ("device_us", "host_us")}
                entry[case] = row
            merge({"step": {"what": what, f"{kind}_n{n}": entry}})
            print("step", kind, n, json.dumps(entry), flush=True)


def train_group(parent, runs, stream, key, what):
    for kind in KINDS:
        sides = {"collected_rollout": (ROOT, "collected"), "parent_native_rollout": (parent, "native")}
        got = {k: [] for k in sides}
        for _ in range(runs):
            for k, (tree, which) in sides.items():                     # alternating
                got[k].append(run_child(tree, "train", kind, which, stream)["iterations_per_s"])
        entry = {k: spread(v) for k, v in got.items()}
        entry["collected_above_parent_max"] = bool(entry["collected_rollout"]["median"] > entry["parent_native_rollout"]["max"])
        merge({key: {"what": what, kind: entry}})
        print(key, kind, json.dumps(entry), flush=True)


def gpu_mode(parent, runs, only):
    if only in (None, "step"):
        step_group(parent, runs)
    if only in (None, "train"):
        train_group(parent, runs, "torch", "train",
                    "loop.train(device_env=True, native_rollout=True, updates_per_step=8) on NativeVecEnv, SAC, 4 envs, B 256, segment_len 8, 4000 "
                    "iterations behind a 400-iteration warm-up: iterations/s; collected_rollout: this build with collected_rollout=True; "
                    "parent_native_rollout: the parent commit's build")
    if only in (None, "engine_stream"):
        train_group(parent, runs, "engine", "train_on_engine_stream",
                    "the train figures with the engine's stream as torch's current stream around loop.train: the env's kernels and the "
                    "engine's on one stream (the stronger baseline)")


def bench_mode(other, runs):
    got = {"this": [], "parent": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["parent"].append(child_bench(other))
    keys = [k for k in ("value", "ms_per_step") if k in got["this"][0]]
    entry = {"what": "bench.py --gpus 1 --steps 3000 --warmup 300 of this checkout and of the parent commit's, alternating processes",
             **{side: {k: spread([r[k] for r in rs]) for k in keys} for side, rs in got.items()}}
    merge({"bench": entry})
    print(json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-child", type=int, default=None, metavar="SEED")
    ap.add_argument("--parent", default=None, metavar="TREE")
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--only", default=None, choices=["step", "train", "engine_stream"])
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.oracle_child is not None:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        print("RESULT " + json.dumps(oracle_run(args.oracle_child)), flush=True)
    elif args.oracle:
        oracle_mode()
    elif args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        kind_args = [int(x) if x.isdigit() else x for x in args.child[1:]]
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](*kind_args)), flush=True)
    elif args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs or 3)
    elif args.parent:
        gpu_mode(os.path.abspath(args.parent), args.runs or RUNS, args.only)
    else:
        ap.error("--oracle, --parent TREE or --bench TREE")
    return 0


if __name__ == "__main__":
    sys.exit(main())
