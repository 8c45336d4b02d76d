#!/usr/bin/env python3
"""Measurements around the rollout cycle (loop.NativeRollout.cycle, loop.train(fused_rollout=True), include/sactd3_rollout_cycle.h) ->
profiles/rollout_cycle.json, by the method of tools/native_rollout_probe.py: one fresh process per measurement, the sides alternating,
5 runs each, median / min / max.  Nothing in the record is a pass / fail bar; "faster" is said of a configuration only where the new
median lies above the parent's BEST run (`fused_above_parent_max`).

    python tools/rollout_cycle_probe.py --parent TREE   # GPU.  TREE: a built checkout of the parent commit
        "train"    loop.train(device_env=True, native_rollout=True), SAC, 4 envs, B 256, iterations/s on the pendulum, the cart-pole and
                   the goal task: this build with fused_rollout=True, this build without, the parent commit's build
        "train_on_engine_stream" (--only engine_stream)  the same three sides with the ENGINE's stream made torch's current stream around
                   loop.train (the one-stream recipe of profiles/native_rollout.json): the stronger baseline
        "issue"    (--only issue) host issue time per loop body, microseconds: NativeRollout.cycle against advance + choose +
                   Agent.iteration, and the node count of the cycle's graphs
    python tools/rollout_cycle_probe.py --bench TREE    # GPU: this checkout's bench.py against TREE's, alternating -> "bench"
    --only train|engine_stream|issue  restricts the first form to one group (a visit's time limit); each run rewrites its own entries."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "rollout_cycle.json")
RUNS = 5
KINDS = ("pendulum", "cartpole", "pointgoal")


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


def train_cfg(kind, num_envs, updates, learning_starts=1000):
    from sac_td3_cudagraphs_pytorch_amd import launcher
    return launcher.job_config("sac", kind, 0, num_envs=num_envs, learning_starts=learning_starts, batch_size=256,
                               num_timesteps=learning_starts + updates * num_envs - 1, eval_every=10 ** 9, rb_capacity=1 << 15)


def new_agent(kind, cfg):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    torch.manual_seed(0)
    return Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), torch.device("cuda", 0), cfg,
                 ReplayBuffer(cfg.rb_capacity), seed=0)


# ---------------------------------------------------------------------------------------------------- GPU children: one measurement each
def child_train(kind, which, stream="torch"):
    """which: "fused" (fused_rollout=True) or "native" (the call sequence; the only one a parent tree has); stream "engine": torch's
    current stream is the engine's own while the loop runs"""
    import contextlib
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    more = dict(native_rollout=True, **(dict(fused_rollout=True) if which == "fused" else {}))
    cfg = train_cfg(kind, 4, 3000)
    env = envs.NativeVecEnv(kind, cfg.num_envs, seed=0, device=torch.device("cuda", 0))
    agent = new_agent(kind, cfg)
    on = torch.cuda.stream(torch.cuda.ExternalStream(agent.engine.device_handles()[0])) if stream == "engine" else contextlib.nullcontext()
    with on:
        loop.train(train_cfg(kind, 4, 200), env, agent, device_env=True, **more)      # graphs instantiated, allocator warm
        agent.engine.sync()
        u0, t0 = agent.qnet_updates_so_far, time.perf_counter()
        cfg.num_timesteps += agent.timesteps_so_far
        loop.train(cfg, env, agent, device_env=True, **more)
        agent.engine.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"iterations_per_s": (agent.qnet_updates_so_far - u0) / dt, "iterations": agent.qnet_updates_so_far - u0}


def child_issue(kind, n):
    """host issue time, microseconds per loop body at n envs, back to back behind a warm-up and a wait (300 bodies: the queue stays
    short of where the runtime makes the host wait), each side on an agent and an env of its own; and the cycle graphs' node counts"""
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    dev = torch.device("cuda", 0)
    res = {}
    for side in ("cycle", "three_calls"):
        cfg = train_cfg(kind, n, 0, learning_starts=0)
        agent = new_agent(kind, cfg)
        env = envs.NativeVecEnv(kind, n, seed=0, device=dev)
        settle = lambda: (torch.cuda.synchronize(), agent.engine.sync())
        ro = loop.NativeRollout(env, agent, 0, 0, 1)
        agent.timesteps_so_far = 0                          # learning_starts 0: choose() asks the policy
        ro.choose()
        i, nodes = 0, set()

        def body():
            nonlocal i
            if side == "cycle":
                ro.cycle(i)
            else:
                ro.advance()
                ro.choose()
                agent.iteration(i)
            i += 1
        for _ in range(100):
            body()
            if side == "cycle":
                nodes.add(ro.cycle_stats()["graph_nodes"])
        settle()
        t0 = time.perf_counter()
        for _ in range(300):
            body()
        dt = time.perf_counter() - t0
        settle()
        res[side] = 1e6 * dt / 300
        if side == "cycle":
            res["graph_nodes_min"], res["graph_nodes_max"] = min(nodes), max(nodes)
        ro.close()
        agent.engine.close()
    return res


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "200"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


CHILDREN = {"train": child_train, "issue": child_issue}


def run_child(tree, *argv, timeout=300):
    """a fresh process per measurement, importing the package of `tree`; -> its JSON.  A child that fails ends the whole probe:
    nothing more is started on the GPU."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", *map(str, argv)], capture_output=True, text=True,
                         timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} in {tree} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def train_group(parent, runs, stream, key, what):
    for kind in KINDS:
        sides = {"fused_rollout": (ROOT, "fused"), "native_rollout": (ROOT, "native"), "parent_native_rollout": (parent, "native")}
        got = {k: [] for k in sides}
        for _ in range(runs):
            for k, (tree, which) in sides.items():                     # alternating
                got[k].append(run_child(tree, "train", kind, which, stream)["iterations_per_s"])
        entry = {k: spread(v) for k, v in got.items()}
        entry["fused_above_parent_max"] = bool(entry["fused_rollout"]["median"] > entry["parent_native_rollout"]["max"])
        merge({key: {"what": what, kind: entry}})
        print(key, kind, json.dumps(entry), flush=True)


def gpu_mode(parent, runs, only):
    if only in (None, "train"):
        train_group(parent, runs, "torch", "train",
                    "loop.train(device_env=True, native_rollout=True) on NativeVecEnv, SAC, 4 envs, B 256, 3000 iterations behind a 200-iteration "
                    "warm-up: iterations/s; fused_rollout: this build with fused_rollout=True; parent_native_rollout: the parent commit's build")
    if only in (None, "engine_stream"):
        train_group(parent, runs, "engine", "train_on_engine_stream",
                    "the train figures with the engine's stream as torch's current stream around loop.train: the env's kernels and the "
                    "engine's on one stream (the stronger baseline)")
    if only in (None, "issue"):
        for kind in ("pendulum", "pointgoal"):
            rs = [run_child(ROOT, "issue", kind, 4) for _ in range(runs)]
            entry = {k: spread([r[k] for r in rs]) for k in ("cycle", "three_calls")}
            entry["graph_nodes"] = [int(min(r["graph_nodes_min"] for r in rs)), int(max(r["graph_nodes_max"] for r in rs))]
            merge({"issue": {"what": "host issue time, microseconds per loop body at 4 envs, B 256, 300 bodies back to back: cycle = "
                                     "NativeRollout.cycle, three_calls = advance + choose + Agent.iteration; graph_nodes: [fewest, most] nodes "
                                     "of a cycle graph over its schedules", kind: entry}})
            print("issue", kind, json.dumps(entry), flush=True)


def bench_mode(other, runs):
    got = {"this": [], "parent": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["parent"].append(child_bench(other))
    keys = [k for k in ("value", "ms_per_step") if k in got["this"][0]]
    entry = {"what": "bench.py --gpus 1 --steps 2000 --warmup 200 of this checkout and of the parent commit's, alternating processes",
             **{side: {k: spread([r[k] for r in rs]) for k in keys} for side, rs in got.items()}}
    merge({"bench": entry})
    print(json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, metavar="TREE")
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--only", default=None, choices=["train", "engine_stream", "issue"])
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        kind_args = [int(x) if x.isdigit() else x for x in args.child[1:]]
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](*kind_args)), flush=True)
    elif args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs)
    elif args.parent:
        gpu_mode(os.path.abspath(args.parent), args.runs, args.only)
    else:
        ap.error("--parent TREE or --bench TREE")
    return 0


if __name__ == "__main__":
    sys.exit(main())
