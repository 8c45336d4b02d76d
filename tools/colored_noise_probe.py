#!/usr/bin/env python3
"""Measurements around coloured exploration noise (include/sactd3_noise.h, Engine.colored_noise, NativeRollout.collect(colored=True),
loop.train(exploration_beta=)) -> profiles/colored_noise.json, by the method of tools/collect_probe.py, whose helpers it uses: one fresh
process per measurement, the sides alternating, 5 runs each, median / min / max.  Nothing in the record is a pass / fail bar of a test.

    python tools/colored_noise_probe.py --gpu            # GPU
        "generate"  device time of one chunk generation, microseconds: (L, S) = (256, 8), (4096, 8), (4096, 8192), beta 1
        "step"      device time per ENV STEP inside collect(64), EXPLORE, pendulum, 4 and 4096 envs: coloured (beta 1, chunks of 256 steps,
                    so one call in four also generates a chunk) against white
        "train"     loop.train(collected_rollout=True, segment_len=8, updates_per_step=8) iterations/s, SAC, 4 envs, B 256: with
                    exploration_beta=1 against without
        "returns"   greedy return (envs.greedy_returns, 16 envs, one horizon) on the pendulum and on the goal task (with hindsight) behind
                    the budgets of profiles/native_env.json / profiles/hindsight.json, beta 0, 1, 2 and the white draw, seeds 0, 1, 2:
                    a finding, not a claim
    python tools/colored_noise_probe.py --bench TREE     # GPU: this checkout's bench.py against TREE's (the parent commit, built), 3 runs each
Each mode rewrites its own entries of the record and leaves the others."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from collect_probe import child_bench, new_agent, spread, train_cfg  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "colored_noise.json")
RUNS = 5
SHAPES = ((256, 8), (4096, 8), (4096, 8192))
BETAS = ("white", 0.0, 1.0, 2.0)
SEEDS = (0, 1, 2)
BUDGET = {"pendulum": 3500, "pointgoal": 4000}      # updates; 4 envs, learning_starts 1000, B 256, segment_len 4, updates_per_step 4


def merge(entries):
    rec = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rec = json.load(f)
    for k, v in entries.items():
        rec[k] = {**rec.get(k, {}), **v}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def timed(call, reps, settle):
    """microseconds per call of device time between two events on torch's current stream, behind a warm-up and a wait"""
    import torch
    for _ in range(max(3, reps // 10)):
        call()
    settle()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    settle()
    return 1e3 * e0.elapsed_time(e1) / reps


def child_generate():
    import torch
    agent = new_agent("pendulum", train_cfg("pendulum", 0, 4, 0, learning_starts=0))
    eng, res = agent.engine, {}
    for L, S in SHAPES:
        out = torch.empty((L, S), dtype=torch.float32, device="cuda")
        chunk = iter(range(10 ** 9))
        res[f"L{L}_S{S}"] = timed(lambda: eng.colored_noise(1.0, L, S, chunk=next(chunk), out=out), 200, lambda: (torch.cuda.synchronize(), eng.sync()))
    return res


def child_step(n, side):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import _lib, envs, loop
    agent = new_agent("pendulum", train_cfg("pendulum", 0, n, 0, learning_starts=0, cap=max(1 << 15, 64 * n)))
    ro = loop.NativeRollout(envs.NativeVecEnv("pendulum", n, seed=0, device=torch.device("cuda", 0)), agent, 0, 0, 1)
    if side == "colored":
        ro.configure_noise(1.0, 256)
    us = timed(lambda: ro.collect(64, _lib.ROLLOUT_EXPLORE, colored=side == "colored"), 32, lambda: (torch.cuda.synchronize(), agent.engine.sync()))
    ro.close()
    return {"device_us_per_step": us / 64}


def child_train(side):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    more = dict(device_env=True, native_rollout=True, collected_rollout=True, updates_per_step=8, **(dict(exploration_beta=1.0) if side == "colored" else {}))
    cfg = train_cfg("pendulum", 0, 4, 4000, segment_len=8, updates_per_step=8)
    env, agent = envs.NativeVecEnv("pendulum", 4, seed=0, device=torch.device("cuda", 0)), new_agent("pendulum", cfg)
    loop.train(train_cfg("pendulum", 0, 4, 400, segment_len=8, updates_per_step=8), env, agent, **more)      # graphs, allocator
    agent.engine.sync()
    u0, t0 = agent.qnet_updates_so_far, time.perf_counter()
    cfg.num_timesteps += agent.timesteps_so_far
    loop.train(cfg, env, agent, **more)
    agent.engine.sync()
    torch.cuda.synchronize()
    return {"iterations_per_s": (agent.qnet_updates_so_far - u0) / (time.perf_counter() - t0)}


def child_returns(kind, beta, seed):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import envs, launcher, loop
    dev = torch.device("cuda", 0)
    cfg = train_cfg(kind, seed, 4, BUDGET[kind], segment_len=4, updates_per_step=4)
    torch.manual_seed(seed)
    agent = new_agent(kind, cfg)
    more = dict(exploration_beta=float(beta)) if beta != "white" else {}
    if kind == "pointgoal":
        more.update(fused=False, hindsight=launcher.hindsight_keywords("PointGoal-native", 4))
    loop.train(cfg, envs.NativeVecEnv(kind, 4, seed=seed, device=dev), agent, device_env=True, native_rollout=True, collected_rollout=True,
               updates_per_step=4, **more)
    got = envs.greedy_returns(envs.NativeVecEnv(kind, 16, seed=seed + 1000, device=dev), agent, 16)
    return {"return": float(got["return"]), "updates": int(agent.qnet_updates_so_far)}


CHILDREN = {"generate": child_generate, "step": child_step, "train": child_train, "returns": child_returns}


def run_child(*argv):
    """a fresh process per measurement; a child that fails ends the whole probe: nothing more is started on the GPU"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *map(str, argv)], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def gpu_mode(runs, only):
    if only in (None, "generate"):
        got = [run_child("generate") for _ in range(runs)]
        merge({"generate": {"what": "device time of one Engine.colored_noise call (beta 1, a fresh chunk each), microseconds, 200 calls a run",
                            **{k: spread([g[k] for g in got]) for k in got[0]}}})
    for key, child, field, cases in (("step", "step", "device_us_per_step", (4, 4096)), ("train", "train", "iterations_per_s", (None,))):
        if only not in (None, key):
            continue
        for case in cases:
            got = {"colored": [], "white": []}
            for _ in range(runs):                                          # alternating
                for side in got:
                    got[side].append(run_child(child, *([case] if case is not None else []), side)[field])
            entry = {side: spread(v) for side, v in got.items()}
            if key == "step":
                entry["colored_median_at_or_below_white_max"] = bool(entry["colored"]["median"] <= entry["white"]["max"])
            else:
                entry["colored_median_at_or_above_white_min"] = bool(entry["colored"]["median"] >= entry["white"]["min"])
            merge({key: {f"n{case}" if case is not None else "sac_pendulum_n4_B256": entry}})
            print(key, case, json.dumps(entry), flush=True)
    if only in (None, "returns"):
        for kind in BUDGET:
            entry = {str(b): [run_child("returns", kind, b, s)["return"] for s in SEEDS] for b in BETAS}
            merge({"returns": {"what": "greedy return behind the budget, per seed 0, 1, 2; 'white': the collect kernel's own draw", kind: entry}})
            print("returns", kind, json.dumps(entry), flush=True)


def bench_mode(other, runs):
    got = {"this": [], "parent": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["parent"].append(child_bench(other))
    entry = {side: spread([r["value"] for r in rs]) for side, rs in got.items()}
    merge({"bench": {"what": "bench.py --gpus 1 --steps 3000 --warmup 300, gradient steps/s, this checkout against the parent commit's, alternating", **entry}})
    print(json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--only", default=None, choices=["generate", "step", "train", "returns"])
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.child:
        argv = [int(x) if x.isdigit() else x for x in args.child[1:]]
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](*argv)), flush=True)
    elif args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs or 3)
    elif args.gpu:
        gpu_mode(args.runs or RUNS, args.only)
    else:
        ap.error("--gpu or --bench TREE")
    return 0


if __name__ == "__main__":
    sys.exit(main())
