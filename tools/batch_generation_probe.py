"""What moving the batch generation into the engine costs (profiles/batch_generation.json): python tools/batch_generation_probe.py --parent TREE

TREE is a built checkout of the parent commit.  One MI355X, child processes of this checkout and of TREE alternating, RUNS each:
  bench   bench.py --gpus 1 --steps 3000 --full --no-baselines: `value` (the headline) and `loop_with_acting_per_s`
  api     the call-by-call path through the mirror on the bench's Hopper SAC shapes (B = 256, 100 000 rows held): rb.sample ->
          update_qnets(handle) -> every third iteration update_actor(handle) x 2 -> update_targ_nets, iterations/s over 3000
          iterations behind 300; and, where the engine has it, Engine.batch_generation() alone, timeit over 10^5 calls
Per figure the record says where this checkout's median lies against the parent's min-max range.  No test reads the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, STEPS, WARMUP, B, HELD, DELAY = 5, 3000, 300, 256, 100_000, 2


def child_api(tree):
    sys.path.insert(0, tree)
    from types import SimpleNamespace
    import numpy as np
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    from oracle.sac_td3_ref import Hps
    o, a = 11, 3
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=B).__dict__, "seed": 0, "num_envs": 4, "rb_capacity": 2 * HELD})
    torch.manual_seed(0)
    ag = P.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                 torch.device("cuda", 0), cfg, P.ReplayBuffer(cfg.rb_capacity))
    eng = ag.engine
    eng.rb_fill_synthetic(HELD, 0)

    def run(i0, n):
        for i in range(i0, i0 + n):
            h = ag.rb.sample(B)
            ag.update_qnets(h)
            ag.qnet_updates_so_far += 1
            if i % (DELAY + 1) == 0:
                for _ in range(DELAY):
                    ag.update_actor(h)
                    ag.actor_updates_so_far += 1
            ag.update_targ_nets()
        eng.sync()
    run(-WARMUP, WARMUP)
    t0 = time.perf_counter()
    run(0, STEPS)
    dt = time.perf_counter() - t0
    res = {"api_iterations_per_s": STEPS / dt, "api_iteration_us": 1e6 * dt / STEPS}
    if hasattr(eng, "batch_generation"):
        res["batch_generation_call_ns"] = 1e9 * min(timeit.repeat(eng.batch_generation, number=100_000, repeat=3)) / 100_000
    eng.close()
    return res


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--full", "--no-baselines"],
                         cwd=tree, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    detail = json.load(open(os.path.join(tree, "bench_detail.json")))
    return {"value": line["value"], "loop_with_acting_per_s": detail["loop_with_acting_per_s"]}


def run_child(what, tree):
    """one measurement in a process of its own; a child that fails ends the probe: nothing more is started on the GPU"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--tree", tree], capture_output=True, text=True, timeout=700)
    if out.returncode != 0:
        raise SystemExit(f"{what} in {tree}: exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, metavar="TREE")
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", default=None, choices=["api", "bench"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_generation.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps((child_api if args.child == "api" else child_bench)(os.path.abspath(args.tree))))
        return
    if not args.parent:
        ap.error("--parent TREE: a built checkout of the parent commit")
    trees = {"change": ROOT, "parent": os.path.abspath(args.parent)}
    got = {side: {} for side in trees}
    for rnd in range(args.runs):
        for what in ("bench", "api"):
            for side, tree in trees.items():
                for k, v in run_child(what, tree).items():
                    got[side].setdefault(k, []).append(v)
                print(rnd, what, side, {k: round(v[-1], 1) for k, v in got[side].items()}, flush=True)
    rec = {"note": "The batch generation kept by the engine (sactd3_batch_generation) against the parent commit, which kept it as a Python "
                   "attribute; MI355X, alternating child processes. bench.py drives the engine directly and never makes a handle; `api` "
                   "is the call-by-call path through Agent / ReplayBuffer, which checks a handle once per update_* call. No number here "
                   "is a bar for a later change.",
           "runs_each": args.runs,
           "change": {k: spread(v) for k, v in got["change"].items()}, "parent": {k: spread(v) for k, v in got["parent"].items()}}
    where = lambda m, r: "below" if m < r["min"] else "above" if m > r["max"] else "inside"
    rec["median_against_parent_range"] = {k: where(rec["change"][k]["median"], rec["parent"][k])
                                          for k in ("value", "loop_with_acting_per_s", "api_iterations_per_s")}
    rec["batch_generation_call_over_api_iteration"] = (rec["change"]["batch_generation_call_ns"]["median"] * 1e-3
                                                       / rec["change"]["api_iteration_us"]["median"])
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_against_parent_range", "batch_generation_call_over_api_iteration")}), flush=True)


if __name__ == "__main__":
    main()
