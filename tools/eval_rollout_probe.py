"""One evaluation as one launch, against the loop it stands in for -> profiles/eval_rollout.json.

    python tools/eval_rollout_probe.py --parent PATH_TO_A_BUILT_CHECKOUT_OF_THE_PARENT_COMMIT [--runs 5] [--out profiles/eval_rollout.json]

Alternating processes, `--runs` of each build (parent, this, parent, this, ...), every process fresh: it builds one SAC agent per native
task (the launcher's defaults, untrained: the cost of an evaluation does not depend on the weights) and times whole evaluations with a
host clock -- every evaluation ends in the host wait that reads the env's books, so the clock covers the device work.  Per process and
configuration: a warm-up, then the median over `REPS` evaluations.

  parent build   envs.greedy_returns(env, agent, n): one loop body per env step (predict_device, then env.step)
  this build     envs.greedy_returns(env, agent, n, one_launch=True): reset + one horizon in one kernel launch;
                 the same call without the keyword (the default path, which must not have moved); envs.q_bias on an env whose horizon
                 is the task's plus the steps gamma needs to fall to the tail tolerance (what the launcher's --q_bias builds)
Configurations: 16 episodes (an evaluation point of the launcher) and 4096 envs, each native task, default horizons.
The bar is relative and per configuration: EVERY one-launch run faster than the parent's FASTEST run; a miss is recorded, not hidden.
Medians and ranges over the processes; nothing is compared across visits."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ("pendulum", "cartpole", "pointgoal")
SIZES = (16, 4096)
REPS = {16: 30, 4096: 5}
CHILD_LIMIT = 420      # seconds per process


def child(role: str, root: str) -> int:
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    envs, launcher = P.envs, P.launcher
    dev = torch.device("cuda", 0)
    out = {"role": role, "library": P.library_path(), "ms": {}}

    def timed(fn, reps):
        fn()
        fn()                                       # warm-up: code objects, first-use scratch, torch's allocator
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()                                   # (ends in a host wait: episode_stats / the final statistics)
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    for task in TASKS:
        o, a, bound, horizon = envs.SPECS[envs.kind_of(task)][:4]
        for n in SIZES:
            cfg = launcher.job_config("sac", task, 0, num_envs=n, rb_capacity=1 << 12)
            torch.manual_seed(0)
            agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), dev, cfg,
                            P.ReplayBuffer(cfg.rb_capacity), seed=0)
            env = envs.NativeVecEnv(task, n, seed=1, device=dev)
            key = f"{task}/n{n}"
            if role == "parent":
                out["ms"][key + "/loop"] = timed(lambda: envs.greedy_returns(env, agent, n), REPS[n])
            else:
                out["ms"][key + "/one_launch"] = timed(lambda: envs.greedy_returns(env, agent, n, one_launch=True), REPS[n])
                if n == 16:
                    out["ms"][key + "/loop"] = timed(lambda: envs.greedy_returns(env, agent, n), REPS[n])
                    g = float(agent.engine.cfg.gamma)
                    long_env = envs.NativeVecEnv(task, n, seed=1, device=dev, horizon=horizon + int(np.ceil(np.log(0.05) / np.log(g))))
                    out["ms"][key + "/q_bias"] = timed(lambda: envs.q_bias(long_env, agent, seed=1), REPS[n])
                    out.setdefault("q_bias_horizon", {})[task] = long_env.horizon
                    long_env.close()
            env.close()
            agent.engine.close()
    print("PROBE " + json.dumps(out), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rollout.json"))
    ap.add_argument("--child", choices=["parent", "new"], help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root)
    if not args.parent or not os.path.isdir(args.parent):
        ap.error("--parent must name a built checkout of the parent commit")
    runs = {"parent": [], "new": []}
    for k in range(args.runs):
        for role, root in (("parent", os.path.abspath(args.parent)), ("new", ROOT)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", role, "--root", root], capture_output=True, text=True,
                               timeout=CHILD_LIMIT)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE ")]
            if p.returncode != 0 or not line:      # nothing more is started on the device behind a failed process
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"eval_rollout_probe: the {role} process of run {k} failed ({p.returncode}); stopping", file=sys.stderr)
                return 1
            runs[role].append(json.loads(line[0][6:]))
            print(f"run {k} {role}: " + ", ".join(f"{key} {v:.3f}" for key, v in runs[role][-1]["ms"].items()), flush=True)

    def series(role, key):
        return [r["ms"][key] for r in runs[role]]

    def stats(xs):
        xs = sorted(xs)
        return {"runs": xs, "median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}
    table = {}
    for task in TASKS:
        for n in SIZES:
            key = f"{task}/n{n}"
            loop, one = stats(series("parent", key + "/loop")), stats(series("new", key + "/one_launch"))
            row = {"parent_loop_ms": loop, "one_launch_ms": one, "speedup_of_medians": loop["median"] / one["median"],
                   "bar_met": one["max"] < loop["min"]}
            if n == 16:
                row["this_build_loop_ms"] = stats(series("new", key + "/loop"))
                row["q_bias_ms"] = stats(series("new", key + "/q_bias"))
            table[key] = row
    rec = {"what": "one evaluation (reset + one horizon of greedy steps, books read once), milliseconds per evaluation; host clock around a call "
                   "that ends in a host wait; medians over REPS evaluations per process, then median / min / max over the processes",
           "method": f"alternating processes, {args.runs} of each build; SAC, untrained, the launcher's defaults; default horizons",
           "reps_per_process": REPS, "bar": "every one-launch run faster than the parent's fastest run, per configuration",
           "q_bias_horizon": runs["new"][0].get("q_bias_horizon", {}), "configurations": table,
           "bar_met_everywhere": all(r["bar_met"] for r in table.values())}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"parent": r["parent_loop_ms"]["median"], "one_launch": r["one_launch_ms"]["median"], "bar_met": r["bar_met"]}
                      for k, r in table.items()}, indent=1))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
