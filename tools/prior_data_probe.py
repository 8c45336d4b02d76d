#!/usr/bin/env python3
"""Learning online from prior data, measured: python tools/prior_data_probe.py [--out profiles/prior_data.json] [--repeats 5]
       [--updates 2000] [--shapes hopper_b256,humanoid_b1024] [--utd 1,4,20] [--headline PARENT_CHECKOUT [--bench-steps 3000]]

What is timed is the loop a user runs: loop.train(fused=False, prior_fraction=0.5, updates_per_step=G) on loop.SyntheticVecEnv (4 envs)
on top of 5000 pinned dataset rows in a 20000-slot ring -- acting, env step, ring append and G gradient iterations per env step -- at
the Hopper shape (ob 11, ac 3, B = 256) and the Humanoid shape (ob 376, ac 17, B = 1024), in three modes:
  mixed_one_launch     loop.train(..., one_launch=True): the mixed draw inside the iteration's graph (sactd3_step_sampled)
  mixed_call_sequence  the same iteration call by call (rb.sample_mixed -> update_qnets -> update_actor x N -> update_targ_nets)
  uniform_fused        loop.train(fused=True, updates_per_step=G) of the same build on the same rows, unpinned: the uniform iteration
Every figure comes from a process of its own: per (shape, G) the parent starts `--repeats` rounds, in each round one fresh child per
mode, the modes alternating; a child warms its agent by `--updates` / 4 gradient iterations, then times `--updates` of them between two
synchronisations of the engine's stream.  Figures are gradient iterations per second of host wall time; median, min and max of the
repeats are kept.  The draw kernel's time per launch is Engine.time_kernel("mix_draw") (sactd3_time_kernel: back-to-back launches of
that kernel alone between two events), beside the staging kernel's ("batch_from_index").
  --headline PARENT_CHECKOUT   also run `bench.py --gpus 1` of that checkout (the parent commit, built) and of this tree as alternating
                               processes, `--repeats` each: the headline must lie inside the parent's own min-max spread
Nothing here is a pass/fail bar: the probe records what it finds."""
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"hopper_b256": (11, 3, 256), "humanoid_b1024": (376, 17, 1024)}
MODES = ("mixed_one_launch", "mixed_call_sequence", "uniform_fused")
ENVS, PRIOR, CAP = 4, 5000, 20000


def summary(vals, digits=1):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits),
            "repeats": [round(v, digits) for v in vals]}


def child(shape, mode, G, updates):
    import numpy as np
    import torch
    import sac_td3_cudagraphs_pytorch_amd as pkg
    from oracle.sac_td3_ref import Hps
    from sac_td3_cudagraphs_pytorch_amd import loop
    o, a, B = SHAPES[shape]
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=B).__dict__, "seed": 0, "num_envs": ENVS, "action_repeat": 1, "learning_starts": 0,
                             "num_timesteps": 0, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": CAP})
    env = loop.SyntheticVecEnv(o, a, ENVS)
    env.action_space.seed(0)
    torch.manual_seed(0)
    ag = pkg.Agent({"ob_shape": (ENVS, o), "ac_shape": (ENVS, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                   torch.device("cuda", 0), cfg, pkg.ReplayBuffer(CAP))
    rng = np.random.default_rng(0)
    data = dict(observations=rng.standard_normal((PRIOR, o), np.float32), actions=rng.uniform(-1, 1, (PRIOR, a)).astype(np.float32),
                rewards=rng.standard_normal(PRIOR, np.float32), next_observations=rng.standard_normal((PRIOR, o), np.float32),
                terminations=rng.random(PRIOR) < 0.01)
    mixed = mode != "uniform_fused"
    loop.load_dataset(ag, data, pin=mixed)
    kw = dict(fused=False, prior_fraction=0.5, one_launch=mode == "mixed_one_launch") if mixed else dict(fused=True)

    def run(n):
        cfg.num_timesteps = ag.timesteps_so_far + (n // G) * ENVS - 1
        ag.engine.sync()
        done0, t = ag.qnet_updates_so_far, time.perf_counter()
        m = loop.train(cfg, env, ag, updates_per_step=G, **kw)
        ag.engine.sync()
        return (ag.qnet_updates_so_far - done0) / (time.perf_counter() - t), m

    run(max(updates // 4, 4 * G))
    rate, m = run(updates)
    out = {"rate": rate, "loss_finite": bool(np.isfinite(m["loss/qf_loss"])), "updates": int(ag.qnet_updates_so_far)}
    if mode == "mixed_one_launch":
        eng = ag.engine
        out["step_sampled_stats"] = eng.step_sampled_stats()
        out["graph_nodes"] = [eng.graph_kernel_count(17), eng.graph_kernel_count(19)]
        out["mix_draw_us"] = round(eng.time_kernel("mix_draw", 200), 2)
        out["batch_from_index_us"] = round(eng.time_kernel("batch_from_index", 200), 2)
    ag.engine.close()
    print("CHILD " + json.dumps(out), flush=True)
    return 0


def spawn(args, cwd=ROOT, tag="CHILD "):
    p = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(tag)]
    if p.returncode != 0 or not lines:
        raise RuntimeError(f"{args}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(lines[-1][len(tag):] if tag != "{" else lines[-1])      # (bench.py's result line is the JSON object itself)


def headline(parent, repeats, steps):
    vals = {"parent": [], "this_tree": []}
    for _ in range(repeats):
        for name, cwd in (("parent", parent), ("this_tree", ROOT)):
            r = spawn(["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(max(steps // 10, 1))], cwd=cwd, tag="{")
            vals[name].append(float(r["value"]))
    p, t = vals["parent"], vals["this_tree"]
    return {"bench": f"bench.py --gpus 1 --steps {steps}", "parent": summary(p), "this_tree": summary(t),
            "this_tree_median_inside_parent_spread": bool(min(p) <= statistics.median(t) <= max(p))}


def main(argv):
    if argv[:1] == ["--child"]:
        return child(argv[1], argv[2], int(argv[3]), int(argv[4]))
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    repeats, updates = int(opt("--repeats", 5)), int(opt("--updates", 2000))
    shapes = opt("--shapes", ",".join(SHAPES)).split(",")
    utd = [int(x) for x in opt("--utd", "1,4,20").split(",")]
    import torch
    path = opt("--out", None)
    res = []
    doc = {"tool": "tools/prior_data_probe.py", "device": torch.cuda.get_device_name(0), "prior_rows_in_ring": PRIOR, "ring_capacity": CAP,
           "envs": ENVS, "prior_fraction": 0.5, "workloads": res}

    def save():      # after every row: a run that is cut short keeps what it measured
        if path:
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")

    if "--headline" in argv:
        doc["headline"] = headline(os.path.abspath(opt("--headline", "")), repeats, int(opt("--bench-steps", 3000)))
        print(json.dumps(doc["headline"]), flush=True)
        save()
    for shape in shapes:
        for G in utd:
            got = {m: [] for m in MODES}
            for _ in range(repeats):
                for m in MODES:
                    got[m].append(spawn([os.path.abspath(__file__), "--child", shape, m, str(G), str(updates)]))
            one = got["mixed_one_launch"][-1]
            row = {"shape": shape, "batch": SHAPES[shape][2], "updates_per_step": G, "repeats": repeats, "updates_per_repeat": updates,
                   "iterations_per_s": {m: summary([c["rate"] for c in v]) for m, v in got.items()},
                   "loss_finite": {m: all(c["loss_finite"] for c in v) for m, v in got.items()},
                   "graph_nodes_one_launch": one["graph_nodes"], "step_sampled_stats": one["step_sampled_stats"],
                   "mix_draw_us": summary([c["mix_draw_us"] for c in got["mixed_one_launch"]], 2),
                   "batch_from_index_us": summary([c["batch_from_index_us"] for c in got["mixed_one_launch"]], 2)}
            med = {m: row["iterations_per_s"][m]["median"] for m in MODES}
            row["one_launch_over_call_sequence"] = round(med["mixed_one_launch"] / med["mixed_call_sequence"], 3)
            row["one_launch_over_uniform_fused"] = round(med["mixed_one_launch"] / med["uniform_fused"], 3)
            res.append(row)
            print(json.dumps(row), flush=True)
            save()
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
