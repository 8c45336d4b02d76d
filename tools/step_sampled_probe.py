#!/usr/bin/env python3
"""The prioritised / n-step iteration as one graph launch, measured beside the call sequence it replaces:
python tools/step_sampled_probe.py [--out profiles/step_sampled.json] [--call-sequence-only] [--baseline FILE ...]

What is timed is the loop a user runs: loop.train(fused=False, ...) on loop.SyntheticVecEnv (4 envs, horizon 50) -- acting, env step,
ring append and one gradient iteration per env step -- at the Hopper shape (ob 11, ac 3, B = 256) and the Humanoid shape (ob 376, ac 17,
B = 1024), for `prioritized`, for `n_step=3` and for both together, with and without `one_launch=True`.  Per (shape, variant) one agent
per mode, warmed by 400 iterations; then 5 repeats of 4000 iterations per mode, the modes alternating, each window closed by a
synchronisation of the engine's stream.  Figures are gradient iterations per second of host wall time.  Nothing here is a pass/fail
bar: the probe records what it finds, the spread of the repeats included.

  --call-sequence-only   time the call-sequence mode alone (the same windows in the same order, nothing in between): what a checkout
                         from before `one_launch` existed can run -- copy this file into it and run it there
  --baseline FILE ...    results of such runs (their --out files): stored under "baseline" with, per (shape, variant), the median of
                         all their repeats, their spread (max - min), and the margin of the one-launch median over it
  graph_nodes            kernel nodes of the one-launch graphs, [critic-only, with the actor updates] (the target update is in both:
                         crit_targ_update_freq is 1), beside the nodes of the call sequence's graphs (critic update, one actor update)
"""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sac_td3_cudagraphs_pytorch_amd as pkg  # noqa: E402
from oracle.sac_td3_ref import Hps  # noqa: E402
from sac_td3_cudagraphs_pytorch_amd import loop  # noqa: E402

REPEATS, ITERS, WARM, ENVS = 5, 4000, 400, 4
SHAPES = (("hopper_b256", 11, 3, 256), ("humanoid_b1024", 376, 17, 1024))
PRIO = dict(alpha=0.6, beta=0.4, eps=1e-6)
VARIANTS = (("prioritized", dict(prioritized=PRIO)), ("n_step_3", dict(n_step=3)), ("prioritized_n_step_3", dict(prioritized=PRIO, n_step=3)))


def summary(vals, digits=1):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits),
            "repeats": [round(v, digits) for v in vals]}


class Run:
    """one agent in one mode: train() continues it by `iters` gradient iterations and returns their rate"""

    def __init__(self, o, a, B, kw):
        self.cfg = SimpleNamespace(**{**Hps.sac(batch_size=B).__dict__, "seed": 0, "num_envs": ENVS, "action_repeat": 1,
                                      "learning_starts": 1000, "num_timesteps": 1000, "eval_every": 10 ** 9, "cudagraphs": True,
                                      "rb_capacity": 100_000})
        self.kw = kw
        self.env = loop.SyntheticVecEnv(o, a, ENVS)
        self.env.action_space.seed(0)
        torch.manual_seed(0)
        self.ag = pkg.Agent({"ob_shape": (ENVS, o), "ac_shape": (ENVS, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                            torch.device("cuda", 0), self.cfg, pkg.ReplayBuffer(self.cfg.rb_capacity))

    def train(self, iters):
        self.cfg.num_timesteps = max(self.ag.timesteps_so_far, self.cfg.learning_starts) + iters * ENVS
        self.ag.engine.sync()
        done0, t = self.ag.qnet_updates_so_far, time.perf_counter()
        self.metrics = loop.train(self.cfg, self.env, self.ag, fused=False, **self.kw)
        self.ag.engine.sync()
        return (self.ag.qnet_updates_so_far - done0) / (time.perf_counter() - t)


def probe(shape, o, a, B, variant, kw, modes):
    runs = {m: Run(o, a, B, dict(kw, one_launch=True) if m == "one_launch" else kw) for m in modes}
    for r in runs.values():
        r.train(WARM)
    rates = {m: [] for m in modes}
    for _ in range(REPEATS):
        for m in modes:
            rates[m].append(runs[m].train(ITERS))
    out = {"shape": shape, "ob_dim": o, "ac_dim": a, "batch": B, "variant": variant, "repeats": REPEATS, "iterations_per_repeat": ITERS,
           "iterations_per_s": {m: summary(v) for m, v in rates.items()},
           "loss_finite": {m: bool(np.isfinite(r.metrics["loss/qf_loss"])) for m, r in runs.items()}}
    eng = runs["call_sequence"].ag.engine
    out["graph_nodes"] = {"call_sequence": {"critic_update": eng.graph_kernel_count(8 if "prioritized" in kw else 0), "actor_update": eng.graph_kernel_count(1)}}
    if "one_launch" in runs:
        eng = runs["one_launch"].ag.engine
        out["graph_nodes"]["one_launch"] = [eng.graph_kernel_count(17), eng.graph_kernel_count(19)]
        out["step_sampled_stats"] = eng.step_sampled_stats()
        a_, b_ = rates["one_launch"], rates["call_sequence"]
        out["one_launch_over_call_sequence"] = round(statistics.median(a_) / statistics.median(b_), 3)
    for r in runs.values():
        r.ag.engine.close()
    return out


def against_baseline(res, files):
    """per (shape, variant): every repeat of the baseline runs, their median and spread, and the one-launch median's margin over it"""
    base = [json.load(open(f)) for f in files]
    out = []
    for r in res:
        vals = [v for b in base for w in b["workloads"] if (w["shape"], w["variant"]) == (r["shape"], r["variant"])
                for v in w["iterations_per_s"]["call_sequence"]["repeats"]]
        if not vals:
            continue
        med, spread = statistics.median(vals), max(vals) - min(vals)
        one = r["iterations_per_s"].get("one_launch", {}).get("median")
        row = {"shape": r["shape"], "variant": r["variant"], "call_sequence": summary(vals), "spread": round(spread, 1)}
        if one is not None:
            row.update(one_launch_median=one, margin=round(one - med, 1), margin_exceeds_spread=bool(one - med > spread),
                       one_launch_over_baseline=round(one / med, 3))
        out.append(row)
    return {"files": [os.path.basename(f) for f in files], "note": "the call-sequence loop of the parent commit, same probe, same order", "rows": out}


def main(argv):
    path = argv[argv.index("--out") + 1] if "--out" in argv else None
    modes = ("call_sequence",) if "--call-sequence-only" in argv else ("call_sequence", "one_launch")
    files = []
    if "--baseline" in argv:
        k = argv.index("--baseline") + 1
        while k < len(argv) and not argv[k].startswith("--"):
            files.append(argv[k])
            k += 1
    res = []
    for shape, o, a, B in SHAPES:
        for variant, kw in VARIANTS:
            res.append(probe(shape, o, a, B, variant, kw, modes))
            print(json.dumps(res[-1]), flush=True)
    doc = {"tool": "tools/step_sampled_probe.py", "device": torch.cuda.get_device_name(0), "modes": list(modes), "workloads": res}
    if files:
        doc["baseline"] = against_baseline(res, files)
        print(json.dumps(doc["baseline"]), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
