#!/usr/bin/env python3
"""What the TD3+BC actor term costs, measured: python tools/td3bc_probe.py [--parent-root DIR] [--out profiles/td3bc.json]

Engine.run_iterations rate (iterations per second, host wall time around a synchronised run of whole periods on a synthetic ring)
of the TD3 engine at two shapes -- HalfCheetah (17, 6), B = 256 and the Humanoid shape (376, 17), B = 1024 -- in three variants:

  bc_on    this build, bc_alpha = 2.5
  bc_off   this build, bc_alpha = 0 (launches exactly the kernels the parent launches: their machine code is unchanged)
  parent   the parent commit: --parent-root names a checkout of it with its library built (its own Python package and library are
           used); the variant is left out, and recorded as "not measured", without it

Every figure comes from a process of its own (a child started per variant and repeat), the variants alternate in an order that
rotates from round to round, REPEATS rounds, median with min - max.  A third shape, HalfCheetah at B = 1024, is there for its node times
only: it takes the 64-thread k_actor_head_bwd_s_bc<4>.  Beside the rates: the per-kernel device time of the
head-backward and weight-gradient nodes of one iteration with actor updates (sactd3_time_nodes, one child per variant of this build).
Nothing here is a pass/fail bar: the probe records what it finds.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TD3BC_PROBE_ROOT") or ROOT)      # (a child of the `parent` variant imports the parent checkout's package)

REPEATS, WARMUP = 5, 3000
SHAPES = {"halfcheetah_td3_b256": dict(o=17, a=6, bound=1.0, B=256, iters=30000),
          "humanoid_td3_b1024": dict(o=376, a=17, bound=0.4, B=1024, iters=9000),
          # node times only: the shape that takes the 64-thread k_actor_head_bwd_s_bc<4> (narrow head at B >= 1024: B / 4 blocks, each summing all B |q|)
          "halfcheetah_td3_b1024": dict(o=17, a=6, bound=1.0, B=1024, iters=0)}


def make_engine(shape, bc_alpha):
    import sac_td3_cudagraphs_pytorch_amd as pkg
    s = SHAPES[shape]
    kw = dict(ob_dim=s["o"], ac_dim=s["a"], batch_size=s["B"], rb_capacity=65536, prefer_td3_over_sac=True, bcq_style_targ_mix=True,
              qnets_lr=3e-4, seed=0)
    if bc_alpha > 0:
        kw["bc_alpha"] = bc_alpha
    eng = pkg.Engine(pkg.Config(**kw), -s["bound"], s["bound"])
    import torch
    torch.manual_seed(0)
    from sac_td3_cudagraphs_pytorch_amd import _lib, schema
    actor, critics = schema.reference_initial_params(s["o"], s["a"], True, True)
    for which, flat in ((_lib.ACTOR, actor), (_lib.ACTOR_TARGET, actor), (_lib.CRITICS, critics), (_lib.CRITICS_TARGET, critics)):
        eng.set_params(which, flat)
    eng.rb_fill_synthetic(65536, 1)
    return eng


def child(shape, bc_alpha, what):
    eng = make_engine(shape, bc_alpha)
    if what == "rate":
        i = eng.run_iterations(0, WARMUP)
        eng.sync()
        t0 = time.perf_counter()
        eng.run_iterations(i, SHAPES[shape]["iters"])
        eng.sync()
        dt = time.perf_counter() - t0
        print("RESULT " + json.dumps({"iters_per_s": SHAPES[shape]["iters"] / dt}))
    else:
        nodes = eng.time_nodes(1, iters=200)
        keep = [n for n in nodes if n["name"].startswith(("k_headbwd_nn", "k_actor_head_bwd", "k_tn", "k_adam_red")) and "actor" in n["name"]]
        print("RESULT " + json.dumps({"nodes": [{"name": n["name"], "us": round(n["us"], 3)} for n in keep],
                                      "iteration_us": round(sum(n["us"] for n in nodes), 2), "node_count": len(nodes)}))
    return 0


def run_child(shape, bc_alpha, what, root=None):
    env = dict(os.environ)
    if root:
        env["TD3BC_PROBE_ROOT"] = os.path.abspath(root)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, str(bc_alpha), what], env=env, capture_output=True,
                         text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"child {shape} {bc_alpha} {what} failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def summary(vals):
    return {"median": round(statistics.median(vals), 1), "min": round(min(vals), 1), "max": round(max(vals), 1), "runs": len(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3bc.json"))
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], float(args.child[1]), args.child[2])
    variants = [("bc_on", 2.5, None), ("bc_off", 0.0, None)] + ([("parent", 0.0, args.parent_root)] if args.parent_root else [])
    rec = {"method": f"separate alternating processes (order rotating per round), {REPEATS} runs each, run_iterations of 30000 (B = 256) / 9000 (B = 1024) iterations after {WARMUP} warm-up, "
                     "host wall time around a synchronised run; medians with min - max", "shapes": {}}
    for shape in SHAPES:
        s = {}
        if SHAPES[shape]["iters"]:
            rates = {v[0]: [] for v in variants}
            for r in range(REPEATS):
                k = r % len(variants)
                for name, alpha, lib in variants[k:] + variants[:k]:      # (the order rotates from round to round)
                    rates[name].append(run_child(shape, alpha, "rate", lib)["iters_per_s"])
                    print(shape, name, round(rates[name][-1]), flush=True)
            s["iters_per_s"] = {k: summary(v) for k, v in rates.items()}
            if not args.parent_root:
                s["iters_per_s"]["parent"] = "not measured"
            s["bc_on_cost_percent"] = round(100.0 * (1.0 - statistics.median(rates["bc_on"]) / statistics.median(rates["bc_off"])), 2)
        else:
            s["iters_per_s"] = "not measured"
        s["nodes"] = {name: run_child(shape, alpha, "nodes") for name, alpha, lib in variants if lib is None}
        rec["shapes"][shape] = s
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
