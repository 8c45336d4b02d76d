"""Time the action-gradient call (include/sactd3_action_gradient.h) on an MI355X against the route it replaces: get_params, the twin
critics rebuilt as float32 torch tensors on the GPU, Q by a forward pass, dQ/da by autograd, and a Python loop for the ascent steps.

    python tools/action_gradient_probe.py [--out profiles/action_gradient.json] [--test_log LOG]     # the call against the torch route
    python tools/action_gradient_probe.py --bench TREE                                                # bench.py of this checkout against TREE's

LOG: the output of `pytest -s tests/test_gpu_action_gradient.py` on the same machine; its "action_gradient" lines become the record's
`accuracy` block (kernel error over the float32 restatement's yardstick, worst case per quantity and row count).  TREE: a built checkout
of the parent commit.  Both modes merge into the output file and keep its other blocks.

Alternating fresh processes, 5 per route (3 per side for the benchmark), each timing every configuration; median and range of the
processes' medians.  Device time: events on torch's current stream around calls that are ordered against it; wall time: a host clock
around the call and a device synchronise."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"hopper": (11, 3), "halfcheetah": (17, 6), "humanoid": (376, 17)}      # the three BASELINE shapes
ROWS, STEPS, LR, RUNS, REPS, BENCH_RUNS = (4, 256, 1024), (0, 4), 0.05, 5, 30, 3


def child(route):
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    from sac_td3_cudagraphs_pytorch_amd import _lib
    from oracle.sac_td3_ref import Hps
    out = {}
    for shape, (o, a) in SHAPES.items():
        eng = P.Engine(P.Config.from_hps(Hps.sac(batch_size=256), o, a, rb_capacity=1024, seed=1), [-1.0] * a, [1.0] * a)
        eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
        g = torch.Generator().manual_seed(2)
        K, H = o + a, 256
        sizes = [(H, K), (H,), (H,), (H,), (H, H), (H,), (H,), (H,), (1, H), (1,)]      # the state_dict order of one critic with LayerNorm
        lo, hi, sc = -torch.ones(a, device="cuda"), torch.ones(a, device="cuda"), torch.ones(a, device="cuda")

        def critics():
            flat, nets = torch.from_numpy(eng.get_params(_lib.CRITICS)).cuda().view(2, -1), []
            for k in range(2):
                parts, off = [], 0
                for s in sizes:
                    cnt = s[0] * (s[1] if len(s) > 1 else 1)
                    parts.append(flat[k, off:off + cnt].view(s))
                    off += cnt
                nets.append(parts)
            return nets

        def q_of(p, x):
            for w, b, gm, be in (p[0:4], p[4:8]):
                x = torch.relu(torch.nn.functional.layer_norm(x @ w.T + b, (H,), gm, be, 1e-5))
            return (x @ p[8].T + p[9])[:, 0]

        for n in ROWS:
            obs, act = torch.randn(n, o, generator=g).cuda(), (torch.rand(n, a, generator=g) * 2 - 1).cuda()
            for steps in STEPS:
                def engine_route():
                    return eng.action_gradient(obs, act, steps=steps, lr=LR)["summary"]

                def torch_route():
                    nets, cur = critics(), act
                    for it in range(steps + 1):
                        x = cur.clone().requires_grad_(True)
                        q = torch.stack([q_of(p, torch.cat([obs, x], 1)) for p in nets], 1)
                        if it == steps and steps:
                            break
                        g1, g2 = (torch.autograd.grad(q[:, k].sum(), x, retain_graph=k == 0)[0] for k in (0, 1))
                        if it == 0:
                            n1, n2 = g1.norm(dim=1), g2.norm(dim=1)
                            first = torch.stack([q.min(1).values.detach(), n1, n2, (g1 * g2).sum(1) / (n1 * n2)], 1)
                        if steps:
                            gu = torch.where((q[:, 0] <= q[:, 1])[:, None], g1, g2) * sc
                            cur = torch.minimum(torch.maximum(cur + (LR * gu / gu.norm(dim=1, keepdim=True).clamp_min(1e-8)) * sc, lo), hi)
                    return first, q.detach(), cur

                call = engine_route if route == "engine" else torch_route
                for _ in range(5):
                    call()
                wall, dev = [], []
                for _ in range(REPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    dev.append(e0.elapsed_time(e1))
                out[f"{shape}-n{n}-steps{steps}"] = {"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev), "device_max_ms": max(dev),
                                                     "device_min_ms": min(dev)}
        eng.close()
    print("RESULT " + json.dumps(out))


def spread(v):
    return {"median": statistics.median(v), "range": [min(v), max(v)]}


def accuracy(log):
    """worst kernel error over the float32 restatement's yardstick (the bound is 4), per quantity and row count, over the test's cases"""
    worst = {}
    for ln in open(log):
        for m in re.finditer(r"action_gradient \(([^)]*)\) (\w+) kernel (\S+) yardstick (\S+)", ln):
            rows, err, yard = m.group(1).split(", ")[-1].strip("'"), float(m.group(3)), float(m.group(4))
            if yard > 0:
                key = f"{m.group(2)}@{rows}"
                worst[key] = max(worst.get(key, 0.0), err / yard)
    return {"what": "tests/test_gpu_action_gradient.py: |kernel - float64| over the yardstick it is held to 4 x of (the float32 CPU "
                    "restatement's own error; in a one-row case the larger of it and the same restatement's on 17 rows), worst case per "
                    "quantity and row count", "ratio": worst}


def merge(out, block):
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec.update(block)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def run(cmd, cwd=ROOT):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=cwd)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    return out.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_gradient.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--test_log", default=None)
    ap.add_argument("--bench", default=None, metavar="TREE")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.bench:
        got = {"this": [], "parent": []}
        for _ in range(BENCH_RUNS):
            for side, tree in (("this", ROOT), ("parent", os.path.abspath(args.bench))):      # alternating
                lines = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3000", "--warmup", "300"], cwd=tree)
                got[side].append(json.loads([ln for ln in lines if ln.startswith("{")][-1])["value"])
        entry = {side: spread(v) for side, v in got.items()}
        merge(args.out, {"bench": {"what": "bench.py --gpus 1 --steps 3000 --warmup 300, gradient steps/s, this checkout against the parent "
                                           "commit's, alternating, 3 runs each", **entry}})
        return print(json.dumps(entry))
    if args.test_log:
        merge(args.out, {"accuracy": accuracy(args.test_log)})
    got = {"engine": [], "torch": []}
    for _ in range(RUNS):
        for route in got:      # alternating processes
            lines = run([sys.executable, __file__, "--child", route])
            got[route].append(json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][7:]))
            print(route, "done", flush=True)
    cases = {case: {route: {k: spread([r[case][k] for r in runs]) for k in ("wall_ms", "device_ms")} for route, runs in got.items()}
             for case in got["engine"][0]}
    for case, c in cases.items():      # the expectation: every run of the new route faster than the replaced route's fastest run
        c["every_engine_run_faster"] = max(r[case]["device_ms"] for r in got["engine"]) < min(r[case]["device_ms"] for r in got["torch"])
    merge(args.out, {"timing": {"what": "one Engine.action_gradient (all outputs but grad_obs) against the torch route (get_params, float32 critics "
                                        "on the GPU, autograd, a Python loop for the steps), ms; SAC with LayerNorm, lr 0.05, alternating fresh "
                                        "processes, 5 per route, 30 timed calls per configuration; every_engine_run_faster compares the "
                                        "processes' medians", "runs": RUNS, "reps": REPS, "cases": cases}})
    print(json.dumps(cases))


if __name__ == "__main__":
    main()
