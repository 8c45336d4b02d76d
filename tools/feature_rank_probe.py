"""Time the feature-rank call (include/sactd3_feature_rank.h) on an MI355X against the route a user had before it: get_params for both
nets (each a stream synchronisation), the three MLPs restated in torch on the GPU, torch.linalg.svdvals of the features, the ranks read
back.  The host route is given the rows as a device tensor it already holds (no ReplayBuffer.rows call): that flatters it.

    python tools/feature_rank_probe.py [--out profiles/feature_rank.json] [--test_log LOG]     # the call against the host route
    python tools/feature_rank_probe.py --bench TREE                                            # bench.py of this checkout against TREE's

LOG: the output of `pytest -s tests/test_gpu_feature_rank.py` on the same machine; its "feature rank" lines become the record's
`accuracy` block.  TREE: a built checkout of the parent commit.  Both modes merge into the output file and keep its other blocks.

Alternating fresh processes, 5 per route and configuration (3 per side for the benchmark); median and range.  Device time: events on
torch's current stream around calls that are ordered against it; wall time: a host clock around the call and the wait for its result."""
import argparse
import ast
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
ROWS, RUNS, REPS, CAP, BENCH_RUNS = (256, 1024, 4096), 5, 30, 1 << 16, 3
NETS = ("actor", "q1", "q2")


def child(route, shape, rows):
    import numpy as np
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    from sac_td3_cudagraphs_pytorch_amd import _lib
    from oracle.sac_td3_ref import Hps
    from tests import init_model
    o, a = SHAPES[shape]
    eng = P.Engine(P.Config.from_hps(Hps.sac(batch_size=256), o, a, rb_capacity=CAP, seed=1), [-1.0] * a, [1.0] * a)
    eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
    g = torch.Generator().manual_seed(2)
    obs, act = torch.randn(CAP, o, generator=g), torch.rand(CAP, a, generator=g) * 2 - 1
    eng.rb_extend(obs.numpy(), act.numpy(), np.zeros(CAP, np.float32), obs.numpy(), np.zeros(CAP, bool))
    x = torch.cat([obs, act], 1).cuda()
    idx = torch.randint(0, CAP, (rows,), generator=g).cuda()

    def engine_route():
        got = eng.feature_rank(idx)
        return [got["srank"][k] for k in NETS], got["sweeps"]

    def host_route():
        params = {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS)}
        sranks = []
        for _, K, nh, flat in init_model.nets_of(params, o, a, False):
            p = {(k, l): torch.as_tensor(np.array(v)).cuda() for k, l, v in init_model.split(flat, K, nh, True)}
            h = x[idx, :K]
            for l in (0, 1):
                h = torch.relu(torch.nn.functional.layer_norm(h @ p[("weight", l)].T + p[("bias", l)], (256,), p[("ln_weight", l)], p[("ln_bias", l)]))
            s = torch.linalg.svdvals(h / rows ** 0.5)
            s = torch.where(s * s > 1e-4 * s[0] * s[0], s, torch.zeros_like(s))
            sranks.append(int((torch.cumsum(s, 0) >= 0.99 * s.sum()).nonzero()[0]) + 1)
        return sranks, None

    call = engine_route if route == "engine" else host_route
    for _ in range(5):
        sranks, sweeps = call()
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
    eng.close()
    print("RESULT " + json.dumps({"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev), "srank": sranks,
                                  **({"sweeps": [sweeps[k] for k in NETS]} if sweeps else {})}))


def spread(v):
    return {"median": statistics.median(v), "range": [min(v), max(v)]}


def accuracy(log):
    """the `accuracy` block from the test's printed figures: ratios to the float32 CPU restatement's own error against float64"""
    rows = [[ast.literal_eval(v) for v in m.groups()] for m in (re.search(
        r"feature rank \(.*?\) gram (\[.*?\]) lambda (\[.*?\]) err (\[.*?\]) trace (\[.*?\]) (\[.*?\]) sweeps (\{.*?\})", ln) for ln in open(log)) if m]
    flat = lambda i: [x for r in rows for x in r[i]]
    sweeps = [x for r in rows for x in r[5].values()]
    return {"what": "tests/test_gpu_feature_rank.py test 1, per net over its cases: error against float64 over the float32 CPU restatement's own",
            "cases": len(rows), "gram_over_yardstick": [min(flat(0)), max(flat(0))], "lambda_over_yardstick": [min(flat(1)), max(flat(1))],
            "lambda_abs_error": [min(flat(2)), max(flat(2))], "trace_invariant_over_yardstick_max": max(t / y for r in rows for t, y in zip(r[3], r[4])),
            "bounds": {"gram": 4, "lambda": 16, "trace_invariant": 8}, "sweeps": [min(sweeps), max(sweeps)], "sweeps_allowed": 16}


def merge(out, block):
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec.update(block)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def run(cmd, cwd=ROOT, env=None):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd, env=env)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    return out.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_rank.json"))
    ap.add_argument("--child", nargs=3, default=None)
    ap.add_argument("--test_log", default=None)
    ap.add_argument("--bench", default=None, metavar="TREE")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]))
    if args.bench:
        got = {"this": [], "parent": []}
        for _ in range(BENCH_RUNS):
            for side, tree in (("this", ROOT), ("parent", os.path.abspath(args.bench))):      # alternating
                lines = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3000", "--warmup", "300"], cwd=tree)
                got[side].append(json.loads([ln for ln in lines if ln.startswith("{")][-1])["value"])
        entry = {side: spread(v) for side, v in got.items()}
        entry["this_median_at_or_above_parent_min"] = bool(entry["this"]["median"] >= entry["parent"]["range"][0])
        merge(args.out, {"bench": {"what": "bench.py --gpus 1 --steps 3000 --warmup 300, gradient steps/s, this checkout against the parent "
                                           "commit's, alternating, 3 runs each", **entry}})
        return print(json.dumps(entry))
    if args.test_log:
        merge(args.out, {"accuracy": accuracy(args.test_log)})
    rec = {}
    for shape in SHAPES:
        for rows in ROWS:
            got = {"engine": [], "host": []}
            for _ in range(RUNS):
                for route in got:      # alternating processes
                    lines = run([sys.executable, __file__, "--child", route, shape, str(rows)])
                    got[route].append(json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][7:]))
            rec[f"{shape}-{rows}"] = {route: {**{k: spread([r[k] for r in runs]) for k in ("wall_ms", "device_ms")}, "srank": runs[0]["srank"],
                                              **({"sweeps": runs[0]["sweeps"]} if "sweeps" in runs[0] else {})} for route, runs in got.items()}
            print(shape, rows, json.dumps(rec[f"{shape}-{rows}"]), flush=True)
    merge(args.out, {"timing": {"what": "one Engine.feature_rank of all three nets against the host route (get_params twice, the MLPs in torch on the "
                                        "GPU, torch.linalg.svdvals, srank read back), ms; alternating processes, 5 runs each of 30 timed calls; srank / "
                                        "sweeps per net (actor, Q1, Q2)", "runs": RUNS, "reps": REPS, "cases": rec}})


if __name__ == "__main__":
    main()
