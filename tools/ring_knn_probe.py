"""Time the nearest-ring-rows call (include/sactd3_ring_knn.h) on an MI355X against the route it replaces: the ring materialised in
torch (ReplayBuffer.rows(arange(len))), torch.cdist against the queries, torch.topk -- the ring walked in blocks where the [n, len]
matrix would pass 256 MB.  Gathering the ring is charged to that route once per call: it is what a caller without the feature pays.

    python tools/ring_knn_probe.py [--out profiles/ring_knn.json] [--lens 65536,1000000]     # the call against the torch route
    python tools/ring_knn_probe.py --bench TREE                                               # bench.py of this checkout against TREE's

TREE: a built checkout of the parent commit.  Both modes merge into the output file and keep its other blocks.

Alternating fresh processes, 5 per route (3 per side for the benchmark), each timing every configuration; median and range of the
processes' medians.  Device time: events on torch's current stream around calls that are ordered against it; wall time: a host clock
around the call and a device synchronise.  `ring_TBps`: the key bytes of the range (len x 4 D, once per tile of 64 queries) over the
engine's median device time, beside the 4.35 - 4.7 TB/s of the gather kernels and the 8 TB/s of the memory."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"hopper": (11, 3), "halfcheetah": (17, 6), "humanoid": (376, 17)}      # the three BASELINE shapes
QUERIES, KS, LENS, RUNS, REPS, BENCH_RUNS = (16, 256, 1024), (1, 16), (65536, 1000000), 5, 10, 3


def child(route, lens):
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    from oracle.sac_td3_ref import Hps
    out = {}
    for shape, (o, a) in SHAPES.items():
        for length in lens:
            eng = P.Engine(P.Config.from_hps(Hps.sac(batch_size=256), o, a, rb_capacity=length, seed=1), [-1.0] * a, [1.0] * a)
            eng.rb_fill_synthetic(length, seed=3)
            rb = P.ReplayBuffer(length)
            rb._bind(eng)
            every = torch.arange(length, device="cuda")
            g = torch.Generator().manual_seed(2)
            block = max(1, (64 << 20) // (4 * 1024))      # ring rows per cdist block at n = 1 024: a 256 MB matrix at most
            for n in QUERIES:
                q = torch.randn(n, o, generator=g).cuda()
                for k in KS:
                    def engine_route():
                        return eng.ring_knn(q, k)

                    def torch_route():
                        keys = rb.rows(every)["observations"]
                        best_d = best_i = None
                        for lo in range(0, length, block):
                            d, i = torch.topk(torch.cdist(q, keys[lo:lo + block]), min(k, length - lo), dim=1, largest=False)
                            d, i = (d, i + lo) if best_d is None else (torch.cat([best_d, d], 1), torch.cat([best_i, i + lo], 1))
                            best_d, pick = torch.topk(d, k, dim=1, largest=False)
                            best_i = torch.gather(i, 1, pick)
                        return best_i, best_d * best_d

                    call = engine_route if route == "engine" else torch_route
                    for _ in range(3):
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
                    out[f"{shape}-len{length}-n{n}-k{k}"] = {"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev)}
            del rb, every
            eng.close()
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def spread(v):
    return {"median": statistics.median(v), "range": [min(v), max(v)]}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_knn.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lens", default=",".join(str(x) for x in LENS))
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--bench", default=None, metavar="TREE")
    args = ap.parse_args()
    lens = [int(x) for x in args.lens.split(",")]
    if args.child:
        return child(args.child, lens)
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
    got = {"engine": [], "torch": []}
    for _ in range(args.runs):
        for route in got:      # alternating processes
            lines = run([sys.executable, __file__, "--child", route, "--lens", args.lens])
            got[route].append(json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][7:]))
            print(route, "done", flush=True)
    cases = {case: {route: {k: spread([r[case][k] for r in runs]) for k in ("wall_ms", "device_ms")} for route, runs in got.items()}
             for case in got["engine"][0]}
    for case, c in cases.items():
        shape, length, n = case.split("-")[0], int(case.split("-")[1][3:]), int(case.split("-")[2][1:])
        c["engine_median_below_torch_fastest"] = c["engine"]["device_ms"]["median"] < c["torch"]["device_ms"]["range"][0]
        c["ring_TBps"] = length * 4 * SHAPES[shape][0] * -(-n // 64) / (c["engine"]["device_ms"]["median"] * 1e-3) / 1e12
    merge(args.out, {"timing": {"what": "one Engine.ring_knn (key `state`) against the torch route (ReplayBuffer.rows(arange(len)), torch.cdist, "
                                        "torch.topk, blocks of 16 384 ring rows), ms; the ring filled by sactd3_rb_fill_synthetic; gathering the "
                                        "ring is charged to the torch route once per call; alternating fresh processes, 10 timed calls per "
                                        "configuration; ring_TBps: len x 4 ob_dim bytes per tile of 64 queries over the engine's median device "
                                        "time (gather kernels: 4.35 - 4.7 TB/s; memory: 8 TB/s); loop order: grid (ring slices) x (query tiles), "
                                        "one pass over the ring per query tile", "runs": args.runs, "reps": REPS, "cases": cases}})
    print(json.dumps(cases))


if __name__ == "__main__":
    main()
