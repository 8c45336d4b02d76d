"""Time the returns-to-go call (include/sactd3_returns.h) on an MI355X against the route it replaces: the ring materialised in torch
(ReplayBuffer.rows(arange(len))), a torch bit-compare of s' against s shifted by `stride`, then a reverse loop of len / stride torch
steps G[t] = r[t] + gamma * link[t] * G[t + 1] over rows of `stride` envs.

    python tools/returns_probe.py [--out profiles/returns.json] [--lens 65536,1000000] [--runs 5]

Alternating fresh processes, 5 per route, each timing every configuration; median and range of the processes' medians.  Device time:
events on torch's current stream around calls that are ordered against it; wall time: a host clock around the call and a device
synchronise.  The torch route's loop is cut at LOOP_CAP steps (a million dependent launches take tens of seconds): its figure is a
LOWER bound of that route wherever `torch_steps_timed` < `torch_steps`, which only makes the comparison harder for the engine.
`ring_TBps`: the bytes the link pass must read (len x 4 x (2 ob_dim + 2), s' and the successor's s and [r, d]) over the engine's
median device time of the whole call, beside the 4.35 - 4.7 TB/s of the gather kernels and the 8 TB/s of the memory."""
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
STRIDES, LENS, RUNS, REPS, LOOP_CAP, GAMMA = (1, 4, 4096), (65536, 1000000), 5, {"engine": 10, "torch": 3}, 2048, 0.99


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
            for stride in STRIDES:
                steps = -(-length // stride)

                def engine_route():
                    return eng.returns_to_go(GAMMA, stride)

                def torch_route():
                    rec = rb.rows(every)
                    s, sn, r, d = rec["observations"], rec["next_observations"], rec["rewards"].reshape(-1), rec["dones"].reshape(-1)
                    link = torch.zeros(steps * stride, device="cuda")
                    link[:length - stride] = ((sn[:length - stride].view(torch.int32) == s[stride:].view(torch.int32)).all(1) & (d[:length - stride] == 0)).float()
                    rr = torch.zeros(steps * stride, device="cuda")
                    rr[:length] = r
                    G, link, rr = torch.zeros(steps + 1, stride, device="cuda"), link.view(steps, stride), rr.view(steps, stride)
                    for t in range(steps - 1, max(steps - 1 - LOOP_CAP, -1), -1):
                        G[t] = rr[t] + GAMMA * link[t] * G[t + 1]
                    return G

                call = engine_route if route == "engine" else torch_route
                call()
                wall, dev = [], []
                for _ in range(REPS[route]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    dev.append(e0.elapsed_time(e1))
                out[f"{shape}-len{length}-stride{stride}"] = {"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev)}
            del rb, every
            eng.close()
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def spread(v):
    return {"median": statistics.median(v), "range": [min(v), max(v)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "returns.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lens", default=",".join(str(x) for x in LENS))
    ap.add_argument("--runs", type=int, default=RUNS)
    args = ap.parse_args()
    lens = [int(x) for x in args.lens.split(",")]
    if args.child:
        return child(args.child, lens)
    got = {"engine": [], "torch": []}
    for _ in range(args.runs):
        for route in got:      # alternating processes
            run = subprocess.run([sys.executable, __file__, "--child", route, "--lens", args.lens], capture_output=True, text=True, timeout=900, cwd=ROOT)
            if run.returncode != 0:
                raise SystemExit(run.stderr[-2000:])
            got[route].append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(route, "done", flush=True)
    cases = {case: {route: {k: spread([r[case][k] for r in runs]) for k in ("wall_ms", "device_ms")} for route, runs in got.items()}
             for case in got["engine"][0]}
    for case, c in cases.items():
        shape, length, stride = case.split("-")[0], int(case.split("-")[1][3:]), int(case.split("-")[2][6:])
        c["torch_steps"], c["torch_steps_timed"] = -(-length // stride), min(-(-length // stride), LOOP_CAP)
        c["engine_median_below_torch_fastest"] = c["engine"]["device_ms"]["median"] < c["torch"]["device_ms"]["range"][0]
        c["ring_TBps"] = length * 4 * (2 * SHAPES[shape][0] + 2) / (c["engine"]["device_ms"]["median"] * 1e-3) / 1e12
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec["timing"] = {"what": "one Engine.returns_to_go (gamma 0.99, all five outputs) against the torch route (ReplayBuffer.rows(arange(len)), bit-compare, "
                             "reverse loop cut at 2 048 steps: a lower bound of that route where torch_steps_timed < torch_steps), ms; the ring filled by "
                             "sactd3_rb_fill_synthetic; alternating fresh processes; ring_TBps: len x 4 (2 ob_dim + 2) bytes over the engine's median "
                             "device time of the whole call (gather kernels: 4.35 - 4.7 TB/s; memory: 8 TB/s)",
                     "runs": args.runs, "reps": REPS, "cases": cases}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(cases))


if __name__ == "__main__":
    main()
