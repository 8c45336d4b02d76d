"""Time the dormant-neuron scan and the ReDo recycler (include/sactd3_dormant.h) on an MI355X against the route a user had before them:
get_params for both nets (each a stream synchronisation), the three MLPs restated in torch on the GPU, the scores read back.  The host
route is given the rows as a device tensor it already holds (no ReplayBuffer.rows call): that flatters it.

    python tools/dormant_probe.py [--out profiles/dormant.json] [--test_log LOG]

LOG: the output of `pytest -s tests/test_gpu_dormant.py` on the same machine; its "dormant scores" lines become the record's
`score_errors` block.  Without it the block the output file already holds is kept.

Alternating fresh processes, 5 per route and configuration; median and range.  Device time: events on torch's current stream around
calls that are ordered against it; wall time: a host clock around the call and the wait for its result."""
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
ROWS, RUNS, REPS, CAP = (256, 1024, 16384), 5, 30, 1 << 16


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
        return eng.dormant_scan(idx, tau=0.025)["dormant"]

    def host_route():
        params = {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS)}
        counts = []
        for _, K, nh, flat in init_model.nets_of(params, o, a, False):
            p = {(k, l): torch.as_tensor(np.array(v)).cuda() for k, l, v in init_model.split(flat, K, nh, True)}
            h = x[idx, :K]
            for l in (0, 1):
                h = torch.relu(torch.nn.functional.layer_norm(h @ p[("weight", l)].T + p[("bias", l)], (256,), p[("ln_weight", l)], p[("ln_bias", l)]))
                m = h.mean(0)
                counts.append(int((m / m.mean() <= 0.025).sum()))
        return counts

    call = engine_route if route == "engine" else host_route
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
    out = {"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev)}
    if route == "engine":      # one scan + redo per repetition; the redo alone between two host clocks, enqueue and wait
        t = []
        for k in range(REPS):
            eng.dormant_scan(idx, tau=10.0)      # (marks most units: a redo with work to do)
            eng.sync()
            t0 = time.perf_counter()
            eng.redo(("actor", "critics"), epoch=k + 1)
            eng.sync()
            t.append((time.perf_counter() - t0) * 1e3)
        out["redo_wall_ms"] = statistics.median(t)
    eng.close()
    print("RESULT " + json.dumps(out))


def score_errors(log, out):
    """the `score_errors` block: from the test's printed figures, else what the record held before"""
    if log is None:
        return json.load(open(out)).get("score_errors") if os.path.exists(out) else None
    rows = [[json.loads(v) for v in re.search(r"kernel (\[.*?\]) bound (\[.*?\])", ln).groups()] for ln in open(log) if "dormant scores" in ln]
    kernel, bound = [x for k, _ in rows for x in k], [x for _, b in rows for x in b]
    return {"what": "tests/test_gpu_dormant.py test 1: max |score - float64| per (net, layer) pair over its cases", "cases": len(rows),
            "kernel": [min(kernel), max(kernel)], "cpu_float32_restatement": [min(bound) / 4, max(bound) / 4],
            "bound": "4 x the cpu_float32 error of the same case and pair", "worst_kernel_over_bound": max(k / b for k, b in zip(kernel, bound))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dormant.json"))
    ap.add_argument("--child", nargs=3, default=None)
    ap.add_argument("--test_log", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]))
    rec, errors = {}, score_errors(args.test_log, args.out)
    for shape in SHAPES:
        for rows in ROWS:
            got = {"engine": [], "host": []}
            for _ in range(RUNS):
                for route in got:      # alternating processes
                    out = subprocess.run([sys.executable, __file__, "--child", route, shape, str(rows)], capture_output=True, text=True, timeout=300)
                    if out.returncode != 0:
                        raise SystemExit(out.stderr[-2000:])
                    got[route].append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            rec[f"{shape}-{rows}"] = {route: {k: {"median": statistics.median(r[k] for r in runs), "range": [min(r[k] for r in runs), max(r[k] for r in runs)]}
                                              for k in runs[0]} for route, runs in got.items()}
            print(shape, rows, json.dumps(rec[f"{shape}-{rows}"]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"what": "dormant_scan / redo against the host route, ms; alternating processes, 5 runs each", "runs": RUNS, "reps": REPS, "cases": rec,
                   **({"score_errors": errors} if errors else {})}, f, indent=1)


if __name__ == "__main__":
    main()
