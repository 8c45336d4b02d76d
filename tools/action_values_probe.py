"""Time the candidate-scoring call (include/sactd3_action_values.h) on an MI355X against the route it replaces, built from the API the
engine had before it: sactd3_policy_device N times for the samples, the observations repeated N-fold in torch, sactd3_qvalues_device on
n N rows and on the n data pairs, torch reductions for the summary.

    python tools/action_values_probe.py [--out profiles/action_values.json] [--test_log LOG]     # the call against the composed route
    python tools/action_values_probe.py --bench TREE                                              # bench.py of this checkout against TREE's

LOG: the output of `pytest -s tests/test_gpu_action_values.py` on the same machine; its "action_values" lines become the record's
`accuracy` block (the kernel's error as a fraction of the test's bound, worst case per output column).  TREE: a built checkout of the
parent commit.  Both modes merge into the output file and keep its other blocks.

Alternating fresh processes, 5 per route (3 per side for the benchmark), each timing every configuration; median and range of the
processes' medians.  Device time: events on torch's current stream around calls that are ordered against it; wall time: a host clock
around the call and a device synchronise."""
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
ROWS, CANDS, RUNS, REPS, BENCH_RUNS = (4, 256, 1024), (16, 64), 5, 30, 3


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
        stream = int(torch.cuda.current_stream().cuda_stream)
        for n in ROWS:
            obs, act = torch.randn(n, o, generator=g).cuda(), (torch.rand(n, a, generator=g) * 2 - 1).cuda()
            for N in CANDS:
                samp, lp = torch.empty(N, n, a, device="cuda"), torch.empty(N, n, device="cuda")
                q, qd = torch.empty(2, n * N, device="cuda"), torch.empty(2, n, device="cuda")

                def engine_route():
                    return eng.action_values(obs, act, candidates=N)["summary"]

                def composed_route():
                    for j in range(N):
                        eng.policy_device(obs.data_ptr(), o, n, {"sample": (samp[j].data_ptr(), a), "sample_logp": (lp[j].data_ptr(), 1)}, stream=stream)
                    rep, acts = obs.repeat_interleave(N, 0), samp.permute(1, 0, 2).reshape(n * N, a)
                    eng.q_values_device(rep.data_ptr(), o, acts.data_ptr(), a, n * N, False, q.data_ptr(), 1, n * N, stream)
                    eng.q_values_device(obs.data_ptr(), o, act.data_ptr(), a, n, False, qd.data_ptr(), 1, n, stream)
                    m, logp = q.min(0).values.view(n, N), lp.t()
                    q_max = m.max(1).values
                    return torch.stack([q_max, m.mean(1), torch.logsumexp(m, 1) - torch.log(torch.tensor(float(N))), m.std(1, unbiased=False),
                                        (m - 0.2 * logp).mean(1), qd.min(0).values, logp.mean(1), torch.isfinite(m).sum(1).float()], 1)

                call = engine_route if route == "engine" else composed_route
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
                out[f"{shape}-n{n}-N{N}"] = {"wall_ms": statistics.median(wall), "device_ms": statistics.median(dev)}
        eng.close()
    print("RESULT " + json.dumps(out))


def spread(v):
    return {"median": statistics.median(v), "range": [min(v), max(v)]}


def accuracy(log):
    """worst kernel error as a fraction of the bound the test holds it to, per output and column, over the test's cases"""
    worst = {}
    for ln in open(log):
        m = re.search(r"action_values (\(.*?\)) (\w+) kernel (\[.*?\]) bound (\[.*?\])", ln)
        if not m:
            continue
        err, bound = ast.literal_eval(m.group(3)), ast.literal_eval(m.group(4))
        for c, (e, b) in enumerate(zip(err, bound)):
            if b > 0:
                key = f"{m.group(2)}[{c}]"
                worst[key] = max(worst.get(key, 0.0), e / b)
    return {"what": "tests/test_gpu_action_values.py test 1: |kernel - float64| over the bound it is held to (K x the float32 CPU restatement's "
                    "yardstick; K = 4, 16 for summary[6] and for a policy candidate), worst case per column", "fraction_of_bound": worst}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_values.json"))
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
    got = {"engine": [], "composed": []}
    for _ in range(RUNS):
        for route in got:      # alternating processes
            lines = run([sys.executable, __file__, "--child", route])
            got[route].append(json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][7:]))
            print(route, "done", flush=True)
    cases = {case: {route: {k: spread([r[case][k] for r in runs]) for k in ("wall_ms", "device_ms")} for route, runs in got.items()}
             for case in got["engine"][0]}
    merge(args.out, {"timing": {"what": "one Engine.action_values (policy source, data actions given, summary + best action) against the composed "
                                        "route (policy_device x N, repeat, q_values_device x 2, torch reductions), ms; SAC, alternating fresh "
                                        "processes, 5 per route, 30 timed calls per configuration", "runs": RUNS, "reps": REPS, "cases": cases}})
    print(json.dumps(cases))


if __name__ == "__main__":
    main()
