#!/usr/bin/env python3
"""One prioritised-replay iteration with the priorities kept by the engine, measured against the route that existed before:
python tools/native_priorities_probe.py [--out profiles/native_priorities.json]

Shapes: SAC Hopper at B = 256 over a 100 000-row ring, SAC Humanoid at B = 1024 over the full 1 000 000-row ring (both filled by
sactd3_rb_fill_synthetic).  Two ways of writing the same iteration -- sample, weighted critic update, write-back -- on ONE agent, in
ONE process, their repeats interleaved, median / min / max over 5 repeats of 200 iterations.  Nothing here is a pass/fail bar: the probe
records what it finds.

  native     rb.sample_prioritized(B, beta) -> agent.update_qnets(handle) -> rb.update_priorities(): five launches around the critic
             update's graph, no torch arithmetic
  sampler    loop.ProportionalSampler.sample -> rb.sample_at(index, weights) -> agent.update_qnets(handle) -> agent.td_errors() ->
             sampler.update: the priorities in a torch tensor, a pow / sum / multinomial over the whole ring per iteration

  wall_us    host wall time per iteration; the window is closed by a synchronisation of the engine's and torch's streams
  device_us  torch events on torch's current stream around the sampler route's 200 iterations (every call of that route is ordered
             against it; the native route never touches torch's stream, so it has no such figure)
  kernel_us  sactd3_time_kernel("prio_sample") (the three launches of a prioritised sample) and ("prio_update") (the write-back kernel)
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import sac_td3_cudagraphs_pytorch_amd as pkg  # noqa: E402
from sac_td3_cudagraphs_pytorch_amd import loop  # noqa: E402

REPEATS, ITERS = 5, 200
SHAPES = (("hopper_sac", 256, 100_000), ("humanoid_sac", 1024, 1_000_000))
ALPHA, BETA, EPS = 0.6, 0.4, 1e-6


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def probe(name, B, rows):
    w = bench.WORKLOADS[name]
    o, a = w["o"], w["a"]
    hps = dict(batch_size=B, rb_capacity=rows, num_envs=4, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    ag = pkg.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                   dev, hps, pkg.ReplayBuffer(rows))
    eng = ag.engine
    ag.rb.enable_priorities(alpha=ALPHA, eps=EPS)
    eng.rb_fill_synthetic(rows, 1)
    sampler = loop.ProportionalSampler(rows, alpha=ALPHA, beta=BETA, eps=EPS, device=dev)
    sampler.extend(rows)
    td_out = torch.empty(2, B, 1, device=dev)

    def native():
        ag.update_qnets(ag.rb.sample_prioritized(B, BETA))
        ag.rb.update_priorities()

    def by_sampler():
        index, weights = sampler.sample(B)
        ag.update_qnets(ag.rb.sample_at(index, weights))
        sampler.update(index, ag.td_errors(out=td_out))

    routes = (("native", native), ("sampler", by_sampler))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        eng.sync()
        torch.cuda.synchronize()
        t0.record()
        t = time.perf_counter()
        for _ in range(ITERS):
            f()
        t1.record()
        eng.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / ITERS * 1e6, t0.elapsed_time(t1) * 1e3 / ITERS

    for _, f in routes:                                          # warm both: graphs, scratch, events, torch's allocator and kernels
        for _ in range(30):
            f()
    wall, device = {r: [] for r, _ in routes}, {r: [] for r, _ in routes}
    for _ in range(REPEATS):
        for r, f in routes:
            wl, dv = timed(f)
            wall[r].append(wl)
            device[r].append(dv)
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "batch": B, "ring_rows": rows, "alpha": ALPHA, "beta": BETA,
           "repeats": REPEATS, "iterations_per_repeat": ITERS,
           "wall_us": {r: summary(v) for r, v in wall.items()}, "device_us": {"sampler": summary(device["sampler"])},
           "wall_ratio_sampler_over_native": round(statistics.median(wall["sampler"]) / statistics.median(wall["native"]), 3),
           "loss_finite": bool(np.isfinite(eng.read_metrics()["loss/qf_loss"])), "prio_stats": eng.prio_stats(),
           "priority_stats": eng.priority_stats()}
    out["kernel_us"] = {k: round(eng.time_kernel(k, 200), 2) for k in ("prio_sample", "prio_update")}
    eng.close()
    return out


def main(argv):
    path = None
    if "--out" in argv:
        k = argv.index("--out")
        path = argv[k + 1]
    res = []
    for name, B, rows in SHAPES:
        res.append(probe(name, B, rows))
        print(json.dumps(res[-1]), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"tool": "tools/native_priorities_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
