#!/usr/bin/env python3
"""One prioritised-replay iteration on the device, measured: python tools/prioritized_probe.py [workload ...] [--out FILE]

On one Agent per workload of bench.WORKLOADS (default: hopper_sac at B = 256 and humanoid_sac at B = 1024), a 4096-row ring and a
loop.ProportionalSampler over it, two ways of writing the same iteration, in ONE process, their repeats interleaved, median / min / max
over 5 repeats of 200 iterations.  Nothing here is a pass/fail bar: the probe records what it finds.

  staged     sampler.sample -> rb.sample_at(index, weights) -> agent.update_qnets(handle) -> agent.td_errors() -> sampler.update:
             the rows never leave the ring, the critic loss carries the importance weights, the TD errors are the update's own
  readout    the same loop against the calls that existed before: sampler.sample -> rb.rows(index) (six tensors out) ->
             agent.update_qnets(those tensors) (packed back into the batch slot; no loss weights: there was no way to pass them) ->
             TD errors restated in torch from two agent.q_values calls, Q(s, a) - [r + gamma (1 - d) min Q_targ(s', pi(s'))] (no
             entropy term: the policy draw of the update cannot be had from outside) -> sampler.update

  wall_us    host wall time per iteration; the window is closed by a synchronisation of the engine's and torch's streams
  device_us  torch events on torch's current stream around the same 200 iterations (every call of both routes is ordered against it)
  kernel_us  sactd3_time_kernel of the staging and TD read-out kernels on batch_size rows, beside the two kernels of the old route
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

REPEATS, ITERS, ROWS = 5, 200, 4096


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def probe(name):
    w = bench.WORKLOADS[name]
    o, a, B = w["o"], w["a"], w["batch"]
    hps = dict(batch_size=B, rb_capacity=ROWS, num_envs=4, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    ag = pkg.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                   dev, hps, pkg.ReplayBuffer(ROWS))
    eng, gamma = ag.engine, float(ag.engine.cfg.gamma)
    eng.rb_fill_synthetic(ROWS, 1)
    sampler = loop.ProportionalSampler(ROWS, alpha=0.6, beta=0.4, eps=1e-6, device=dev)
    sampler.extend(ROWS)
    td_out = torch.empty(2, B, 1, device=dev)
    q_out, qn_out = torch.empty(2, B, 1, device=dev), torch.empty(2, B, 1, device=dev)

    def staged():
        index, weights = sampler.sample(B)
        ag.update_qnets(ag.rb.sample_at(index, weights))
        sampler.update(index, ag.td_errors(out=td_out))

    def readout():
        index, _ = sampler.sample(B)
        rows = ag.rb.rows(index)
        ag.update_qnets(rows)
        q = ag.q_values(rows, out=q_out)
        qn = ag.q_values({"observations": rows["next_observations"]}, target=True, out=qn_out)
        y = rows["rewards"] + gamma * (~rows["dones"]) * qn.min(0).values
        sampler.update(index, q - y)

    routes = (("staged", staged), ("readout", readout))
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
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "batch": B, "ring_rows": ROWS, "repeats": REPEATS, "iterations_per_repeat": ITERS,
           "wall_us": {r: summary(v) for r, v in wall.items()}, "device_us": {r: summary(v) for r, v in device.items()},
           "wall_ratio_readout_over_staged": round(statistics.median(wall["readout"]) / statistics.median(wall["staged"]), 3),
           "loss_finite": bool(np.isfinite(eng.read_metrics()["loss/qf_loss"])), "priority_stats": eng.priority_stats()}
    out["kernel_us"] = {k: round(eng.time_kernel(k, 200), 2) for k in ("batch_from_index", "td_to_field", "rows_to_fields", "batch_from_fields")}
    eng.close()
    return out


def main(argv):
    path = None
    if "--out" in argv:
        k = argv.index("--out")
        path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    res = []
    for name in argv or ["hopper_sac", "humanoid_sac"]:
        res.append(probe(name))
        print(json.dumps(res[-1]), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"tool": "tools/prioritized_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
