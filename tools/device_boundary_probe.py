#!/usr/bin/env python3
"""The call-by-call API path on device tensors, measured: python tools/device_boundary_probe.py [workload ...] [--out FILE]

The reference's loop hands the agent CUDA tensors (orchestrator.py:100-113, :338-348).  One Agent + ReplayBuffer per workload of
bench.WORKLOADS (default: hopper_sac, humanoid_sac), `engine.device_inputs` toggled inside ONE process, the repeats of the two
routes interleaved (device host device host ...), host clock, median / min / max over 5 repeats:

  stage_us            host wall time per call of staging a caller-owned CUDA batch (Agent._stage: what every update_*(batch) pays)
  extend_us           host wall time per rb.extend of 4 rows of CUDA tensors
  api_loop_per_s      iterations per second of: rb.extend (4 rows) + update_qnets(batch) + every third iteration 2 x update_actor(batch)
                      + update_targ_nets, on dict-of-CUDA-tensor batches, 3 000 iterations after 300 of warm-up, closed by a sync
  kernel_us           device time (HIP events around 200 back-to-back launches, sactd3_time_kernel): the device route's two pack kernels
                      at the workload's shapes (batch_size rows / 4 rows); for the host route the replay gather, which is the kernel
                      its staged batch goes through (its two blocking copies and the host pack are inside stage_us, not here)

`device` = the arrays are read where they are (sactd3_load_batch_device / sactd3_rb_extend_fields_device); `host` = the route every
input took before: .cpu().numpy() per field, pack on the host, copy back.
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

REPEATS, CALLS, ITERS, WARMUP = 5, 200, 3000, 300
ROUTES = (("device", True), ("host", False))


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def probe(name):
    w = bench.WORKLOADS[name]
    o, a, B, n = w["o"], w["a"], w["batch"], 4
    hps = dict(batch_size=B, rb_capacity=100_000, num_envs=n, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ag = pkg.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                   dev, hps, pkg.ReplayBuffer(hps["rb_capacity"]))
    eng = ag.engine

    def td(rows, seed):
        g = torch.Generator().manual_seed(seed)
        done = torch.rand(rows, 1, generator=g) < 0.01
        return {"observations": torch.randn(rows, o, generator=g).to(dev), "next_observations": torch.randn(rows, o, generator=g).to(dev),
                "actions": ((torch.rand(rows, a, generator=g) * 2 - 1) * w["bound"]).to(dev), "rewards": torch.randn(rows, 1, generator=g).to(dev),
                "terminations": done.to(dev), "dones": done.to(dev)}
    batches, steps = [td(B, k) for k in range(4)], [td(n, 10 + k) for k in range(4)]

    def iteration(i):
        ag.rb.extend(steps[i % 4])
        batch = batches[i % 4]
        ag.update_qnets(batch)
        ag.qnet_updates_so_far += 1
        if i % 3 == 0:
            ag.update_actor(batch)
            ag.update_actor(batch)
        ag.update_targ_nets()

    def per_call_us(f):
        eng.sync()
        t = time.perf_counter()
        for k in range(CALLS):
            f(k)
        dt = time.perf_counter() - t
        eng.sync()
        return dt / CALLS * 1e6

    def rate():
        for i in range(WARMUP):
            iteration(i)
        eng.sync()
        t = time.perf_counter()
        for i in range(ITERS):
            iteration(i)
        eng.sync()
        return ITERS / (time.perf_counter() - t)

    for _, on in ROUTES:      # warm both routes: graphs, the runtime's signal pools, torch's allocator
        eng.device_inputs = on
        for i in range(WARMUP):
            iteration(i)
    eng.sync()
    vals = {k: {r: [] for r, _ in ROUTES} for k in ("stage_us", "extend_us", "api_loop_per_s")}
    for _ in range(REPEATS):
        for route, on in ROUTES:
            eng.device_inputs = on
            vals["stage_us"][route].append(per_call_us(lambda k: ag._stage(batches[k % 4])))
            vals["extend_us"][route].append(per_call_us(lambda k: ag.rb.extend(steps[k % 4])))
    for _ in range(REPEATS):
        for route, on in ROUTES:
            eng.device_inputs = on
            vals["api_loop_per_s"][route].append(rate())
    eng.device_inputs = True
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "batch_size": B, "extend_rows": n, "repeats": REPEATS, "calls_per_repeat": CALLS,
           "loop_iterations": ITERS, "loop_warmup": WARMUP, "batch_bytes": 4 * B * (2 * o + a + 1) + B}
    for k, d in vals.items():
        out[k] = {r: summary(v, 1 if k.endswith("per_s") else 2) for r, v in d.items()}
    out["kernel_us"] = {"device": {"k_batch_from_fields": round(eng.time_kernel("batch_from_fields", 200), 2),
                                   "k_rb_ingest_fields": round(eng.time_kernel("rb_ingest_fields", 200), 2)},
                        "host": {"k_gather": round(eng.time_kernel("gather", 200), 2)}}
    out["boundary_stats"] = eng.boundary_stats()
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
            json.dump({"tool": "tools/device_boundary_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
