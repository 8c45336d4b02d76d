#!/usr/bin/env python3
"""The way OUT of the engine, measured: python tools/device_readout_probe.py [workload ...] [--out FILE]

The reference's rb.sample() returns a device TensorDict (main.py:167-171, orchestrator.py:338).  One Agent + ReplayBuffer per workload of
bench.WORKLOADS (default: hopper_sac, humanoid_sac), both read-backs in ONE process, their repeats interleaved (device host device host
...), host clock, median / min / max over 5 repeats:

  touch_us            host wall time per "rb.sample(B), then have batch['observations'] as a CUDA tensor torch can compute on":
                      `device` = BatchHandle.on_device() (one k_batch_to_fields launch, no host wait);
                      `host`   = the read-back as it was before (sactd3_read_batch: a stream synchronise, five copies to the host and an
                                 unpack) followed by torch.as_tensor(...).cuda() -- the baseline
                      (200 calls per repeat; the window is closed by a synchronisation of the engine's and torch's streams, inside the figure)
  kernel_us           device time (HIP events around 200 back-to-back launches, sactd3_time_kernel) of the two read-out kernels on
                      batch_size rows, next to the replay gather that filled the slot

and once, on a Humanoid ring of 100 000 rows that is full: k_rows_to_fields for 65 536 rows with indices drawn by torch.randint --
device time between two events on the engine's stream around 20 back-to-back unordered calls, a fresh index set each -- beside sactd3_time_gather_sweep at the same n in
the same process, 5 alternating repeats: the gather (aligned 16-byte stores into a packed slot) is the yardstick, and `ratio` says
what the dword stores to the caller's unaligned rows cost.
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
from sac_td3_cudagraphs_pytorch_amd import agent as agent_mod  # noqa: E402

REPEATS, CALLS = 5, 200
BIG_N, BIG_RING, BIG_CALLS = 65536, 100_000, 20


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make_agent(w, capacity):
    o, a, B = w["o"], w["a"], w["batch"]
    hps = dict(batch_size=B, rb_capacity=capacity, num_envs=4, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    torch.manual_seed(0)
    return pkg.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                     torch.device("cuda", 0), hps, pkg.ReplayBuffer(capacity))


def probe(name):
    w = bench.WORKLOADS[name]
    o, a, B = w["o"], w["a"], w["batch"]
    ag = make_agent(w, 100_000)
    eng, rb = ag.engine, ag.rb
    eng.rb_fill_synthetic(100_000, seed=0)
    dev = torch.device("cuda", 0)
    sink = torch.zeros((), device=dev)

    def touch_device():
        batch = rb.sample(B)
        sink.add_(batch.on_device()["observations"][0, 0])

    def touch_host():
        batch = rb.sample(B)
        sink.add_(torch.as_tensor(batch["observations"]).cuda()[0, 0])

    def per_call_us(f):
        eng.sync()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(CALLS):
            f()
        eng.sync()
        torch.cuda.synchronize()                                 # the window ends when the device has done the work, on either route
        return (time.perf_counter() - t) / CALLS * 1e6

    routes = (("device", touch_device), ("host", touch_host))
    for _, f in routes:      # warm both: the events, torch's allocator, the runtime's signal pools
        for _ in range(300):
            f()
    vals = {r: [] for r, _ in routes}
    for _ in range(REPEATS):
        for r, f in routes:
            vals[r].append(per_call_us(f))
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "batch_size": B, "repeats": REPEATS, "calls_per_repeat": CALLS,
           "batch_bytes": 4 * B * (2 * o + a + 1) + B + 8 * B,
           "touch_us": {r: summary(v) for r, v in vals.items()}}
    out["touch_us"]["host_over_device"] = round(out["touch_us"]["host"]["median"] / out["touch_us"]["device"]["median"], 2)
    eng.rb_sample()
    out["kernel_us"] = {"k_batch_to_fields": round(eng.time_kernel("batch_to_fields", 200), 2),
                        "k_rows_to_fields": round(eng.time_kernel("rows_to_fields", 200), 2),
                        "k_gather": round(eng.time_kernel("gather", 200), 2)}
    out["readout_stats"] = eng.readout_stats()
    eng.close()
    return out


def probe_large():
    """65 536 Humanoid rows out of a full ring: k_rows_to_fields beside the gather sweep at the same n"""
    w = bench.WORKLOADS["humanoid_sac"]
    ag = make_agent(w, BIG_RING)
    eng = ag.engine
    eng.rb_fill_synthetic(BIG_RING, seed=0)
    dev = torch.device("cuda", 0)
    idx = [torch.randint(0, BIG_RING, (BIG_N,), device=dev, generator=torch.Generator(device=dev).manual_seed(k)) for k in range(BIG_CALLS)]
    outs, fields = agent_mod._device_outputs(eng, BIG_N)         # the destinations, allocated once
    learner = ag._ext_stream                                     # the engine's own stream, as torch sees it
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def rows_us():
        torch.cuda.synchronize()
        eng.sync()
        t0.record(learner)                                       # unordered calls: nothing but the launches between the two events
        for k in range(BIG_CALLS):
            eng.rb_read_rows_device(idx[k].data_ptr(), 1, BIG_N, fields, ordered=False)
        t1.record(learner)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / BIG_CALLS

    rows_us()
    eng.time_gather_sweep(BIG_N, BIG_CALLS)
    r, g, nbytes = [], [], 0.0
    for _ in range(REPEATS):
        r.append(rows_us())
        us, nbytes = eng.time_gather_sweep(BIG_N, BIG_CALLS)
        g.append(us)
    out = {"workload": "humanoid_sac", "rows": BIG_N, "ring_rows": BIG_RING, "calls_per_repeat": BIG_CALLS, "repeats": REPEATS,
           "k_rows_to_fields_us": summary(r), "k_gather_us": summary(g), "algo_bytes": nbytes,
           "rows_GBps": round(nbytes / statistics.median(r) * 1e-3, 1), "gather_GBps": round(nbytes / statistics.median(g) * 1e-3, 1),
           "ratio_rows_over_gather": round(statistics.median(r) / statistics.median(g), 3), "readout_stats": eng.readout_stats()}
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
    large = probe_large()
    print(json.dumps(large), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"tool": "tools/device_readout_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res, "large_rows": large}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
