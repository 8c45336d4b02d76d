#!/usr/bin/env python3
"""Acting for a GPU-resident vector env, measured: python tools/device_acting_probe.py [workload ...] [--rows 4,64,1024] [--ab FILE] [--out FILE]

One Agent per (workload of bench.WORKLOADS, number of envs n) holds both routes in ONE process; the repeats of the two routes are
interleaved (device host device host ...), host clock unless said otherwise, median / min / max over 5 repeats:

  call_us             (a) host wall time per Agent.predict_device call (200 calls, contiguous CUDA observations, preallocated `out`)
  device_us           (b) device time per call: HIP events on the engine's stream around 200 back-to-back sactd3_predict_device calls
                      (no event waits inserted); when the host issues a call slower than the GPU runs it, this is the host's pace
  kernel_us           (b) the pack and unpack kernels alone (sactd3_time_kernel, max_envs = n rows)
  loop_per_s          (c) env steps per second of  choose -> step(i % 3 == 0) -> advance  on loop.SyntheticDeviceVecEnv, 3 000 iterations
                      after 300, closed by one synchronisation.  `device` = loop.DeviceRollout (predict_device; nothing waits on the
                      host inside the loop); `host_copy` = the only route device observations had before: obs.cpu() -> predict ->
                      torch.as_tensor(actions).to(device), then the same env step and the same rb.extend of device tensors
  host_predict_us     for scale: Agent.predict on host observations of the same n

--ab FILE embeds the lines tools/two_builds_ab.py printed in the same visit (parent build against this one: step / period rate).
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

REPEATS, CALLS, ITERS, WARMUP = 5, 200, 3000, 300


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


class HostCopyRollout(loop.DeviceRollout):
    """the device env driven through the host call: the observations go to the host, the actions come back"""

    def choose(self):
        actions = self.agent.predict({"observations": self.obs.cpu()}, explore=True)
        self.actions = torch.as_tensor(actions).to(self.obs.device)


def probe(name, n, iters=ITERS, warmup=WARMUP, repeats=REPEATS):
    w = bench.WORKLOADS[name]
    o, a, B = w["o"], w["a"], w["batch"]
    hps = dict(batch_size=B, rb_capacity=100_000, num_envs=n, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ag = pkg.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                   dev, hps, pkg.ReplayBuffer(hps["rb_capacity"]))
    eng = ag.engine
    eng.rb_fill_synthetic(20_000, seed=0)
    eng.instantiate_graphs()
    obs = torch.randn(n, o, device=dev)
    out = torch.empty(n, a, device=dev)
    obs_host = obs.cpu().numpy()
    td = {"observations": obs}

    def per_call_us(f, calls=CALLS):
        torch.cuda.synchronize()
        eng.sync()
        t = time.perf_counter()
        for _ in range(calls):
            f()
        dt = time.perf_counter() - t
        torch.cuda.synchronize()
        eng.sync()
        return dt / calls * 1e6

    def device_us():
        torch.cuda.synchronize()
        eng.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        args = (obs.data_ptr(), o, n, True, out.data_ptr(), a, 0, False)
        t0.record(ag._ext_stream)
        for _ in range(CALLS):
            eng.predict_device(*args)
        t1.record(ag._ext_stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / CALLS

    rollouts = {}
    for route, cls in (("device", loop.DeviceRollout), ("host_copy", HostCopyRollout)):
        env = loop.SyntheticDeviceVecEnv(o, a, n, horizon=200, term_at=6.0, bound=w["bound"], device=dev)
        rollouts[route] = cls(env, ag, 0, 0, 1)                         # learning_starts = 0: every action comes from the policy

    def rate(ro, count):
        for i in range(warmup):
            ro.choose(); eng.step(i % 3 == 0); ro.advance()
        torch.cuda.synchronize()
        eng.sync()
        t = time.perf_counter()
        for i in range(count):
            ro.choose(); eng.step(i % 3 == 0); ro.advance()
        torch.cuda.synchronize()
        eng.sync()
        return count / (time.perf_counter() - t)

    for ro in rollouts.values():                                        # warm: graphs, signal pools, torch's allocator
        rate(ro, warmup)
    per_call_us(lambda: ag.predict_device(td, explore=True, out=out))
    vals = {"call_us": [], "device_us": [], "host_predict_us": [], "loop_per_s": {r: [] for r in rollouts}}
    for _ in range(repeats):
        vals["call_us"].append(per_call_us(lambda: ag.predict_device(td, explore=True, out=out)))
        vals["host_predict_us"].append(per_call_us(lambda: eng.predict(obs_host, True)))
        vals["device_us"].append(device_us())
    for _ in range(repeats):
        for route, ro in rollouts.items():
            vals["loop_per_s"][route].append(rate(ro, iters))
    res = {"workload": name, "ob_dim": o, "ac_dim": a, "batch_size": B, "envs": n, "repeats": repeats, "calls_per_repeat": CALLS,
           "loop_iterations": iters, "loop_warmup": warmup,
           "call_us": summary(vals["call_us"]), "device_us": summary(vals["device_us"]), "host_predict_us": summary(vals["host_predict_us"]),
           "kernel_us": {"k_obs_from_field": round(eng.time_kernel("obs_from_field", 200), 2),
                         "k_act_to_field": round(eng.time_kernel("act_to_field", 200), 2)},
           "loop_per_s": {r: summary(v, 1) for r, v in vals["loop_per_s"].items()},
           "predict_device_stats": eng.predict_device_stats(), "boundary_stats": eng.boundary_stats()}
    res["loop_device_over_host_copy"] = round(res["loop_per_s"]["device"]["median"] / res["loop_per_s"]["host_copy"]["median"], 3)
    eng.close()
    return res


def main(argv):
    opts = {"--out": None, "--ab": None, "--rows": "4,64,1024", "--iters": str(ITERS), "--repeats": str(REPEATS)}
    for k in list(opts):
        if k in argv:
            i = argv.index(k)
            opts[k] = argv[i + 1]
            argv = argv[:i] + argv[i + 2:]
    iters, repeats = int(opts["--iters"]), int(opts["--repeats"])
    res = []

    def dump():
        if opts["--out"]:
            doc = {"tool": "tools/device_acting_probe.py", "device": torch.cuda.get_device_name(0), "shapes": res}
            if opts["--ab"]:
                doc["two_builds_ab"] = [json.loads(ln) for ln in open(opts["--ab"]) if ln.startswith("{")]
            with open(opts["--out"], "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")
    for name in argv or ["hopper_sac", "halfcheetah_td3", "humanoid_sac"]:
        for n in [int(x) for x in opts["--rows"].split(",")]:
            res.append(probe(name, n, iters, max(iters // 10, 1), repeats))
            print(json.dumps(res[-1]), flush=True)
            dump()
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
