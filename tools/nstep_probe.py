#!/usr/bin/env python3
"""What the n-step staging costs, measured beside the 1-step staging it extends:
python tools/nstep_probe.py [--out profiles/nstep.json]

Shapes: the three BASELINE workloads (SAC Hopper B = 256 and TD3 HalfCheetah B = 256 over 100 000 rows, SAC Humanoid B = 1024 over the
full 1 000 000-row ring, filled by sactd3_rb_fill_synthetic).  Nothing here is a pass/fail bar: the probe records what it finds.

  staging_us   device time of one sactd3_rb_sample_nstep_device call at steps 1, 3, 5 and 16 (stride 4, B uniform random start slots, no
               weights): torch events on torch's current stream around 200 calls -- every call is ordered against that stream --
               median / min / max over 5 repeats, the step counts interleaved.  The synthetic rows are unrelated, so every chain is
               cut after its first row; the kernel issues the loads of all `steps` candidate links whatever they hold, so this is the
               full traffic of the link phase, B (steps + 1) records' worth, with the copy phase of a 1-step staging behind it.
  kernel_us    sactd3_time_kernel("batch_from_index") and ("batch_from_index_nstep") (steps 3, stride 1), same engine, same run
  loop         loop.train(fused=False) on loop.SyntheticVecEnv (4 envs, horizon 50) at n_step 1 and 3: gradient steps per second
               over the learning phase of one run each, and what sactd3_nstep_stats counted
"""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import sac_td3_cudagraphs_pytorch_amd as pkg  # noqa: E402
from sac_td3_cudagraphs_pytorch_amd import loop  # noqa: E402

REPEATS, ITERS = 5, 200
SHAPES = ("hopper_sac", "halfcheetah_td3", "humanoid_sac")
STEPS = (1, 3, 5, 16)
STRIDE = 4


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def probe(name):
    w = bench.WORKLOADS[name]
    o, a, B, rows = w["o"], w["a"], w["batch"], w["rows"]
    hps = dict(batch_size=B, rb_capacity=rows, num_envs=STRIDE, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    ag = pkg.Agent({"ob_shape": (STRIDE, o), "ac_shape": (STRIDE, a)}, np.full(a, -w["bound"], np.float32),
                   np.full(a, w["bound"], np.float32), dev, hps, pkg.ReplayBuffer(rows))
    eng = ag.engine
    eng.rb_fill_synthetic(rows, 1)
    idx = torch.randint(0, rows, (B,), device=dev, dtype=torch.int64, generator=torch.Generator(device=dev).manual_seed(1))
    stream = int(torch.cuda.current_stream(0).cuda_stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(steps):
        eng.sync()
        torch.cuda.synchronize()
        t0.record()
        for _ in range(ITERS):
            eng.rb_sample_nstep_device(idx.data_ptr(), 1, 0, 1, B, steps, STRIDE, stream)
        t1.record()
        eng.sync()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / ITERS

    for s in STEPS:
        timed(s)
    dev_us = {s: [] for s in STEPS}
    for _ in range(REPEATS):
        for s in STEPS:
            dev_us[s].append(timed(s))
    eng.rb_sample()                                              # (time_kernel takes its indices from the current slot's)
    rec = eng.rb_layout()["record_floats"] * 4
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "batch": B, "ring_rows": rows, "record_bytes": rec, "stride": STRIDE,
           "repeats": REPEATS, "calls_per_repeat": ITERS,
           "staging_us": {str(s): summary(v) for s, v in dev_us.items()},
           "expected_mbytes": {str(s): round(B * (s + 1) * rec / 1e6, 3) for s in STEPS},
           "kernel_us": {k: round(eng.time_kernel(k, 200), 2) for k in ("batch_from_index", "batch_from_index_nstep")},
           "nstep_stats": eng.nstep_stats()}
    eng.close()
    return out


def loop_rate(n_step):
    o, a, n = 11, 3, 4
    from oracle.sac_td3_ref import Hps
    cfg = SimpleNamespace(**{**Hps.sac(batch_size=256).__dict__, "seed": 0, "num_envs": n, "action_repeat": 1, "learning_starts": 1000,
                             "num_timesteps": 9000, "eval_every": 10 ** 9, "cudagraphs": True, "rb_capacity": 20000})
    env = loop.SyntheticVecEnv(o, a, n)
    env.action_space.seed(0)
    torch.manual_seed(0)
    ag = pkg.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -1.0, np.float32), np.full(a, 1.0, np.float32),
                   torch.device("cuda", 0), cfg, pkg.ReplayBuffer(cfg.rb_capacity))
    warm = SimpleNamespace(**{**cfg.__dict__, "num_timesteps": 1400})
    loop.train(warm, env, ag, fused=False, n_step=n_step)        # the random phase and the first hundred iterations: graphs, scratch
    ag.engine.sync()
    done0, t = ag.qnet_updates_so_far, time.perf_counter()
    m = loop.train(cfg, env, ag, fused=False, n_step=n_step)
    ag.engine.sync()
    dt = time.perf_counter() - t
    out = {"n_step": n_step, "gradient_steps": int(ag.qnet_updates_so_far - done0), "seconds": round(dt, 3),
           "gradient_steps_per_s": round((ag.qnet_updates_so_far - done0) / dt, 1), "loss_finite": bool(np.isfinite(m["loss/qf_loss"])),
           "nstep_stats": ag.engine.nstep_stats()}
    ag.engine.close()
    return out


def main(argv):
    path = None
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    res = []
    for name in SHAPES:
        res.append(probe(name))
        print(json.dumps(res[-1]), flush=True)
    loops = [loop_rate(1), loop_rate(3)]
    for r in loops:
        print(json.dumps(r), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"tool": "tools/nstep_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res,
                       "loop_fused_false_hopper_shape_b256": loops}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
