#!/usr/bin/env python3
"""Querying the policy, measured: python tools/policy_probe.py [workload ...] [--out FILE] [--merge FILE]

Agent.policy / sactd3_policy_device (include/sactd3.h) on one Agent per workload of bench.WORKLOADS (default: the three BASELINE
shapes), at n = 4, 256, 1024 and 65 536 rows of CUDA tensors, asking for `mode` only and for everything (SAC: given actions and a
native sample -> mode, mean, log_std, sample, sample_log_prob, eps, log_prob; TD3 has `mode` only, so its two cases coincide); beside it
the only way there was before -- the host alternative: get_params(ACTOR), the reference's actor rebuilt as torch tensors on cuda:0,
and torch's forward pass (with torch.randn draws and the same formulas) on the same rows.  All routes in ONE process, their repeats
interleaved, median / min / max over 5 repeats.  Nothing here is a pass/fail bar: the probe records what it finds.

  wall_us             host wall time per call (200 calls per repeat, 20 at 65 536 rows); the window is closed by a synchronisation of
                      the engine's and torch's streams, inside the figure (`device`: Agent.policy into preallocated `out` arrays;
                      `host_alternative`: get_params + upload + torch forward, every call -- the parameters change with every update)
  device_us           HIP events on the engine's stream around back-to-back unordered sactd3_policy_device calls
  torch_forward_us    the torch forward alone on parameters already uploaded (what the alternative costs when nothing was updated)
  kernel_us           sactd3_time_kernel("pi_head"): the head kernel alone on 1024 rows, every output wanted
  max_abs_diff        |engine - torch| over `mode`: a sanity figure, not a parity test (tests/test_gpu_policy.py is)

--merge FILE: a JSON object whose keys are copied into the output beside "workloads" (the measurements that nothing else moved --
the assembly comparison and the bench.py runs of the parent commit against this tree -- which are taken outside this process).
"""
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
import sac_td3_cudagraphs_pytorch_amd as pkg  # noqa: E402
from sac_td3_cudagraphs_pytorch_amd import _lib, schema  # noqa: E402

REPEATS = 5
ROWS = (4, 256, 1024, 65536)
KEYS = {"mode": "mode", "mean": "mean", "log_std": "log_std", "sample": "sample", "sample_log_prob": "sample_logp", "eps": "eps_out",
        "log_prob": "action_logp"}


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make_agent(w):
    o, a, B = w["o"], w["a"], w["batch"]
    hps = dict(batch_size=B, rb_capacity=4096, num_envs=4, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    torch.manual_seed(0)
    return pkg.Agent({"ob_shape": (4, o), "ac_shape": (4, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                     torch.device("cuda", 0), hps, pkg.ReplayBuffer(4096))


def mlp(sd, x):
    for blk in ("fc_block_1", "fc_block_2"):
        x = F.linear(x, sd[f"fc_stack.{blk}.fc.weight"], sd[f"fc_stack.{blk}.fc.bias"])
        x = F.relu(F.layer_norm(x, (schema.HID,), sd[f"fc_stack.{blk}.ln.weight"], sd[f"fc_stack.{blk}.ln.bias"], 1e-5))
    return F.linear(x, sd["head.weight"], sd["head.bias"])


def torch_actor(ag, dev):
    """the host alternative's first half: parameters to the host, then up again as torch tensors"""
    sd = schema.flat_to_dict(ag.engine.get_params(_lib.ACTOR), ag.ob_dim, ag._nh(), True)
    return {k: torch.as_tensor(v).to(dev) for k, v in sd.items()}


def torch_forward(ag, sd, obs, act, everything, td3):
    """the same quantities with torch ops"""
    head = mlp(sd, obs)
    a = ag.ac_dim
    scale = torch.as_tensor((ag.max_ac - ag.min_ac) / 2.0, device=obs.device)
    bias = torch.as_tensor((ag.max_ac + ag.min_ac) / 2.0, device=obs.device)
    out = {"mode": torch.tanh(head[:, :a]) * scale + bias}
    if td3 or not everything:
        return out
    mean, raw = head[:, :a], head[:, a:]
    log_std = -5.0 + 3.5 * (torch.tanh(raw) + 1.0)
    std = log_std.exp()
    eps = torch.randn_like(mean)
    x = mean + eps * std
    y = torch.tanh(x)
    c = 0.5 * math.log(2.0 * math.pi)
    lp = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - c - torch.log(scale * (1 - y * y) + 1e-6)).sum(1, keepdim=True)
    v = ((act - bias) / scale).clamp(-(1.0 - 1e-6), 1.0 - 1e-6)
    xa = torch.atanh(v)
    la = (-((xa - mean) ** 2) / (2 * std ** 2) - log_std - c - torch.log(scale * (1 - v * v) + 1e-6)).sum(1, keepdim=True)
    out.update(mean=mean, log_std=log_std, sample=y * scale + bias, sample_log_prob=lp, eps=eps, log_prob=la)
    return out


def probe(name):
    w = bench.WORKLOADS[name]
    o, a, td3 = w["o"], w["a"], bool(w["td3"])
    ag = make_agent(w)
    eng = ag.engine
    dev = torch.device("cuda", 0)
    learner = ag._ext_stream
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.Generator().manual_seed(1)
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "repeats": REPEATS, "cases": []}
    for n in ROWS:
        calls = 200 if n <= 1024 else 20
        obs = torch.randn(n, o, generator=g).to(dev)
        act = ((torch.rand(n, a, generator=g) * 2 - 1) * w["bound"]).to(dev)
        for everything in ((False,) if td3 else (False, True)):
            full = everything and not td3
            td = {"observations": obs, "actions": act} if full else {"observations": obs}
            keys = list(KEYS) if full else (["mode"] if td3 else ["mode", "mean", "log_std"])
            dst = {k: torch.empty(n, 1 if k.endswith("log_prob") else a, device=dev) for k in keys}
            # the C call with exactly the outputs of the case ("mode only": nothing else is stored)
            fields = {KEYS[k]: (v.data_ptr(), v.shape[1]) for k, v in dst.items() if full or k == "mode"}
            if full:
                fields["actions"] = (act.data_ptr(), a)
            sd = torch_actor(ag, dev)

            def device_route():
                ag.policy(td, sample=full, out=dst)

            def host_alternative():
                torch_forward(ag, torch_actor(ag, dev), obs, act, full, td3)

            def forward_only():
                torch_forward(ag, sd, obs, act, full, td3)

            def wall_us(f):
                eng.sync()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(calls):
                    f()
                eng.sync()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / calls * 1e6

            def device_us():
                torch.cuda.synchronize()
                eng.sync()
                t0.record(learner)                                   # unordered calls: nothing but the launches between the two events
                for _ in range(calls):
                    eng.policy_device(obs.data_ptr(), o, n, fields, ordered=False)
                t1.record(learner)
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3 / calls

            routes = (("device", device_route), ("host_alternative", host_alternative), ("torch_forward", forward_only))
            for _, f in routes:                                      # warm all: scratch, events, torch's allocator and kernels
                for _ in range(10):
                    f()
            vals = {r: [] for r, _ in routes}
            dev_us = []
            for _ in range(REPEATS):
                for r, f in routes:
                    vals[r].append(wall_us(f))
                dev_us.append(device_us())
            got = ag.policy(td, sample=full, out=dst)
            diff = float((got["mode"] - torch_forward(ag, sd, obs, act, False, td3)["mode"]).abs().max())
            out["cases"].append({"rows": n, "outputs": "everything" if full else ("mode" if td3 else "mode (Agent.policy: + mean, log_std)"),
                                 "calls_per_repeat": calls, "wall_us": {r: summary(v) for r, v in vals.items() if r != "torch_forward"},
                                 "device_us": summary(dev_us), "torch_forward_us": summary(vals["torch_forward"]), "max_abs_diff_mode": diff})
    out["kernel_us"] = {"k_pi_head": round(eng.time_kernel("pi_head", 200), 2)}
    out["policy_stats"] = eng.policy_stats()
    eng.close()
    return out


def main(argv):
    opts = {}
    for flag in ("--out", "--merge"):
        if flag in argv:
            k = argv.index(flag)
            opts[flag] = argv[k + 1]
            argv = argv[:k] + argv[k + 2:]
    res = []
    for name in argv or ["hopper_sac", "halfcheetah_td3", "humanoid_sac"]:
        res.append(probe(name))
        print(json.dumps(res[-1]), flush=True)
    if "--out" in opts:
        doc = {"tool": "tools/policy_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res}
        if "--merge" in opts:
            with open(opts["--merge"]) as fh:
                doc.update(json.load(fh))
        with open(opts["--out"], "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
