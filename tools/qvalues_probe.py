#!/usr/bin/env python3
"""Scoring state-action pairs, measured: python tools/qvalues_probe.py [workload ...] [--out FILE]

Agent.q_values / sactd3_qvalues_device (include/sactd3.h) on one Agent per workload of bench.WORKLOADS (default: the three BASELINE
shapes), at n = 4, 256 and 1024 rows of CUDA tensors, with explicit actions and in the policy form (s, pi(s)), online critics; beside
it the only way there was before -- the host alternative: get_params(CRITICS) (+ ACTOR for the policy form), the reference's critics
rebuilt as torch tensors on cuda:0, and torch's forward pass on the same rows.  All routes in ONE process, their repeats interleaved,
median / min / max over 5 repeats.  Nothing here is a pass/fail bar: the probe records what it finds.

  wall_us             host wall time per call, 200 calls per repeat; the window is closed by a synchronisation of the engine's and
                      torch's streams, inside the figure (`device`: Agent.q_values into a preallocated `out`; `host_alternative`:
                      get_params + upload + torch forward, every call -- the parameters change with every update)
  device_us           HIP events on the engine's stream around 200 back-to-back unordered sactd3_qvalues_device calls
  torch_forward_us    the torch forward alone on parameters already uploaded (what the alternative costs when nothing was updated)
  kernel_us           sactd3_time_kernel of the two new kernels on 1024 rows
  max_abs_diff        |engine - torch| over the scored values: a sanity figure, not a parity test (tests/test_gpu_qvalues.py is)
"""
import json
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

REPEATS, CALLS = 5, 200
ROWS = (4, 256, 1024)


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


def torch_nets(ag, dev, policy):
    """the host alternative's first half: parameters to the host, then up again as torch tensors"""
    eng, o, a = ag.engine, ag.ob_dim, ag.ac_dim
    up = lambda sd: {k: torch.as_tensor(v).to(dev) for k, v in sd.items()}
    q = eng.get_params(_lib.CRITICS).reshape(2, -1)
    nets = {"q": [up(schema.flat_to_dict(q[k], o + a, 1, True)) for k in range(2)]}
    if policy:
        nets["pi"] = up(schema.flat_to_dict(eng.get_params(_lib.ACTOR), o, ag._nh(), True))
    return nets


def torch_forward(ag, nets, obs, act):
    if act is None:
        head = mlp(nets["pi"], obs)
        scale = torch.as_tensor((ag.max_ac - ag.min_ac) / 2.0, device=obs.device)
        bias = torch.as_tensor((ag.max_ac + ag.min_ac) / 2.0, device=obs.device)
        act = torch.tanh(head[:, :ag.ac_dim]) * scale + bias        # SAC: tanh(mean); TD3: the head is ac_dim wide
    x = torch.cat([obs, act], 1)
    return torch.stack([mlp(sd, x) for sd in nets["q"]], 0)


def probe(name):
    w = bench.WORKLOADS[name]
    o, a = w["o"], w["a"]
    ag = make_agent(w)
    eng = ag.engine
    dev = torch.device("cuda", 0)
    learner = ag._ext_stream
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.Generator().manual_seed(1)
    out = {"workload": name, "ob_dim": o, "ac_dim": a, "repeats": REPEATS, "calls_per_repeat": CALLS, "cases": []}
    for n in ROWS:
        obs = torch.randn(n, o, generator=g).to(dev)
        act = ((torch.rand(n, a, generator=g) * 2 - 1) * w["bound"]).to(dev)
        for policy in (False, True):
            td = {"observations": obs} if policy else {"observations": obs, "actions": act}
            dst = torch.empty(2, n, 1, device=dev)
            nets = torch_nets(ag, dev, policy)

            def device_route():
                ag.q_values(td, out=dst)

            def host_alternative():
                torch_forward(ag, torch_nets(ag, dev, policy), obs, None if policy else act)

            def forward_only():
                torch_forward(ag, nets, obs, None if policy else act)

            def wall_us(f):
                eng.sync()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(CALLS):
                    f()
                eng.sync()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / CALLS * 1e6

            def device_us():
                torch.cuda.synchronize()
                eng.sync()
                t0.record(learner)                                   # unordered calls: nothing but the launches between the two events
                for _ in range(CALLS):
                    eng.q_values_device(obs.data_ptr(), o, 0 if policy else act.data_ptr(), a, n, False, dst.data_ptr(), 1, n, ordered=False)
                t1.record(learner)
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3 / CALLS

            routes = (("device", device_route), ("host_alternative", host_alternative), ("torch_forward", forward_only))
            for _, f in routes:                                      # warm all: scratch, events, torch's allocator and kernels
                for _ in range(20):
                    f()
            vals = {r: [] for r, _ in routes}
            dev_us = []
            for _ in range(REPEATS):
                for r, f in routes:
                    vals[r].append(wall_us(f))
                dev_us.append(device_us())
            ag.q_values(td, out=dst)
            diff = float((dst - torch_forward(ag, nets, obs, None if policy else act)).abs().max())
            out["cases"].append({"rows": n, "actions": "policy" if policy else "explicit",
                                 "wall_us": {r: summary(v) for r, v in vals.items() if r != "torch_forward"},
                                 "device_us": summary(dev_us), "torch_forward_us": summary(vals["torch_forward"]), "max_abs_diff": diff})
    out["kernel_us"] = {"k_sa_from_fields": round(eng.time_kernel("sa_from_fields", 200), 2), "k_q_head": round(eng.time_kernel("q_head", 200), 2)}
    out["qvalues_stats"] = eng.qvalues_stats()
    eng.close()
    return out


def main(argv):
    path = None
    if "--out" in argv:
        k = argv.index("--out")
        path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    res = []
    for name in argv or ["hopper_sac", "halfcheetah_td3", "humanoid_sac"]:
        res.append(probe(name))
        print(json.dumps(res[-1]), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"tool": "tools/qvalues_probe.py", "device": torch.cuda.get_device_name(0), "workloads": res}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
