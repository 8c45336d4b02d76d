#!/usr/bin/env python3
"""Host cost per call of the mirror's device routes, two checkouts in ONE process: python tools/mirror_ab.py PARENT_CHECKOUT [--out FILE]

PARENT_CHECKOUT is a checkout of the commit to compare against, with its own built library; "change" is this tree.  Both packages are
imported side by side (each loads the library next to it), one Agent each at SAC Hopper B = 256 with 4 envs, and the repeats of the
two alternate (parent change parent change ...): host clock around 200 calls, median / min / max over 9 repeats.

  stage_us            Agent._stage of a caller-owned CUDA batch          extend_us     rb.extend of 4 rows of CUDA tensors
  predict_device_us   Agent.predict_device, 4 rows, preallocated `out`   q_values_us   Agent.q_values, 256 rows with actions, `out`
  rows_us             ReplayBuffer.rows of 256 ring slots into preallocated tensors

One process on purpose: on a shared box the host pace of these calls differs between two processes of the SAME code by more than
any change to the mirror moves it (profiles/README.md), and inside one process it does not."""
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

REPEATS, CALLS = 9, 200


def load(root, name):
    d = os.path.join(root, "sac-td3-cudagraphs-pytorch_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def setup(pkg, w, n=4):
    o, a, B = w["o"], w["a"], w["batch"]
    hps = dict(batch_size=B, rb_capacity=100_000, num_envs=n, seed=0, prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ag = pkg.Agent({"ob_shape": (n, o), "ac_shape": (n, a)}, np.full(a, -w["bound"], np.float32), np.full(a, w["bound"], np.float32),
                   dev, hps, pkg.ReplayBuffer(hps["rb_capacity"]))
    ag.engine.rb_fill_synthetic(20_000, seed=0)

    def td(rows, seed):
        g = torch.Generator().manual_seed(seed)
        done = torch.rand(rows, 1, generator=g) < 0.01
        return {"observations": torch.randn(rows, o, generator=g).to(dev), "next_observations": torch.randn(rows, o, generator=g).to(dev),
                "actions": ((torch.rand(rows, a, generator=g) * 2 - 1) * w["bound"]).to(dev), "rewards": torch.randn(rows, 1, generator=g).to(dev),
                "terminations": done.to(dev), "dones": done.to(dev)}
    batches, steps = [td(B, k) for k in range(4)], [td(n, 10 + k) for k in range(4)]
    obs4, out4 = torch.randn(n, o, device=dev), torch.empty(n, a, device=dev)
    qtd = {"observations": batches[0]["observations"], "actions": batches[0]["actions"]}
    qout = torch.empty(2, B, 1, device=dev)
    idx = torch.randint(0, 20_000, (B,), device=dev)
    rows_out = ag.rb.rows(idx)
    return ag, {
        "stage_us": lambda k: ag._stage(batches[k % 4]),
        "extend_us": lambda k: ag.rb.extend(steps[k % 4]),
        "predict_device_us": lambda k: ag.predict_device({"observations": obs4}, explore=True, out=out4),
        "q_values_us": lambda k: ag.q_values(qtd, out=qout),
        "rows_us": lambda k: ag.rb.rows(idx, out=rows_out),
    }


def per_call_us(eng, f):
    torch.cuda.synchronize()
    eng.sync()
    t = time.perf_counter()
    for k in range(CALLS):
        f(k)
    dt = time.perf_counter() - t      # (the enqueue pace of the host, as tools/device_boundary_probe.py takes it)
    torch.cuda.synchronize()
    eng.sync()
    return dt / CALLS * 1e6


def main(argv):
    w = bench.WORKLOADS["hopper_sac"]
    sides = {"parent": load(os.path.abspath(argv[0]), "pkg_parent"), "change": load(ROOT, "pkg_change")}
    made = {k: setup(p, w) for k, p in sides.items()}
    libs = {k: p.library_path() for k, p in sides.items()}
    assert libs["parent"] != libs["change"], libs
    names = list(made["parent"][1])
    for ag, fs in made.values():      # warm every path of both sides
        for name in names:
            for k in range(300):
                fs[name](k)
        ag.engine.sync()
    vals = {name: {k: [] for k in made} for name in names}
    for name in names:
        for _ in range(REPEATS):
            for k, (ag, fs) in made.items():
                vals[name][k].append(per_call_us(ag.engine, fs[name]))
    res = {"tool": "tools/mirror_ab.py", "device": torch.cuda.get_device_name(0), "workload": "hopper_sac", "repeats": REPEATS,
           "calls_per_repeat": CALLS, "libraries": libs}
    for name in names:
        res[name] = {k: summary(v) for k, v in vals[name].items()}
        p, c = res[name]["parent"], res[name]["change"]
        res[name]["change_median_within_parent_range"] = p["min"] <= c["median"] <= p["max"]
    print(json.dumps(res), flush=True)
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    for ag, _ in made.values():
        ag.engine.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
