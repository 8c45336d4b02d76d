#!/usr/bin/env python3
"""What initialising the networks on the device costs, against the host route it replaces -> profiles/param_init.json.

    python tools/param_init_probe.py                # GPU.  At the three BASELINE shapes (bench.WORKLOADS): the device time (events on
                                                    # the engine's stream) and the host wall time (call to return; call to sync) of one
                                                    # Engine.init_params(all), and the wall time of the host route -- schema.
                                                    # reference_initial_params (torch's CPU orthogonal_) + four set_params + the Adam and
                                                    # alpha writes -- each the median of RUNS.  And per shape of tests/test_gpu_param_init.py
                                                    # the worst |W - float64 model| over that test's tolerance ("model_ratio").
    python tools/param_init_probe.py --bench TREE   # GPU: this checkout's bench.py against TREE's (a built checkout of the parent
                                                    # commit), alternating processes, RUNS each -> "bench"; the median of this build has
                                                    # to lie inside the parent's min .. max range: no engine kernel changed.
There is no speed bar on the init itself: it runs once per 10^4 .. 10^6 updates."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "param_init.json")
RUNS = 5


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": len(v)}


def merge(entry):
    data = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            data = json.load(f)
    data.update(entry)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


def shapes_mode(runs):
    import numpy as np
    import torch
    import bench
    import sac_td3_cudagraphs_pytorch_amd as pkg
    from sac_td3_cudagraphs_pytorch_amd import _lib, schema
    out = {"what": "milliseconds, median / min / max of `runs`; init_device: events around Engine.init_params(all) on the engine's stream; "
                   "init_host_return: the call until it returns; init_host_synced: until the stream is idle; host_route: "
                   "reference_initial_params + 4 set_params + the Adam and alpha writes, until the stream is idle"}
    for name, w in bench.WORKLOADS.items():
        cfg = pkg.Config(ob_dim=w["o"], ac_dim=w["a"], batch_size=w["batch"], rb_capacity=4096, max_envs=4, prefer_td3_over_sac=w["td3"],
                         bcq_style_targ_mix=w["td3"], qnets_lr=3e-4 if w["td3"] else 1e-3, seed=0)
        eng = pkg.Engine(cfg, [-w["bound"]] * w["a"], [w["bound"]] * w["a"])
        what = _lib.INIT_ACTOR | _lib.INIT_CRITICS | (0 if w["td3"] else _lib.INIT_ALPHA)
        stream = torch.cuda.ExternalStream(eng.device_handles()[0])
        eng.init_params(what, 0, 0)      # (the first call allocates the scratch)
        eng.sync()
        dev, ret, synced, host = [], [], [], []
        for r in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            eng.init_params(what, 0, r + 1)
            t1 = time.perf_counter()
            e1.record(stream)
            eng.sync()
            t2 = time.perf_counter()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
            ret.append(1e3 * (t1 - t0))
            synced.append(1e3 * (t2 - t0))
            torch.manual_seed(r)
            t0 = time.perf_counter()
            actor, critics = schema.reference_initial_params(w["o"], w["a"], w["td3"], True)
            for which, flat in ((_lib.ACTOR, actor), (_lib.ACTOR_TARGET, actor), (_lib.CRITICS, critics), (_lib.CRITICS_TARGET, critics)):
                eng.set_params(which, flat)
            for which, flat in ((_lib.ACTOR, actor), (_lib.CRITICS, critics)):
                z = np.zeros_like(flat)
                eng.set_adam_state(which, z, z, 0)
            if not w["td3"]:
                eng.set_params(_lib.LOG_ALPHA, np.log(np.float32([cfg.alpha_init])))
                eng.set_adam_state(_lib.LOG_ALPHA, np.zeros(1, np.float32), np.zeros(1, np.float32), 0)
            eng.sync()
            host.append(1e3 * (time.perf_counter() - t0))
        out[name] = {"init_device": spread(dev), "init_host_return": spread(ret), "init_host_synced": spread(synced), "host_route": spread(host),
                     "columns_redrawn": eng.init_stats()["columns_redrawn"]}
        print(name, json.dumps(out[name]), flush=True)
        eng.close()
    merge({"init": out})
    # the float64 model's ratio at the shapes of the GPU test (tests/init_model.py; the test's own tolerance)
    from tests import init_model as im
    ratios = {"what": "worst |W - float64 model| / tolerance per shape; tolerance = 8 x the distance of torch's fp32 QR (sign-fixed) of the "
                      "model's G from the model (tests/test_gpu_param_init.py, test 2)"}
    for name, (td3, o, a) in {"sac-o3a1": (False, 3, 1), "td3-o11a3": (True, 11, 3), "sac-o376a17": (False, 376, 17)}.items():
        cfg = pkg.Config(ob_dim=o, ac_dim=a, batch_size=8, rb_capacity=64, max_envs=2, prefer_td3_over_sac=td3, seed=11)
        eng = pkg.Engine(cfg, [-1.0] * a, [1.0] * a)
        eng.init_params(3 if td3 else 7, 11, 0)
        got = {"actor": eng.get_params(_lib.ACTOR), "critics": eng.get_params(_lib.CRITICS)}
        worst = 0.0
        for net, in_dim, n_head, flat in im.nets_of(got, o, a, td3):
            for kind, layer, W in im.split(flat, in_dim, n_head, True):
                if kind != "weight":
                    continue
                W64, G = im.weight64(11, 3 * net + layer, 0, *W.shape)
                q, r = torch.linalg.qr(torch.from_numpy(np.asarray(G, np.float32)))
                q = (q * torch.sign(torch.diagonal(r))).numpy().astype(np.float64)
                tol = 8.0 * float(np.abs((q if W.shape[0] >= W.shape[1] else q.T) - W64).max())
                worst = max(worst, float(np.abs(W.astype(np.float64) - W64).max()) / tol)
        ratios[name] = round(worst, 4)
        eng.close()
    merge({"model_ratio": ratios})
    print("model_ratio", json.dumps(ratios), flush=True)


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "200"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:      # a child that fails ends the whole probe: nothing more is started on the GPU
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def bench_mode(other, runs):
    got = {"this": [], "parent": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["parent"].append(child_bench(other))
    keys = [k for k in ("value", "ms_per_step") if k in got["this"][0]]
    entry = {"what": "bench.py --gpus 1 --steps 2000 --warmup 200 of this checkout and of the parent commit's, alternating processes",
             **{side: {k: spread([r[k] for r in rs]) for k in keys} for side, rs in got.items()}}
    k = keys[0]
    entry["this_median_inside_parent_range"] = bool(entry["parent"][k]["min"] <= entry["this"][k]["median"] <= entry["parent"][k]["max"])
    merge({"bench": entry})
    print(json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--runs", type=int, default=RUNS)
    args = ap.parse_args()
    if args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs)
    else:
        shapes_mode(args.runs)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
