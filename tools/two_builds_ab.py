#!/usr/bin/env python3
"""Two builds of the engine in ONE process: python tools/two_builds_ab.py OTHER_CHECKOUT [workload ...]

OTHER_CHECKOUT is another checkout of this repository with its own built libsactd3_hip.so (for instance the parent commit).  Its
package is imported under a second module name, so each build runs through its own Python binding; one engine per build, and every
measurement alternates between the two live engines, 9 rounds, the order reversed every round.  Two processes of the SAME build
differ by more than most changes are worth (a 4-row predict: 15.0 .. 16.6 us from one process to the next); two engines in one
process share the clocks, the runtime and the moment.  Measures what both builds have: the predict round trip, the step-only rate,
the rate of whole periods (sactd3_step_period, in iterations per second) and the serial acting loops (a) predict -> rb_extend -> step and (b) predict -> step -> rb_extend.  One JSON object per workload."""
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

ROUNDS = 9


def load_package(name, checkout):
    d = os.path.join(checkout, "sac-td3-cudagraphs-pytorch_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_engine(pkg, w):
    """bench.make_engine through `pkg`"""
    cfg = pkg.Config(ob_dim=w["o"], ac_dim=w["a"], batch_size=w["batch"], rb_capacity=w["capacity"], max_envs=4,
                     prefer_td3_over_sac=w["td3"], bcq_style_targ_mix=w["td3"], qnets_lr=3e-4 if w["td3"] else 1e-3, seed=0)
    eng = pkg.Engine(cfg, [-w["bound"]] * w["a"], [w["bound"]] * w["a"])
    torch.manual_seed(0)
    actor, critics = pkg.schema.reference_initial_params(w["o"], w["a"], w["td3"], True)
    for which, flat in ((0, actor), (2, actor), (1, critics), (3, critics)):
        eng.set_params(which, flat)
    eng.rb_fill_synthetic(w["rows"], seed=0)
    eng.instantiate_graphs()
    eng.sync()
    return eng


def compare(name, pkgs):
    w = bench.WORKLOADS[name]
    order = list(pkgs)
    engs = {k: make_engine(pkgs[k], w) for k in order}
    ob = np.zeros((4, w["o"]), np.float32)
    rows = [np.zeros((4, w["o"]), np.float32), np.zeros((4, w["a"]), np.float32), np.zeros(4, np.float32),
            np.zeros((4, w["o"]), np.float32), np.zeros(4, bool)]

    def rate(eng, f, n=600):
        eng.sync()
        t = time.perf_counter()
        for i in range(n):
            f(i)
        eng.sync()
        return n / (time.perf_counter() - t)

    forms = {"predict_us": lambda e: 1e6 / rate(e, lambda i: e.predict(ob, True), 300),
             "step_per_s": lambda e: rate(e, lambda i: e.step(i % 3 == 0)),
             "period_iters_per_s": lambda e: 3 * rate(e, lambda i: e.step_period(), 200),
             "loop_a_per_s": lambda e: rate(e, lambda i: (e.predict(ob, True), e.rb_extend(*rows), e.step(i % 3 == 0))),
             "loop_b_per_s": lambda e: rate(e, lambda i: (e.predict(ob, True), e.step(i % 3 == 0), e.rb_extend(*rows)))}
    for e in engs.values():          # warm: signal pools of the async copies, graphs, clocks
        for _ in range(700):
            e.rb_extend(*rows)
        for f in forms.values():
            f(e)
    vals = {k: {f: [] for f in forms} for k in engs}
    for r in range(ROUNDS):
        for f in forms:
            for k in (order if r % 2 == 0 else order[::-1]):
                vals[k][f].append(forms[f](engs[k]))
    out = {"workload": name, "order": order, "rounds": ROUNDS}
    for k in engs:
        out[k] = {f: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for f, v in vals[k].items()}
        engs[k].close()
    return out


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    pkgs = {"other": load_package("sactd3_other_build", os.path.abspath(argv[0])), "this": load_package("sactd3_this_build", ROOT)}
    for name in argv[1:] or ["hopper_sac", "halfcheetah_td3", "humanoid_sac"]:
        print(json.dumps(compare(name, pkgs)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
