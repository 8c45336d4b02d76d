#!/usr/bin/env python3
"""Acting concurrent with learning, measured: python tools/acting_overlap_probe.py [workload ...] [--label TEXT]

One JSON object per workload of bench.WORKLOADS (default: all three), host clock, median / min / max over 5 repeats:

  predict_us          round trip of predict (4 rows, exploring) on an idle engine
  begin_end_us        round trip of predict_begin + predict_end on an idle engine
  step_per_s          600 x step(i % 3 == 0), nothing else
  loop_a_per_s        600 x [predict -> rb_extend -> step]                        (the order of bench.py's loop_with_acting_per_s)
  loop_b_per_s        600 x [predict -> step -> rb_extend]
  loop_c_per_s        600 x [predict_begin(after_all) -> step -> predict_end -> rb_extend]
  loop_d_per_s        600 x [predict_begin -> step -> predict_end -> rb_extend]   (waits for the learner only behind actor updates)

The repeats of the loop forms are interleaved (a b c d a b c d ...), every one closed by a sync.  A library without the two-stream
entry points (an older build) reports the other figures and leaves begin_end / c / d out, so the same script compares two builds.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402

REPEATS, ITERS = 5, 600


def summary(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def probe(name, label):
    w = bench.WORKLOADS[name]
    eng = bench.make_engine(w, 0, 0)
    two_streams = hasattr(eng, "predict_begin")
    ob = np.zeros((4, w["o"]), np.float32)
    rows = [np.zeros((4, w["o"]), np.float32), np.zeros((4, w["a"]), np.float32), np.zeros(4, np.float32),
            np.zeros((4, w["o"]), np.float32), np.zeros(4, bool)]

    def begin_end():
        eng.predict_begin(ob, True)
        return eng.predict_end()

    def loop_a(i):
        eng.predict(ob, True); eng.rb_extend(*rows); eng.step(i % 3 == 0)

    def loop_b(i):
        eng.predict(ob, True); eng.step(i % 3 == 0); eng.rb_extend(*rows)

    def loop_c(i):
        eng.predict_begin(ob, True, True); eng.step(i % 3 == 0); eng.predict_end(); eng.rb_extend(*rows)

    def loop_d(i):
        eng.predict_begin(ob, True); eng.step(i % 3 == 0); eng.predict_end(); eng.rb_extend(*rows)

    forms = {"a": loop_a, "b": loop_b}
    if two_streams:
        forms.update(c=loop_c, d=loop_d)
    # warm: graphs of every (explore, n) used, the runtime's signal pools (they grow over the first few hundred async copies), clocks
    for _ in range(700):
        eng.rb_extend(*rows)
    for i in range(300):
        eng.predict(ob, True)
        eng.step(i % 3 == 0)
    for f in forms.values():
        for i in range(150):
            f(i)
    eng.sync()

    def per_call_us(f, n=300):
        vals = []
        for _ in range(REPEATS):
            eng.sync()
            t = time.perf_counter()
            for _ in range(n):
                f()
            vals.append((time.perf_counter() - t) / n * 1e6)
        return summary(vals)

    def rate(f):
        eng.sync()
        t = time.perf_counter()
        for i in range(ITERS):
            f(i)
        eng.sync()
        return ITERS / (time.perf_counter() - t)

    out = {"workload": name, "label": label, "two_streams": two_streams, "repeats": REPEATS, "iterations": ITERS}
    out["predict_us"] = per_call_us(lambda: eng.predict(ob, True))
    if two_streams:
        out["begin_end_us"] = per_call_us(begin_end)
    out["step_per_s"] = summary([rate(lambda i: eng.step(i % 3 == 0)) for _ in range(REPEATS)], 1)
    vals = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, f in forms.items():
            vals[k].append(rate(f))
    for k in forms:
        out[f"loop_{k}_per_s"] = summary(vals[k], 1)
    if two_streams:
        out["acting_stats"] = eng.acting_stats()
    eng.close()
    return out


def main(argv):
    label = ""
    if "--label" in argv:
        k = argv.index("--label")
        label = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    for name in argv or ["hopper_sac", "halfcheetah_td3", "humanoid_sac"]:
        print(json.dumps(probe(name, label)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
