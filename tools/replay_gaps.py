#!/usr/bin/env python3
"""Where the device idles between two kernels of the timed loop, from ONE rocprofv3 --kernel-trace run (as tools/boundary_table.py):

  rocprofv3 --kernel-trace --output-format csv -d out/trace -- python3 bench.py --workload hopper_sac --steps 900 --warmup 150
  python tools/replay_gaps.py --trace out/trace --steps 900 [--nodes-per-period 21] [--json out.json]

tools/boundary_table.py groups boundaries by kernel pair, and the pair that ends a graph replay (the last node of a period, the first of
the next) is also a pair INSIDE a graph that holds several periods.  This one keeps the order instead: over the last `steps` iterations
of the trace it counts the boundaries above --min-gap-us per period, says at which node of the period they stand (0 = in front of the
period's first node) and how far apart they are, and gives their median."""
import argparse
import collections
import json
import statistics

from boundary_table import load_trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", required=True)
    ap.add_argument("--steps", type=int, required=True, help="timed iterations of the traced run: the last ones of the trace")
    ap.add_argument("--nodes-per-period", type=int, default=21)
    ap.add_argument("--period", type=int, default=3, help="iterations per period")
    ap.add_argument("--min-gap-us", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    npp = a.nodes_per_period
    rows = [r for r in load_trace(a.trace) if r[2].startswith("k_")][-(a.steps // a.period) * npp:]
    gaps = [(b[0] - x[1]) * 1e-3 for x, b in zip(rows, rows[1:])]
    at = [i + 1 for i, g in enumerate(gaps) if g > a.min_gap_us]
    big = [gaps[i - 1] for i in at]
    periods = len(rows) / npp
    out = {"nodes": len(rows), "periods": periods, "us_per_iteration_traced": round((rows[-1][1] - rows[0][0]) * 1e-3 / (periods * a.period), 3),
           "boundaries_above_min_gap": len(at), "per_period": round(len(at) / periods, 3),
           "in_front_of_a_period": sum(i % npp == 0 for i in at), "inside_a_period": sum(i % npp != 0 for i in at),
           "gap_us_median": round(statistics.median(big), 2) if big else None,
           "gap_us_median_in_front_of_a_period": round(statistics.median([g for i, g in zip(at, big) if i % npp == 0] or [0.0]), 2),
           "idle_us_per_iteration": round(sum(big) / (periods * a.period), 3),
           "most_common_spacings_in_nodes": collections.Counter(y - x for x, y in zip(at, at[1:])).most_common(4)}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
