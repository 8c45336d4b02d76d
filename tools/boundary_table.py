#!/usr/bin/env python3
"""Node boundaries of the timed graph from ONE rocprofv3 --kernel-trace run, next to the bytes the predecessor wrote.

  rocprofv3 --kernel-trace --output-format csv -d out/trace -- python3 bench.py --workload hopper_sac --steps 600 --warmup 100 --timed-only
  python tools/boundary_table.py --trace out/trace --pmc profiles/r03_pmc_hopper_sac.csv [--json out.json]

For every pair of kernels that follow each other on the device (dispatch order by start time): boundary = start(next) - end(this),
median over all occurrences; pairs seen fewer than --min-calls times and gaps above --max-gap-us (the host between two replays)
are left out.  `write_bytes` of `this` comes from the WRITE_SIZE summary of tools/pmc_summary.py (counters are collected in a run of
their own), matched by kernel instance and total threads.  The last line fits boundary = a + bytes / bw over the pairs (least
squares): the premise "a kernel boundary waits for the predecessor's dirty lines" predicts bw of a few TB/s and a > 0."""
import argparse
import csv
import glob
import json
import os
import statistics
from collections import defaultdict

from pmc_summary import norm


def load_trace(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "Grid_Size" in r:
                    threads = int(r["Grid_Size"])
                else:
                    threads = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), norm(r["Kernel_Name"]), threads))
    rows.sort()
    return rows


def load_writes(path):
    out = {}
    if path:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                out[(r["kernel"], int(r["threads"]))] = float(r["write_bytes"])
    return out


def table(rows, writes, min_calls, max_gap_us):
    gaps, durs = defaultdict(list), defaultdict(list)
    for (s0, e0, k0, t0), (s1, _e1, k1, t1) in zip(rows, rows[1:]):
        gap = (s1 - e0) * 1e-3
        if not k0.startswith("k_") or not k1.startswith("k_") or gap > max_gap_us:
            continue
        gaps[(k0, t0, k1, t1)].append(gap)
        durs[(k0, t0, k1, t1)].append((e0 - s0) * 1e-3)
    out = []
    for key, g in gaps.items():
        if len(g) < min_calls:
            continue
        out.append({"this": key[0], "this_threads": key[1], "next": key[2], "next_threads": key[3], "n": len(g),
                    "boundary_us_median": round(statistics.median(g), 3), "boundary_us_p10": round(sorted(g)[len(g) // 10], 3),
                    "this_duration_us_median": round(statistics.median(durs[key]), 3),
                    "this_write_bytes": writes.get((key[0], key[1]))})
    out.sort(key=lambda r: -(r["this_write_bytes"] or 0))
    return out


def fit(tab):
    pts = [(r["this_write_bytes"], r["boundary_us_median"]) for r in tab if r["this_write_bytes"] is not None]
    if len(pts) < 3:
        return None
    n = len(pts)
    sx, sy = sum(p[0] for p in pts), sum(p[1] for p in pts)
    sxx, sxy = sum(p[0] * p[0] for p in pts), sum(p[0] * p[1] for p in pts)
    den = n * sxx - sx * sx
    if den == 0:
        return None
    slope = (n * sxy - sx * sy) / den          # us per byte
    return {"intercept_us": round((sy - slope * sx) / n, 3), "us_per_mb": round(slope * 1e6, 4), "pairs": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", required=True, help="output dir of the --kernel-trace run (or its kernel_trace.csv)")
    ap.add_argument("--pmc", default=None, help="profiles/*_pmc_<workload>.csv with write_bytes per (kernel, threads)")
    ap.add_argument("--min-calls", type=int, default=100)
    ap.add_argument("--max-gap-us", type=float, default=15.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    tab = table(load_trace(a.trace), load_writes(a.pmc), a.min_calls, a.max_gap_us)
    f = fit(tab)
    for r in tab:
        wb = "      -" if r["this_write_bytes"] is None else "%7.2f" % (r["this_write_bytes"] / 1e6)
        print("%-28s %7d -> %-28s n %5d  boundary %6.2f us (p10 %5.2f)  this ran %6.2f us  wrote %s MB" % (
            r["this"], r["this_threads"], r["next"], r["n"], r["boundary_us_median"], r["boundary_us_p10"], r["this_duration_us_median"], wb))
    print("fit boundary = a + b * MB written:", f)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"pairs": tab, "fit": f}, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
