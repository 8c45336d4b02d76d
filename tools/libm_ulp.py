#!/usr/bin/env python3
"""Worst ULP error of the device's tanhf, expf and logf against numpy float64, over the ranges the squashed-Gaussian chain reaches
(tools/libm_ulp.hip evaluates them on the GPU).  Writes profiles/libm_ulp.json; tests/bounds.py's LIBM_ULP are these figures rounded
up to an integer plus 1 ulp for the rounding of the comparison itself.  This measures the device library against the float64
reference, not the engine against itself.  Not a test: one run of a few seconds.

    python tools/libm_ulp.py --build        # compile tools/libm_ulp (no GPU needed)
    python tools/libm_ulp.py                # run it (compiling first if the program is missing) and write the record
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "libm_ulp.hip")
EXE = os.path.join(ROOT, "tools", "libm_ulp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FUNCS = (("tanhf", np.tanh), ("expf", np.exp), ("logf", np.log))
RANGES = {"tanhf": "[-16, 16] linear, +-[7, 10.5] dense (first results of +-1)", "expf": "[-5, 2] linear", "logf": "[1e-6, 8] geometric"}


def build():
    # the engine Makefile's code-generation flags: -O3, no fast-math
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", SRC, "-o", EXE], check=True)


def ulp_of(v):
    """spacing of float32 at |v| (v float64, normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 23)


def ulp_error(got32, exact64):
    return np.abs(got32.astype(np.float64) - exact64) / ulp_of(exact64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true", help="compile only")
    ap.add_argument("--timeout", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "libm_ulp.json"))
    args = ap.parse_args()
    if args.build or not os.path.exists(EXE):
        build()
        if args.build:
            return 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "libm.bin")
        subprocess.run([EXE, path], check=True, timeout=args.timeout)
        raw = np.fromfile(path, dtype=np.uint8)
    n = int(raw[:4].view(np.int32)[0])
    data = raw[4:].view(np.float32).reshape(3, 2, n)
    rec = {"what": "worst |device result - float64 result| in units of the float32 spacing at the float64 result", "points_per_function": n,
           "functions": {}}
    for k, (name, ref) in enumerate(FUNCS):
        x, y = data[k, 0], data[k, 1]
        err = ulp_error(y, ref(x.astype(np.float64)))
        i = int(np.argmax(err))
        rec["functions"][name] = {"range": RANGES[name], "max_ulp": float(err[i]), "at": float(x[i]), "got": float(y[i]),
                                  "mean_ulp": float(err.mean())}
        if name == "tanhf":
            ax = np.abs(x)
            sat = ax[np.abs(y) == 1.0]
            rec["functions"][name]["first_exact_one_at"] = float(sat.min()) if sat.size else None
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["functions"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
