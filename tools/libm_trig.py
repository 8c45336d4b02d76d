#!/usr/bin/env python3
"""Worst absolute error of the device's sinf and cosf over [-3.15, 3.15] -- every float32 argument, 2.1e9 of them -- against float64
(tools/libm_trig.hip evaluates them on the GPU and keeps each block's worst argument; this script recomputes the error at those
candidates with numpy float64, so the recorded figure is the library against numpy, the device's double sin / cos only chose where
to look).  Writes profiles/libm_trig.json; tests/env_model.py reads `sinf_abs` and `cosf_abs` from it as they stand, with no factor
on top, as the trig term of the env step's bound.  profiles/libm_ulp.json (tools/libm_ulp.py) is another record and is not touched.
Not a test: one run of a few seconds.

    python tools/libm_trig.py --build        # compile tools/libm_trig (no GPU needed)
    python tools/libm_trig.py                # run it (compiling first if the program is missing) and write the record
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "libm_trig.hip")
EXE = os.path.join(ROOT, "tools", "libm_trig")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WORST = np.dtype([("x", np.float32), ("got", np.float32), ("err", np.float64)])


def build():
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", SRC, "-o", EXE], check=True)


def record(raw):
    blocks = int(raw[:4].view(np.int32)[0])
    top = raw[4:8].view(np.float32)[0]
    cand = raw[8:].view(WORST).reshape(2, blocks)
    rec = {"what": "worst |device result - numpy float64 result| of the library's sinf / cosf, every float32 argument of [-top, top]",
           "top": float(top), "arguments": 2 * (int(raw[4:8].view(np.uint32)[0]) + 1), "candidates_per_function": blocks}
    for k, (name, ref) in enumerate((("sinf", np.sin), ("cosf", np.cos))):
        x, got = cand[k]["x"].astype(np.float64), cand[k]["got"].astype(np.float64)
        err = np.abs(got - ref(x))
        i = int(np.argmax(err))
        rec[name + "_abs"] = float(err[i])
        rec[name] = {"at": float(x[i]), "got": float(got[i]), "device_double_figure": float(cand[k]["err"].max()),
                     "numpy_vs_device_double_at_candidates": float(np.abs(err - cand[k]["err"]).max())}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true", help="compile only")
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "libm_trig.json"))
    args = ap.parse_args()
    if args.build or not os.path.exists(EXE):
        build()
        if args.build:
            return 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "trig.bin")
        subprocess.run([EXE, path], check=True, timeout=args.timeout)
        raw = np.fromfile(path, dtype=np.uint8)
    rec = record(raw)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
