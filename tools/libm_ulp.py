#!/usr/bin/env python3
"""Worst ULP error of the device's tanhf, expf and logf against numpy float64, over the ranges the squashed-Gaussian chain reaches
(tools/libm_ulp.hip evaluates them on the GPU).  Writes profiles/libm_ulp.json; tests/bounds.py's LIBM_ULP are these figures rounded
up to an integer plus 1 ulp for the rounding of the comparison itself.  This measures the device library against the float64
reference, not the engine against itself.  Not a test: one run of a few seconds.

Under the key "noise": the pieces of the engine's normal draws, exhaustively over the 2^24 arguments of philox_u01 -- the radius
and the two hardware trig units of philox_normal / philox_normal4 (csrc/kernels.h, whose three arithmetic lines tools/libm_ulp.hip
restates), and the library sinf / cosf / logf of k_rb_fill at its own fp32 angle t = 2 pi_f32 u.  tests/bounds.py's NOISE constants
are these figures rounded up to the next power of two (tests/test_noise_model.py ties the two).

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
NOISE_FNS = ("u", "rad", "sin_rev", "cos_rev", "t", "sinf", "cosf", "logf", "rad_libm")     # enum NoiseFn of tools/libm_ulp.hip


def build():
    # the engine Makefile's code-generation flags: -O3, no fast-math
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", SRC, "-o", EXE], check=True)


def ulp_of(v):
    """spacing of float32 at |v| (v float64, normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 23)


def ulp_error(got32, exact64):
    return np.abs(got32.astype(np.float64) - exact64) / ulp_of(exact64)


def u01_all():
    """philox_u01 (csrc/philox.h) of every 24-bit argument, in numpy float32: the add rounds to nearest even as on the device"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return (i.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def worst(err, u, got):
    i = int(np.argmax(err))
    return {"max": float(err[i]), "at_u": float(u[i]), "got": float(got[i])}


def noise_record(z):
    """z: [len(NOISE_FNS), 2^24] device results -> the record under "noise" """
    d = dict(zip(NOISE_FNS, z))
    u = u01_all()
    if not np.array_equal(u, d["u"]):
        raise SystemExit("philox_u01 on the device differs from its numpy float32 restatement")
    u64 = u.astype(np.float64)
    rec = {"what": "exhaustive over the 2^24 values x >> 8 of philox_u01; float64 references by numpy", "points": int(u.size),
           "distinct_u": int(np.unique(u).size), "u_min": float(u.min()), "u_max": float(u.max())}
    for key, ref in (("rad", np.sqrt(-2.0 * np.log(u64))), ("rad_libm", np.sqrt(-2.0 * np.log(u64)))):
        got = d[key].astype(np.float64)
        rel = np.where(ref > 0, np.abs(got - ref) / np.where(ref > 0, ref, 1.0), np.abs(got))      # (at ref == 0 the result must be 0)
        rec[key] = {"what": "sqrtf(-2 ln2 v_log_f32(u))" if key == "rad" else "sqrtf(-2 logf(u))", "max_rel": worst(rel, u, d[key]),
                    "at_one": float(d[key][u == np.float32(1.0)].max()), "exact_zero_at_one": bool((d[key][u == np.float32(1.0)] == 0).all()),
                    "nan": int(np.isnan(d[key]).sum()), "negative": int((d[key] < 0).sum()),
                    "largest": float(d[key].max()), "largest_at_u": float(u[int(np.argmax(d[key]))]),
                    "largest_float64": float(ref.max())}
    ang = 2.0 * np.pi * u64
    rec["sin_rev"] = {"what": "v_sin_f32(u) against sin(2 pi u)", "max_abs": worst(np.abs(d["sin_rev"] - np.sin(ang)), u, d["sin_rev"])}
    rec["cos_rev"] = {"what": "v_cos_f32(u) against cos(2 pi u)", "max_abs": worst(np.abs(d["cos_rev"] - np.cos(ang)), u, d["cos_rev"])}
    t = d["t"]
    if not np.array_equal(t, np.float32(6.283185307179586) * u):
        raise SystemExit("the device's fp32 angle 2 pi_f32 u differs from numpy's")
    t64 = t.astype(np.float64)
    rec["sinf"] = {"what": "sinf(t) against sin(t), t = fl32(6.283185307179586f u)", "max_abs": worst(np.abs(d["sinf"] - np.sin(t64)), u, d["sinf"])}
    rec["cosf"] = {"what": "cosf(t) against cos(t), t = fl32(6.283185307179586f u)", "max_abs": worst(np.abs(d["cosf"] - np.cos(t64)), u, d["cosf"])}
    # the trig error of the fill's normals against the angle 2 pi u itself: what the rounding of t adds
    rec["angle_abs"] = worst(np.abs(t64 - ang), u, t)
    lg = np.log(u64)
    err = np.where(lg != 0, ulp_error(d["logf"], lg), np.abs(d["logf"].astype(np.float64)) / 2.0 ** -149)      # (ln 1: exactly 0, or counted in denormal steps)
    i = int(np.argmax(err))
    rec["logf"] = {"what": "logf(u) in units of the float32 spacing at ln u; the entry functions.logf starts at 1e-6 and does not cover "
                           "u down to 2^-25", "max_ulp": float(err[i]), "at_u": float(u[i]), "got": float(d["logf"][i])}
    return rec


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
    end = 4 + 4 * 6 * n
    data = raw[4:end].view(np.float32).reshape(3, 2, n)
    m = int(raw[end:end + 4].view(np.int32)[0])
    noise = raw[end + 4:].view(np.float32).reshape(len(NOISE_FNS), m)
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
    rec["noise"] = noise_record(noise)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"functions": rec["functions"], "noise": rec["noise"]}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
