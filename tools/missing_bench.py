"""Missing observations (NaN in y) at BASELINE configs[2]'s shape (OILMM, 32 latents, p = 64, n = 16384).  In one process, end-to-end
logpdf time (device-resident x and y, --reps repetitions after a warm-up, median) of
  * lmm_oilmm_logpdf on the full data (the baseline every case is compared with),
  * lmm_oilmm_logpdf_missing with 0 %, 10 % and 50 % of the entries missing at random (about n patterns; every point keeps at least m
    observed outputs), and with 10 % missing confined to 4 patterns.
The front end is O(n p m) plus at most n (p m^2 + m^3) flops, ~3e9 here against 4.7e13 for the factorisations, so an overhead that
shows would be host grouping or launch latency; "front_ms" is lmm_oilmm_project_missing alone (mask, grouping, patterns, apply).
Prints one JSON line per case and writes them all to --out (default profiles/missing_bench.json).

    python tools/missing_bench.py [--n N] [--m M] [--p P] [--reps R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import lmm_amd
from lmm_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--m", type=int, default=32)
ap.add_argument("--p", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="profiles/missing_bench.json")
args = ap.parse_args()

lmm_amd.init(0)
lib = L.load()
rng = np.random.default_rng(0)
n, m, p = args.n, args.m, args.p
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
S = np.linspace(2.0, 1.0, m)
x = torch.from_numpy(np.sort(rng.uniform(0.0, 20.0, n))).cuda()
Yfull = rng.standard_normal((p, n))
gps = L.gps_array([{"kind": "matern52", "variance": float(rng.uniform(0.8, 1.2)), "lengthscale": float(rng.uniform(2.0, 4.0))}
                   for _ in range(m)])
Ua, Sa, xa = L.Arr(np.ascontiguousarray(U.T.reshape(-1))), L.Arr(S), L.Arr(x)


def random_missing(frac):
    """Each point loses Binomial(p, frac) outputs at random, never more than p - m."""
    Y = Yfull.copy()
    for t in range(n):
        k = min(int(rng.binomial(p, frac)), p - m)
        Y[rng.choice(p, size=k, replace=False), t] = np.nan
    return Y


def four_patterns(frac):
    Y = Yfull.copy()
    k = int(round(frac * p * 4 / 3))                   # one of the four patterns is "nothing missing"
    pats = [()] + [tuple(rng.choice(p, size=min(k, p - m), replace=False)) for _ in range(3)]
    for t in range(n):
        Y[list(pats[t % 4]), t] = np.nan
    return Y


def timed(fn, Y):
    yd = torch.from_numpy(np.ascontiguousarray(Y.reshape(-1))).cuda()
    ya, out = L.Arr(yd), C.c_double()

    def call():
        L.check(fn(xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(0.1), gps, 0, m, 1, C.byref(out)))
    call(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return out.value, ts, ya


def front(ya):
    reg, npat = C.c_double(), C.c_int()
    ts = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        L.check(lib.lmm_oilmm_project_missing(ya.ptr, n, p, Ua.ptr, Sa.ptr, m, C.c_double(0.1), None, None, None, C.byref(reg),
                                              C.byref(npat)))
        ts.append(time.perf_counter() - t0)
    return npat.value, float(np.median(ts[1:])) * 1e3


results = []
base_val, base_ts, _ = timed(lib.lmm_oilmm_logpdf, Yfull)
base = float(np.median(base_ts)) * 1e3
results.append({"case": "full data, lmm_oilmm_logpdf", "ms_all": [round(t * 1e3, 3) for t in base_ts], "ms": round(base, 3)})
print(json.dumps(results[-1]), flush=True)
cases = [("0 % missing", Yfull), ("10 % missing at random", random_missing(0.1)), ("50 % missing at random", random_missing(0.5)),
         ("10 % missing in 4 patterns", four_patterns(0.1))]
for name, Y in cases:
    val, ts, ya = timed(lib.lmm_oilmm_logpdf_missing, Y)
    npat, fms = front(ya)
    ms = float(np.median(ts)) * 1e3
    line = {"case": name + ", lmm_oilmm_logpdf_missing", "missing_fraction": round(float(np.isnan(Y).mean()), 4), "patterns": npat,
            "ms_all": [round(t * 1e3, 3) for t in ts], "ms": round(ms, 3), "front_ms": round(fms, 3),
            "over_full_data": round(ms / base, 4)}
    if name.startswith("0 %"):
        line["rel_diff_to_lmm_oilmm_logpdf"] = abs(val - base_val) / abs(base_val)
    line.update({"n": n, "m": m, "p": p})
    results.append(line)
    print(json.dumps(line), flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
