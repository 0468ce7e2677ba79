"""Locally periodic latents (SE x Periodic, LocallyPeriodicKernel) at BASELINE configs[2]'s shape (OILMM, 32 latents, p = 64,
n = 16384).  In one process, at d = 1 (sorted inputs) and d = 3, --reps repetitions each, for all-Matern52, all-periodic and
all-locally-periodic latents:
  * the Gram-assembly time and rate (profile class "gram" of lmm_profile_begin(1) / lmm_profile_end) of one logpdf; the periodic
    repetitions give the run-to-run spread the locally periodic figure is to be read against (one FMA chain more before the same exp);
  * end-to-end logpdf and logpdf_and_gradient time.
Prints one JSON line per measurement and writes them all to --out (default profiles/locally_periodic_bench.json).

    python tools/locally_periodic_bench.py [--n N] [--m M] [--reps R] [--out FILE]
"""
import argparse
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
ap.add_argument("--out", default="profiles/locally_periodic_bench.json")
args = ap.parse_args()

lmm_amd.init(0)
lib = L.load()
rng = np.random.default_rng(0)
n, m, p = args.n, args.m, args.p
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
H = lmm_amd.Orthogonal(np.ascontiguousarray(U), S)
yd = torch.from_numpy(rng.standard_normal(n * p)).cuda()
var = rng.uniform(0.8, 1.2, m)
ls = rng.uniform(2.0, 4.0, m)
rho = rng.uniform(0.6, 1.5, m)
decay = rng.uniform(2.0, 6.0, m)
KINDS = ("matern52", "periodic", "locally_periodic")
KERNEL = {"matern52": lambda l: lmm_amd.Matern52Kernel(var[l], ls[l]),
          "periodic": lambda l: lmm_amd.PeriodicKernel(var[l], ls[l], r=rho[l]),
          "locally_periodic": lambda l: lmm_amd.LocallyPeriodicKernel(var[l], ls[l], r=rho[l], decay=decay[l])}
results = []


def emit(line):
    line.update({"n": n, "m": m, "p": p})
    results.append(line)
    print(json.dumps(line), flush=True)


def model(kind, xin):
    return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(KERNEL[kind](l)) for l in range(m)]), H)(xin, 0.1)


for d in (1, 3):
    x = np.sort(rng.uniform(0.0, 20.0, n)) if d == 1 else rng.uniform(0.0, 20.0, size=(d, n))
    xin = lmm_amd.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p)
    gi = L.PROF_CLASSES.index("gram")
    for kind in KINDS:
        f = model(kind, xin)
        lmm_amd.logpdf(f, yd); torch.cuda.synchronize()                      # warm-up
        ms, tbs = [], []
        for _ in range(args.reps):
            L.check(lib.lmm_profile_begin(1))
            lmm_amd.logpdf(f, yd)
            ent = (L.ProfEntryT * len(L.PROF_CLASSES))()
            L.check(lib.lmm_profile_end(ent))
            ms.append(ent[gi].ms)
            tbs.append(ent[gi].bytes / (ent[gi].ms * 1e-3) / 1e12 if ent[gi].ms > 0 else 0.0)
        emit({"phase": "gram", "kind": kind, "d": d, "ms_all": [round(t, 3) for t in ms], "ms": round(float(np.median(ms)), 3),
              "TBps_all": [round(t, 3) for t in tbs], "TBps": round(float(np.median(tbs)), 3)})
    for phase, call in (("logpdf", lmm_amd.logpdf), ("logpdf_and_gradient", lmm_amd.logpdf_and_gradient)):
        for kind in KINDS:
            f = model(kind, xin)
            call(f, yd); torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                call(f, yd)
                torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            emit({"phase": phase, "kind": kind, "d": d, "ms_all": [round(t * 1e3, 3) for t in ts], "ms": round(float(np.median(ts)) * 1e3, 3)})

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
