"""Isotropic vs per-dimension (ARD) lengthscales at BASELINE configs[2]'s shape (OILMM, 32 Matern52 latents, p = 64, n = 16384) with
d-dimensional inputs (default 4): logpdf and logpdf_and_gradient, median of --reps timed calls each.  Prints one JSON line per phase
and, with --copy, times a device-to-device copy of --copy-gib GiB (the HBM copy ceiling the gradient reduction is compared with; under
`rocprofv3 --kernel-trace --stats` its kernel and grad_reduce_ard_kernel appear side by side).

    python tools/ard_bench.py [--n N] [--m M] [--d D] [--reps R] [--grad] [--copy]
"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import lmm_amd

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--m", type=int, default=32)
ap.add_argument("--p", type=int, default=64)
ap.add_argument("--d", type=int, default=4)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--grad", action="store_true", help="also time logpdf_and_gradient")
ap.add_argument("--copy", action="store_true", help="also time a device-to-device copy (HBM ceiling)")
ap.add_argument("--copy-gib", type=float, default=2.0)
args = ap.parse_args()

lmm_amd.init(0)
rng = np.random.default_rng(0)
n, m, p, d = args.n, args.m, args.p, args.d
x = rng.uniform(0.0, 20.0, size=(d, n))
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
y = rng.standard_normal(n * p)
var = rng.uniform(0.8, 1.2, m)
ls_iso = rng.uniform(2.0, 4.0, m)
ls_ard = [rng.uniform(2.0, 4.0, d) for _ in range(m)]
xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
xin = lmm_amd.MOInputIsotopicByOutputs(xd, p)
H = lmm_amd.Orthogonal(np.ascontiguousarray(U), S)


def fx(ard):
    ks = [lmm_amd.Matern52Kernel(var[l], ls_ard[l] if ard else ls_iso[l]) for l in range(m)]
    return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(k) for k in ks]), H)(xin, 0.1)


def timed(name, fn, extra=None):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    line = {"phase": name, "ms": round(float(np.median(ts)) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in ts],
            "n": n, "m": m, "p": p, "d": d}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return float(np.median(ts))


for ard in (False, True):
    f = fx(ard)
    timed(f"logpdf_{'ard' if ard else 'iso'}", lambda: lmm_amd.logpdf(f, yd))
if args.grad:
    for ard in (False, True):
        f = fx(ard)
        # the gradient reduction reads the lower triangle of each latent's n x n inverse once: n (n + 64) / 2 doubles per latent
        timed(f"grad_{'ard' if ard else 'iso'}", lambda: lmm_amd.logpdf_and_gradient(f, yd),
              {"reduce_bytes_per_latent": n * (n + 64) / 2 * 8})
if args.copy:
    cnt = int(args.copy_gib * (1 << 30)) // 8
    a = torch.empty(cnt, dtype=torch.float64, device="cuda").fill_(1.0)
    b = torch.empty_like(a)
    dt = timed("d2d_copy", lambda: b.copy_(a))
    print(json.dumps({"phase": "d2d_copy_rate", "GBps_read_plus_write": round(2 * cnt * 8 / dt / 1e9, 1)}), flush=True)
