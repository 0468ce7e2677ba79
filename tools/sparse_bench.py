"""Inducing-point (VFE) inference on an OILMM with 32 Matern52 latents and p = 64, device-resident x and y: for
n in {16384, 262144, 1048576} and M in {128, 512, 1024} (x uniform on [0, 2000], z equispaced over it, lengthscales 2 to 4, so that K_uu stays
well conditioned at M = 1024; DESIGN.md 4.16 has the numerics of closer inducing points), the median over --reps repetitions after a
warm-up of
  * elbo_ms      lmm_oilmm_elbo end to end,
  * moments_ms   lmm_dev_sparse_moments for ONE latent (the moments kernel and its reduction), with its TFLOP/s at n M^2 flops and the
                 kernel evaluations per second at n M (K_uf elements; the tiling evaluates each ceil(M / 64) times),
  * at n = 16384 exact_ms, lmm_oilmm_logpdf on the same data.
Prints one JSON line per case and writes them all to --out (default profiles/sparse_bench.json).

    python tools/sparse_bench.py [--ns 16384,262144,1048576] [--Ms 128,512,1024] [--m 32] [--p 64] [--reps R] [--out FILE]
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
ap.add_argument("--ns", default="16384,262144,1048576")
ap.add_argument("--Ms", default="128,512,1024")
ap.add_argument("--m", type=int, default=32)
ap.add_argument("--p", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="profiles/sparse_bench.json")
args = ap.parse_args()

lmm_amd.init(0)
lib = L.load()
rng = np.random.default_rng(0)
m, p = args.m, args.p
XMAX = 2000.0          # inputs and inducing inputs span [0, XMAX]: at M = 1024 neighbouring inducing points are about a lengthscale apart
U, _, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
S = np.linspace(2.0, 1.0, m)
descs = [{"kind": "matern52", "variance": float(rng.uniform(0.8, 1.2)), "lengthscale": float(rng.uniform(2.0, 4.0))} for _ in range(m)]
gps, gp1 = L.gps_array(descs), L.gps_array(descs[:1])
Ua, Sa = L.Arr(np.ascontiguousarray(U.T.reshape(-1))), L.Arr(S)


def median_ms(call):
    call(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


results = []
for n in map(int, args.ns.split(",")):
    x = torch.from_numpy(np.sort(rng.uniform(0.0, XMAX, n))).cuda()
    y = torch.from_numpy(rng.standard_normal(n * p)).cuda()
    w = torch.full((n,), 0.07, dtype=torch.float64, device="cuda")
    r = torch.from_numpy(rng.standard_normal(n)).cuda()
    xa, ya = L.Arr(x), L.Arr(y)
    exact = None
    if n <= 16384:
        out = C.c_double()
        exact = median_ms(lambda: L.check(lib.lmm_oilmm_logpdf(xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(0.1), gps, 0, m, 1,
                                                               C.byref(out))))
    for M in map(int, args.Ms.split(",")):
        z = torch.linspace(0.0, XMAX, M, dtype=torch.float64, device="cuda")
        e, t = C.c_double(), C.c_double()
        elbo_ms = median_ms(lambda: L.check(lib.lmm_oilmm_elbo(xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, 0.1, gps, 0, m, z.data_ptr(), M,
                                                               1e-6, 1, C.byref(e), C.byref(t))))
        Phi = torch.empty(M * M, dtype=torch.float64, device="cuda")
        b, sc = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
        mom_ms = median_ms(lambda: L.check(lib.lmm_dev_sparse_moments(x.data_ptr(), 1, n, z.data_ptr(), M, gp1, w.data_ptr(), r.data_ptr(),
                                                                      0, Phi.data_ptr(), M, b.data_ptr(), sc.data_ptr())))
        line = {"n": n, "M": M, "m": m, "p": p, "elbo_ms": round(elbo_ms, 3), "elbo": e.value, "dtc": t.value,
                "moments_ms_one_latent": round(mom_ms, 3), "moments_tflops": round(float(n) * M * M / (mom_ms * 1e-3) / 1e12, 3),
                "kuf_elements_per_s": float(n) * M / (mom_ms * 1e-3),
                "kernel_evaluations_per_s": float(n) * M * ((M + 63) // 64) / (mom_ms * 1e-3)}
        if exact is not None:
            line["exact_logpdf_ms"] = round(exact, 3)
        results.append(line)
        print(json.dumps(line), flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
