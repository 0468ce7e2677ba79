"""Gradient of the inducing-point (VFE) bound at the shapes and inputs of tools/sparse_bench.py: an OILMM with 32
Matern52 latents and p = 64, device-resident x and y, n in {16384, 262144, 1048576} and M in {128, 512, 1024} (x uniform on [0, 2000], z
equispaced over it, lengthscales 2 to 4).  Per case, in one process and on the same data, the median over --reps repetitions after a
warm-up of
  * elbo_grad_ms   lmm_oilmm_elbo_grad end to end (every output requested) and elbo_ms, lmm_oilmm_elbo, with their ratio,
  * grad_pass_ms   lmm_dev_sparse_grad for ONE latent (the second pass over the points and its reduction) and moments_ms,
                   lmm_dev_sparse_moments for the same latent, with their ratio.
No pass / fail threshold: the ratios are recorded beside DESIGN.md 4.16's expectation of 2-3x.  Prints one JSON line per case and
writes them all to --out (default profiles/sparse_grad_bench.json).

    python tools/sparse_grad_bench.py [--ns 16384,262144,1048576] [--Ms 128,512,1024] [--m 32] [--p 64] [--reps R] [--out FILE]
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
ap.add_argument("--out", default="profiles/sparse_grad_bench.json")
args = ap.parse_args()

lmm_amd.init(0)
lib = L.load()
rng = np.random.default_rng(0)
m, p = args.m, args.p
XMAX = 2000.0          # as tools/sparse_bench.py: at M = 1024 neighbouring inducing points are about a lengthscale apart
U, _, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
S = np.linspace(2.0, 1.0, m)
descs = [{"kind": "matern52", "variance": float(rng.uniform(0.8, 1.2)), "lengthscale": float(rng.uniform(2.0, 4.0))} for _ in range(m)]
gps, gp1 = L.gps_array(descs), L.gps_array(descs[:1])
Ua, Sa = L.Arr(np.ascontiguousarray(U.T.reshape(-1))), L.Arr(S)
dev = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")


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
    gy = dev(n * p)
    for M in map(int, args.Ms.split(",")):
        z = torch.linspace(0.0, XMAX, M, dtype=torch.float64, device="cuda")
        e, t, v, gs2 = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        gS, gU, gg, gz = np.empty(m), np.empty(p * m), (L.GpGradT * m)(), dev(M)
        elbo_ms = median_ms(lambda: L.check(lib.lmm_oilmm_elbo(xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, 0.1, gps, 0, m, z.data_ptr(), M,
                                                               1e-6, 1, C.byref(e), C.byref(t))))
        grad_ms = median_ms(lambda: L.check(lib.lmm_oilmm_elbo_grad(xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, 0.1, gps, 0, m, z.data_ptr(),
                                                                    M, 1e-6, 1, C.byref(v), gy.data_ptr(), C.byref(gs2),
                                                                    gS.ctypes.data, gU.ctypes.data, gg, gz.data_ptr())))
        assert v.value == e.value
        Phi, b, sc = dev(M * M), dev(M), dev(3)
        mom_ms = median_ms(lambda: L.check(lib.lmm_dev_sparse_moments(x.data_ptr(), 1, n, z.data_ptr(), M, gp1, w.data_ptr(), r.data_ptr(),
                                                                      0, Phi.data_ptr(), M, b.data_ptr(), sc.data_ptr())))
        A = torch.from_numpy(rng.standard_normal((M, M))).cuda()
        PhiBar, beta = (0.5 * (A + A.T)).contiguous(), torch.from_numpy(rng.standard_normal(M)).cuda()
        rec, gz1, gr = dev(4 * 11), dev(M), dev(n)
        pass_ms = median_ms(lambda: L.check(lib.lmm_dev_sparse_grad(x.data_ptr(), 1, n, z.data_ptr(), M, gp1, w.data_ptr(), r.data_ptr(),
                                                                    PhiBar.data_ptr(), M, beta.data_ptr(), 0, rec.data_ptr(),
                                                                    gz1.data_ptr(), gr.data_ptr())))
        line = {"n": n, "M": M, "m": m, "p": p, "elbo_ms": round(elbo_ms, 3), "elbo_grad_ms": round(grad_ms, 3),
                "grad_over_elbo": round(grad_ms / elbo_ms, 3), "elbo": e.value,
                "moments_ms_one_latent": round(mom_ms, 3), "grad_pass_ms_one_latent": round(pass_ms, 3),
                "grad_pass_over_moments": round(pass_ms / mom_ms, 3),
                "grad_pass_tflops": round(2.0 * float(n) * M * M / (pass_ms * 1e-3) / 1e12, 3),
                "kernel_evaluations_per_s": float(n) * M * (((M + 63) // 64) + 1) / (pass_ms * 1e-3)}
        results.append(line)
        print(json.dumps(line), flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
