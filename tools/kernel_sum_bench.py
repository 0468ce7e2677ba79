"""Sum latents (KernelSum) at BASELINE configs[2]'s shape (OILMM, 32 latents, p = 64, n = 16384): all-Matern52 vs all-(Matern52 + SE)
vs 4-term latents (Matern52 + SE + Matern12 + RQ) with d-dimensional inputs (d = 1 sorted and d = 4 by default): logpdf and, with
--grad, logpdf_and_gradient, median of --reps timed calls each.  Prints one JSON line per (config, d, phase).  Under
`rocprofv3 --kernel-trace --stats` the sum instantiation of gram_batch_kernel (template argument 5) appears next to Matern52's.

    python tools/kernel_sum_bench.py [--n N] [--m M] [--dims 1,4] [--configs m52,m52+se,4term] [--reps R] [--grad]
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
ap.add_argument("--dims", default="1,4")
ap.add_argument("--configs", default="m52,m52+se,4term")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--grad", action="store_true", help="also time logpdf_and_gradient")
args = ap.parse_args()

lmm_amd.init(0)
rng = np.random.default_rng(0)
n, m, p = args.n, args.m, args.p
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
H = lmm_amd.Orthogonal(np.ascontiguousarray(U), S)
y = rng.standard_normal(n * p)
yd = torch.from_numpy(y).cuda()
var = rng.uniform(0.8, 1.2, m)
ls = rng.uniform(2.0, 4.0, m)
KERNEL = {"m52": lambda l: lmm_amd.Matern52Kernel(var[l], ls[l]),
          "m52+se": lambda l: lmm_amd.Matern52Kernel(var[l], ls[l]) + lmm_amd.SEKernel(0.3, 10.0),
          "4term": lambda l: lmm_amd.KernelSum(lmm_amd.Matern52Kernel(var[l], ls[l]), lmm_amd.SEKernel(0.3, 10.0),
                                               lmm_amd.Matern12Kernel(0.1, 0.5), lmm_amd.RationalQuadraticKernel(0.2, 3.0))}


def timed(name, fn, extra):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    line = {"phase": name, "ms": round(float(np.median(ts)) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in ts], "n": n, "m": m, "p": p}
    line.update(extra)
    print(json.dumps(line), flush=True)


for d in (int(s) for s in args.dims.split(",")):
    x = np.sort(rng.uniform(0.0, 20.0, n)) if d == 1 else rng.uniform(0.0, 20.0, size=(d, n))
    xin = lmm_amd.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p)
    for cfg in args.configs.split(","):
        f = lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(KERNEL[cfg](l)) for l in range(m)]), H)(xin, 0.1)
        timed("logpdf", lambda: lmm_amd.logpdf(f, yd), {"config": cfg, "d": d})
        if args.grad:
            timed("grad", lambda: lmm_amd.logpdf_and_gradient(f, yd), {"config": cfg, "d": d})
