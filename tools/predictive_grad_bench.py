"""Cost of the predictive-marginal input gradient at one GPU's share of BASELINE configs[3] (OILMM, H 128 x 64, ml latents of the
shard, n = n* = 8192, Matern52, d = 1, Float64): mean_and_var, mean_and_var_vjp with both cotangents, mean, and the mean-only VJP,
median of --reps timed calls each on one posterior.  Prints one JSON line per phase and a "ratio" line (VJP against its forward
call).  Under `rocprofv3 --kernel-trace --stats` the right solve appears as trsm_nn_kernel and the pair pass as pred_grad_x_kernel.

    python tools/predictive_grad_bench.py [--ml 8] [--n 8192] [--ns 8192] [--reps 3]
"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import lmm_amd
from lmm_amd import workloads as W      # input generation only

ap = argparse.ArgumentParser()
ap.add_argument("--ml", type=int, default=8, help="latents of this GPU's shard (configs[3]: 64 latents over 8 GPUs)")
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--ns", type=int, default=8192)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

lmm_amd.init(0)
m, p, n, ns, ml = 64, 128, args.n, args.ns, args.ml
P = W.synthetic_problem(m, p, n, "matern52", True, s2=0.1, seed=0)
fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel()) for _ in range(m)])
H = lmm_amd.Orthogonal(P["U"], P["S"])
xd, yd = torch.from_numpy(P["x"]).cuda(), torch.from_numpy(P["y"]).cuda()
xs = torch.from_numpy(np.linspace(P["x"][0], P["x"][-1], ns) + 0.5 * 20.0 / 575.0).cuda()
post = lmm_amd.posterior(lmm_amd.ILMM(fs, H, shard=(0, ml))(lmm_amd.MOInputIsotopicByOutputs(xd, p), 0.1), yd)
fx = post(lmm_amd.MOInputIsotopicByOutputs(xs, p), 0.1)
rng = np.random.default_rng(1)
dmean, dvar = torch.from_numpy(rng.standard_normal(ns * p)).cuda(), torch.from_numpy(rng.standard_normal(ns * p)).cuda()


def timed(name, fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    print(json.dumps({"phase": name, "ms": round(t * 1e3, 3), "ms_all": [round(v * 1e3, 3) for v in ts], "n": n, "ns": ns, "ml": ml,
                      "p": p}), flush=True)
    return t


t_mv = timed("mean_and_var", lambda: lmm_amd.mean_and_var(fx))
t_vjp = timed("mean_and_var_vjp", lambda: lmm_amd.mean_and_var_vjp(fx, dmean, dvar))
t_m = timed("mean", lambda: lmm_amd.mean(fx))
t_mvjp = timed("mean_vjp", lambda: lmm_amd.mean_and_var_vjp(fx, dmean))
# the right solve alone costs ml n^2 n* flops (the forward solve's count)
print(json.dumps({"phase": "ratio", "vjp_over_mean_and_var": round(t_vjp / t_mv, 3), "mean_vjp_over_mean": round(t_mvjp / t_m, 3),
                  "right_solve_flops": ml * n * n * ns}), flush=True)
