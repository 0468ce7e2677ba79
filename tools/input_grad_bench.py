"""Cost of the input-location gradient at BASELINE configs[2]'s shape (OILMM, 32 Matern52 latents, p = 64, n = 16384): for d = 1 and
d = 4, logpdf_and_gradient with and without inputs=True, median of --reps timed calls each.  Prints one JSON line per (d, phase); an
"overhead" line gives inputs=True against inputs=False in percent.  Under `rocprofv3 --kernel-trace --stats` grad_x_kernel appears
next to grad_reduce_kernel, and --copy adds a device-to-device copy of --copy-gib GiB (the HBM copy ceiling).

    python tools/input_grad_bench.py [--n N] [--m M] [--ds 1,4] [--reps R] [--copy]
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
ap.add_argument("--ds", default="1,4")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--copy", action="store_true", help="also time a device-to-device copy (HBM ceiling)")
ap.add_argument("--copy-gib", type=float, default=2.0)
args = ap.parse_args()

lmm_amd.init(0)
rng = np.random.default_rng(0)
n, m, p = args.n, args.m, args.p
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
H = lmm_amd.Orthogonal(np.ascontiguousarray(U), S)
y = rng.standard_normal(n * p)
var, ls = rng.uniform(0.8, 1.2, m), rng.uniform(2.0, 4.0, m)
yd = torch.from_numpy(y).cuda()
f = lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel(var[l], ls[l])) for l in range(m)]), H)


def timed(name, fn, extra=None):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    line = {"phase": name, "ms": round(float(np.median(ts)) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in ts], "n": n, "m": m, "p": p}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return float(np.median(ts))


for d in [int(v) for v in args.ds.split(",")]:
    x = rng.uniform(0.0, 20.0, n) if d == 1 else rng.uniform(0.0, 20.0, size=(d, n))
    fx = f(lmm_amd.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p), 0.1)
    base = timed("grad", lambda: lmm_amd.logpdf_and_gradient(fx, yd), {"d": d})
    # the input gradient reads the lower triangle of each latent's n x n inverse twice: n (n + 64) doubles per latent
    t = timed("grad_inputs", lambda: lmm_amd.logpdf_and_gradient(fx, yd, inputs=True),
              {"d": d, "grad_x_bytes_per_latent": n * (n + 64) * 8})
    print(json.dumps({"phase": "overhead", "d": d, "overhead_pct": round(100.0 * (t - base) / base, 2)}), flush=True)
if args.copy:
    cnt = int(args.copy_gib * (1 << 30)) // 8
    a = torch.empty(cnt, dtype=torch.float64, device="cuda").fill_(1.0)
    b = torch.empty_like(a)
    dt = timed("d2d_copy", lambda: b.copy_(a))
    print(json.dumps({"phase": "d2d_copy_rate", "GBps_read_plus_write": round(2 * cnt * 8 / dt / 1e9, 1)}), flush=True)
