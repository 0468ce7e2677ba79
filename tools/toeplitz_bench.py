"""Times the Toeplitz path beside the dense path of the same build -> profiles/toeplitz_bench.json.
Two models of 32 latents over p = 64 outputs, data on the device: SE latents, and Matern52 + SE * Periodic sums (the locally
periodic kind is SE * Periodic).  n = 2048, 8192 and the cap if it is larger.  Per (model, n): medians of 3 after a warm-up of
toeplitz_logpdf, toeplitz_logpdf_and_gradient, logpdf and logpdf_and_gradient, and the agreement of the two values.
Usage: python tools/toeplitz_bench.py [--out profiles/toeplitz_bench.json] [--dense-max-n 8192]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lmm_amd as lmm  # noqa: E402

M, P, S2 = 32, 64, 0.1


def model(kind, rng):
    if kind == "se":
        ks = [lmm.SEKernel(1.0, 0.5 + 0.05 * l) for l in range(M)]
    else:
        ks = [lmm.KernelSum(lmm.Matern52Kernel(0.5, 2.0 + 0.1 * l), lmm.LocallyPeriodicKernel(1.0, 1.0, 1.0, 5.0 + 0.1 * l)) for l in range(M)]
    U = np.linalg.qr(rng.standard_normal((P, M)))[0]
    return lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, np.linspace(1.0, 2.0, M)))


def timed(fn):
    fn()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "toeplitz_bench.json"))
    ap.add_argument("--dense-max-n", type=int, default=8192)
    a = ap.parse_args()
    lmm.init(0)
    cap = lmm.load().lmm_toeplitz_max_n()
    rows = []
    for kind in ("se", "matern52+se*periodic"):
        for n in sorted({2048, 8192, cap} & set(range(cap + 1))):
            rng = np.random.default_rng(n)
            x = torch.linspace(0.0, 0.01 * (n - 1), n, dtype=torch.float64, device="cuda")
            y = torch.tensor(rng.standard_normal(n * P), device="cuda")
            fx = model(kind, rng)(lmm.MOInputIsotopicByOutputs(x, P), S2)
            rec = {"model": kind, "n": n, "m": M, "p": P}
            rec["toeplitz_logpdf_ms"], v = timed(lambda: lmm.toeplitz_logpdf(fx, y))
            rec["toeplitz_logpdf_and_gradient_ms"], _ = timed(lambda: lmm.toeplitz_logpdf_and_gradient(fx, y))
            if n <= a.dense_max_n:
                rec["logpdf_ms"], vd = timed(lambda: lmm.logpdf(fx, y))
                rec["logpdf_and_gradient_ms"], _ = timed(lambda: lmm.logpdf_and_gradient(fx, y))
                rec["value_rel_diff"] = abs(v - vd) / abs(vd)
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/toeplitz_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
