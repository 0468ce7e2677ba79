"""Timings of SHO latents on the state-space and Cholesky paths (DESIGN.md 4.18 "SHO latents") -> profiles/sho_bench.json.

The settings of tools/statespace_bench.py: 32 latents, p = 64, d = 1, medians of `--runs` (>= 3) timed calls after one warm-up call.
For 32 SHO latents and for 32 Matern32 latents (the same state dimension; the SHO point step adds one sincos to Matern32's exp), at
n = 16384, 262144 and 1048576: statespace_logpdf, statespace_logpdf_and_gradient and one posterior statespace_rand sample (device
normals), and the ratios SHO / Matern32 of the same build.  At n = 16384 also logpdf (the Cholesky path) with both kinds, and its
relative difference from statespace_logpdf.  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.statespace_bench import M_LAT, P_OUT, S2, timed


def make_problem(lmm, kind, n, seed=0):
    """tools/statespace_bench.make_problem with SHO (period around 40 spacings, Q = 2 .. 8) or Matern32 latents."""
    import torch
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((P_OUT, M_LAT)))[0]
    S = rng.uniform(0.5, 2.0, M_LAT)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.cumsum(0.05 * (0.5 + torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)), 0)
    y = torch.randn(n * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
    if kind == "sho":
        ks = [lmm.SHOKernel(0.5 + 0.03 * l, 1.6 + 0.04 * l, 2.0 + 0.2 * l) for l in range(M_LAT)]
    else:
        ks = [lmm.Matern32Kernel(0.5 + 0.03 * l, 0.8 + 0.02 * l) for l in range(M_LAT)]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, S))
    torch.cuda.synchronize()
    return f, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sho_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--exact-n", type=int, default=16384)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "sigma2": S2, "runs": a.runs, "device": torch.cuda.get_device_name(0), "sizes": []}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for n in a.sizes:
        row = {"n": n}
        for kind in ("sho", "matern32"):
            f, x, y = make_problem(lmm, kind, n)
            fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
            rng = lmm.DeviceNormals(1)
            t, tr, v = timed(lambda: lmm.statespace_logpdf(fx, y), a.runs)
            row[f"{kind}_logpdf_ms"], row[f"{kind}_logpdf_runs_ms"], row[f"{kind}_logpdf_value"] = t * 1e3, [q * 1e3 for q in tr], v
            t, tr, g = timed(lambda: lmm.statespace_logpdf_and_gradient(fx, y), a.runs)
            row[f"{kind}_gradient_ms"], row[f"{kind}_gradient_runs_ms"] = t * 1e3, [q * 1e3 for q in tr]
            assert g["value"] == v
            t, tr, _ = timed(lambda: lmm.statespace_rand(rng, fx, y), a.runs)      # the draws are part of the call, for both kinds alike
            row[f"{kind}_rand_posterior_ms"], row[f"{kind}_rand_posterior_runs_ms"] = t * 1e3, [q * 1e3 for q in tr]
            if n == a.exact_n:
                t, tr, vc = timed(lambda: lmm.logpdf(fx, y), a.runs)
                row[f"{kind}_dense_logpdf_ms"], row[f"{kind}_dense_logpdf_runs_ms"] = t * 1e3, [q * 1e3 for q in tr]
                row[f"{kind}_dense_relative_difference"] = abs(v - vc) / abs(vc)
            del f, fx, x, y
            torch.cuda.empty_cache()
        for what in ("logpdf", "gradient", "rand_posterior") + (("dense_logpdf",) if n == a.exact_n else ()):
            row[f"ratio_sho_over_matern32_{what}"] = row[f"sho_{what}_ms"] / row[f"matern32_{what}_ms"]
        res["sizes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if "runs" not in k}), flush=True)
        save()


if __name__ == "__main__":
    main()
