"""Timings of the gradient of the state-space logpdf -> profiles/statespace_grad_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), n = 16384 / 262144 / 1048576:
  * statespace_logpdf_and_gradient against statespace_logpdf at every n: what the smoother, the forward-mode (dual number) pass and the
    chain rule cost on top of the value;
  * at n = 16384 only, against logpdf_and_gradient (the Cholesky path) of the same build, with the largest relative difference of the
    two gradients, and both against central differences of statespace_logpdf (step 1e-4) in sigma2 and in latent 0's variance,
    lengthscale and mean: the value is shared by both paths, so the differences say which gradient a disagreement belongs to.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  A figure no run produced is written as "not measured".  No threshold is
asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from statespace_bench import M_LAT, P_OUT, S2, make_problem, timed

FD_STEP = 1e-4


def finite_differences(lmm, f, x, y):
    """Central differences of statespace_logpdf in sigma2 and in latent 0's (variance, lengthscale, mean)."""
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)

    def value(s2=S2, dv=0.0, dl=0.0, dm=0.0):
        k0 = f.f.fs[0].kernel
        g0 = lmm.GP(f.f.fs[0].mean + dm, lmm.Matern52Kernel(k0.variance + dv, k0.lengthscale + dl))
        return lmm.statespace_logpdf(lmm.ILMM(lmm.independent_mogp([g0] + list(f.f.fs[1:])), f.H)(xin, s2), y)

    h = FD_STEP
    return {"sigma2": (value(s2=S2 + h) - value(s2=S2 - h)) / (2 * h), "variance": (value(dv=h) - value(dv=-h)) / (2 * h),
            "lengthscale": (value(dl=h) - value(dl=-h)) / (2 * h), "mean": (value(dm=h) - value(dm=-h)) / (2 * h)}


def flat(g):
    """Every gradient of a dict as one host vector: y, sigma2, S, U and the latents' variance, lengthscale and mean."""
    y = g["y"].cpu().numpy() if hasattr(g["y"], "cpu") else np.asarray(g["y"])
    gps = np.array([[q["variance"], q["lengthscale"], q["mean"]] for q in g["gps"]])
    return {"y": y, "sigma2": np.array([g["sigma2"]]), "S": np.asarray(g["S"]), "U": np.asarray(g["U"]).reshape(-1),
            "variance": gps[:, 0], "lengthscale": gps[:, 1], "mean": gps[:, 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_grad_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--exact-n", type=int, default=16384)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "kernel": "matern52", "sigma2": S2, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "sizes": []}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for n in a.sizes:
        f, x, y = make_problem(lmm, n)
        fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
        row = {"n": n, "logpdf_and_gradient_ms": "not measured"}
        tv, tvr, v = timed(lambda: lmm.statespace_logpdf(fx, y), a.runs)
        tg, tgr, g = timed(lambda: lmm.statespace_logpdf_and_gradient(fx, y), a.runs)
        row.update(statespace_logpdf_ms=tv * 1e3, statespace_logpdf_runs_ms=[q * 1e3 for q in tvr],
                   statespace_logpdf_and_gradient_ms=tg * 1e3, statespace_logpdf_and_gradient_runs_ms=[q * 1e3 for q in tgr],
                   gradient_over_value=tg / tv, value_bitwise_equal=bool(g["value"] == v))
        if n == a.exact_n:
            tc, tcr, gc = timed(lambda: lmm.logpdf_and_gradient(fx, y), a.runs)
            a1, a2 = flat(g), flat(gc)
            row.update(logpdf_and_gradient_ms=tc * 1e3, logpdf_and_gradient_runs_ms=[q * 1e3 for q in tcr], speedup_over_cholesky_path=tc / tg,
                       relative_difference={k: float(np.abs(a1[k] - a2[k]).max() / np.abs(a2[k]).max()) for k in a1})
            fd = finite_differences(lmm, f, x, y)
            pick = lambda d, k: d["sigma2"] if k == "sigma2" else d["gps"][0][k]
            row["finite_differences"] = {k: {"central_difference": fd[k], "statespace": pick(g, k), "cholesky_path": pick(gc, k)} for k in fd}
            del gc
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        save()
        del f, fx, x, y, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
