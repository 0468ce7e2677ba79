"""Timings of the gradients with respect to locations on the state-space path (DESIGN.md 4.18 "Gradients with respect to locations")
-> profiles/statespace_input_grad_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_grad_bench.py), n = 16384 / 262144 / 1048576:
  * statespace_logpdf_and_gradient with and without inputs=True at every n: what "x" costs on top of the other gradients;
  * at n = 16384 only, logpdf_and_gradient(inputs=True) of the Cholesky path beside it, with the largest relative difference of the two
    "x", and both against central differences of statespace_logpdf (step 1e-4, 1 / 250 of the smallest spacing) in four of the x_t: the
    value is shared by both paths, so the differences say which gradient a disagreement belongs to;
  * at the largest n, post.mean_and_var_vjp beside post.mean_and_var at 1024 and 65536 device queries on one posterior object.
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


def finite_differences(lmm, f, x, y, points):
    """Central differences of statespace_logpdf in x_t for t in points (the spacings are >= 0.025: the points stay sorted)."""
    out = {}
    for t in points:
        vals = []
        for sign in (1.0, -1.0):
            xt = x.clone()
            xt[t] += sign * FD_STEP
            vals.append(lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(xt, P_OUT), S2), y))
        out[t] = (vals[0] - vals[1]) / (2 * FD_STEP)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_input_grad_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--exact-n", type=int, default=16384)
    ap.add_argument("--queries", type=int, nargs="*", default=[1024, 65536])
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "kernel": "matern52", "sigma2": S2, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "sizes": [], "queries": "not measured"}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    ms = lambda ts: [q * 1e3 for q in ts]
    for n in a.sizes:
        f, x, y = make_problem(lmm, n)
        fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
        row = {"n": n, "logpdf_and_gradient_inputs_ms": "not measured", "x_relative_difference": "not measured"}
        tg, tgr, g = timed(lambda: lmm.statespace_logpdf_and_gradient(fx, y), a.runs)
        tx, txr, gx = timed(lambda: lmm.statespace_logpdf_and_gradient(fx, y, inputs=True), a.runs)
        row.update(statespace_logpdf_and_gradient_ms=tg * 1e3, statespace_logpdf_and_gradient_runs_ms=ms(tgr),
                   statespace_logpdf_and_gradient_inputs_ms=tx * 1e3, statespace_logpdf_and_gradient_inputs_runs_ms=ms(txr),
                   inputs_over_without=tx / tg, other_entries_bitwise_equal=bool(gx["value"] == g["value"] and bool((gx["y"] == g["y"]).all())))
        if n == a.exact_n:
            tc, tcr, gc = timed(lambda: lmm.logpdf_and_gradient(fx, y, inputs=True), a.runs)
            host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
            d = float(np.abs(host(gx["x"]) - host(gc["x"])).max() / np.abs(host(gc["x"])).max())
            row.update(logpdf_and_gradient_inputs_ms=tc * 1e3, logpdf_and_gradient_inputs_runs_ms=ms(tcr), speedup_over_cholesky_path=tc / tx,
                       x_relative_difference=d)
            print(f"n = {n}: largest relative difference of the two \"x\": {d:.3e}", flush=True)
            fd = finite_differences(lmm, f, x, y, [1, n // 3, n // 2, n - 2])
            row["finite_differences"] = {str(t): {"central_difference": v, "statespace": float(host(gx["x"])[t]),
                                                  "cholesky_path": float(host(gc["x"])[t])} for t, v in fd.items()}
            del gc
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        save()
        if n == max(a.sizes):
            res["queries"] = []
            gen = torch.Generator(device="cuda").manual_seed(1)
            with lmm.statespace_posterior(fx, y) as post:
                for ns in a.queries:
                    xs = float(x[0]) + (float(x[-1]) - float(x[0])) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
                    dm = torch.randn(ns * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
                    dv = torch.randn(ns * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
                    tq, tqr, _ = timed(lambda: post.mean_and_var(xs), a.runs)
                    tv, tvr, _ = timed(lambda: post.mean_and_var_vjp(xs, dm, dv), a.runs)
                    qrow = {"n": n, "ns": ns, "mean_and_var_ms": tq * 1e3, "mean_and_var_runs_ms": ms(tqr), "mean_and_var_vjp_ms": tv * 1e3,
                            "mean_and_var_vjp_runs_ms": ms(tvr), "vjp_over_mean_and_var": tv / tq}
                    res["queries"].append(qrow)
                    print(json.dumps(qrow), flush=True)
                    save()
        del f, fx, x, y, g, gx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
