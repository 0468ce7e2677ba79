"""Timings of ToeplitzPosterior.mean_and_var_vjp (DESIGN.md 4.22 "Gradients with respect to the queries") -> profiles/toeplitz_vjp_bench.json.

32 latents, p = 64, an evenly spaced grid, data, queries and cotangents on the device, for SE latents and for Matern52 + SE x Periodic
latents, n = 2048 / 8192 and one row at n = 65536 (a blocked handle; no dense route exists there), ns = 64 / 1024 / 8192 uniform queries
over the range of x and a little beyond (ns = 64 / 1024 at n = 65536).  Per (latents, n, ns), in the same run:
  * post.mean_and_var_vjp(xs, dmean, dvar), the same with dvar=None (no GEMM), and post.mean_and_var(xs) / post.mean(xs); the ratio
    vjp_gemm_over_var_gemm compares (vjp - vjp without dvar) with (mean_and_var - mean): toep_predict_grad_kernel against
    toep_predict_kernel, 4 n (n + 1) ns against 2 n (n + 1) ns flops per latent; the rate is taken against the 78.6 TFLOP/s FP64 peak;
  * at n <= 8192 the dense route: mean_and_var_vjp of posterior(fx, y) at the same queries and cotangents, and the largest difference
    of the two "x" relative to the largest entry.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  Every (latents, n) is a child process of its own with its own time limit; after a
step that fails or runs out of time nothing more is started.  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.toeplitz_posterior_bench import M, P_OUT, PEAK, S2, timed      # noqa: E402

DENSE_MAX_N = 8192


def step(kind, n, runs):
    import numpy as np
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    rng = np.random.default_rng(n)
    ls = 0.5 + rng.random(M)
    ks = [lmm.SEKernel(1.0, l) if kind == "se" else lmm.KernelSum(lmm.Matern52Kernel(1.0, l), lmm.LocallyPeriodicKernel(0.8, 1.0, 1.2, 4.0 * l))
          for l in ls]
    U = np.linalg.qr(rng.standard_normal((P_OUT, M)))[0]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, 0.5 + rng.random(M)))
    x = torch.tensor(0.01 * np.arange(n), device="cuda")
    y = torch.tensor(rng.standard_normal(n * P_OUT), device="cuda")
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    row = {"latents": kind, "n": n, "device": torch.cuda.get_device_name(0)}
    post = lmm.toeplitz_posterior(fx, y, blocked=n > DENSE_MAX_N)
    dense = lmm.posterior(fx, y) if n <= DENSE_MAX_N else None
    gen = torch.Generator(device="cuda").manual_seed(n)
    for ns in (64, 1024, 8192) if n <= DENSE_MAX_N else (64, 1024):
        xs = -0.5 + (0.01 * n + 1.0) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
        dm, dv = (torch.randn(ns * P_OUT, dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
        tv, tvm = timed(lambda: post.mean_and_var_vjp(xs, dm, dv), runs), timed(lambda: post.mean_and_var_vjp(xs, dm), runs)
        tq, tm = timed(lambda: post.mean_and_var(xs), runs), timed(lambda: post.mean(xs), runs)
        r = {"vjp_ms": tv * 1e3, "vjp_dvar_none_ms": tvm * 1e3, "mean_and_var_ms": tq * 1e3, "mean_ms": tm * 1e3, "vjp_over_mean_and_var": tv / tq,
             "vjp_gemm_over_var_gemm": (tv - tvm) / max(tq - tm, 1e-9),
             "vjp_gemm_fraction_of_fp64_peak": 4.0 * n * (n + 1) * ns * M / max(tv - tvm, 1e-9) / PEAK}
        if dense is not None:
            fxs = dense(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2)
            r["dense_vjp_ms"] = timed(lambda: lmm.mean_and_var_vjp(fxs, dm, dv), runs) * 1e3
            r["dense_vjp_dvar_none_ms"] = timed(lambda: lmm.mean_and_var_vjp(fxs, dm), runs) * 1e3
            r["dense_over_handle"] = r["dense_vjp_ms"] / r["vjp_ms"]
            gx, dx = post.mean_and_var_vjp(xs, dm, dv)["x"], lmm.mean_and_var_vjp(fxs, dm, dv)["x"].reshape(-1)
            r["x_difference_relative_to_largest"] = float((gx - dx).abs().max() / dx.abs().max())
        row[f"ns{ns}"] = r
    post.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toeplitz_vjp_bench.json"))
    ap.add_argument("--cases", nargs="*", default=["se:2048", "se:8192", "sum:2048", "sum:8192", "se:65536"], help="latents:n")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=["se", "sum"], help="(internal) run one step in this process and print its row")
    ap.add_argument("--n", type=int)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    if a.step:
        print("ROW " + json.dumps(step(a.step, a.n, a.runs)), flush=True)
        return 0
    res = {"latents": M, "p": P_OUT, "sigma2": S2, "runs": a.runs, "fp64_peak_tflops": PEAK / 1e12, "rows": []}
    for case in a.cases:
        kind, n = case.split(":")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--n", n, "--runs", str(a.runs)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            rows = [ln[4:] for ln in done.stdout.splitlines() if ln.startswith("ROW ")]
            if done.returncode != 0 or not rows:
                res["stopped"] = f"step {case} failed (exit {done.returncode}); nothing more was started: {done.stderr[-2000:]}"
        except subprocess.TimeoutExpired:
            res["stopped"] = f"step {case} ran out of its {a.step_timeout} s; nothing more was started"
        if "stopped" not in res:
            res["rows"].append(json.loads(rows[-1]))
            print(rows[-1], flush=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        if "stopped" in res:
            print(res["stopped"], flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
