"""Timings of the Toeplitz posterior handle (DESIGN.md 4.22 "Posterior handle") -> profiles/toeplitz_posterior_bench.json.

32 latents, p = 64, an evenly spaced grid, data and queries on the device, for SE latents and for Matern52 + SE x Periodic latents,
n = 2048 / 8192, ns = 64 / 1024 / 8192 uniform queries over the range of x and a little beyond:
  * toeplitz_posterior(fx, y): the recursion, alpha, the handle;
  * post.mean_and_var(xs) and post.mean(xs); their difference is taken as the time of toep_predict_kernel and its finish, and the
    rate counts 2 n (n + 1) ns flops per latent against the 78.6 TFLOP/s FP64 matrix peak;
  * beside them, in the same run, the dense route: posterior(fx, y) and mean_and_var of it at the same queries.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  Every (latents, n) is a child process of its own with its own time limit; after a
step that fails or runs out of time nothing more is started.  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M, P_OUT, S2, PEAK = 32, 64, 0.1, 78.6e12
NS = (64, 1024, 8192)


def timed(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


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

    def create():
        lmm.toeplitz_posterior(fx, y).close()

    def dense_create():
        lmm.posterior(fx, y)

    row["create_ms"], row["dense_posterior_ms"] = timed(create, runs) * 1e3, timed(dense_create, runs) * 1e3
    post, dense = lmm.toeplitz_posterior(fx, y), lmm.posterior(fx, y)
    gen = torch.Generator(device="cuda").manual_seed(n)
    for ns in NS:
        xs = -0.5 + (0.01 * n + 1.0) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
        fxs = dense(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2)
        tq, tm, td = timed(lambda: post.mean_and_var(xs), runs), timed(lambda: post.mean(xs), runs), timed(lambda: lmm.mean_and_var(fxs), runs)
        gm, gv, dm, dv = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (*post.mean_and_var(xs), *lmm.mean_and_var(fxs)))
        row[f"ns{ns}"] = {"mean_and_var_ms": tq * 1e3, "mean_ms": tm * 1e3, "dense_mean_and_var_ms": td * 1e3, "dense_over_handle": td / tq,
                          "variance_fraction_of_fp64_peak": 2.0 * n * (n + 1) * ns * M / max(tq - tm, 1e-9) / PEAK,
                          "var_difference_relative_to_largest": float(np.abs(gv - dv).max() / dv.max()),
                          "mean_difference_relative": float(np.abs(gm - dm).max() / np.abs(dm).max())}
    post.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toeplitz_posterior_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 8192])
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
    for kind in ("se", "sum"):
        for n in a.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--n", str(n), "--runs", str(a.runs)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
                rows = [ln[4:] for ln in done.stdout.splitlines() if ln.startswith("ROW ")]
                if done.returncode != 0 or not rows:
                    res["stopped"] = f"step {kind} n={n} failed (exit {done.returncode}); nothing more was started: {done.stderr[-2000:]}"
            except subprocess.TimeoutExpired:
                res["stopped"] = f"step {kind} n={n} ran out of its {a.step_timeout} s; nothing more was started"
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
