"""Timings of the joint predictive of the Toeplitz posterior handle (DESIGN.md 4.22 "Joint predictive")
-> profiles/toeplitz_joint_bench.json.

32 SE latents, p = 64, an evenly spaced grid, data and queries on the device, as tools/toeplitz_posterior_bench.py sets them up;
n = 8192 / 65536 (the blocked schedule from 8193 on), ns = 256 / 1024 / 4096 uniform queries over the range of x and a little beyond:
  * post.predictive_logpdf(xs, ys) and one post.rand(rng, xs=xs) sample (device normals);
  * the split of predictive_logpdf between the storing GEMM, the Gram kernel and the factorisation (the finish kernel and the batched
    Cholesky), by the events the library records on the call's stream (lmm_toeplitz_joint_last_ms);
  * at n = 8192, in the same run, the dense route: logpdf(posterior(fx, y)(xs, sigma2), ys).
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  Every n is a child process of its own with its own time limit; after a step
that fails or runs out of time nothing more is started.  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]
from toeplitz_posterior_bench import M, P_OUT, S2, timed      # noqa: E402

NS = (256, 1024, 4096)


def split(lmm, fn, runs):
    """medians over `runs` calls of fn of the library's event times of its three stages, in ms"""
    import numpy as np
    ms = []
    for _ in range(runs):
        fn()
        t = [C.c_double() for _ in range(3)]
        lmm.load().lmm_toeplitz_joint_last_ms(*map(C.byref, t))
        ms.append([v.value for v in t])
    return dict(zip(("store_gemm_ms", "gram_ms", "factor_ms"), np.median(ms, axis=0).tolist()))


def step(n, runs):
    import numpy as np
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    rng = np.random.default_rng(n)
    U = np.linalg.qr(rng.standard_normal((P_OUT, M)))[0]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.SEKernel(1.0, l)) for l in 0.5 + rng.random(M)]), lmm.Orthogonal(U, 0.5 + rng.random(M)))
    x = torch.tensor(0.01 * np.arange(n), device="cuda")
    y = torch.tensor(rng.standard_normal(n * P_OUT), device="cuda")
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    row = {"n": n, "device": torch.cuda.get_device_name(0)}
    post = lmm.toeplitz_posterior(fx, y, blocked=n > 8192)
    dense = lmm.posterior(fx, y) if n <= 8192 else None
    gen = torch.Generator(device="cuda").manual_seed(n)
    for ns in NS:
        xs = -0.5 + (0.01 * n + 1.0) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
        ys = torch.randn(ns * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
        r = {"predictive_logpdf_ms": timed(lambda: post.predictive_logpdf(xs, ys), runs) * 1e3,
             "rand_one_sample_ms": timed(lambda: post.rand(lmm.DeviceNormals(1), jitter=1e-6, xs=xs), runs) * 1e3}
        r.update(split(lmm, lambda: post.predictive_logpdf(xs, ys), runs))
        if dense is not None:
            fxs = dense(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2)
            r["dense_logpdf_ms"] = timed(lambda: lmm.logpdf(fxs, ys), runs) * 1e3
            r["logpdf_difference_relative"] = abs(post.predictive_logpdf(xs, ys) - lmm.logpdf(fxs, ys)) / abs(lmm.logpdf(fxs, ys))
        row[f"ns{ns}"] = r
    post.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toeplitz_joint_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--step", type=int, help="(internal) run the step of this n in this process and print its row")
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    if a.step:
        print("ROW " + json.dumps(step(a.step, a.runs)), flush=True)
        return 0
    res = {"latents": M, "p": P_OUT, "sigma2": S2, "runs": a.runs, "rows": []}
    for n in a.sizes:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--runs", str(a.runs)], capture_output=True,
                                  text=True, timeout=a.step_timeout)
            rows = [ln[4:] for ln in done.stdout.splitlines() if ln.startswith("ROW ")]
            if done.returncode != 0 or not rows:
                res["stopped"] = f"step n={n} failed (exit {done.returncode}); nothing more was started: {done.stderr[-2000:]}"
        except subprocess.TimeoutExpired:
            res["stopped"] = f"step n={n} ran out of its {a.step_timeout} s; nothing more was started"
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
