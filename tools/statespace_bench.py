"""Timings of the state-space path -> profiles/statespace_bench.json.

32 Matern52 latents, p = 64, d = 1 (the kernel and mixing shape of BASELINE configs[2]).
  * n = 16384: statespace_logpdf against logpdf (the Cholesky path) of the same build, and their relative difference;
  * n = 262144 and 1048576: statespace_logpdf against elbo at M = 128 and 512 inducing points;
  * the filter building block on one latent with chunk = n (one sequential thread) against the library's plan: what the scan buys.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M_LAT, P_OUT, S2 = 32, 64, 0.1


def timed(fn, runs):
    """(median seconds, all run times, last value) of fn() after one warm-up call."""
    fn()
    ts, val = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        val = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts, val


def make_problem(lmm, n, seed=0):
    """Device-resident data: x sorted with spacings around 0.05 lengthscales, y standard normal (the timings do not depend on y)."""
    import torch
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((P_OUT, M_LAT)))[0]
    S = rng.uniform(0.5, 2.0, M_LAT)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.cumsum(0.05 * (0.5 + torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)), 0)
    y = torch.randn(n * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
    fs = lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel(0.5 + 0.03 * l, 0.8 + 0.02 * l)) for l in range(M_LAT)])
    f = lmm.ILMM(fs, lmm.Orthogonal(U, S))
    torch.cuda.synchronize()
    return f, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[262144, 1048576])
    ap.add_argument("--exact-n", type=int, default=16384)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    from lmm_amd import _lib as L
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "kernel": "matern52", "sigma2": S2, "runs": a.runs, "device": torch.cuda.get_device_name(0)}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    # 1. against the Cholesky path
    f, x, y = make_problem(lmm, a.exact_n)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    ts, tsr, vs = timed(lambda: lmm.statespace_logpdf(fx, y), a.runs)
    tc, tcr, vc = timed(lambda: lmm.logpdf(fx, y), a.runs)
    res["exact"] = {"n": a.exact_n, "statespace_logpdf_ms": ts * 1e3, "logpdf_ms": tc * 1e3, "statespace_runs_ms": [t * 1e3 for t in tsr],
                    "logpdf_runs_ms": [t * 1e3 for t in tcr], "statespace_value": vs, "logpdf_value": vc,
                    "relative_difference": abs(vs - vc) / abs(vc)}
    print(json.dumps(res["exact"]), flush=True)
    save()

    # 2. against the inducing-point bound, and the filter block sequential against planned
    res["linear"] = []
    for n in a.sizes:
        f, x, y = make_problem(lmm, n)
        fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
        row = {"n": n}
        t, tr, v = timed(lambda: lmm.statespace_logpdf(fx, y), a.runs)
        row.update(statespace_logpdf_ms=t * 1e3, statespace_runs_ms=[q * 1e3 for q in tr], statespace_value=v)
        for M in (128, 512):
            z = torch.linspace(float(x[0]), float(x[-1]), M, dtype=torch.float64, device="cuda")
            vfe = lmm.VFE(z)
            try:
                t, tr, v = timed(lambda: lmm.elbo(vfe, fx, y), a.runs)
            except (RuntimeError, ValueError, NotImplementedError) as e:      # recorded, not hidden: the other figures still stand
                row[f"elbo_M{M}_error"] = str(e)
                continue
            row[f"elbo_M{M}_ms"] = t * 1e3
            row[f"elbo_M{M}_runs_ms"] = [q * 1e3 for q in tr]
            row[f"elbo_M{M}_value"] = v
        del y
        # one latent: w constant, r standard normal
        w = torch.full((n,), S2, dtype=torch.float64, device="cuda")
        r = torch.randn(n, dtype=torch.float64, device="cuda")
        fm, fv, lml = torch.empty_like(r), torch.empty_like(r), torch.empty(1, dtype=torch.float64, device="cuda")
        gp = L.gps_array([dict(lmm.Matern52Kernel(1.0, 1.0).desc(), mean=0.0)])
        lib = lmm.load()
        torch.cuda.synchronize()

        def block(chunk):
            L.check(lib.lmm_dev_statespace_filter(x.data_ptr(), n, gp, w.data_ptr(), r.data_ptr(), chunk, fm.data_ptr(), fv.data_ptr(),
                                                  lml.data_ptr()))
            return float(lml.cpu()[0])

        tp, tpr, vp = timed(lambda: block(0), a.runs)
        tq, tqr, vq = timed(lambda: block(n), a.runs)
        row.update(filter_block_planned_ms=tp * 1e3, filter_block_sequential_ms=tq * 1e3, filter_block_planned_runs_ms=[q * 1e3 for q in tpr],
                   filter_block_sequential_runs_ms=[q * 1e3 for q in tqr], filter_block_speedup=tq / tp,
                   filter_block_relative_difference=abs(vp - vq) / abs(vq))
        res["linear"].append(row)
        print(json.dumps(row), flush=True)
        save()
        del f, fx, x, w, r, fm, fv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
