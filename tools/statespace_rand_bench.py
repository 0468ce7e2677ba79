"""Timings of state-space sampling (DESIGN.md 4.18 "Sampling") -> profiles/statespace_rand_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), normals from DeviceNormals (generated on the device, so
the figures include their generation and no host transfer), n = 16384 / 262144 / 1048576:
  * statespace_rand(rng, fx): one prior sample;
  * statespace_rand(rng, fx, y) and statespace_rand(rng, fx, y, N=8): one and eight posterior samples at the training inputs;
  * statespace_mean_and_var(fx, y) at the same n: the filter and smoother a posterior sample runs once per sample;
  * at n = 16384 only, rand(rng, fx) of the same build: the exact prior sample through one n x n factorisation per latent.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  A figure no run produced is written as "not measured".  No threshold is
asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from statespace_bench import M_LAT, P_OUT, S2, make_problem, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_rand_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--exact-n", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=8)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "kernel": "matern52", "sigma2": S2, "runs": a.runs, "samples": a.samples,
           "normals": "DeviceNormals", "device": torch.cuda.get_device_name(0), "sizes": []}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for n in a.sizes:
        f, x, y = make_problem(lmm, n)
        fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
        rng = lmm.DeviceNormals(1)
        row = {"n": n, "rand_ms": "not measured"}

        def sync(fn):
            out = fn()
            torch.cuda.synchronize()
            return None if out is None else bool(torch.isfinite(out if torch.is_tensor(out) else out[0]).all())

        for name, fn in (("prior", lambda: lmm.statespace_rand(rng, fx)), ("posterior", lambda: lmm.statespace_rand(rng, fx, y)),
                         (f"posterior_N{a.samples}", lambda: lmm.statespace_rand(rng, fx, y, N=a.samples)),
                         ("mean_and_var", lambda: lmm.statespace_mean_and_var(fx, y))):
            t, tr, ok = timed(lambda: sync(fn), a.runs)
            row[f"{name}_ms"] = t * 1e3
            row[f"{name}_runs_ms"] = [q * 1e3 for q in tr]
            row[f"{name}_finite"] = ok
        row["posterior_over_mean_and_var"] = row["posterior_ms"] / row["mean_and_var_ms"]
        row[f"posterior_N{a.samples}_per_sample_ms"] = row[f"posterior_N{a.samples}_ms"] / a.samples
        if n == a.exact_n:
            t, tr, ok = timed(lambda: sync(lambda: lmm.rand(rng, fx)), a.runs)
            row.update(rand_ms=t * 1e3, rand_runs_ms=[q * 1e3 for q in tr], rand_finite=ok, rand_over_prior=t * 1e3 / row["prior_ms"])
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        save()
        del f, fx, x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
