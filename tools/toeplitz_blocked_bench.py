"""Times the blocked schedule of the Toeplitz path (DESIGN.md 4.22 "Blocked schedule") -> profiles/toeplitz_blocked_bench.json.
The models of tools/toeplitz_bench.py: 32 latents over p = 64 outputs, data on the device, SE latents and Matern52 + SE * Periodic
sums; medians of 3 after a warm-up.
  1. n = 2048, 8192: blocked=True against blocked=False in the same run, value and value + gradient, and the agreement of the values.
  2. n = 16384, 65536, 131072: value, value + gradient and posterior create, blocked; at 16384 the dense logpdf beside them.  The
     recursion's own time is the call lmm_dev_toeplitz_factor_blocked cannot give for 32 latents, so the value call (first columns,
     projection and recursion) stands for it: `fp64_share` and `hbm_share` are that whole call's useful operations (7 n^2 per
     latent: 8 per row and step on the (a, b) side with r, 6 on the (p, q) side) and the bytes its launches move (per launch and
     latent 4 doubles in and out per row on either side, 2 more for r on the (a, b) side, and the halo's loads) over the peaks
     below: end-to-end figures, lower bounds of the kernel's shares.
  3. n = 16384, 65536, 131072 with Matern52 latents: the relative difference of the value and of every gradient key between
     blocked=True and the state-space path: the accuracy record where no dense reference exists.
Usage: python tools/toeplitz_blocked_bench.py [--out profiles/toeplitz_blocked_bench.json] [--sizes 16384,65536,131072]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lmm_amd as lmm  # noqa: E402
from toeplitz_bench import M, P, S2, model, timed  # noqa: E402

PEAK_FP64_VECTOR, PEAK_HBM = 78.6e12, 8.0e12      # FLOP/s and bytes/s of the MI355X
J, V = 64, 448                                    # steps of a launch, rows a wave stores of the 512 it loads


def data(n):
    rng = np.random.default_rng(n)
    x = torch.linspace(0.0, 0.01 * (n - 1), n, dtype=torch.float64, device="cuda")
    return rng, x, torch.tensor(rng.standard_normal(n * P), device="cuda")


def flat(g):
    """every gradient key as (name, array)"""
    out = [(k, np.atleast_1d(np.asarray(g[k].cpu() if torch.is_tensor(g[k]) else g[k], dtype=float))) for k in ("value", "y", "sigma2", "S", "U")]
    keys = sorted(k for k in g["gps"][0] if np.isscalar(g["gps"][0][k]))
    return out + [("gps." + k, np.array([q[k] for q in g["gps"]])) for k in keys]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "toeplitz_blocked_bench.json"))
    ap.add_argument("--sizes", default="16384,65536,131072")
    a = ap.parse_args()
    big = [int(s) for s in a.sizes.split(",")]
    lmm.init(0)
    rows = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/toeplitz_blocked_bench.py", "device": torch.cuda.get_device_name(0), "steps_per_launch": J,
                       "steps_per_launch_128": "not measured", "rows": rows}, f, indent=1)

    for kind in ("se", "matern52+se*periodic"):
        for n in (2048, 8192):
            rng, x, y = data(n)
            fx = model(kind, rng)(lmm.MOInputIsotopicByOutputs(x, P), S2)
            rec = {"part": 1, "model": kind, "n": n, "m": M, "p": P}
            for b, tag in ((False, "unblocked"), (True, "blocked")):
                rec[tag + "_logpdf_ms"], v = timed(lambda: lmm.toeplitz_logpdf(fx, y, blocked=b))
                rec[tag + "_logpdf_and_gradient_ms"], _ = timed(lambda: lmm.toeplitz_logpdf_and_gradient(fx, y, blocked=b))
                rec[tag + "_value"] = v
            rec["value_rel_diff"] = abs(rec["blocked_value"] - rec["unblocked_value"]) / abs(rec["unblocked_value"])
            emit(rec)
    for kind in ("se", "matern52+se*periodic"):
        for n in big:
            rng, x, y = data(n)
            fx = model(kind, rng)(lmm.MOInputIsotopicByOutputs(x, P), S2)
            rec = {"part": 2, "model": kind, "n": n, "m": M, "p": P}
            rec["blocked_logpdf_ms"], v = timed(lambda: lmm.toeplitz_logpdf(fx, y, blocked=True))
            rec["blocked_logpdf_and_gradient_ms"], _ = timed(lambda: lmm.toeplitz_logpdf_and_gradient(fx, y, blocked=True))
            rec["blocked_posterior_create_ms"], _ = timed(lambda: lmm.toeplitz_posterior(fx, y, blocked=True).close())
            launches = (n + J - 1) // J
            flops = 7.0 * n * n * M
            nbytes = 8.0 * M * launches * (n + J) * (4 + 1 + 2 * J / V)      # r's two doubles on half the rows on average
            t = 1e-3 * rec["blocked_logpdf_ms"]
            rec.update(useful_flops=flops, launch_bytes=nbytes, fp64_share=flops / t / PEAK_FP64_VECTOR, hbm_share=nbytes / t / PEAK_HBM)
            if n <= 16384:
                rec["logpdf_ms"], vd = timed(lambda: lmm.logpdf(fx, y))
                rec["value_rel_diff_to_dense"] = abs(v - vd) / abs(vd)
            emit(rec)
    for n in big:
        rng, x, y = data(n)
        U = np.linalg.qr(rng.standard_normal((P, M)))[0]
        f = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel(1.0, 0.5 + 0.05 * l)) for l in range(M)]), lmm.Orthogonal(U, np.linspace(1.0, 2.0, M)))
        fx = f(lmm.MOInputIsotopicByOutputs(x, P), S2)
        got, ref = lmm.toeplitz_logpdf_and_gradient(fx, y, blocked=True), lmm.statespace_logpdf_and_gradient(fx, y)
        rec = {"part": 3, "model": "matern52", "n": n, "m": M, "p": P,
               "value_call_rel_diff": abs(lmm.toeplitz_logpdf(fx, y, blocked=True) - lmm.statespace_logpdf(fx, y)) / abs(ref["value"])}
        for (k, gv), (_, rv) in zip(flat(got), flat(ref)):
            rec["rel_diff_" + k] = float(np.abs(gv - rv).max() / np.abs(rv).max())
        emit(rec)


if __name__ == "__main__":
    main()
