"""Times sampling on the Toeplitz path (DESIGN.md 4.22 "Sampling") -> profiles/toeplitz_rand_bench.json.
The models of tools/toeplitz_bench.py: 32 latents over p = 64 outputs, SE latents and Matern52 + SE * Periodic sums, x and y on the
device, normals from DeviceNormals (their generation is inside the timed call); medians of 3 after a warm-up.  Per n: a prior sample
and a posterior sample from a handle (post.rand) with N = 1 and N = 8, a posterior sample with horizon = n / 8 (where n + horizon is
within the cap), toeplitz_posterior create beside them, and the dense rand where it runs (n <= 16384).  `recursion_ms` and `rest_ms`
split the library call of the last timed repeat by device events (lmm_toeplitz_rand_last_ms): toep_schur_sample_kernel's launches, and
everything else (first columns, the per-sample Toeplitz products of the conditioning, mixing, copies).  The prior's jitter is JITTER
on every latent: at h = 0.01 the SE Grams are far too ill-conditioned for the default.
Usage: python tools/toeplitz_rand_bench.py [--out profiles/toeplitz_rand_bench.json] [--sizes 8192,16384,65536,131072]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lmm_amd as lmm  # noqa: E402
from toeplitz_bench import M, P, S2, model, timed  # noqa: E402

JITTER, DENSE_MAX_N = 1e-6, 16384


def split():
    a, b = C.c_double(), C.c_double()
    lmm.load().lmm_toeplitz_rand_last_ms(C.byref(a), C.byref(b))
    return {"recursion_ms": a.value, "rest_ms": b.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "toeplitz_rand_bench.json"))
    ap.add_argument("--sizes", default="8192,16384,65536,131072")
    a = ap.parse_args()
    lmm.init(0)
    cap, rows = lmm.load().lmm_toeplitz_blocked_max_n(), []
    for kind in ("se", "matern52+se*periodic"):
        for n in [int(s) for s in a.sizes.split(",")]:
            rng = np.random.default_rng(n)
            x = torch.linspace(0.0, 0.01 * (n - 1), n, dtype=torch.float64, device="cuda")
            y = torch.tensor(rng.standard_normal(n * P), device="cuda")
            fx = model(kind, rng)(lmm.MOInputIsotopicByOutputs(x, P), S2)
            rec = {"model": kind, "n": n, "m": M, "p": P, "jitter": JITTER}
            rec["posterior_create_ms"], _ = timed(lambda: lmm.toeplitz_posterior(fx, y, blocked=True).close())
            with lmm.toeplitz_posterior(fx, y, blocked=True) as post:
                for N in (1, 8):
                    rec[f"prior_N{N}_ms"], _ = timed(lambda: lmm.toeplitz_rand(lmm.DeviceNormals(1), fx, N=N, jitter=JITTER))
                    rec[f"prior_N{N}_split"] = split()
                    rec[f"posterior_N{N}_ms"], _ = timed(lambda: post.rand(lmm.DeviceNormals(2), N=N, jitter=JITTER))
                    rec[f"posterior_N{N}_split"] = split()
                if n + n // 8 <= cap:
                    rec["posterior_horizon_ms"], _ = timed(lambda: post.rand(lmm.DeviceNormals(3), horizon=n // 8, jitter=JITTER))
                    rec["posterior_horizon_split"] = split()
                else:
                    rec["posterior_horizon_ms"] = "not measured: n + n / 8 is beyond lmm_toeplitz_blocked_max_n"
            if n <= DENSE_MAX_N:
                for N in (1, 8):
                    rec[f"dense_rand_N{N}_ms"], _ = timed(lambda: lmm.rand(lmm.DeviceNormals(4), fx, N, (1e-9, 1e-12, JITTER)))
            else:
                rec["dense_rand_N1_ms"] = rec["dense_rand_N8_ms"] = "not measured: the dense rand factors an n x n matrix per latent"
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/toeplitz_rand_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
