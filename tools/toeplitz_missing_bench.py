"""Times toeplitz_logpdf_missing beside toeplitz_logpdf on the complete data (DESIGN.md 4.22 "Missing observations")
-> profiles/toeplitz_missing_bench.json.  32 SE latents over p = 64 outputs, data on the device, n = 8192 (one workgroup per latent)
and 65536 (the blocked schedule).  Gaps: one outage of k = 64, 1024, 4096 points without data, and k = 1024 scattered points that
each miss one output.  Per row: medians of 3 after a warm-up, the split of the last call's device time by events (recursion, inverse
block, finish + Cholesky) and the inverse block kernel's rate against the FP64 matrix peak.
Usage: python tools/toeplitz_missing_bench.py [--out profiles/toeplitz_missing_bench.json] [--n 8192 65536]"""
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

PEAK, TILE, CHUNK = 78.6, 128, 16      # TFLOP/s; the kernel's tile and K chunk


def block_flops(S):
    """what toep_inverse_block_kernel issues per latent: per tile on or below the diagonal, two panels per chunk up to the column block's largest index"""
    k, nt, tot = len(S), (len(S) + TILE - 1) // TILE, 0
    for tj in range(nt):
        chunks = S[min(tj * TILE + TILE, k) - 1] // CHUNK + 1
        tot += (nt - tj) * chunks * 2 * CHUNK * TILE * TILE * 2
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "toeplitz_missing_bench.json"))
    ap.add_argument("--n", type=int, nargs="+", default=[8192, 65536])
    a = ap.parse_args()
    lmm.init(0)
    lib, rows = lmm.load(), []
    for n in a.n:
        blocked = n > lib.lmm_toeplitz_max_n()
        rng = np.random.default_rng(n)
        x = torch.linspace(0.0, 0.01 * (n - 1), n, dtype=torch.float64, device="cuda")
        y = torch.tensor(rng.standard_normal(n * P), device="cuda")
        fx = model("se", rng)(lmm.MOInputIsotopicByOutputs(x, P), S2)
        complete_ms, _ = timed(lambda: lmm.toeplitz_logpdf(fx, y, blocked=blocked))
        for gaps, k in (("outage", 64), ("outage", 1024), ("outage", 4096), ("scattered", 1024)):
            Y = y.clone().reshape(P, n)
            if gaps == "outage":
                S = n // 2 + np.arange(k)
                Y[:, torch.tensor(S, device="cuda")] = float("nan")
            else:
                S = np.sort(rng.choice(n, k, replace=False))
                Y[0, torch.tensor(S, device="cuda")] = float("nan")
            yg = Y.reshape(-1)
            rec = {"n": n, "m": M, "p": P, "blocked": blocked, "gaps": gaps, "k": k, "toeplitz_logpdf_complete_ms": complete_ms}
            rec["toeplitz_logpdf_missing_ms"], _ = timed(lambda: lmm.toeplitz_logpdf_missing(fx, yg, blocked))
            ms = [C.c_double() for _ in range(3)]
            lib.lmm_toeplitz_missing_last_ms(*[C.byref(v) for v in ms])
            rec["recursion_ms"], rec["inverse_block_ms"], rec["cholesky_ms"] = (v.value for v in ms)
            rec["inverse_block_tflops"] = M * block_flops(S) / (1e9 * rec["inverse_block_ms"])
            rec["inverse_block_of_peak"] = rec["inverse_block_tflops"] / PEAK
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/toeplitz_missing_bench.py", "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
