"""Times toeplitz_posterior_missing and its mean_and_var beside toeplitz_posterior on the complete data (DESIGN.md 4.22 "Posterior
handle for gappy grids") -> profiles/toeplitz_missing_posterior_bench.json.  32 SE latents over p = 64 outputs, data on the device,
n = 8192 (one workgroup per latent) and 65536 (the blocked schedule), ns = 64 and 1024 queries spread over the grid and the gap.  Gaps
as tools/toeplitz_missing_bench.py: one outage of k = 64, 1024, 4096 points without data, and k = 1024 scattered points that each miss
one output.  Per row: medians of 3 after a warm-up, the split of the last query's device time by events (predict, storing GEMM,
inverse rows, solve) and the inverse-rows kernel's rate against the FP64 matrix peak, beside the inverse-block kernel's rate of the
create on the same gap.  At n = 8192, k = 1024 also the dense posterior + mean_and_var on the same data.
Usage: python tools/toeplitz_missing_posterior_bench.py [--out profiles/toeplitz_missing_posterior_bench.json] [--n 8192 65536]"""
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
from toeplitz_missing_bench import CHUNK, PEAK, TILE, block_flops  # noqa: E402


def rows_flops(S, n, ns):
    """what toep_inverse_rows_kernel issues per latent: per point tile and query tile, two panels per chunk up to the tile's largest index"""
    k, tot = len(S), 0
    for ti in range((k + TILE - 1) // TILE):
        chunks = S[min(ti * TILE + TILE, k) - 1] // CHUNK + 1
        tot += ((ns + TILE - 1) // TILE) * chunks * 2 * CHUNK * TILE * TILE * 2
    return tot


def last_ms(fn, count):
    ms = [C.c_double() for _ in range(count)]
    fn(*[C.byref(v) for v in ms])
    return [v.value for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "toeplitz_missing_posterior_bench.json"))
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
        xq = {ns: torch.tensor(np.sort(rng.uniform(0.0, 0.01 * n, ns)), device="cuda") for ns in (64, 1024)}
        complete = {"create_ms": timed(lambda: lmm.toeplitz_posterior(fx, y, blocked).close())[0]}
        with lmm.toeplitz_posterior(fx, y, blocked) as full:
            for ns, q in xq.items():
                complete[f"mean_and_var_ns{ns}_ms"], _ = timed(lambda: full.mean_and_var(q))
        for gaps, k in (("outage", 64), ("outage", 1024), ("outage", 4096), ("scattered", 1024)):
            Y = y.clone().reshape(P, n)
            if gaps == "outage":
                S = n // 2 + np.arange(k)
                Y[:, torch.tensor(S, device="cuda")] = float("nan")
            else:
                S = np.sort(rng.choice(n, k, replace=False))
                Y[0, torch.tensor(S, device="cuda")] = float("nan")
            yg = Y.reshape(-1)
            rec = {"n": n, "m": M, "p": P, "blocked": blocked, "gaps": gaps, "k": k, "complete": complete}
            rec["create_ms"], _ = timed(lambda: lmm.toeplitz_posterior_missing(fx, yg, blocked).close())
            block_ms = last_ms(lib.lmm_toeplitz_missing_last_ms, 3)[1]
            rec["inverse_block_ms"], rec["inverse_block_tflops"] = block_ms, M * block_flops(S) / (1e9 * block_ms)
            with lmm.toeplitz_posterior_missing(fx, yg, blocked) as post:
                for ns, q in xq.items():
                    rec[f"mean_and_var_ns{ns}_ms"], _ = timed(lambda: post.mean_and_var(q))
                    parts = last_ms(lib.lmm_toeplitz_missing_post_last_ms, 4)
                    rec[f"split_ns{ns}_ms"] = dict(zip(("predict", "storing_gemm", "inverse_rows", "solve"), parts))
                    rec[f"inverse_rows_ns{ns}_tflops"] = M * rows_flops(S, n, ns) / (1e9 * parts[2])
                    rec[f"inverse_rows_ns{ns}_of_peak"] = rec[f"inverse_rows_ns{ns}_tflops"] / PEAK
            if n <= 8192 and k == 1024:
                try:
                    rec["dense_create_ms"], dense = timed(lambda: lmm.posterior(fx, yg))
                    for ns, q in xq.items():
                        rec[f"dense_mean_and_var_ns{ns}_ms"], _ = timed(lambda: lmm.mean_and_var(dense(lmm.MOInputIsotopicByOutputs(q, P), S2)))
                    del dense
                except Exception as e:      # the dense path's own refusals
                    rec["dense"] = f"not measured: {type(e).__name__}: {e}"
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/toeplitz_missing_posterior_bench.py", "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
