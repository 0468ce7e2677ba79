"""Driver of the crossover table of the emulation's shape rule: logpdf of nb Matern52 latents at n points, one
lock-step batch on one stream, for each nb given, twice each (the second evaluation is the warm one), with the K >= 2048 updates
either all emulated or all on the f64 kernel.  Run it under `rocprofv3 --kernel-trace -f csv` and read the trace with
tools/emul_level_times.py (emulated: the per-update lines; f64: --f64 NR NC with NR = n + 64, NC = n).

    python tools/emul_crossover.py {emul|f64} N NB [NB ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lmm_amd  # noqa: E402


def main(mode, n, nbs):
    lmm_amd.init(0)
    lib = lmm_amd.load()
    assert lib.lmm_dev_set_f64_emul(1 if mode == "emul" else 0, 2048, 16) == 0
    rng = np.random.default_rng(n)
    x = torch.from_numpy(np.sort(rng.uniform(0.0, 0.01 * n, n))).cuda()
    for m in nbs:
        y = torch.from_numpy(rng.standard_normal(n * m)).cuda()
        fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel()) for _ in range(m)])
        fx = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(np.eye(m), 0.5 + np.arange(m) / m))(lmm_amd.MOInputIsotopicByOutputs(x, m), 0.1)
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = float(lmm_amd.logpdf(fx, y))
            print(f"{mode} n={n} nb={m} rep={rep}: {1e3 * (time.perf_counter() - t0):.2f} ms, logpdf {v:.6e}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), [int(a) for a in sys.argv[3:]])
