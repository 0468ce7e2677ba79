"""The back substitution's outputs of two builds, bit for bit: python tools/solve_chain_bitwise.py LIB_A LIB_B [--out FILE]

Every single-stream back-substitution case of tests/test_gpu_solve_chain.py (sizes x batch sizes, and the 32 right-hand sides on one
16384-column factor) runs once per library in a child process (LMM_HIP_LIB chooses the build; both need lmm_dev_backsolve; LMM_DETERMINISTIC=1, because a
factorisation with split-K atomics is not the same twice and the comparison needs the same factor on both sides), which
prints the SHA-256 of the factor, of the inverse blocks and of alpha; this process compares the digests and writes one line per case.
Needs the GPU."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import ctypes as C
    import numpy as np
    import torch
    import lmm_amd as lmm
    import test_gpu_solve_chain as T
    lmm.init(0)
    lib = lmm.load()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {}
    for n in T.BACKSOLVE_N:
        for nb in (1, 3, 32):
            A, W, _, _ = T.batch_of(lmm, n, nb)
            Z = np.random.default_rng([n, nb, 7]).standard_normal((nb, n))
            got = T.run_backsolve(lmm, A, W, A.shape[1] // 64, A.shape[2], Z, n)
            out[f"n={n} nb={nb}"] = [sha(A.cpu().numpy()), sha(W.cpu().numpy()), sha(got)]
    n, nb = 16384, 32
    A = torch.zeros(n, n + 2, dtype=torch.float64, device="cuda")
    G = torch.randn(n, n + 8, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
    A[:, :n] = torch.triu(G @ G.T / n + 0.5 * torch.eye(n, dtype=torch.float64, device="cuda"))
    del G
    W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), n, n, n + 2, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0
    Z = np.random.default_rng([n, nb, 7]).standard_normal((nb, n))
    got = T.run_backsolve(lmm, A, W, n // 64, n + 2, Z, n, shared=True)
    out[f"n={n} nb={nb} shared factor"] = [sha(A.cpu().numpy()), sha(W.cpu().numpy()), sha(got)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runs = []
    for lib in a.libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, LMM_HIP_LIB=os.path.abspath(lib), LMM_DETERMINISTIC="1"),
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{lib}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines, differ = [f"A = {a.libs[0]}", f"B = {a.libs[1]}", "case: factor | inverse blocks | alpha  (A against B, bitwise)"], 0
    for case, da in runs[0].items():
        same = ["equal" if x == y else "DIFFER" for x, y in zip(da, runs[1][case])]
        differ += same.count("DIFFER")
        lines.append(f"{case}: {' | '.join(same)}  alpha sha256 {da[2][:16]}")
    lines.append(f"{len(runs[0])} cases, {differ} digests differ")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main()
