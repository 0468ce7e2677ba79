"""Outputs of the state-space entry points under two builds of liblmm_hip.so, byte for byte, on one GPU.

    python tools/statespace_bitwise.py PARENT.so NEW.so > bitwise_vs_parent.txt

tools/bitwise_vs_parent.py's scheme for the state-space path: three child processes, one after the other and never two at once, each
under a time limit -- PARENT, PARENT again (the control) and NEW, all on the same inputs.  The tool stops at the first child that exits
non-zero.  Every output array of NEW is compared with PARENT's bytes, one line per operation; an operation the two PARENT runs disagree
on is listed as `not comparable`.  Exit status 0 when no comparable array differs.

The inputs are those of the existing tests (tests/test_gpu_statespace.py `problem` and `nan_problem`, tests/test_gpu_statespace_posterior.py
`complete_problem` with the SHO latent) at n = 1, 63, 333 and 5000 (two plans of the scan: 16 and 64 points per thread): statespace_logpdf with
and without the regulariser, statespace_mean_and_var at the training inputs and at new ones, statespace_posterior with its logpdf,
mean_and_var, mean_and_var_vjp, window and rand at the queries of the tests, statespace_logpdf_and_gradient without and with the
inputs, and statespace_rand of the prior and of the posterior."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 333, 5000)
CHILD_SECONDS = 300


def child(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes
    import torch  # noqa: F401  (first, as lmm_amd.load does: one HIP runtime per process)
    import lmm_amd as lmm
    from lmm_amd import _lib as L
    probe = ctypes.CDLL(L.LIB_PATH)             # PARENT may lack entry points that NEW adds: they are not bound, and nothing here calls them
    for name in [s for s in L.STATESPACE_ARGTYPES if not hasattr(probe, s)]:
        del L.STATESPACE_ARGTYPES[name]
    import test_gpu_statespace as GS
    import test_gpu_statespace_posterior as PP
    import test_statespace_posterior_abi as PA
    lmm.init(0)
    out = {}

    def leaves(v):
        if isinstance(v, dict):
            return [e for k in sorted(v, key=str) for e in leaves(v[k])]
        if isinstance(v, (list, tuple)):
            return [e for w in v for e in leaves(w)]
        if v is None or isinstance(v, str):
            return []
        return [np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.float64).reshape(-1)]

    def rec(name, v):
        arrs = leaves(v)
        out[name] = np.concatenate(arrs + [np.array([float(len(arrs))])])

    for n in SIZES:
        for tag, (x, U, Sv, Y, gps) in (("complete", PP.complete_problem(n, True)), ("nan", PP.nan_problem(n, True))):
            p, y = Y.shape[0], Y.reshape(-1)
            fx = PP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), GS.S2)
            Q = PA.queries(x)
            t = f"n={n} {tag}"
            rec(f"{t} logpdf", lmm.statespace_logpdf(fx, y))
            rec(f"{t} logpdf no regulariser", lmm.statespace_logpdf(fx, y, False))
            rec(f"{t} mean_and_var", lmm.statespace_mean_and_var(fx, y))
            rec(f"{t} mean_and_var xs", lmm.statespace_mean_and_var(fx, y, False, xs=Q))
            with lmm.statespace_posterior(fx, y) as post:
                rec(f"{t} posterior logpdf", post.logpdf)
                rec(f"{t} posterior mean_and_var", post.mean_and_var(Q))
                rec(f"{t} posterior mean_and_var no noise", post.mean_and_var(Q, False))
                rec(f"{t} posterior vjp", post.mean_and_var_vjp(Q, np.ones(len(Q) * p), np.linspace(-1.0, 1.0, len(Q) * p)))
                rec(f"{t} posterior window", list(post.window(Q)))
                rec(f"{t} posterior rand", post.rand(np.random.default_rng(n), Q, 3))
                rec(f"{t} posterior rand no noise", post.rand(np.random.default_rng(n), Q, None, False))
            g = lmm.statespace_logpdf_and_gradient(fx, y)
            rec(f"{t} logpdf_and_gradient", [g["value"], g["y"], g["sigma2"], g["gps"]] + ([] if tag == "nan" else [g["S"], g["U"]]))
            g = lmm.statespace_logpdf_and_gradient(fx, y, True, True)
            rec(f"{t} logpdf_and_gradient inputs", [g["value"], g["y"], g["x"]])
            rec(f"{t} rand prior", lmm.statespace_rand(np.random.default_rng(n + 1), fx, None, 2))
            rec(f"{t} rand posterior", lmm.statespace_rand(np.random.default_rng(n + 2), fx, y, 2))
            rec(f"{t} rand posterior xs", lmm.statespace_rand(np.random.default_rng(n + 3), fx, y, None, True, Q))
    np.savez(out_path, **out)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    parent, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for i, lib in enumerate([parent, parent, new]):
            path = os.path.join(tmp, f"run{i}.npz")
            env = dict(os.environ, LMM_HIP_LIB=os.path.abspath(lib))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=CHILD_SECONDS).returncode
            if rc != 0:
                print(f"child {i} ({lib}) exited with {rc}: stopping")
                return 3
            with np.load(path) as zf:
                runs.append({k: zf[k] for k in zf.files})
    a, c, b = runs
    print(f"# {parent} and {new}, each in its own process on one GPU, same inputs; every output compared byte for byte.")
    print(f"# n = {SIZES}, the problems of tests/test_gpu_statespace_posterior.py with the SHO latent; control: {parent} twice.")
    differ = unsure = 0
    for k in a:
        if k not in b or k not in c or a[k].shape != b[k].shape:
            print(f"MISSING OR RESHAPED  {k}")
            differ += 1
            continue
        nd = int(np.sum(a[k].view(np.uint64) != b[k].view(np.uint64)))
        control = a[k].tobytes() == c[k].tobytes()
        word = "not comparable" if not control else "identical" if nd == 0 else "DIFFERENT"
        differ += word == "DIFFERENT"
        unsure += not control
        print(f"{word:<14} {int(a[k][-1]):>3} arrays {a[k].size - 1:>7} values, {nd} differ  nan={int(np.isnan(a[k]).sum())}  {k}")
    extra = [k for k in b if k not in a]
    for k in extra:
        print(f"ONLY IN NEW  {k}")
    print(f"# {len(a)} operations, {int(sum(v[-1] for v in a.values()))} arrays, {differ + len(extra)} operations differ, {unsure} not comparable")
    return 1 if differ or extra else 0


if __name__ == "__main__":
    sys.exit(main())
