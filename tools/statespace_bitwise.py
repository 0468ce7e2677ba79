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
inputs, and statespace_rand of the prior and of the posterior.  Where the build has them: predictive_logpdf at those queries (ys with
NaN holes; the handle's sigma2 and an explicit one); append in three steps (k = 1, the single launch; k = 17, two chunks of the default
plan; one more point than the capacity holds, which grows the buffers) with every query taken again afterwards, smoothed lazily and
after an explicit smooth(); and the building blocks that take `chunk` at chunk = 1 (`blocks`)."""
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
            if not hasattr(probe, "lmm_oilmm_statespace_post_logpdf"):
                continue
            rng = np.random.default_rng([n, 11])
            Yq = rng.standard_normal((p, len(Q)))
            Yq[0, ::3] = np.nan
            Yq[:, 1] = np.nan                                    # one query with nothing observed
            yq = np.ascontiguousarray(Yq).reshape(-1)

            def answers(post, label):
                rec(f"{t} {label} mean_and_var", post.mean_and_var(Q))
                rec(f"{t} {label} vjp", post.mean_and_var_vjp(Q, np.ones(len(Q) * p), np.linspace(-1.0, 1.0, len(Q) * p)))
                rec(f"{t} {label} rand", post.rand(np.random.default_rng(n), Q, 3))
                rec(f"{t} {label} predictive_logpdf", post.predictive_logpdf(Q, yq))
                rec(f"{t} {label} predictive_logpdf sigma2", post.predictive_logpdf(Q, yq, sigma2=0.37))

            for explicit in (False, True):                       # the same appends; the queries smooth lazily, or after post.smooth()
                with lmm.statespace_posterior(fx, y) as post:
                    if not explicit:
                        answers(post, "posterior")
                    for step, k in enumerate((1, 17, None)):     # one chunk (the single launch); two chunks of the default plan; a growth
                        k = post.capacity - post.n + 1 if k is None else k
                        xn = float(np.max(x)) + step * 100.0 + np.cumsum(rng.uniform(0.05, 0.4, k))     # behind everything so far
                        Yn = rng.standard_normal((p, k))
                        Yn[0, ::4] = np.nan
                        cap = post.capacity
                        rec(f"{t} append {step} smooth={explicit}", [post.append(xn, np.ascontiguousarray(Yn).reshape(-1)), post.logpdf])
                        if step == 2:
                            assert post.capacity > cap, (post.capacity, cap)
                    if explicit:
                        post.smooth()
                    answers(post, f"appended smooth={explicit}")
    blocks(lmm, probe, rec)
    np.savez(out_path, **out)


def blocks(lmm, probe, rec):
    """The building blocks that take `chunk`, one latent of each model at chunk = 1: lengths 1 (one chunk), 2 (a prefix, one workgroup
    of the scan) and 130 (two workgroups at 128 aggregates each, three at 64, so ss_addprefix_kernel runs).  For the two blocks over a
    window the length is the window's: W = 1, 2 and 129 over the states of 130 points."""
    import test_gpu_statespace_append as GA
    import test_gpu_statespace_post_rand as GR
    import test_gpu_statespace_posterior as PP
    import test_gpu_statespace_predictive_logpdf as GL
    import test_sho_abi as S
    import test_statespace_abi as T
    import test_statespace_posterior_abi as PA
    have = lambda name: hasattr(probe, name)
    for lat in tuple(T.KINDS) + (("sho", S.QS[0]),):
        model = PA.model_of(lat, 0.9, 1.3) if lat in T.KINDS else S.sho(0.9, 1.7, lat[1])
        D = model.D
        for n in (1, 2, 130):
            rng = np.random.default_rng([n, 13])
            x, w, r = np.cumsum(rng.uniform(0.05, 0.6, n)), rng.uniform(0.1, 0.5, n), rng.standard_normal(n)
            if n > 2:
                w[n // 2] = np.inf
            t = f"block {lat} n={n} chunk=1"
            if have("lmm_dev_statespace_filter_from"):
                rec(f"{t} filter_from", list(GA.gpu_filter_from(lmm, model, np.full(D, 0.3), 0.5 * np.eye(D), x[0] - 0.2, x, w, r, 1)))
            fs, ss = PP.gpu_states(lmm, model, x, w, r, 1)
            rec(f"{t} states", [fs, ss])
        mid = 0.5 * (x[:-1] + x[1:])                             # x, fs, ss: the 130 points
        for W, q in ((1, mid[40:41]), (2, np.array([mid[40], mid[40] + 1e-3])), (129, mid[:65])):
            rng = np.random.default_rng([W, 17])
            t = f"block {lat} W={W} chunk=1"
            if have("lmm_dev_statespace_post_sample"):
                rec(f"{t} post_sample", GR.gpu_post_sample(lmm, model, x, fs, ss, q, rng.standard_normal((2, D * W)), 1))
            if have("lmm_dev_statespace_post_logpdf"):
                ws = rng.uniform(0.1, 0.5, len(q))
                ws[len(q) // 2] = np.inf if len(q) > 2 else ws[len(q) // 2]
                rec(f"{t} post_logpdf", GL.gpu_window_logpdf(lmm, model, x, fs, ss, q, ws, rng.standard_normal(len(q)), 1))


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
