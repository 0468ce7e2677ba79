"""Outputs of the dense per-latent path and of the dense-H ILMM path under two builds of liblmm_hip.so, byte for byte, on one GPU.

    python tools/bitwise_vs_parent.py PARENT.so NEW.so > bitwise_vs_parent.txt
    python tools/bitwise_vs_parent.py factor PARENT.so NEW.so >> bitwise_vs_parent.txt      (the factorisation alone, below)

Three child processes, one after the other and never two at once, each under a time limit and with LMM_DETERMINISTIC=1 (no split-K
atomics): PARENT, PARENT again (the control) and NEW, all on the same inputs.  The tool stops at the first child that exits non-zero.
Every output array of NEW is compared with PARENT's bytes, one line per operation (its output arrays back to back); an operation the
two PARENT runs disagree on, or whose repeated calls within one child do (the Float32 dense-H gradients, below), is listed as `not comparable`
and is no evidence either way.  Exit status 0 when no comparable array differs.

The inputs reach every branch of the launch dispatchers and every entry-point preamble: n = 200 (two 128-column panels), ns = 70, p = 9,
m = 7 latents (SE, Matern-5/2, RQ, periodic, locally periodic, SHO -- Matern-1/2 in its place for d > 1 and where SHO is not served -- and
a sum with a periodic term), shards [0, 7) and [2, 5), d = 1, 3 (isotropic and ARD), 6 and 12 (ARD), y complete and with single outputs
NaN, Float64 and (logpdf and posterior paths) the Float32 compute dtype, lmm_oilmm_logpdf_multi with ncol = 3, the inducing-point bound, its
gradient (with and without the regulariser; on the shard [2, 5) through the entry point, as the model refuses a sharded bound) and its
posterior's mean_and_var at nz = 70, the IndependentMOGP entry points, and the building blocks lmm_dev_gram / lmm_dev_sparse_moments / _grad per kind.

The dense-H ILMM (one (mn) x (mn) factorisation, n m = 1400: eleven 128-column panels) runs on the same inputs and the same (d, ARD, SHO)
loop with a dense 9 x 7 mixing matrix, in both compute dtypes: the prior logpdf with ILMM_ALLOW_DECOUPLED off and on (mixed kernels, seven
identical kernels -- the decoupled branch -- and a Y of 3 columns), logpdf_and_gradient without and with inputs, the posterior's
mean_and_var, mean_and_cov, logpdf and rand, a second conditioning batch with its own noise (mean_and_var, logpdf), the predictive
gradient with inputs after one and after two batches (joint 1890), and the latent view's logpdf, rand and gradient.

`factor`: n = 200 never reaches the region, panel, 64-column-tail, emulated or screened paths of the blocked Cholesky, so this mode
factors (NR, NC) = (320, 256), (1088, 1024), (1280, 1216) and (2368, 2304) -- the smallest shapes at which each of them runs -- under
the default switches, lmm_dev_set_f64_emul(1, 256, 16), lmm_dev_set_f64_screen(1, 256) and lmm_dev_set_zero_extents_min_cols(0):
one matrix assembled by lmm_dev_train_gram (Matern-5/2, sorted inputs a lengthscale of 0.6 spacings apart, three rider rows) through
lmm_dev_potrf and through lmm_dev_potrf_zext with the extents that launch kept -- factor, rider rows, inverse diagonal blocks and info
word are the record -- and, as those entry points factor one matrix, a batch of three through lmm.logpdf and the posterior's
mean_and_var of a three-latent OILMM with n = NC."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NS, P, M, NZ = 200, 70, 9, 7, 70
CHILD_SECONDS = 420
F32_GRAD_CALLS = 8


def kernels(lmm, d, ard, sho):
    ls = (lambda s: list(s * (1.0 + 0.1 * np.arange(d)))) if ard else (lambda s: s)
    per = lmm.PeriodicKernel(0.8, ls(1.3), r=0.9)
    return [lmm.SEKernel(1.1, ls(0.7)), lmm.Matern52Kernel(0.9, ls(0.9)), lmm.RationalQuadraticKernel(1.2, ls(0.8), alpha=1.7), per,
            lmm.LocallyPeriodicKernel(0.7, ls(1.1), r=1.2, decay=2.0), lmm.SHOKernel(1.0, 0.6, quality=2.5) if sho else lmm.Matern12Kernel(1.0, ls(0.6)),
            lmm.KernelSum(lmm.SEKernel(0.6, ls(0.5)), lmm.PeriodicKernel(0.4, ls(1.7), r=1.1), variance=1.3, lengthscale=1.1)]


def child(out_path):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import lmm_amd as lmm
    from lmm_amd import _lib as L, model as Mo
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

    def rec(name, v, pivot_may_fail=False, calls=1):      # one record per operation: all its output arrays back to back, and their number
        if callable(v):
            try:
                fn, v = v, v()
                for _ in range(calls - 1):      # the operation again on the same inputs: do the calls of ONE process agree?
                    if not all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(leaves(v), leaves(fn()))):
                        out["unstable::" + name] = np.ones(1)
            except (NotImplementedError, ValueError, TypeError) as e:      # a refusal (made before any launch) is an output too
                name, v = name + " [refused]", np.frombuffer(str(e).encode(), dtype=np.uint8)
            except ArithmeticError as e:      # a failed pivot is not hidden in a clean line: the record says so, and only `pivot_may_fail` lets the run go on
                if not pivot_may_fail:
                    raise
                name, v = name + " [FAILED PIVOT]", np.frombuffer(str(e).encode(), dtype=np.uint8)
        ls = leaves(v)
        out[name] = np.concatenate(ls + [np.array([float(len(ls))])])

    def elbo_grad_entry(vfe, fx, y, shard):      # lmm_oilmm_elbo_grad on a shard, every output
        xi, (Ua, Sa, p, m) = fx.x, Mo._H_args(fx.f.H)
        val, gs2 = C.c_double(), C.c_double()
        gy, gS, gU, gz = np.empty(xi.n * p), np.empty(m), np.empty(p * m), np.empty(xi.dim * vfe.nz)
        gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in fx.f.f.fs])
        L.check(L.load().lmm_oilmm_elbo_grad(xi.carr().ptr, xi.dim, xi.n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), ga, shard[0], shard[1],
                                             vfe.carr().ptr, vfe.nz, vfe.jitter, 1, C.byref(val), L.Arr(gy, True).ptr, C.byref(gs2), L.Arr(gS, True).ptr,
                                             L.Arr(gU, True).ptr, gg, L.Arr(gz, True).ptr))
        return [val.value, gy, gs2.value, gS, gU, [[g.variance, g.lengthscale, g.mean] for g in gg], gz]

    rng = np.random.default_rng(7)
    U = np.linalg.qr(rng.standard_normal((P, M)))[0]
    S = rng.uniform(0.5, 2.0, M)
    means = list(rng.standard_normal(M) * 0.3)
    Hd = np.random.default_rng(11).standard_normal((P, M))      # the dense mixing matrix (its own stream: the other inputs stay as they were)
    for d, ard, sho in [(1, False, True), (1, False, False), (3, False, False), (3, True, False), (6, False, False), (12, True, False)]:
        x = np.sort(rng.uniform(0.0, 4.0, N)) if d == 1 else rng.uniform(0.0, 2.0, (d, N))
        xs = np.sort(rng.uniform(0.0, 4.0, NS)) if d == 1 else rng.uniform(0.0, 2.0, (d, NS))
        x2 = xs[:40] + 0.013 if d == 1 else xs[:, :40] + 0.013
        z = np.linspace(0.05, 3.95, NZ) if d == 1 else rng.uniform(0.0, 2.0, (d, NZ))
        y, ys, Y3 = rng.standard_normal(N * P), rng.standard_normal(NS * P), rng.standard_normal((N * P, 3))
        ynan = y.copy()
        ynan[rng.integers(0, P, 60) * N + rng.choice(N, 60, replace=False)] = np.nan      # 60 points miss one output each
        fs = lmm.independent_mogp([lmm.GP(mu, k) for mu, k in zip(means, kernels(lmm, d, ard, sho))])
        for shard in [(0, M), (2, 5)]:
            tag = f"d={d}{' ard' if ard else ''}{' sho' if sho else ''} [{shard[0]},{shard[1]})"
            f = lmm.ILMM(fs, lmm.Orthogonal(U, S), shard=shard)
            fx, fxs, fx2 = (f(lmm.MOInputIsotopicByOutputs(a, P), 0.1) for a in (x, xs, x2))
            xr = lmm.MOInputIsotopicByOutputs(xs[..., ::6], P)      # 12 points: a joint sample factors their covariance with a jitter of 1e-18
            for f32 in (0, 1):
                lmm.set_compute_dtype("f32" if f32 else "f64")
                t = tag + (" f32" if f32 else "")
                rec(f"{t} logpdf", lambda: lmm.logpdf(fx, y))
                rec(f"{t} logpdf no regulariser", lambda: lmm.logpdf(fx, y, with_regulariser=False))
                rec(f"{t} logpdf multi", lambda: Mo._logpdf_matrix(fx, Y3))
                rec(f"{t} logpdf missing", lambda: lmm.logpdf(fx, ynan))
                po = lmm.posterior(fx, y)
                rec(f"{t} post mean_and_var", lambda: lmm.mean_and_var(po(fxs.x, 0.1)))
                rec(f"{t} post logpdf", lambda: lmm.logpdf(po(fxs.x, 0.1), ys))
                rec(f"{t} post missing mean_and_var", lambda: lmm.mean_and_var(lmm.posterior(fx, ynan)(fxs.x, 0.1)))
            lmm.set_compute_dtype("f64")
            po = lmm.posterior(fx, y)
            rec(f"{tag} grad", lambda: lmm.logpdf_and_gradient(fx, y, inputs=not sho))
            rec(f"{tag} grad missing", lambda: lmm.logpdf_and_gradient(fx, ynan))
            rec(f"{tag} prior mean_and_var", lambda: lmm.mean_and_var(fxs))
            rec(f"{tag} prior rand", lambda: lmm.rand(np.random.default_rng(3), f(xr, 0.1), 2))
            rec(f"{tag} post mean", lambda: lmm.mean(po(fxs.x, 0.1)))
            rec(f"{tag} post mean_and_cov", lambda: lmm.mean_and_cov(po(fxs.x, 0.1)))
            rec(f"{tag} post rand", lambda: lmm.rand(np.random.default_rng(3), po(xr, 0.1), 2))
            po2 = lmm.posterior(po(fx2.x, 0.2), ys[:40 * P])
            rec(f"{tag} post post mean_and_var", lambda: lmm.mean_and_var(po2(fxs.x, 0.1)))
            if not sho:
                rec(f"{tag} post logpdf grad", lambda: lmm.logpdf_and_gradient(po(fxs.x, 0.1), ys, inputs=True))
                rec(f"{tag} post post logpdf grad", lambda: lmm.logpdf_and_gradient(po2(fxs.x, 0.1), ys, inputs=True))
                rec(f"{tag} post vjp", lambda: lmm.mean_and_var_vjp(po(fxs.x, 0.1), dmean=ys, dvar=np.abs(ys)))
                rec(f"{tag} post vjp mean only", lambda: lmm.mean_and_var_vjp(po(fxs.x, 0.1), dmean=ys))
            if shard == (0, M):
                lat = lmm.get_latent_gp(po)
                rec(f"{tag} latent marginals", lambda: lmm.mean_and_var(lat(lmm.MOInputIsotopicByOutputs(xs, M), 1e-9)))
                rec(f"{tag} latent cross cov", lambda: Mo._mogp_cross_cov(lat, lmm.MOInputIsotopicByOutputs(xs[..., :20], M), lmm.MOInputIsotopicByOutputs(x2[..., :24], M)))
                if not sho:
                    vfe = lmm.VFE(z, 1e-6)
                    rec(f"{tag} elbo", lambda: lmm.elbo(vfe, fx, y))
                    rec(f"{tag} dtc no regulariser", lambda: lmm.dtc(vfe, fx, y, with_regulariser=False))
                    rec(f"{tag} elbo grad", lambda: lmm.elbo_and_gradient(vfe, fx, y))
                    rec(f"{tag} elbo grad no regulariser", lambda: lmm.elbo_and_gradient(vfe, fx, y, with_regulariser=False))
                    rec(f"{tag} approx post mean_and_var", lambda: lmm.mean_and_var(lmm.approx_posterior(vfe, fx, y)(fxs.x, 0.1)))
            elif not sho:      # the model refuses a sharded bound: the entry point itself
                rec(f"{tag} elbo grad", lambda: elbo_grad_entry(lmm.VFE(z, 1e-6), fx, y, shard))
        # the dense-H ILMM: one (mn) x (mn) factorisation, n m = 1400 (eleven 128-column panels); the joint of a predictive gradient is 1890
        tag = f"d={d}{' ard' if ard else ''}{' sho' if sho else ''} dense-H"
        g = lmm.ILMM(fs, Hd)
        g1 = lmm.ILMM(lmm.independent_mogp([lmm.GP(mu, kernels(lmm, d, ard, sho)[1]) for mu in means]), Hd)      # seven identical kernels
        gx, gxs, gx2 = (g(lmm.MOInputIsotopicByOutputs(a, P), s2) for a, s2 in ((x, 0.1), (xs, 0.1), (x2, 0.2)))
        zs = ys[:NS * M]
        for f32 in (0, 1):
            lmm.set_compute_dtype("f32" if f32 else "f64")
            t = tag + (" f32" if f32 else "")
            # Builds before backsolve_finish_kernel (a parent this tool may be given): the Float32 back substitution
            # (backsolve_step_kernel<float>) is not a function of its inputs there: every workgroup of step b reads
            # z[64 b .. 64 b + 63] while workgroup 0 of the same launch overwrites them with alpha_b, so the weights alpha = L^-T z of the
            # dense-H gradient, and all it computes from them, come out in several versions (profiles/dense_h_refactor/
            # f32_gradient_reproducibility.txt).  Each Float32 dense-H gradient is therefore called F32_GRAD_CALLS times in every child, and a
            # record whose calls disagree in any child is listed `not comparable`, like one the control differs on.
            settle = F32_GRAD_CALLS if f32 else 1
            for allow in (False, True):
                Mo.ILMM_ALLOW_DECOUPLED = allow
                ta = t + (" decoupled allowed" if allow else "")
                rec(f"{ta} logpdf", lambda: lmm.logpdf(gx, y))
                rec(f"{ta} logpdf identical kernels", lambda: lmm.logpdf(g1(gx.x, 0.1), y))
                rec(f"{ta} logpdf multi", lambda: lmm.logpdf(gx, Y3))
                rec(f"{ta} grad", lambda: lmm.logpdf_and_gradient(gx, y), calls=settle)
                rec(f"{ta} grad inputs", lambda: lmm.logpdf_and_gradient(gx, y, inputs=not sho), calls=settle)
            po = lmm.posterior(gx, y)
            rec(f"{t} post mean_and_var", lambda: lmm.mean_and_var(po(gxs.x, 0.1)))
            rec(f"{t} post mean_and_cov", lambda: lmm.mean_and_cov(po(gxs.x, 0.1)))
            rec(f"{t} post logpdf", lambda: lmm.logpdf(po(gxs.x, 0.1), ys))
            # lmm_ilmm_post_rand: one sample per call; its jitter of 1e-12 is below Float32 resolution, where the pivot may fail
            rec(f"{t} post rand", lambda: lmm.rand(np.random.default_rng(3), po(xr, 0.1)), pivot_may_fail=bool(f32))
            po2 = lmm.posterior(po(gx2.x, 0.2), ys[:40 * P])
            rec(f"{t} post post mean_and_var", lambda: lmm.mean_and_var(po2(gxs.x, 0.1)))
            rec(f"{t} post post logpdf", lambda: lmm.logpdf(po2(gxs.x, 0.1), ys))
            rec(f"{t} post logpdf grad", lambda: lmm.logpdf_and_gradient(po(gxs.x, 0.1), ys, inputs=not sho), calls=settle)
            rec(f"{t} post post logpdf grad", lambda: lmm.logpdf_and_gradient(po2(gxs.x, 0.1), ys, inputs=not sho), calls=settle)
            lat = lmm.get_latent_gp(po)(lmm.MOInputIsotopicByOutputs(xs, M), 0.1)
            rec(f"{t} latent logpdf", lambda: lmm.logpdf(lat, zs))
            rec(f"{t} latent rand", lambda: lmm.rand(np.random.default_rng(3), lmm.get_latent_gp(po)(lmm.MOInputIsotopicByOutputs(xs[..., ::6], M), 0.1), 2))
            rec(f"{t} latent logpdf grad", lambda: lmm.logpdf_and_gradient(lat, zs, inputs=not sho), calls=settle)
            del po, po2, lat
        lmm.set_compute_dtype("f64")
        Mo.ILMM_ALLOW_DECOUPLED = True
        # the IndependentMOGP entry points
        tag = f"d={d}{' ard' if ard else ''}{' sho' if sho else ''} mogp"
        ym = y[:N * M]
        gx = fs(lmm.MOInputIsotopicByOutputs(x, M), 0.1)
        rec(f"{tag} logpdf", lambda: lmm.logpdf(gx, ym))
        rec(f"{tag} logpdf diag", lambda: lmm.logpdf(fs(lmm.MOInputIsotopicByOutputs(x, M), rng.uniform(0.05, 0.2, N * M)), ym))
        rec(f"{tag} post mean_and_var", lambda: lmm.mean_and_var(lmm.posterior(gx, ym)(lmm.MOInputIsotopicByOutputs(xs, M), 0.1)))
        # the building blocks, one latent kind at a time
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
        xd, zd = dev(np.atleast_2d(x).T), dev(np.atleast_2d(z).T)
        w, r, beta = dev(rng.uniform(0.05, 0.5, N)), dev(rng.standard_normal(N)), dev(rng.standard_normal(NZ))
        A = rng.standard_normal((NZ, NZ))
        PhiBar = dev(0.5 * (A + A.T))
        for l, k in enumerate(kernels(lmm, d, ard, sho)):
            gp = L.gps_array([dict(k.desc(), mean=0.0)])
            G = torch.zeros((256, 256), dtype=torch.float64, device="cuda")
            L.check(L.load().lmm_dev_gram(C.c_void_p(G.data_ptr()), 256, 256, 256, C.c_void_p(xd.data_ptr()), d, N, gp, C.c_double(0.25)))
            torch.cuda.synchronize()
            rec(f"{tag} dev_gram latent {l}", lambda: G)
            if k.kind == "sho":
                continue
            Phi, b, sc = torch.zeros((NZ, NZ), dtype=torch.float64, device="cuda"), torch.zeros(NZ, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
            L.check(L.load().lmm_dev_sparse_moments(xd.data_ptr(), d, N, zd.data_ptr(), NZ, gp, w.data_ptr(), r.data_ptr(), 64, Phi.data_ptr(), NZ, b.data_ptr(), sc.data_ptr()))
            recs = torch.zeros(L.SUM_MAX_TERMS * (16 + d), dtype=torch.float64, device="cuda")
            gz, gr = torch.zeros((NZ, d), dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
            L.check(L.load().lmm_dev_sparse_grad(xd.data_ptr(), d, N, zd.data_ptr(), NZ, gp, w.data_ptr(), r.data_ptr(), PhiBar.data_ptr(), NZ, beta.data_ptr(), 64,
                                                 recs.data_ptr(), gz.data_ptr(), gr.data_ptr()))
            torch.cuda.synchronize()
            rec(f"{tag} dev_sparse_moments latent {l}", [torch.tril(Phi.T), b, sc])
            rec(f"{tag} dev_sparse_grad latent {l}", [recs, gz, gr])
    np.savez(out_path, **out)


FACTOR_SHAPES = [(320, 256), (1088, 1024), (1280, 1216), (2368, 2304)]
FACTOR_RIDERS = 3


def child_factor(out_path):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import lmm_amd as lmm
    from lmm_amd import _lib as L
    lmm.init(0)
    lib = lmm.load()
    lib.lmm_dev_set_f64_emul.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.lmm_dev_set_f64_screen.argtypes = [C.c_int, C.c_int]
    lib.lmm_dev_set_zero_extents_min_cols.argtypes = [C.c_int]
    lib.lmm_dev_potrf_zext.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.lmm_dev_train_gram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(L.GpT), C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    settings = {"default": lambda: 0, "emul from 256": lambda: lib.lmm_dev_set_f64_emul(1, 256, 16), "f64 screen from 256": lambda: lib.lmm_dev_set_f64_screen(1, 256),
                "zero extents at every width": lambda: lib.lmm_dev_set_zero_extents_min_cols(0)}
    out = {}

    def rec(name, arrays):
        ls = [np.asarray(a.cpu() if hasattr(a, "cpu") else a, dtype=np.float64).reshape(-1) for a in arrays]
        out[name] = np.concatenate(ls + [np.array([float(len(ls))])])

    for sname, apply in settings.items():
        assert lib.lmm_dev_set_f64_emul(-1, 0, 0) == 0 and lib.lmm_dev_set_f64_screen(-1, 0) == 0 and lib.lmm_dev_set_zero_extents_min_cols(-1) == 0
        assert apply() == 0, lib.lmm_last_error_string()
        for NR, NC in FACTOR_SHAPES:
            rng = np.random.default_rng(NC)
            xd = torch.arange(NC, dtype=torch.float64, device="cuda")
            rid = torch.from_numpy(rng.standard_normal(FACTOR_RIDERS * NC)).cuda()
            noise = np.full(1, 0.1)
            ext = np.full(NR // 64, -7, dtype=np.int32)
            G = torch.zeros(NC * NR, dtype=torch.float64, device="cuda")
            gps = L.gps_array([{"kind": "matern52", "variance": 1.0, "lengthscale": 0.6, "mean": 0.0}])
            torch.cuda.synchronize()
            L.check(lib.lmm_dev_train_gram(C.c_void_p(G.data_ptr()), NR, NR, NC, C.c_void_p(xd.data_ptr()), 1, NC, gps, 1, C.c_void_p(noise.ctypes.data), None,
                                           C.c_void_p(rid.data_ptr()), FACTOR_RIDERS, C.c_void_p(ext.ctypes.data)))
            zx = torch.from_numpy(ext).cuda()
            for how, z in (("potrf", None), ("potrf_zext", zx)):
                A = G.clone()
                W = torch.zeros(NC // 64 * 4096, dtype=torch.float64, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                L.check(lib.lmm_dev_potrf_zext(C.c_void_p(A.data_ptr()), NR, NC, NR, C.c_void_p(W.data_ptr()), NC, C.c_void_p(info.data_ptr()),
                                               None if z is None else C.c_void_p(z.data_ptr())))
                torch.cuda.synchronize()
                rec(f"{sname}: {how} {NR} x {NC}, {int((ext > 0).sum())} of {ext.size} row blocks with zeros", [A, W, info])
            # a batch of three through the per-latent path
            n, p, m = NC, 3, 3
            x = np.arange(n, dtype=np.float64)
            U = np.linalg.qr(rng.standard_normal((p, m)))[0]
            f = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel(1.0 + 0.1 * l, 0.6 + 0.7 * l)) for l in range(m)]), lmm.Orthogonal(U, np.linspace(2.0, 1.0, m)))
            fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
            y = rng.standard_normal(n * p)
            rec(f"{sname}: logpdf, 3 latents, n = {n}", [lmm.logpdf(fx, y)])
            rec(f"{sname}: posterior mean_and_var, 3 latents, n = {n}", list(lmm.mean_and_var(lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(x[:40] + 0.3, p), 0.1))))
    np.savez(out_path, **out)


def main():
    if len(sys.argv) == 3 and sys.argv[1] in ("--child", "--child-factor"):
        return (child if sys.argv[1] == "--child" else child_factor)(sys.argv[2])
    factor = sys.argv[1] == "factor"
    parent, new = sys.argv[-2], sys.argv[-1]
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for i, lib in enumerate([parent, parent, new]):
            path = os.path.join(tmp, f"run{i}.npz")
            env = dict(os.environ, LMM_HIP_LIB=os.path.abspath(lib), LMM_DETERMINISTIC="1")
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-factor" if factor else "--child", path], env=env, timeout=CHILD_SECONDS).returncode
            if rc != 0:
                print(f"child {i} ({lib}) exited with {rc}: stopping")
                return 3
            with np.load(path) as zf:
                runs.append({k: zf[k] for k in zf.files})
    unstable = {k[len("unstable::"):] for r in runs for k in r if k.startswith("unstable::")}
    a, c, b = ({k: v for k, v in r.items() if not k.startswith("unstable::")} for r in runs)
    print(f"# {parent} and {new}, each in its own process on one GPU, LMM_DETERMINISTIC=1, same inputs; every output compared byte for byte.")
    print(f"# factor mode: (NR, NC) in {FACTOR_SHAPES}; control: {parent} twice." if factor else f"# n = {N}, ns = {NS}, p = {P}, m = {M}, nz = {NZ}; control: {parent} twice.")
    differ = unsure = 0
    for k in a:
        if k not in b or k not in c or a[k].shape != b[k].shape:      # (a record that ends [refused] or [FAILED PIVOT] in one run only is missing in the others)
            print(f"MISSING OR RESHAPED  {k}")
            differ += 1
            continue
        nd = int(np.sum(a[k].view(np.uint64) != b[k].view(np.uint64)))
        control = a[k].tobytes() == c[k].tobytes() and k not in unstable
        word = "not comparable" if not control else "identical" if nd == 0 else "DIFFERENT"
        differ += word == "DIFFERENT"
        unsure += not control
        print(f"{word:<14} {int(a[k][-1]):>3} arrays {a[k].size - 1:>7} values, {nd} differ  nan={int(np.isnan(a[k]).sum())}  {k}")
    extra = [k for k in b if k not in a]
    for k in extra:
        print(f"ONLY IN NEW  {k}")
    print(f"# {len(a)} operations, {int(sum(v[-1] for v in a.values()))} arrays, {differ + len(extra)} operations differ, {unsure} not comparable (the control differs, or an operation's repeated calls in one process do)")
    return 1 if differ or extra else 0


if __name__ == "__main__":
    sys.exit(main())
