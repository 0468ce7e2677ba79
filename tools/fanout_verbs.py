"""Every per-latent verb of the library at small shapes (two batches of latents), each output written as raw float64 bytes: python tools/fanout_verbs.py OUTDIR
Run on two builds (LMM_HIP_LIB) and compare the directories byte for byte, or run under rocprofv3 --kernel-trace and compare the
traces with tools/compare_kernel_traces.py (profiles/host_fanout/)."""
import os, sys
sys.path.insert(0, ".")
import numpy as np
import lmm_amd as lmm

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
lmm.init(0)
rng = np.random.default_rng(7)
m, p, n, d, ns, s2 = 40, 44, 100, 2, 30, 0.2
kinds = [lmm.SEKernel, lmm.Matern32Kernel, lmm.Matern52Kernel]
mogp = lmm.independent_mogp([lmm.GP(float(rng.normal()), kinds[l % 3](float(rng.uniform(0.5, 2)), float(rng.uniform(0.5, 2)))) for l in range(m)])
U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
H = lmm.Orthogonal(np.ascontiguousarray(U), S)
x, x2, xs = rng.uniform(0, 6, (d, n)), rng.uniform(0, 6, (d, 60)), rng.uniform(0, 6, (d, ns))
y, y2, ys = rng.standard_normal(n * p), rng.standard_normal(60 * p), rng.standard_normal(ns * p)
ym = y.reshape(p, n).copy(); ym[3, 10:20] = np.nan; ym[7, 40:50] = np.nan; ym = ym.reshape(-1)
I = lambda a: lmm.MOInputIsotopicByOutputs(a, p)


def dump(name, v):
    if isinstance(v, dict):
        for k, w in v.items():
            dump(f"{name}.{k}", w)
    elif isinstance(v, (list, tuple)):
        for i, w in enumerate(v):
            dump(f"{name}.{i}", w)
    else:
        if hasattr(v, "cpu"):
            v = v.cpu().numpy()
        np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tofile(os.path.join(out_dir, name + ".f64"))


f = lmm.ILMM(mogp, H)
fx = f(I(x), s2)
dump("logpdf", lmm.logpdf(fx, y))
dump("grad", dict(lmm.logpdf_and_gradient(fx, y, True, inputs=True)))
dump("grad_missing", dict(lmm.logpdf_and_gradient(fx, ym, True)))
post = lmm.posterior(fx, y)
dump("mean_and_var", lmm.mean_and_var(post(I(xs), s2)))
dump("mean_and_var_vjp", lmm.mean_and_var_vjp(post(I(xs), s2), rng.standard_normal(ns * p), rng.standard_normal(ns * p)))
dump("post_logpdf", lmm.logpdf(post(I(xs), s2), ys))
post2 = lmm.posterior(post(I(x2), 0.3), y2)          # two conditioning batches + the test block: three noise blocks
dump("post_grad", dict(lmm.logpdf_and_gradient(post2(I(xs), 0.25), ys, True, inputs=True)))
dump("rand", lmm.rand(np.random.default_rng(3), post(I(xs), s2), 3))
dump("rand_prior", lmm.rand(np.random.default_rng(3), f(I(xs), s2), 3))
xc = xs[:, :12]
dump("mean_and_cov", lmm.mean_and_cov(lmm.ILMM(mogp, H, shard=(0, 6))(I(xc), s2)))
dump("mean_and_cov_post", lmm.mean_and_cov(lmm.posterior(lmm.ILMM(mogp, H, shard=(0, 6))(I(x), s2), y)(I(xc), s2)))
vfe = lmm.VFE(rng.uniform(0, 6, (d, 24)), 1e-6)
dump("elbo", lmm.elbo(vfe, fx, y))
dump("elbo_grad", dict(lmm.elbo_and_gradient(vfe, fx, y)))
print("verbs done:", len(os.listdir(out_dir)), "outputs")
