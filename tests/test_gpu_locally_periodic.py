"""-m gpu: locally periodic latents (SE x Periodic as one base kind; include/lmm_hip.h LMM_KERNEL_LOCALLY_PERIODIC) against identities
that need no reference and against the CPU oracle extended inside this file: oracle.lmm_oracle.kernelmatrix is patched with a numpy
Gram evaluated by DIRECT differences (the periodic part reduced modulo 1, then sin(pi .); the SE part from the same differences), "sum"
descriptors are routed through it (the outer lengthscale scales the period AND the decay), and gp_mean_var's prior variance of a sum
is taken from that kernel at r = 0.  Gradients are central finite differences of the patched oracle (step 1e-6; rel 2e-5, abs 1e-6,
the bar of tests/test_gpu_kernel_families.py).

Shapes: n = 70 is one ragged tile (generic path only), n = 1000 has interior and border tiles, n = 2100 is past 2048 (more than one
block column; rider and pad tiles after an interior region).  Periods are drawn from [0.5, 3], r from [0.5, 2] and decay from
[0.5, 4], so |x| / P <= 100 and the angle-difference form of the interior tiles stays ~1e-13 from the direct form, far
inside rel = 1e-9."""
import ctypes as C
import gc

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
RTOL32 = 2e-4          # fp32 OILMM logpdf (include/lmm_hip.h, tests/test_gpu_f32.py)
H_FD = 1e-6
PERIODIC_KINDS = ("periodic", "locally_periodic")


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def _base_gram(g, a, b, s0=1.0):
    """One base kernel (any kind, scalar or per-dimension lengthscale / period) between the column sets a and b; s0: the outer
    lengthscale of the sum the kernel is a term of (it scales the lengthscale / period and a locally periodic term's decay)."""
    ls = g.get("lengthscale", 1.0)
    s = s0 * np.asarray(ls, dtype=np.float64).reshape(-1, 1) if np.ndim(ls) else s0 * float(ls)
    v = float(g.get("variance", 1.0))
    if g["kind"] in PERIODIC_KINDS:
        q = np.zeros((a.shape[1], b.shape[1]))
        D2 = np.zeros((a.shape[1], b.shape[1]))
        sv = np.broadcast_to(s, (a.shape[0], 1)) if np.ndim(s) else np.full((a.shape[0], 1), s)
        for k in range(a.shape[0]):
            dx = a[k][:, None] - b[k][None, :]
            t = dx / sv[k, 0]
            t = t - np.rint(t)                                     # modulo 1: whole periods drop out
            q += np.sin(np.pi * t) ** 2
            D2 += dx * dx
        rho = float(g.get("r", 1.0))
        e = -0.5 * q / rho ** 2
        if g["kind"] == "locally_periodic":
            e = e - 0.5 * D2 / (s0 * float(g.get("decay", 1.0))) ** 2
        return v * np.exp(e)
    a, b = a / s, b / s
    r2 = np.zeros((a.shape[1], b.shape[1]))
    for k in range(a.shape[0]):
        t = a[k][:, None] - b[k][None, :]
        r2 += t * t
    return O.kernel_eval(g["kind"], v, 1.0, np.sqrt(r2))


@pytest.fixture(autouse=True)
def locally_periodic_oracle(monkeypatch):
    def kernelmatrix(gp, x, x2=None):
        a = O._as_cols(x)
        b = a if x2 is None else O._as_cols(x2)
        if gp["kind"] != "sum":
            return _base_gram(gp, a, b)
        s0 = float(gp.get("lengthscale", 1.0))
        return float(gp.get("variance", 1.0)) * sum(_base_gram(t, a, b, s0) for t in gp["terms"])

    orig_mv = O.gp_mean_var

    def gp_mean_var(gp, x):
        m, v = orig_mv(gp, x)
        if gp["kind"] == "sum":
            x0 = O._as_cols(x)[:, :1]
            v = v + (kernelmatrix(gp, x0)[0, 0] - float(gp.get("variance", 1.0)))
        return m, v

    monkeypatch.setattr(O, "kernelmatrix", kernelmatrix)
    monkeypatch.setattr(O, "gp_mean_var", gp_mean_var)


def _base_kernel(lmm, t):
    if t["kind"] == "locally_periodic":
        return lmm.LocallyPeriodicKernel(t["variance"], t["lengthscale"], r=t["r"], decay=t["decay"])
    if t["kind"] == "periodic":
        return lmm.PeriodicKernel(t["variance"], t["lengthscale"], r=t["r"])
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    return K[t["kind"]](t["variance"], t["lengthscale"])


def _kernel(lmm, g):
    if g["kind"] == "sum":
        return lmm.KernelSum(*[_base_kernel(lmm, t) for t in g["terms"]], variance=g["variance"], lengthscale=g["lengthscale"])
    return _base_kernel(lmm, g)


def _model(lmm, gps):
    return lmm.independent_mogp([lmm.GP(g.get("mean", 0.0), _kernel(lmm, g)) for g in gps])


def _lp(rng, r=None, decay=None, d=None, mean=True, kind="locally_periodic"):
    g = {"kind": kind, "variance": float(rng.uniform(0.5, 1.5)),
         "lengthscale": rng.uniform(0.5, 3.0, d) if d else float(rng.uniform(0.5, 3.0)),
         "r": float(rng.uniform(0.5, 2.0)) if r is None else r}
    if kind == "locally_periodic":
        g["decay"] = float(rng.uniform(0.5, 4.0)) if decay is None else decay
    if mean:
        g["mean"] = float(rng.normal())
    return g


def _term(rng, kind, d=None):
    return {"kind": kind, "variance": float(rng.uniform(0.4, 1.2)),
            "lengthscale": rng.uniform(0.6, 2.0, d) if d else float(rng.uniform(0.5, 2.0))}


def _sum(rng, terms, s0=1.0):
    return {"kind": "sum", "variance": float(rng.uniform(0.7, 1.5)), "lengthscale": s0, "mean": float(rng.normal()), "terms": terms}


def _mixed(rng, d):
    """locally periodic; one with the library's defaults r = 1, decay = 1; locally periodic (per-dimension periods when d > 1) +
    Matern32; periodic + locally periodic; plain Matern52."""
    dv = d if d > 1 else None
    return [_lp(rng), _lp(rng, r=1.0, decay=1.0),
            _sum(rng, [_lp(rng, d=dv, mean=False), _term(rng, "matern32")]),
            _sum(rng, [_lp(rng, mean=False, kind="periodic"), _lp(rng, mean=False)]),
            {"kind": "matern52", "variance": float(rng.uniform(0.6, 1.6)), "lengthscale": float(rng.uniform(0.7, 1.8)),
             "mean": float(rng.normal())}]


def _orth(rng, p, m):
    U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
    return np.ascontiguousarray(U), S


def _inputs(rng, case, n):
    if case == "d1sorted":
        return np.sort(rng.uniform(0.0, 0.02 * n, n))
    if case == "d1spread":
        return rng.uniform(0.0, 30.0, n)
    return rng.uniform(0.0, 3.0, size=(3 if case == "d3" else 12, n))


def _dim(x):
    return 1 if np.ndim(x) == 1 else x.shape[0]


def _cols(x):
    return x.reshape(1, -1) if np.ndim(x) == 1 else x


# ---------------------------------------------------------------------------------------------------
# 1. values through every Gram path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [70, 1000, 2100])
@pytest.mark.parametrize("case", ["d1sorted", "d1spread", "d3", "d12"])
def test_values_through_every_gram_path(lmm, case, n):
    rng = np.random.default_rng(10100 + n + len(case))
    p = 7
    x = _inputs(rng, case, n)
    gps = _mixed(rng, _dim(x))
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    ref = O.oilmm_logpdf(gps, U, S, x, 0.1, y)
    print(f"locally periodic logpdf {case} n={n}: got {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.3e}")
    assert got == pytest.approx(ref, rel=1e-9)


# ---------------------------------------------------------------------------------------------------
# 2. identities that need no oracle
# ---------------------------------------------------------------------------------------------------
def _logpdf_of(lmm, kernels, x, p, U, S, y, s2=0.1):
    fs = lmm.independent_mogp([lmm.GP(0.1 * (l + 1), k) for l, k in enumerate(kernels)])
    return lmm.logpdf(lmm.ILMM(fs, lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2), y)


@pytest.mark.parametrize("case", ["d1spread", "d3"])
def test_limits_are_the_periodic_and_the_se_latent(lmm, case):
    """decay = 1e8: the SE factor differs from 1 by <= 5e-14 for |x - x'| <= 30, so the latent is the library's PeriodicKernel latent;
    r = 1e8: the periodic factor is 1 to 5e-17 d, so it is the SEKernel latent of lengthscale decay.  n = 1000: interior tiles too."""
    rng = np.random.default_rng(10200 + len(case))
    n, p = 1000, 3
    x = _inputs(rng, case, n)
    d = _dim(x)
    P = rng.uniform(0.5, 3.0, d) if d > 1 else 1.7
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    other = lmm.Matern52Kernel(0.8, 0.9)
    a = _logpdf_of(lmm, [lmm.LocallyPeriodicKernel(0.9, P, r=0.8, decay=1e8), other], x, p, U, S, y)
    b = _logpdf_of(lmm, [lmm.PeriodicKernel(0.9, P, r=0.8), other], x, p, U, S, y)
    assert a == pytest.approx(b, rel=1e-9)
    a = _logpdf_of(lmm, [lmm.LocallyPeriodicKernel(0.9, P, r=1e8, decay=1.3), other], x, p, U, S, y)
    b = _logpdf_of(lmm, [lmm.SEKernel(0.9, 1.3), other], x, p, U, S, y)
    assert a == pytest.approx(b, rel=1e-9)


def test_product_and_equal_vector_period(lmm):
    """The product IS the explicit class (equal objects, equal descriptors: checked exactly on the host), so the device sees the same
    input twice.  The results are compared to rel 1e-12 (value) and 1e-9 (gradients), not bitwise: two identical calls may differ in
    the last places, because the last-round tiles of the Cholesky updates are summed along K with f64 atomics in a run-dependent
    order (a 1-ulp difference of d/d decay between two such calls was observed on MI355X)."""
    rng = np.random.default_rng(10210)
    d, n, p = 3, 300, 3
    x = rng.uniform(0.0, 3.0, size=(d, n))
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    other = lmm.GP(lmm.SEKernel(0.8, 0.9))
    K = lmm.LocallyPeriodicKernel
    grad = lambda k: lmm.logpdf_and_gradient(lmm.ILMM(lmm.independent_mogp([lmm.GP(0.1, k), other]), lmm.Orthogonal(U, S))(xin, 0.2), y)
    Gs = grad(K(0.9, 1.7, r=0.6, decay=2.2))
    Gv = grad(K(0.9, np.full(d, 1.7), r=0.6, decay=2.2))
    assert Gv["value"] == pytest.approx(Gs["value"], rel=1e-12)
    assert np.sum(Gv["gps"][0]["lengthscale"]) == pytest.approx(Gs["gps"][0]["lengthscale"], rel=1e-9)
    for key in ("r", "decay", "variance"):
        assert Gv["gps"][0][key] == pytest.approx(Gs["gps"][0][key], rel=1e-9)
    for prod in (lmm.SEKernel(0.5, 2.2) * lmm.PeriodicKernel(1.8, 1.7, r=0.6), lmm.PeriodicKernel(1.8, 1.7, r=0.6) * lmm.SEKernel(0.5, 2.2)):
        explicit = K(0.9, 1.7, r=0.6, decay=2.2)
        assert type(prod) is K and prod == explicit and prod.key() == explicit.key() and prod.desc() == explicit.desc()
        Gp = grad(prod)
        print(f"product vs class: value {Gp['value']!r} {Gs['value']!r}; decay {Gp['gps'][0]['decay']!r} {Gs['gps'][0]['decay']!r}")
        assert Gp["value"] == pytest.approx(Gs["value"], rel=1e-12)
        for key in ("lengthscale", "r", "decay", "variance"):
            assert Gp["gps"][0][key] == pytest.approx(Gs["gps"][0][key], rel=1e-9)


@pytest.mark.parametrize("key,vals", [("decay", (0.9, 2.6)), ("r", (0.6, 1.7))])
def test_dense_shortcut_compares_decay_and_rho(lmm, key, vals):
    """Two latents differing only in decay (only in r): the batched Gram launch and the dense-H decoupled shortcut keep them apart."""
    from lmm_amd import model as Mdl
    rng = np.random.default_rng(10220)
    n, p = 150, 3
    x = rng.uniform(0.0, 4.0, size=(2, n))
    base = {"kind": "locally_periodic", "variance": 1.1, "lengthscale": 1.3, "mean": 0.2, "r": 0.8, "decay": 1.5}
    gps = [dict(base, **{key: vals[0]}), dict(base, **{key: vals[1]})]
    same = [dict(base, **{key: vals[0]}), dict(base, **{key: vals[0]})]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    a = lmm.logpdf(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(xin, 0.1), y)
    b = lmm.logpdf(lmm.ILMM(_model(lmm, same), lmm.Orthogonal(U, S))(xin, 0.1), y)
    assert a == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)
    assert b == pytest.approx(O.oilmm_logpdf(same, U, S, x, 0.1, y), rel=1e-9)
    assert abs(a - b) > 1e-3 * abs(a)
    H = rng.uniform(size=(p, 2))
    for g, path in ((gps, "dense"), (same, "decoupled")):
        got = lmm.logpdf(lmm.ILMM(_model(lmm, g), H)(xin, 0.1), y)
        assert Mdl.ILMM_LAST_PATH == path
        assert got == pytest.approx(O.ilmm_logpdf(g, H, x, 0.1, y), rel=1e-9)


# ---------------------------------------------------------------------------------------------------
# 3. the other verbs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [9, 70, 130])
@pytest.mark.parametrize("d", [1, 3])
def test_verbs_with_locally_periodic_latents(lmm, d, ns):
    rng = np.random.default_rng(10300 + d + ns)
    n, n2, p = 300, 60, 4
    mk = (lambda k: rng.uniform(0.0, 3.0, size=(d, k))) if d > 1 else (lambda k: rng.uniform(0.0, 6.0, k))
    x, x2, xs = mk(n), mk(n2), mk(ns)
    gps = _mixed(rng, d)[:4]
    m = len(gps)
    U, S = _orth(rng, p, m)
    H = O.orthogonal_dense(U, S)
    y, y2 = rng.standard_normal(n * p), rng.standard_normal(n2 * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    po = O.oilmm_posterior(gps, U, S, x, 0.1, y)
    pox = post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1)
    mo, vo = O.oilmm_mean_var(po, U, S, xs, 0.1)
    mu, v = lmm.mean_and_var(pox)
    np.testing.assert_allclose(mu, mo, rtol=1e-9, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-9)
    np.testing.assert_allclose(lmm.mean(pox), mo, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(lmm.marginals(pox).sigma, np.sqrt(vo), rtol=1e-9)
    mo0, vo0 = O.oilmm_mean_var(gps, U, S, xs, 0.1)                       # prior marginals: kappa(0) = v
    mu0, v0 = lmm.mean_and_var(f(lmm.MOInputIsotopicByOutputs(xs, p), 0.1))
    np.testing.assert_allclose(mu0, mo0, rtol=1e-10, atol=1e-12); np.testing.assert_allclose(v0, vo0, rtol=1e-10)
    # rand given the normals: a prior with explicit jitters of 1e-6, and a posterior.  Both sides factor K + 1e-6 I, whose condition
    # number is ~1e6 n, so the reference's own sample carries ~eps * 1e6 * n ~ 1e-8 relative: the bar is tests/test_gpu_periodic.py's
    jit = (1e-9, 1e-6, 1e-6)
    got = lmm.rand(np.random.default_rng(9), f(lmm.MOInputIsotopicByOutputs(xs, p), 0.1), jitters=jit)
    g2 = np.random.default_rng(9); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(gps)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + np.sqrt(0.1) * eps, rtol=1e-6, atol=1e-7)
    got = lmm.rand(np.random.default_rng(4), pox, jitters=jit)
    g2 = np.random.default_rng(4); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(po)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + np.sqrt(0.1) * eps, rtol=1e-6, atol=1e-7)
    # sequential conditioning
    po2 = lmm.posterior(post(lmm.MOInputIsotopicByOutputs(x2, p), 0.3), y2)
    ro = O.oilmm_posterior(po, U, S, x2, 0.3, y2)
    mu, v = lmm.mean_and_var(po2(lmm.MOInputIsotopicByOutputs(xs, p), 0.2))
    mo, vo = O.oilmm_mean_var(ro, U, S, xs, 0.2)
    np.testing.assert_allclose(mu, mo, rtol=1e-9, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-9)
    # IndependentMOGP: cov(f, x), cov(f, x, y) prior and posterior
    fm = _model(lmm, gps)
    ym = rng.standard_normal(n * m)
    na, nb = min(ns, 40), 20
    xsub, x2sub = (xs[:na], x2[:nb]) if d == 1 else (xs[:, :na], x2[:, :nb])
    xa, xb = lmm.MOInputIsotopicByOutputs(xsub, m), lmm.MOInputIsotopicByOutputs(x2sub, m)
    np.testing.assert_allclose(lmm.cov(fm, xa), O.mogp_cov(gps, xsub), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(lmm.cov(fm, xa, xb), O.mogp_cross_cov(gps, xsub, x2sub), rtol=1e-10, atol=1e-12)
    pm = lmm.posterior(fm(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    rm = O.mogp_posterior(gps, x, 0.2, ym)
    np.testing.assert_allclose(lmm.cov(pm, xa, xb), O.mogp_cross_cov(rm, xsub, x2sub), rtol=1e-9, atol=1e-9)
    # dense-H ILMM: logpdf, mean_and_cov, sequential conditioning
    xd, yd = (x[:60], y[:60 * p]) if d == 1 else (x[:, :60], y[:60 * p])
    Hd = rng.uniform(size=(p, m))
    fdx = lmm.ILMM(_model(lmm, gps), Hd)(lmm.MOInputIsotopicByOutputs(xd, p), 0.1)
    assert lmm.logpdf(fdx, yd) == pytest.approx(O.ilmm_logpdf(gps, Hd, xd, 0.1, yd), rel=1e-9)
    pd = lmm.posterior(fdx, yd)
    rd = O.ilmm_posterior(gps, Hd, xd, 0.1, yd)
    nd_ = min(ns, 12)
    xs12 = xs[:nd_] if d == 1 else xs[:, :nd_]
    xsi = lmm.MOInputIsotopicByOutputs(xs12, p)
    M, Cm = lmm.mean_and_cov(pd(xsi, 0.1))
    Mr, Cr = O.ilmm_mean_cov(rd, Hd, xs12, 0.1)
    np.testing.assert_allclose(M, Mr, rtol=1e-9, atol=1e-9); np.testing.assert_allclose(Cm, Cr, rtol=1e-9, atol=1e-9)
    x30 = x2[:30] if d == 1 else x2[:, :30]
    pd2 = lmm.posterior(pd(lmm.MOInputIsotopicByOutputs(x30, p), 0.25), y2[:30 * p])
    rd2 = O.ilmm_posterior_condition(rd, Hd, x30, 0.25, y2[:30 * p])
    mu, v = lmm.mean_and_var(pd2(xsi, 0.1))
    mo, vo = O.ilmm_mean_var(rd2, Hd, xs12, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-9, atol=1e-9); np.testing.assert_allclose(v, vo, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------
# 4. gradients against central finite differences of the patched oracle
# ---------------------------------------------------------------------------------------------------
def _perturb(gps, path, t):
    g2 = [dict(g, terms=[dict(tt) for tt in g["terms"]]) if g["kind"] == "sum" else dict(g) for g in gps]
    l, c, key, k = path
    tgt = g2[l] if c is None else g2[l]["terms"][c]
    if k is None:
        tgt[key] = tgt[key] + t
    else:
        v = np.array(tgt[key], dtype=np.float64)
        v[k] += t
        tgt[key] = v
    return g2


def _check_entry(G, g, fun, gps, l, c, rel, abs_, h):
    fd = lambda key, k=None: (fun(_perturb(gps, (l, c, key, k), h)) - fun(_perturb(gps, (l, c, key, k), -h))) / (2 * h)
    keys = ["variance"] + (["mean"] if c is None else []) + (["r"] if g["kind"] in PERIODIC_KINDS else [])
    keys += ["decay"] if g["kind"] == "locally_periodic" else []
    assert ("r" in G) == (g["kind"] in PERIODIC_KINDS) and ("decay" in G) == (g["kind"] == "locally_periodic"), (l, c)
    for key in keys:
        assert G[key] == pytest.approx(fd(key), rel=rel, abs=abs_), (l, c, key)
    if np.ndim(g["lengthscale"]) == 0:
        assert G["lengthscale"] == pytest.approx(fd("lengthscale"), rel=rel, abs=abs_), (l, c, "lengthscale")
    else:
        for k in range(len(g["lengthscale"])):
            assert G["lengthscale"][k] == pytest.approx(fd("lengthscale", k), rel=rel, abs=abs_), (l, c, "lengthscale", k)


def _check_grads(G, gps, fun, rel=2e-5, abs_=1e-6, h=H_FD):
    for l, g in enumerate(gps):
        _check_entry(G["gps"][l], g, fun, gps, l, None, rel, abs_, h)
        if g["kind"] == "sum":
            assert len(G["gps"][l]["terms"]) == len(g["terms"])
            for c, t in enumerate(g["terms"]):
                _check_entry(G["gps"][l]["terms"][c], t, fun, gps, l, c, rel, abs_, h)


def _grad_latents(rng, d):
    """scalar period; vector period (length d, also d = 1: folded); a sum with an outer lengthscale != 1 (d/ds0 collects the period's
    and the decay's part) of locally periodic (vector period) + Matern32; periodic + locally periodic; plain Matern52."""
    dv = d if d > 1 else None
    return [_lp(rng), _lp(rng, d=dv) if dv else _lp(rng, d=1),
            _sum(rng, [_lp(rng, d=dv, mean=False), _term(rng, "matern32")], s0=1.25),
            _sum(rng, [_lp(rng, mean=False, kind="periodic"), _lp(rng, mean=False)], s0=0.8),
            {"kind": "matern52", "variance": 0.9, "lengthscale": 1.2, "mean": 0.3}]


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_oilmm_prior(lmm, d):
    rng = np.random.default_rng(10400 + d)
    n, p = 120, 4
    x = rng.uniform(0.0, 3.0, size=(d, n)) if d > 1 else np.sort(rng.uniform(0.0, 5.0, n))
    gps = _grad_latents(rng, d)[:4]
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(xin, 0.2), y, inputs=True)
    fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    fs2 = lambda s: O.oilmm_logpdf(gps, U, S, x, s, y)
    assert G["sigma2"] == pytest.approx((fs2(0.2 + H_FD) - fs2(0.2 - H_FD)) / (2 * H_FD), rel=2e-5, abs=1e-6)
    X = _cols(x)
    gx = _cols(np.asarray(G["x"]))
    sh = (lambda A: A[0]) if d == 1 else (lambda A: A)
    for i in (0, n // 2, n - 1):
        for k in range(d):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            fd = (O.oilmm_logpdf(gps, U, S, sh(Xp), 0.2, y) - O.oilmm_logpdf(gps, U, S, sh(Xm), 0.2, y)) / (2 * H_FD)
            assert gx[k, i] == pytest.approx(fd, rel=2e-5, abs=1e-6), (i, k)


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_oilmm_predictive_two_batches(lmm, d):
    rng = np.random.default_rng(10500 + d)
    n1, n2, ns, p = 70, 50, 20, 4
    mk = (lambda k: rng.uniform(0.0, 3.0, size=(d, k))) if d > 1 else (lambda k: rng.uniform(0.0, 5.0, k))
    x1, x2, xs = mk(n1), mk(n2), mk(ns)
    gps = _grad_latents(rng, d)[:4]
    U, S = _orth(rng, p, len(gps))
    y1, y2, ys = rng.standard_normal(n1 * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    po = lmm.posterior(lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x1, p), 0.2), y1)(lmm.MOInputIsotopicByOutputs(x2, p), 0.2), y2)
    G = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.15), ys, inputs=True)

    def fun(g2, xs_=xs, x1_=x1):
        ro = O.oilmm_posterior(O.oilmm_posterior(g2, U, S, x1_, 0.2, y1), U, S, x2, 0.2, y2)
        return O.oilmm_logpdf(ro, U, S, xs_, 0.15, ys)

    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    sh = (lambda A: A[0]) if d == 1 else (lambda A: A)
    gxs, gx1 = _cols(np.asarray(G["x"])), _cols(np.asarray(G["x_train"][0]))
    for i in (0, ns // 2, ns - 1):
        for k in range(d):
            Xp, Xm = _cols(xs).copy(), _cols(xs).copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            assert gxs[k, i] == pytest.approx((fun(gps, sh(Xp)) - fun(gps, sh(Xm))) / (2 * H_FD), rel=2e-5, abs=1e-6), ("x", i, k)
            Xp, Xm = _cols(x1).copy(), _cols(x1).copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            fd = (fun(gps, xs, sh(Xp)) - fun(gps, xs, sh(Xm))) / (2 * H_FD)
            assert gx1[k, i] == pytest.approx(fd, rel=2e-5, abs=1e-6), ("x_train", i, k)


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_dense_prior_and_predictive(lmm, d):
    rng = np.random.default_rng(10600 + d)
    n, ns, p = 45, 15, 3
    mk = (lambda k: rng.uniform(0.0, 3.0, size=(d, k))) if d > 1 else (lambda k: rng.uniform(0.0, 5.0, k))
    x, xs = mk(n), mk(ns)
    gps = _grad_latents(rng, d)[1:4]
    H = rng.uniform(size=(p, len(gps)))
    y, ys = rng.standard_normal(n * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), H)
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y, inputs=True)
    fun = lambda g2, x_=x: O.ilmm_logpdf(g2, H, x_, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    X = _cols(x)
    gx = _cols(np.asarray(G["x"]))
    sh = (lambda A: A[0]) if d == 1 else (lambda A: A)
    for i in (0, n // 2, n - 1):
        for k in range(d):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            assert gx[k, i] == pytest.approx((fun(gps, sh(Xp)) - fun(gps, sh(Xm))) / (2 * H_FD), rel=2e-5, abs=1e-6), (i, k)
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    G = lmm.logpdf_and_gradient(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys)
    fun = lambda g2: O.ilmm_logpdf(O.ilmm_posterior(g2, H, x, 0.2, y), H, xs, 0.2, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)


@pytest.mark.parametrize("with_var", [True, False])
@pytest.mark.parametrize("d", [1, 3])
def test_mean_and_var_vjp(lmm, d, with_var):
    """Reference: central differences (step 1e-5) of the library's own mean_and_var, whose values test 3 pins to the oracle."""
    rng = np.random.default_rng(10700 + d)
    n, ns, p, s2 = 150, 40, 3, 0.1
    mk = (lambda k: rng.uniform(0.0, 3.0, size=(d, k))) if d > 1 else (lambda k: rng.uniform(0.0, 5.0, k))
    x, xs = mk(n), mk(ns)
    gps = _grad_latents(rng, d)[1:4]
    U, S = _orth(rng, p, len(gps))
    post = lmm.posterior(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2),
                         rng.standard_normal(n * p))
    dmean = rng.standard_normal(ns * p)
    dvar = rng.standard_normal(ns * p) if with_var else None
    got = _cols(np.asarray(lmm.mean_and_var_vjp(post(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]))

    def per_point(xv):
        mu, v = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xv, p), s2))
        return (dmean * mu + (dvar * v if with_var else 0.0)).reshape(p, ns).sum(0)

    X = _cols(xs)
    for k in range(d):
        e = 1e-5
        Xp, Xm = X.copy(), X.copy()
        Xp[k] += e; Xm[k] -= e
        sh = (lambda A: A[0].copy()) if d == 1 else (lambda A: A)
        fd = (per_point(sh(Xp)) - per_point(sh(Xm))) / (2 * e)
        np.testing.assert_allclose(got[k], fd, rtol=2e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------
# 5. fp32 mode, 6. shards, 7. handles, 8. errors
# ---------------------------------------------------------------------------------------------------
def _flat(Gl):
    v = [Gl["variance"], *np.ravel(Gl["lengthscale"]), Gl["mean"], Gl.get("r", 0.0), Gl.get("decay", 0.0)]
    for t in Gl.get("terms", []):
        v += [t["variance"], *np.ravel(t["lengthscale"]), t.get("r", 0.0), t.get("decay", 0.0)]
    return np.array(v, dtype=np.float64)


def test_f32_mode(lmm):
    rng = np.random.default_rng(10800)
    n, p = 1000, 4
    x = np.sort(rng.uniform(0.0, 20.0, n))
    gps = _mixed(rng, 1)[:4]
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    ref = O.oilmm_logpdf(gps, U, S, x, 0.1, y)
    G64 = lmm.logpdf_and_gradient(f(xin, 0.1), y)
    lmm.set_compute_dtype("f32")
    try:
        v32 = lmm.logpdf(f(xin, 0.1), y)
        G32 = lmm.logpdf_and_gradient(f(xin, 0.1), y)
    finally:
        lmm.set_compute_dtype("f64")
    print(f"locally periodic fp32 logpdf: got {v32!r} ref {ref!r} rel {abs(v32 - ref) / abs(ref):.3e}")
    assert v32 == pytest.approx(ref, rel=RTOL32)
    for l in range(len(gps)):                                   # kernel parameters: rtol 2e-3 + 1e-2 absolute (include/lmm_hip.h)
        a, b = _flat(G32["gps"][l]), _flat(G64["gps"][l])
        assert np.all(np.abs(a - b) <= 2e-3 * np.abs(b) + 1e-2), (l, a, b)


def test_latent_shards_add_up(lmm):
    rng = np.random.default_rng(10850)
    n, p = 150, 6
    x = rng.uniform(0.0, 3.0, size=(3, n))
    gps = _mixed(rng, 3)
    m = len(gps)
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    G = [lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S), shard=sh)(xin, 0.2), y, with_regulariser=False)
         for sh in (None, (0, 2), (2, m))]          # (the regulariser is not per latent)
    assert G[1]["value"] + G[2]["value"] == pytest.approx(G[0]["value"], rel=1e-12)
    for l in range(m):
        assert ("decay" in G[0]["gps"][l]) == (gps[l]["kind"] == "locally_periodic")
        np.testing.assert_allclose(_flat(G[1]["gps"][l]) + _flat(G[2]["gps"][l]), _flat(G[0]["gps"][l]), rtol=1e-9, atol=1e-12)


def test_handle_outlives_its_tag(lmm):
    rng = np.random.default_rng(10900)
    d, n, p = 2, 90, 3
    x, xs = rng.uniform(0.0, 3.0, size=(d, n)), rng.uniform(0.0, 3.0, size=(d, 25))
    gps = [_lp(rng, r=0.55, decay=0.9), _lp(rng, r=1.8, decay=3.1, d=d),
           _sum(rng, [_lp(rng, mean=False), _term(rng, "se")], s0=1.1)]
    U, S = _orth(rng, p, 3)
    y = rng.standard_normal(n * p)
    post = lmm.posterior(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    gc.collect()                                                # the mirror destroyed the tags once posterior() returned
    mu, v = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1))
    mo, vo = O.oilmm_mean_var(O.oilmm_posterior(gps, U, S, x, 0.1, y), U, S, xs, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-9, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-9)


def test_error_paths_and_untagged_defaults(lmm):
    from lmm_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(10950)
    n, p = 50, 3
    xr = rng.uniform(0.0, 3.0, size=(3, n))
    x = np.ascontiguousarray(xr.T).reshape(-1)          # d x n column-major
    U, S = _orth(rng, p, 1)
    y = rng.standard_normal(n * p)
    Uc = np.asfortranarray(U).reshape(-1, order="F")
    out = C.c_double(0.0)

    def call(arr):
        return lib.lmm_oilmm_logpdf(x.ctypes.data_as(DP), 3, n, y.ctypes.data_as(DP), p, Uc.ctypes.data_as(DP),
                                    np.ascontiguousarray(S).ctypes.data_as(DP), 1, C.c_double(0.1), arr, 0, 1, 1, C.byref(out))

    LP = L.KERNEL_LOCALLY_PERIODIC
    untagged = L.gps_array([{"kind": "locally_periodic", "lengthscale": 1.5}])
    assert untagged[0].kind == LP and call(untagged) == L.LMM_OK              # untagged: r = 1, decay = 1
    ref = O.oilmm_logpdf([{"kind": "locally_periodic", "variance": 1.0, "lengthscale": 1.5, "r": 1.0, "decay": 1.0, "mean": 0.0}],
                         U, S, xr, 0.1, y)
    assert out.value == pytest.approx(ref, rel=1e-9)
    assert call(L.gps_array([{"kind": "locally_periodic", "lengthscale": [1.0, 2.0], "r": 0.7, "decay": 2.0}])) == L.LMM_ERR_DIM
    tagged = L.gps_array([{"kind": "locally_periodic", "lengthscale": 1.5, "r": 0.7, "decay": 2.0}])
    tag = tagged[0].kind >> 8
    for kind in (0, 4, 7):                                       # a locally periodic tag on any other base kind
        tagged[0].kind = kind | (tag << 8)
        assert call(tagged) == L.LMM_ERR_ARG, kind
    rq = L.gps_array([{"kind": "rq", "lengthscale": 1.5, "alpha": 3.0}])
    rq[0].kind = LP | ((rq[0].kind >> 8) << 8)                   # an alpha tag on kind 10
    assert call(rq) == L.LMM_ERR_ARG
    per = L.gps_array([{"kind": "periodic", "lengthscale": 1.5, "r": 0.7}])
    per[0].kind = LP | ((per[0].kind >> 8) << 8)                 # a plain rho tag on kind 10
    assert call(per) == L.LMM_ERR_ARG
    for code in (6, 8, 9, 11):
        bad = L.gps_array([{"kind": "se"}])
        bad[0].kind = code
        assert call(bad) == L.LMM_ERR_UNSUPPORTED, code
