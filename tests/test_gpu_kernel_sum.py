"""-m gpu: sum latents (KernelFunctions' KernelSum; include/lmm_hip.h LMM_KERNEL_SUM) against identities that need no reference and
against the CPU oracle extended inside this file: oracle.lmm_oracle.kernelmatrix is patched to evaluate a "sum" descriptor as
v0 * sum of its terms' Grams (each term per kind -- Matern12 and RQ by direct differences -- with its lengthscale s0 * l_c, per
dimension for a vector), and gp_mean_var's prior variance is taken from that kernel at r = 0.  The dense-H oracle reaches the kernel
through kernelmatrix too."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
RTOL32 = 2e-4          # fp32 OILMM logpdf (include/lmm_hip.h, tests/test_gpu_f32.py)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def _base_gram(g, a, b):
    """One base kernel (any kind, scalar or per-dimension lengthscale) between the column sets a and b."""
    ls = g.get("lengthscale", 1.0)
    s = np.asarray(ls, dtype=np.float64).reshape(-1, 1) if np.ndim(ls) else float(ls)
    a, b = a / s, b / s
    r2 = np.zeros((a.shape[1], b.shape[1]))
    for k in range(a.shape[0]):
        t = a[k][:, None] - b[k][None, :]
        r2 += t * t
    v = float(g.get("variance", 1.0))
    if g["kind"] == "matern12":
        return v * np.exp(-np.sqrt(r2))
    if g["kind"] == "rq":
        al = float(g.get("alpha", 2.0))
        return v * np.exp(-al * np.log1p(r2 / (2.0 * al)))
    return O.kernel_eval(g["kind"], v, 1.0, np.sqrt(r2))


@pytest.fixture(autouse=True)
def sum_oracle(monkeypatch):
    def kernelmatrix(gp, x, x2=None):
        a = O._as_cols(x)
        b = a if x2 is None else O._as_cols(x2)
        if gp["kind"] != "sum":
            return _base_gram(gp, a, b)
        s0 = float(gp.get("lengthscale", 1.0))
        K = sum(_base_gram(dict(t, lengthscale=s0 * np.asarray(t["lengthscale"], dtype=np.float64)), a, b) for t in gp["terms"])
        return float(gp.get("variance", 1.0)) * K

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
    if t["kind"] == "rq":
        return lmm.RationalQuadraticKernel(t["variance"], t["lengthscale"], alpha=t.get("alpha", 2.0))
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel, "matern12": lmm.Matern12Kernel}
    return K[t["kind"]](t["variance"], t["lengthscale"])


def _kernel(lmm, g):
    if g["kind"] == "sum":
        return lmm.KernelSum(*[_base_kernel(lmm, t) for t in g["terms"]], variance=g["variance"], lengthscale=g["lengthscale"])
    return _base_kernel(lmm, g)


def _model(lmm, gps):
    return lmm.independent_mogp([lmm.GP(g["mean"], _kernel(lmm, g)) for g in gps])


def _term(rng, kind, alpha=None, d=None):
    t = {"kind": kind, "variance": float(rng.uniform(0.4, 1.2)),
         "lengthscale": rng.uniform(0.6, 2.0, d) if d else float(rng.uniform(0.5, 2.0))}
    if alpha is not None:
        t["alpha"] = alpha
    return t


def _sum(rng, terms, mean=None):
    return {"kind": "sum", "variance": float(rng.uniform(0.7, 1.5)), "lengthscale": float(rng.uniform(0.7, 1.4)),
            "mean": float(rng.normal()) if mean is None else mean, "terms": terms}


def _plain(rng, kind):
    return {"kind": kind, "variance": float(rng.uniform(0.6, 1.6)), "lengthscale": float(rng.uniform(0.7, 1.8)),
            "mean": float(rng.normal())}


def _mixed(rng, d):
    """plain Matern52; Matern52 + SE; an ARD-term sum (d > 1); an RQ-term 3-term sum; a 4-term sum."""
    dv = d if d > 1 else None
    return [_plain(rng, "matern52"),
            _sum(rng, [_term(rng, "matern52"), _term(rng, "se")]),
            _sum(rng, [_term(rng, "se", d=dv), _term(rng, "matern12")]),
            _sum(rng, [_term(rng, "rq", 0.7), _term(rng, "matern32"), _term(rng, "rq", 4.0, d=dv)]),
            _sum(rng, [_term(rng, "se"), _term(rng, "matern12"), _term(rng, "matern32"), _term(rng, "matern52")])]


def _orth(rng, p, m):
    U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
    return np.ascontiguousarray(U), S


def _inputs(rng, case, n):
    if case == "d1sorted":
        return np.sort(rng.uniform(0.0, 0.02 * n, n))
    if case == "d1spread":
        return rng.uniform(0.0, 30.0, n)
    return rng.uniform(0.0, 3.0, size=(3, n))


def _dim(x):
    return 1 if np.ndim(x) == 1 else x.shape[0]


def _cols(x):
    return x.reshape(1, -1) if np.ndim(x) == 1 else x


# ---------------------------------------------------------------------------------------------------
# 1. identities that need no oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_sum_of_equal_se_terms_is_one_se(lmm, d):
    rng = np.random.default_rng(7100 + d)
    n, p = 300, 3
    x = np.sort(rng.uniform(0.0, 8.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (d, n))
    a, b, ls = 0.7, 0.45, 1.3
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    fs = lmm.independent_mogp([lmm.GP(0.3, lmm.SEKernel(a, ls) + lmm.SEKernel(b, ls)), lmm.GP(lmm.Matern52Kernel(0.8, 0.9))])
    fp = lmm.independent_mogp([lmm.GP(0.3, lmm.SEKernel(a + b, ls)), lmm.GP(lmm.Matern52Kernel(0.8, 0.9))])
    Gs = lmm.logpdf_and_gradient(lmm.ILMM(fs, lmm.Orthogonal(U, S))(xin, 0.2), y)
    Gp = lmm.logpdf_and_gradient(lmm.ILMM(fp, lmm.Orthogonal(U, S))(xin, 0.2), y)
    assert Gs["value"] == pytest.approx(Gp["value"], rel=1e-12)
    ts = Gs["gps"][0]["terms"]
    gv = Gp["gps"][0]["variance"]
    assert ts[0]["variance"] == pytest.approx(gv, rel=1e-10) and ts[1]["variance"] == pytest.approx(gv, rel=1e-10)
    # outer variance v0 = 1: d/dv0 = a d/da + b d/db = (a + b) d/dv;  outer lengthscale s0 = 1: d/ds0 = ls d/dls
    assert Gs["gps"][0]["variance"] == pytest.approx((a + b) * gv, rel=1e-10)
    assert ts[0]["lengthscale"] + ts[1]["lengthscale"] == pytest.approx(Gp["gps"][0]["lengthscale"], rel=1e-10)
    assert Gs["gps"][0]["lengthscale"] == pytest.approx(ls * Gp["gps"][0]["lengthscale"], rel=1e-10)
    assert Gs["gps"][0]["mean"] == pytest.approx(Gp["gps"][0]["mean"], rel=1e-10)
    np.testing.assert_allclose(Gs["S"], Gp["S"], rtol=1e-10)
    assert Gs["gps"][1]["variance"] == pytest.approx(Gp["gps"][1]["variance"], rel=1e-10)


@pytest.mark.parametrize("d", [1, 3])
def test_one_term_sum_is_the_plain_latent(lmm, d):
    rng = np.random.default_rng(7200 + d)
    n, p = 250, 4
    x = np.sort(rng.uniform(0.0, 8.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (d, n))
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    fs = lmm.independent_mogp([lmm.GP(0.1, lmm.KernelSum(lmm.SEKernel(0.9, 1.1))), lmm.GP(lmm.SEKernel(1.2, 0.7))])
    fp = lmm.independent_mogp([lmm.GP(0.1, lmm.SEKernel(0.9, 1.1)), lmm.GP(lmm.SEKernel(1.2, 0.7))])
    vs = lmm.logpdf(lmm.ILMM(fs, lmm.Orthogonal(U, S))(xin, 0.1), y)
    vp = lmm.logpdf(lmm.ILMM(fp, lmm.Orthogonal(U, S))(xin, 0.1), y)
    assert vs == pytest.approx(vp, rel=1e-12)


# ---------------------------------------------------------------------------------------------------
# 2. values against the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [70, 2100])
@pytest.mark.parametrize("case", ["d1sorted", "d1spread", "d3"])
def test_mixed_latents_oilmm_and_mogp_logpdf(lmm, case, n):
    rng = np.random.default_rng(7300 + n + len(case))
    p = 6
    x = _inputs(rng, case, n)
    gps = _mixed(rng, _dim(x))
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    assert got == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)
    m = len(gps)
    ym = rng.standard_normal(n * m)
    got = lmm.logpdf(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    assert got == pytest.approx(O.mogp_logpdf(gps, x, 0.2, ym), rel=1e-9)


def test_verbs_with_sum_latents(lmm):
    rng = np.random.default_rng(7400)
    d, n, n2, ns, p = 3, 150, 70, 33, 4
    x, x2, xs = (rng.uniform(0.0, 3.0, size=(d, k)) for k in (n, n2, ns))
    gps = _mixed(rng, d)[1:4]
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
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    np.testing.assert_allclose(lmm.mean(pox), mo, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(lmm.marginals(pox).sigma, np.sqrt(vo), rtol=1e-8)
    # prior marginals: kappa(0) = v0 sum v_c
    mo0, vo0 = O.oilmm_mean_var(gps, U, S, xs, 0.1)
    mu0, v0 = lmm.mean_and_var(f(lmm.MOInputIsotopicByOutputs(xs, p), 0.1))
    np.testing.assert_allclose(mu0, mo0, rtol=1e-10, atol=1e-12); np.testing.assert_allclose(v0, vo0, rtol=1e-10)
    # rand given the normals (prior and posterior)
    jit = (1e-9, 1e-6, 1e-6)
    got = lmm.rand(np.random.default_rng(9), f(lmm.MOInputIsotopicByOutputs(xs, p), 0.1), jitters=jit)
    g2 = np.random.default_rng(9); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(gps)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + np.sqrt(0.1) * eps, rtol=1e-7, atol=1e-8)
    got = lmm.rand(np.random.default_rng(4), pox, jitters=jit)
    g2 = np.random.default_rng(4); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(po)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + np.sqrt(0.1) * eps, rtol=1e-6, atol=1e-8)
    # sequential conditioning
    po2 = lmm.posterior(post(lmm.MOInputIsotopicByOutputs(x2, p), 0.3), y2)
    ro = O.oilmm_posterior(po, U, S, x2, 0.3, y2)
    mu, v = lmm.mean_and_var(po2(lmm.MOInputIsotopicByOutputs(xs, p), 0.2))
    mo, vo = O.oilmm_mean_var(ro, U, S, xs, 0.2)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    # IndependentMOGP posterior and its covariance
    ym = rng.standard_normal(n * m)
    pm = lmm.posterior(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    rm = O.mogp_posterior(gps, x, 0.2, ym)
    xsm = lmm.MOInputIsotopicByOutputs(xs, m)
    mu, v = lmm.mean_and_var(pm(xsm, 0.2))
    mo, vo = O.mogp_mean_var(rm, xs)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo + 0.2, rtol=1e-8)
    np.testing.assert_allclose(lmm.cov(_model(lmm, gps), xsm), O.mogp_cov(gps, xs), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("case", ["d1spread", "d3"])
def test_dense_h_with_sum_latents(lmm, case):
    rng = np.random.default_rng(7450 + len(case))
    n, n2, ns, p = 70, 30, 17, 4
    x, x2, xs = _inputs(rng, case, n), _inputs(rng, case, n2), _inputs(rng, case, ns)
    gps = _mixed(rng, _dim(x))[:4]
    H = rng.uniform(size=(p, len(gps)))
    y, y2 = rng.standard_normal(n * p), rng.standard_normal(n2 * p)
    f = lmm.ILMM(_model(lmm, gps), H)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    assert lmm.logpdf(fx, y) == pytest.approx(O.ilmm_logpdf(gps, H, x, 0.1, y), rel=1e-9)
    post = lmm.posterior(fx, y)
    rd = O.ilmm_posterior(gps, H, x, 0.1, y)
    xsi = lmm.MOInputIsotopicByOutputs(xs, p)
    mu, v = lmm.mean_and_var(post(xsi, 0.1))
    mo, vo = O.ilmm_mean_var(rd, H, xs, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(v, vo, rtol=1e-7)
    M, Cm = lmm.mean_and_cov(post(xsi, 0.1))
    Mr, Cr = O.ilmm_mean_cov(rd, H, xs, 0.1)
    np.testing.assert_allclose(M, Mr, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(Cm, Cr, rtol=1e-7, atol=1e-9)
    mu0, v0 = lmm.mean_and_var(f(xsi, 0.1))                     # prior: kappa(0) = v0 sum_c v_c
    mo0, vo0 = O.ilmm_mean_var(gps, H, xs, 0.1)
    np.testing.assert_allclose(mu0, mo0, rtol=1e-9, atol=1e-11); np.testing.assert_allclose(v0, vo0, rtol=1e-9)
    post2 = lmm.posterior(post(lmm.MOInputIsotopicByOutputs(x2, p), 0.25), y2)
    rd2 = O.ilmm_posterior_condition(rd, H, x2, 0.25, y2)
    mu, v = lmm.mean_and_var(post2(xsi, 0.1))
    mo, vo = O.ilmm_mean_var(rd2, H, xs, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(v, vo, rtol=1e-7)


def test_dense_h_decoupled_shortcut_compares_terms(lmm):
    from lmm_amd import model as Mdl
    rng = np.random.default_rng(7460)
    n, p = 60, 4
    x = rng.uniform(0.0, 6.0, n)
    same = _sum(rng, [_term(rng, "matern52"), _term(rng, "rq", 0.8)], mean=0.2)
    other = dict(same, terms=[same["terms"][0], dict(same["terms"][1], alpha=3.0)])      # differs in one term's alpha only
    H = rng.uniform(size=(p, 3))
    y = rng.standard_normal(n * p)
    for gps, path in (([same, dict(same), dict(same)], "decoupled"), ([same, other, dict(same)], "dense")):
        f = lmm.ILMM(_model(lmm, gps), H)
        got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
        assert Mdl.ILMM_LAST_PATH == path
        assert got == pytest.approx(O.ilmm_logpdf(gps, H, x, 0.1, y), rel=1e-9)


# ---------------------------------------------------------------------------------------------------
# 3. gradients against central finite differences of the patched oracle
# ---------------------------------------------------------------------------------------------------
H_FD = 1e-6


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


def _fd(fun, gps, path, h=H_FD):
    return (fun(_perturb(gps, path, h)) - fun(_perturb(gps, path, -h))) / (2 * h)


def _check_grads(G, gps, fun, rel=2e-5, abs_=1e-6, h=H_FD):
    _fd_h = lambda fun_, gps_, path: _fd(fun_, gps_, path, h)
    for l, g in enumerate(gps):
        Gl = G["gps"][l]
        for key in ("variance", "lengthscale", "mean"):
            assert Gl[key] == pytest.approx(_fd_h(fun, gps, (l, None, key, None)), rel=rel, abs=abs_), (l, key)
        if g["kind"] != "sum":
            continue
        assert len(Gl["terms"]) == len(g["terms"])
        for c, t in enumerate(g["terms"]):
            Gt = Gl["terms"][c]
            assert ("alpha" in Gt) == ("alpha" in t), (l, c)
            assert Gt["variance"] == pytest.approx(_fd_h(fun, gps, (l, c, "variance", None)), rel=rel, abs=abs_), (l, c, "variance")
            if "alpha" in t:
                assert Gt["alpha"] == pytest.approx(_fd_h(fun, gps, (l, c, "alpha", None)), rel=rel, abs=abs_), (l, c, "alpha")
            if np.ndim(t["lengthscale"]) == 0:
                assert Gt["lengthscale"] == pytest.approx(_fd_h(fun, gps, (l, c, "lengthscale", None)), rel=rel, abs=abs_), (l, c)
            else:
                for k in range(len(t["lengthscale"])):
                    assert Gt["lengthscale"][k] == pytest.approx(_fd_h(fun, gps, (l, c, "lengthscale", k)), rel=rel, abs=abs_), (l, c, k)


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_oilmm_prior(lmm, d):
    rng = np.random.default_rng(7500 + d)
    n, p = 120, 7
    x = rng.uniform(0.0, 3.0, size=(d, n)) if d > 1 else np.sort(rng.uniform(0.0, 5.0, n))
    gps = _mixed(rng, d)
    if d == 1:                          # a term with a length-1 lengthscale vector: folded into the isotropic term
        gps.append(_sum(rng, [_term(rng, "se", d=1), _term(rng, "matern12")]))
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(xin, 0.2), y, inputs=True)
    fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    fs2 = lambda s: O.oilmm_logpdf(gps, U, S, x, s, y)
    assert G["sigma2"] == pytest.approx((fs2(0.2 + H_FD) - fs2(0.2 - H_FD)) / (2 * H_FD), rel=2e-5, abs=1e-6)
    # d logpdf / d x at a few points
    X = _cols(x)
    gx = _cols(np.asarray(G["x"]))
    for i in (0, n // 2, n - 1):
        for k in range(d):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            sh = (lambda A: A[0]) if d == 1 else (lambda A: A)
            fd = (O.oilmm_logpdf(gps, U, S, sh(Xp), 0.2, y) - O.oilmm_logpdf(gps, U, S, sh(Xm), 0.2, y)) / (2 * H_FD)
            assert gx[k, i] == pytest.approx(fd, rel=2e-5, abs=1e-6), (i, k)


def test_gradient_oilmm_predictive_two_batches(lmm):
    rng = np.random.default_rng(7600)
    d, n1, n2, ns, p = 2, 50, 40, 20, 4
    x1, x2, xs = (rng.uniform(0.0, 3.0, size=(d, k)) for k in (n1, n2, ns))
    gps = _mixed(rng, d)[1:4]
    U, S = _orth(rng, p, len(gps))
    y1, y2, ys = rng.standard_normal(n1 * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    po = lmm.posterior(lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x1, p), 0.2), y1)(lmm.MOInputIsotopicByOutputs(x2, p), 0.2), y2)
    G = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.15), ys, inputs=True)

    def fun(g2, xs_=xs):
        ro = O.oilmm_posterior(O.oilmm_posterior(g2, U, S, x1, 0.2, y1), U, S, x2, 0.2, y2)
        return O.oilmm_logpdf(ro, U, S, xs_, 0.15, ys)

    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_grads(G, gps, fun, rel=5e-5)
    for i in (0, ns - 1):
        for k in range(d):
            Xp, Xm = xs.copy(), xs.copy()
            Xp[k, i] += H_FD; Xm[k, i] -= H_FD
            fd = (fun(gps, Xp) - fun(gps, Xm)) / (2 * H_FD)
            assert np.asarray(G["x"])[k, i] == pytest.approx(fd, rel=5e-5, abs=1e-6), (i, k)


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_dense_prior_and_predictive(lmm, d):
    rng = np.random.default_rng(7650 + d)
    n, ns, p = 45, 15, 3
    x = rng.uniform(0.0, 3.0, size=(d, n)) if d > 1 else rng.uniform(0.0, 5.0, n)
    xs = rng.uniform(0.0, 3.0, size=(d, ns)) if d > 1 else rng.uniform(0.0, 5.0, ns)
    dv = d if d > 1 else 1
    gps = [_sum(rng, [_term(rng, "se", d=dv), _term(rng, "rq", 0.9)]), _plain(rng, "matern32"),
           _sum(rng, [_term(rng, "matern52"), _term(rng, "matern12")])]
    H = rng.uniform(size=(p, len(gps)))
    y, ys = rng.standard_normal(n * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), H)
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y, inputs=True)
    fun = lambda g2: O.ilmm_logpdf(g2, H, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    h = 1e-4            # the dense oracle's logpdf carries ~1e-10 absolute rounding: a 1e-6 step leaves ~1e-4 noise in the difference
    _check_grads(G, gps, fun, h=h)
    X = _cols(x)
    gx = _cols(np.asarray(G["x"]))
    sh = (lambda A: A[0]) if d == 1 else (lambda A: A)
    for i in (0, n - 1):
        for k in range(d):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, i] += h; Xm[k, i] -= h
            fd = (O.ilmm_logpdf(gps, H, sh(Xp), 0.2, y) - O.ilmm_logpdf(gps, H, sh(Xm), 0.2, y)) / (2 * h)
            assert gx[k, i] == pytest.approx(fd, rel=2e-5, abs=1e-6), (i, k)
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    G = lmm.logpdf_and_gradient(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys)
    fun = lambda g2: O.ilmm_logpdf(O.ilmm_posterior(g2, H, x, 0.2, y), H, xs, 0.2, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_grads(G, gps, fun, h=h)


@pytest.mark.parametrize("d", [1, 3])
def test_mean_and_var_vjp(lmm, d):
    rng = np.random.default_rng(7700 + d)
    n, ns, p, s2 = 150, 40, 3, 0.1
    x = rng.uniform(0.0, 3.0, size=(d, n)) if d > 1 else rng.uniform(0.0, 5.0, n)
    xs = rng.uniform(0.0, 3.0, size=(d, ns)) if d > 1 else rng.uniform(0.0, 5.0, ns)
    gps = _mixed(rng, d)[1:4]
    U, S = _orth(rng, p, len(gps))
    post = lmm.posterior(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2),
                         rng.standard_normal(n * p))
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    got = _cols(np.asarray(lmm.mean_and_var_vjp(post(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]))

    def per_point(xv):
        mu, v = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xv, p), s2))
        return (dmean * mu + dvar * v).reshape(p, ns).sum(0)

    X = _cols(xs)
    for k in range(d):
        e = 1e-5
        Xp, Xm = X.copy(), X.copy()
        Xp[k] += e; Xm[k] -= e
        sh = (lambda A: A[0].copy()) if d == 1 else (lambda A: A)
        fd = (per_point(sh(Xp)) - per_point(sh(Xm))) / (2 * e)
        assert np.abs(got[k] - fd).max() <= 1e-6 * max(np.abs(fd).max(), 1.0), k


# ---------------------------------------------------------------------------------------------------
# 4. shards, fp32, determinism, error paths
# ---------------------------------------------------------------------------------------------------
def _logpdf_shard(lmm, x, y, U, S, gps, s2, l0, l1, reg=1):
    from lmm_amd import _lib as L
    lib = L.load()
    arr = L.gps_array(gps)
    X = np.ascontiguousarray(_cols(x).T).reshape(-1)        # d x n column-major
    p, m = U.shape
    out = C.c_double(0.0)
    Uc, Sc = np.asfortranarray(U).reshape(-1, order="F"), np.ascontiguousarray(S)
    rc = lib.lmm_oilmm_logpdf(X.ctypes.data_as(DP), _dim(x), X.size // _dim(x), y.ctypes.data_as(DP), p, Uc.ctypes.data_as(DP),
                              Sc.ctypes.data_as(DP), m, C.c_double(s2), arr, l0, l1, reg, C.byref(out))
    return rc, out.value, arr


def test_latent_shards_add_up(lmm):
    rng = np.random.default_rng(7800)
    n, p = 200, 6
    x = rng.uniform(0.0, 3.0, size=(3, n))
    gps = _mixed(rng, 3)
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    rc, whole, _ = _logpdf_shard(lmm, x, y, U, S, gps, 0.1, 0, len(gps), reg=0)     # (the regulariser is not per latent)
    assert rc == 0
    rc1, a, _ = _logpdf_shard(lmm, x, y, U, S, gps, 0.1, 0, 2, reg=0)
    rc2, b, _ = _logpdf_shard(lmm, x, y, U, S, gps, 0.1, 2, len(gps), reg=0)
    assert rc1 == 0 and rc2 == 0
    assert a + b == pytest.approx(whole, rel=1e-12)


def test_latent_shard_gradients_add_up(lmm):
    rng = np.random.default_rng(7850)
    n, p = 150, 6
    x = rng.uniform(0.0, 3.0, size=(3, n))
    gps = _mixed(rng, 3)
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    G = [lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S), shard=sh)(xin, 0.2), y)
         for sh in (None, (0, 2), (2, len(gps)))]

    def flat(Gl):
        v = [Gl["variance"], Gl["lengthscale"], Gl["mean"]]
        for t in Gl.get("terms", []):
            v += [t["variance"], *np.ravel(t["lengthscale"]), t.get("alpha", 0.0)]
        return np.array(v, dtype=np.float64)

    for l in range(len(gps)):
        np.testing.assert_allclose(flat(G[1]["gps"][l]) + flat(G[2]["gps"][l]), flat(G[0]["gps"][l]), rtol=1e-9, atol=1e-12)


def test_f32_logpdf(lmm):
    rng = np.random.default_rng(7900)
    n, p = 600, 5
    x = np.sort(rng.uniform(0.0, 12.0, n))
    gps = _mixed(rng, 1)
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    ref = O.oilmm_logpdf(gps, U, S, x, 0.1, y)
    lmm.set_compute_dtype("f32")
    try:
        got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    finally:
        lmm.set_compute_dtype("f64")
    assert got == pytest.approx(ref, rel=RTOL32)


_DET_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import lmm_amd as lmm
lmm.init(0)
rng = np.random.default_rng(8000)
n, p = 700, 5
x = rng.uniform(0.0, 3.0, size=(3, n))
ks = [lmm.Matern52Kernel(0.9, 1.1), lmm.KernelSum(lmm.SEKernel(0.5, np.array([1.0, 2.0, 0.7])), lmm.Matern12Kernel(0.4, 0.8)),
      lmm.RationalQuadraticKernel(0.3, 1.2, alpha=0.7) + lmm.Matern32Kernel(0.6, 0.5)]
U, S, _ = np.linalg.svd(rng.uniform(size=(p, 3)), full_matrices=False)
y = rng.standard_normal(n * p)
f = lmm.ILMM(lmm.independent_mogp([lmm.GP(0.2, k) for k in ks]), lmm.Orthogonal(np.ascontiguousarray(U), S))
out = []
for _ in range(2):
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, inputs=True)
    v = [G["value"], G["sigma2"]] + list(np.ravel(G["x"]))
    for g in G["gps"]:
        v += [g["variance"], g["lengthscale"], g["mean"]]
        for t in g.get("terms", []):
            v += [t["variance"]] + list(np.ravel(t["lengthscale"])) + [t.get("alpha", 0.0)]
    out.append(np.array(v, dtype=np.float64).tobytes().hex())
print("SAME" if out[0] == out[1] else "DIFFERENT")
"""


def test_deterministic_calls_are_bitwise_equal(lmm):
    """Two identical gradient calls with LMM_DETERMINISTIC=1 (read once per process: a fresh child process) are bitwise equal."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LMM_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", _DET_SCRIPT, root], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "SAME"


def test_error_paths(lmm):
    from lmm_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(8100)
    n, p = 50, 3
    x = rng.uniform(0.0, 3.0, size=(3, n))
    gps = [_sum(rng, [_term(rng, "se", d=3), _term(rng, "matern12")]), _plain(rng, "se")]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    rc, val, arr = _logpdf_shard(lmm, x, y, U, S, gps, 0.1, 0, 2)
    assert rc == 0 and val == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)
    # a term ARD tag of the wrong d
    bad = [dict(gps[0], terms=[_term(rng, "se", d=2), gps[0]["terms"][1]]), gps[1]]
    rc, _, _ = _logpdf_shard(lmm, x, y, U, S, bad, 0.1, 0, 2)
    assert rc == L.LMM_ERR_DIM
    # a destroyed term tag: the sum tag stays live
    term_tag = arr.ard.terms[0].tags[0]
    assert lib.lmm_ard_destroy(term_tag) == 0
    X = np.ascontiguousarray(x.T).reshape(-1)
    Uc = np.asfortranarray(U).reshape(-1, order="F")
    out = C.c_double(0.0)
    rc = lib.lmm_oilmm_logpdf(X.ctypes.data_as(DP), 3, n, y.ctypes.data_as(DP), p, Uc.ctypes.data_as(DP),
                              np.ascontiguousarray(S).ctypes.data_as(DP), 2, C.c_double(0.1), arr, 0, 2, 1, C.byref(out))
    assert rc == L.LMM_ERR_ARG
    assert b"latent 0" in lib.lmm_last_error_string()
