"""-m gpu: per-dimension (ARD) lengthscales (include/lmm_hip.h lmm_ard_*) against the CPU oracle made ARD-aware inside this file:
oracle.lmm_oracle.kernelmatrix is patched to divide coordinate k of the inputs by l_k and call the original with lengthscale 1.  Every
oracle verb used here reaches the kernel through kernelmatrix (gp_mean_var's prior variance is kappa(0) = variance for any
lengthscale)."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
KINDS = ["se", "matern32", "matern52"]


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(autouse=True)
def ard_oracle(monkeypatch):
    orig = O.kernelmatrix

    def kernelmatrix(gp, x, x2=None):
        ls = gp.get("lengthscale", 1.0)
        if np.ndim(ls) == 0:
            return orig(gp, x, x2)
        s = np.asarray(ls, dtype=np.float64)[:, None]
        g = dict(gp, lengthscale=1.0)
        return orig(g, O._as_cols(x) / s, None if x2 is None else O._as_cols(x2) / s)

    monkeypatch.setattr(O, "kernelmatrix", kernelmatrix)


def _gps(rng, d, kinds, ard):
    """ard[l]: latent l gets its own lengthscale vector (else an isotropic float)."""
    out = []
    for k, a in zip(kinds, ard):
        ls = rng.uniform(0.6, 2.5, d) if a else float(rng.uniform(0.7, 1.8))
        out.append({"kind": k, "variance": float(rng.uniform(0.6, 1.6)), "lengthscale": ls, "mean": float(rng.normal())})
    return out


def _model(lmm, gps):
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    return lmm.independent_mogp([lmm.GP(g["mean"], K[g["kind"]](g["variance"], g["lengthscale"])) for g in gps])


def _orth(rng, p, m):
    U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
    return np.ascontiguousarray(U), S


def _x(rng, d, n, hi=3.0):
    return rng.uniform(0.0, hi, size=(d, n))


# ---------------------------------------------------------------------------------------------------
# 1. values: the d <= 8 fast path of the Gram kernel (d = 2, 3) and the generic path (d = 9)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 9])
def test_ard_value_parity(lmm, d):
    rng = np.random.default_rng(700 + d)
    n, n2, ns, p, m = 150, 70, 33, 4, 3
    x, x2, xs = _x(rng, d, n), _x(rng, d, n2), _x(rng, d, ns)
    gps = _gps(rng, d, KINDS, [True, False, True])          # ARD and isotropic latents in one model
    U, S = _orth(rng, p, m)
    H = O.orthogonal_dense(U, S)
    y, y2, ys = rng.standard_normal(n * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    # OILMM logpdf, posterior + marginals
    assert lmm.logpdf(fx, y) == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)
    post = lmm.posterior(fx, y)
    po = O.oilmm_posterior(gps, U, S, x, 0.1, y)
    pox = post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1)
    mo, vo = O.oilmm_mean_var(po, U, S, xs, 0.1)
    mu, v = lmm.mean_and_var(pox)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    np.testing.assert_allclose(lmm.marginals(pox).sigma, np.sqrt(vo), rtol=1e-8)
    assert lmm.logpdf(pox, ys) == pytest.approx(O.oilmm_logpdf(po, U, S, xs, 0.1, ys), rel=1e-8)
    # rand given the normals (prior and posterior)
    jit = (1e-9, 1e-6, 1e-6)
    got = lmm.rand(np.random.default_rng(9), f(lmm.MOInputIsotopicByOutputs(xs, p), 0.1), jitters=jit)
    g2 = np.random.default_rng(9); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(gps)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + math.sqrt(0.1) * eps, rtol=1e-7, atol=1e-8)
    got = lmm.rand(np.random.default_rng(4), pox, jitters=jit)
    g2 = np.random.default_rng(4); z = g2.standard_normal(m * ns); eps = g2.standard_normal(ns * p)
    X = np.stack([O.gp_rand(g, xs, 1e-6, z[l * ns:(l + 1) * ns]) for l, g in enumerate(po)])
    np.testing.assert_allclose(got, (H @ X).reshape(-1) + math.sqrt(0.1) * eps, rtol=1e-6, atol=1e-8)
    # sequential conditioning, a second batch with its own noise
    po2 = lmm.posterior(post(lmm.MOInputIsotopicByOutputs(x2, p), 0.3), y2)
    ro = O.oilmm_posterior(po, U, S, x2, 0.3, y2)
    mu, v = lmm.mean_and_var(po2(lmm.MOInputIsotopicByOutputs(xs, p), 0.2))
    mo, vo = O.oilmm_mean_var(ro, U, S, xs, 0.2)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    # IndependentMOGP logpdf, cov(f, x, y) prior and posterior
    fm = _model(lmm, gps)
    ym = rng.standard_normal(n * m)
    assert lmm.logpdf(fm(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym) == pytest.approx(O.mogp_logpdf(gps, x, 0.2, ym), rel=1e-9)
    xa, xb = lmm.MOInputIsotopicByOutputs(xs, m), lmm.MOInputIsotopicByOutputs(x2[:, :20], m)
    np.testing.assert_allclose(lmm.cov(fm, xa, xb), O.mogp_cross_cov(gps, xs, x2[:, :20]), rtol=1e-12, atol=1e-13)
    pm = lmm.posterior(fm(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    rm = O.mogp_posterior(gps, x, 0.2, ym)
    np.testing.assert_allclose(lmm.cov(pm, xa, xb), O.mogp_cross_cov(rm, xs, x2[:, :20]), rtol=1e-8, atol=1e-10)
    # dense-H ILMM: logpdf, posterior marginals and mean_and_cov, sequential conditioning
    Hd = rng.uniform(size=(p, m))
    fd = lmm.ILMM(_model(lmm, gps), Hd)
    xin = lmm.MOInputIsotopicByOutputs(x[:, :60], p)
    yd = y[: 60 * p]
    fdx = fd(xin, 0.1)
    assert lmm.logpdf(fdx, yd) == pytest.approx(O.ilmm_logpdf(gps, Hd, x[:, :60], 0.1, yd), rel=1e-8)
    pd = lmm.posterior(fdx, yd)
    rd = O.ilmm_posterior(gps, Hd, x[:, :60], 0.1, yd)
    xsi = lmm.MOInputIsotopicByOutputs(xs[:, :12], p)
    M, Cm = lmm.mean_and_cov(pd(xsi, 0.1))
    Mr, Cr = O.ilmm_mean_cov(rd, Hd, xs[:, :12], 0.1)
    np.testing.assert_allclose(M, Mr, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(Cm, Cr, rtol=1e-7, atol=1e-9)
    mu, v = lmm.mean_and_var(pd(xsi, 0.1))
    np.testing.assert_allclose(mu, Mr, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(v, np.diag(Cr), rtol=1e-7)
    pd2 = lmm.posterior(pd(lmm.MOInputIsotopicByOutputs(x2[:, :30], p), 0.25), y2[: 30 * p])
    rd2 = O.ilmm_posterior_condition(rd, Hd, x2[:, :30], 0.25, y2[: 30 * p])
    mu, v = lmm.mean_and_var(pd2(xsi, 0.1))
    mo, vo = O.ilmm_mean_var(rd2, Hd, xs[:, :12], 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(v, vo, rtol=1e-7)


# ---------------------------------------------------------------------------------------------------
# 2. folding: all-equal factors and d = 1 are the isotropic latent
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 4])
def test_ard_folding_is_isotropic(lmm, d):
    rng = np.random.default_rng(800 + d)
    n, p, m = 130, 3, 3
    x = _x(rng, d, n)
    iso = _gps(rng, d, KINDS, [False] * m)
    ard = [dict(g, lengthscale=np.full(d, g["lengthscale"])) for g in iso]
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    xin = lmm.MOInputIsotopicByOutputs(x if d > 1 else x[0], p)
    vals = [lmm.logpdf(lmm.ILMM(_model(lmm, g), lmm.Orthogonal(U, S))(xin, 0.1), y) for g in (iso, ard)]
    assert vals[1] == pytest.approx(vals[0], rel=1e-12)
    Hd = rng.uniform(size=(p, m))
    vals = [lmm.logpdf(lmm.ILMM(_model(lmm, g), Hd)(xin, 0.1), y) for g in (iso, ard)]
    assert vals[1] == pytest.approx(vals[0], rel=1e-12)
    # the gradient of a folded latent: sum_k l_k d/dl_k = l d/dl of the isotropic latent
    G = [lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, g), lmm.Orthogonal(U, S))(xin, 0.1), y) for g in (iso, ard)]
    for l in range(m):
        gl = np.asarray(G[1]["gps"][l]["lengthscale"])
        assert gl.shape == (d,)
        assert float(np.dot(ard[l]["lengthscale"], gl)) == pytest.approx(iso[l]["lengthscale"] * G[0]["gps"][l]["lengthscale"], rel=1e-9)
        assert G[1]["gps"][l]["variance"] == pytest.approx(G[0]["gps"][l]["variance"], rel=1e-10)


# ---------------------------------------------------------------------------------------------------
# 3. production tile counts: multi-latent batched Gram launches with distinct tags
# ---------------------------------------------------------------------------------------------------
def test_ard_production_shape_latent0_vs_numpy_cholesky(lmm):
    rng = np.random.default_rng(900)
    m, p, n, d = 8, 16, 4096, 4
    x = _x(rng, d, n, hi=8.0)
    gps = [{"kind": "matern52", "variance": float(rng.uniform(0.7, 1.4)), "lengthscale": rng.uniform(0.8, 3.0, d), "mean": 0.0}
           for _ in range(m)]
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S), shard=(0, 1))
    got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, with_regulariser=False)
    # latent 0 by hand: explicit ARD Matern52 Gram, numpy Cholesky, Gaussian log density of its projected data
    T, ST = O.project_orthogonal(U, S, 0.1)
    t = (T @ y.reshape(p, n))[0]
    g = gps[0]
    xs = x / g["lengthscale"][:, None]
    r2 = np.zeros((n, n))
    for k in range(d):
        diff = xs[k][:, None] - xs[k][None, :]
        r2 += diff * diff
    r = np.sqrt(r2)
    s = math.sqrt(5.0) * r
    K = g["variance"] * (1.0 + s + 5.0 * r2 / 3.0) * np.exp(-s) + ST[0] * np.eye(n)
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L, t)
    ref = -0.5 * (a @ a) - np.sum(np.log(np.diag(L))) - 0.5 * n * math.log(2 * math.pi)
    assert got == pytest.approx(ref, rel=1e-9)
    # the whole model through all 8 latents (one batched Gram launch of 8 distinct vectors)
    fw = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    assert lmm.logpdf(fw(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y) == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-8)


# ---------------------------------------------------------------------------------------------------
# 4. gradients against central finite differences of the patched oracle
# ---------------------------------------------------------------------------------------------------
H_FD = 1e-6


def _fd_ls(fun, gps, l, k):
    def at(t):
        g2 = [dict(g) for g in gps]
        ls = np.array(g2[l]["lengthscale"], dtype=np.float64)
        ls[k] += t
        g2[l]["lengthscale"] = ls
        return fun(g2)
    return (at(H_FD) - at(-H_FD)) / (2 * H_FD)


def _check_ls_grads(G, gps, fun, d):
    for l, g in enumerate(gps):
        gl = G["gps"][l]["lengthscale"]
        if np.ndim(g["lengthscale"]) == 0:
            assert np.ndim(gl) == 0
            continue
        assert np.shape(gl) == (d,)
        for k in range(d):
            assert gl[k] == pytest.approx(_fd_ls(fun, gps, l, k), rel=2e-5, abs=1e-6), (l, k)


def _gp_arr(lib, L, gps, mult):
    """lmm_gp_t array with the ARD latents' vectors registered as factors of the multiplier `mult` (tags returned)."""
    arr = (L.GpT * len(gps))()
    tags = []
    for l, g in enumerate(gps):
        arr[l].kind = L.KERNEL_KINDS[g["kind"]]
        arr[l].variance, arr[l].mean = g["variance"], g["mean"]
        if np.ndim(g["lengthscale"]) == 0:
            arr[l].lengthscale = g["lengthscale"]
            tags.append(0)
            continue
        fac = np.ascontiguousarray(np.asarray(g["lengthscale"]) / mult)
        t = C.c_int()
        L.check(lib.lmm_ard_create(fac.size, fac.ctypes.data_as(DP), C.byref(t)))
        arr[l].kind |= t.value << 8
        arr[l].lengthscale = mult
        tags.append(t.value)
    return arr, tags


def test_ard_gradient_oilmm_prior_abi(lmm):
    """lmm_oilmm_logpdf_grad with a common multiplier != 1: lmm_ard_grad (d/d ard_k) and grad_gps.lengthscale (d/d multiplier)
    against finite differences; sum_k ard_k d/d ard_k = multiplier d/d multiplier; shard partials sum to the whole."""
    from lmm_amd import _lib as L
    lib = lmm.load()
    rng = np.random.default_rng(1100)
    d, n, p, m, mult = 3, 90, 4, 3, 1.3
    x = _x(rng, d, n)
    gps = _gps(rng, d, KINDS, [True, False, True])
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    arr, tags = _gp_arr(lib, L, gps, mult)
    xc, yc = np.asfortranarray(x).ravel(order="F"), np.ascontiguousarray(y)

    def call(l0, l1, reg):
        val = C.c_double()
        gg = (L.GpGradT * m)()
        L.check(lib.lmm_oilmm_logpdf_grad(xc.ctypes.data_as(DP), d, n, yc.ctypes.data_as(DP), p, L.Arr(L.colmajor(U)).ptr,
                                          L.Arr(S).ptr, m, C.c_double(0.2), arr, l0, l1, int(reg), C.byref(val), None, None, None,
                                          None, gg))
        out = {}
        for l in (0, 2):
            g = np.zeros(d)
            L.check(lib.lmm_ard_grad(tags[l], g.ctypes.data_as(DP)))
            out[l] = g
        return val.value, gg, out

    try:
        val, gg, ga = call(0, m, True)
        assert val == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.2, y), rel=1e-9)
        fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
        for l in (0, 2):
            for k in range(d):
                # d/d ard_k = mult * d/d l_k
                assert ga[l][k] == pytest.approx(mult * _fd_ls(fun, gps, l, k), rel=2e-5, abs=1e-6), (l, k)
            fac = np.asarray(gps[l]["lengthscale"]) / mult

            def at(t, l=l, fac=fac):
                g2 = [dict(g) for g in gps]
                g2[l]["lengthscale"] = (mult + t) * fac
                return fun(g2)
            assert gg[l].lengthscale == pytest.approx((at(H_FD) - at(-H_FD)) / (2 * H_FD), rel=2e-5, abs=1e-6)
            assert float(np.dot(fac, ga[l])) == pytest.approx(mult * gg[l].lengthscale, rel=1e-9)
        # shard partials sum to the full-model gradient
        parts = [call(0, 2, True), call(2, 3, False)]
        for l in (0, 2):
            np.testing.assert_allclose(parts[0][2][l] + parts[1][2][l], ga[l], rtol=1e-9, atol=1e-12)
        # grad_gps NULL: the tags' gradients read zeros
        val2 = C.c_double()
        L.check(lib.lmm_oilmm_logpdf_grad(xc.ctypes.data_as(DP), d, n, yc.ctypes.data_as(DP), p, L.Arr(L.colmajor(U)).ptr,
                                          L.Arr(S).ptr, m, C.c_double(0.2), arr, 0, m, 1, C.byref(val2), None, None, None, None, None))
        g = np.ones(d)
        L.check(lib.lmm_ard_grad(tags[0], g.ctypes.data_as(DP)))
        assert np.array_equal(g, np.zeros(d))
    finally:
        for t in tags:
            if t:
                lib.lmm_ard_destroy(t)


def test_ard_gradient_oilmm_predictive_two_batches(lmm):
    rng = np.random.default_rng(1200)
    d, n1, n2, ns, p, m = 3, 50, 40, 20, 3, 2
    x1, x2, xs = _x(rng, d, n1), _x(rng, d, n2), _x(rng, d, ns)
    gps = _gps(rng, d, ["matern52", "se"], [True, True])
    U, S = _orth(rng, p, m)
    y1, y2, ys = rng.standard_normal(n1 * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    po = lmm.posterior(lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x1, p), 0.2), y1)(lmm.MOInputIsotopicByOutputs(x2, p), 0.2), y2)
    G = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.15), ys)

    def fun(g2):
        ro = O.oilmm_posterior(O.oilmm_posterior(g2, U, S, x1, 0.2, y1), U, S, x2, 0.2, y2)
        return O.oilmm_logpdf(ro, U, S, xs, 0.15, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_ls_grads(G, gps, fun, d)


def test_ard_gradient_dense_prior_and_predictive(lmm):
    rng = np.random.default_rng(1300)
    d, n, ns, p, m = 4, 45, 15, 3, 2
    x, xs = _x(rng, d, n), _x(rng, d, ns)
    gps = _gps(rng, d, ["matern32", "matern52"], [True, False])
    H = rng.uniform(size=(p, m))
    y, ys = rng.standard_normal(n * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), H)
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    fun = lambda g2: O.ilmm_logpdf(g2, H, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_ls_grads(G, gps, fun, d)
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    G = lmm.logpdf_and_gradient(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys)
    fun = lambda g2: O.ilmm_logpdf(O.ilmm_posterior(g2, H, x, 0.2, y), H, xs, 0.2, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_ls_grads(G, gps, fun, d)


@pytest.mark.parametrize("d", [6, 12])
def test_ard_gradient_wide_inputs(lmm, d):
    """The 4 < d <= 8 and 8 < d <= 32 instantiations of the ARD gradient reduction (d = 3, 4 above take the d <= 4 one), OILMM prior
    and IndependentMOGP, against finite differences."""
    rng = np.random.default_rng(1500 + d)
    n, p, m = 90, 3, 2
    x = _x(rng, d, n)
    gps = _gps(rng, d, ["matern52", "se"], [True, True])
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_ls_grads(G, gps, fun, d)
    ym = rng.standard_normal(n * m)
    G = lmm.logpdf_and_gradient(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    fun = lambda g2: O.mogp_logpdf(g2, x, 0.2, ym)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_ls_grads(G, gps, fun, d)


# ---------------------------------------------------------------------------------------------------
# 5. errors and handle lifetime
# ---------------------------------------------------------------------------------------------------
def test_ard_errors_and_handle_outlives_tags(lmm):
    from lmm_amd import _lib as L
    lib = lmm.load()
    rng = np.random.default_rng(1400)
    d, n, p, m = 3, 60, 3, 2
    x = _x(rng, d, n)
    U, S = _orth(rng, p, m)
    y = rng.standard_normal(n * p)
    gps = _gps(rng, d, ["se", "matern32"], [True, True])
    xc = np.asfortranarray(x).ravel(order="F")
    val = C.c_double()

    def mogp_logpdf(arr):
        return lib.lmm_mogp_logpdf(xc.ctypes.data_as(DP), d, n, np.ascontiguousarray(y[: n * m]).ctypes.data_as(DP), m,
                                   C.c_double(0.1), arr, 0, m, C.byref(val))
    # a tag of the wrong d: LMM_ERR_DIM, the message naming the latent (the Python mirror raises RuntimeError)
    bad = [dict(g) for g in gps]
    bad[1]["lengthscale"] = np.array([1.0, 2.0])
    arr, tags = _gp_arr(lib, L, bad, 1.0)
    try:
        assert mogp_logpdf(arr) == L.LMM_ERR_DIM
        assert "latent 1" in lib.lmm_last_error_string().decode()
    finally:
        for t in tags:
            lib.lmm_ard_destroy(t)
    with pytest.raises(RuntimeError, match="latent 1"):
        lmm.logpdf(lmm.ILMM(_model(lmm, bad), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    # a destroyed tag is refused (LMM_ERR_ARG)
    arr, tags = _gp_arr(lib, L, gps, 1.0)
    for t in tags:
        assert lib.lmm_ard_destroy(t) == L.LMM_OK
    assert mogp_logpdf(arr) == L.LMM_ERR_ARG
    # a posterior handle keeps its own lengthscales: the Python mirror's tags are gone once posterior() returns
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    gc.collect()
    xs = _x(rng, d, 25)
    mu, v = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1))
    mo, vo = O.oilmm_mean_var(O.oilmm_posterior(gps, U, S, x, 0.1, y), U, S, xs, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
