"""-m gpu: Matern12 (ExponentialKernel) and RationalQuadratic latents (include/lmm_hip.h LMM_KERNEL_MATERN12 / LMM_KERNEL_RQ) against
the CPU oracle extended inside this file: oracle.lmm_oracle.kernelmatrix is patched to evaluate "matern12" and "rq" (alpha read from
the gp dict, default 2) by direct differences, and to apply per-dimension lengthscales (as tests/test_gpu_ard.py does) for every kind.
Every oracle verb used here reaches the kernel through kernelmatrix (gp_mean_var's prior variance is kappa(0) = variance)."""
import ctypes as C
import gc
import math

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


@pytest.fixture(autouse=True)
def family_oracle(monkeypatch):
    orig = O.kernelmatrix

    def kernelmatrix(gp, x, x2=None):
        ls = gp.get("lengthscale", 1.0)
        if gp["kind"] not in ("matern12", "rq"):
            if np.ndim(ls) == 0:
                return orig(gp, x, x2)
            s = np.asarray(ls, dtype=np.float64)[:, None]
            return orig(dict(gp, lengthscale=1.0), O._as_cols(x) / s, None if x2 is None else O._as_cols(x2) / s)
        a = O._as_cols(x)
        b = a if x2 is None else O._as_cols(x2)
        s = np.asarray(ls, dtype=np.float64).reshape(-1, 1) if np.ndim(ls) else float(ls)
        a, b = a / s, b / s
        r2 = np.zeros((a.shape[1], b.shape[1]))
        for k in range(a.shape[0]):
            t = a[k][:, None] - b[k][None, :]
            r2 += t * t
        v = float(gp.get("variance", 1.0))
        if gp["kind"] == "matern12":
            return v * np.exp(-np.sqrt(r2))
        al = float(gp.get("alpha", 2.0))
        return v * np.exp(-al * np.log1p(r2 / (2.0 * al)))

    monkeypatch.setattr(O, "kernelmatrix", kernelmatrix)


def _kernel(lmm, g):
    if g["kind"] == "rq":
        return lmm.RationalQuadraticKernel(g["variance"], g["lengthscale"], alpha=g.get("alpha", 2.0))
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel, "matern12": lmm.Matern12Kernel}
    return K[g["kind"]](g["variance"], g["lengthscale"])


def _model(lmm, gps):
    return lmm.independent_mogp([lmm.GP(g["mean"], _kernel(lmm, g)) for g in gps])


def _gp(rng, kind, alpha=None, d=None):
    g = {"kind": kind, "variance": float(rng.uniform(0.6, 1.6)), "mean": float(rng.normal()),
         "lengthscale": rng.uniform(0.6, 2.5, d) if d else float(rng.uniform(0.7, 1.8))}
    if alpha is not None:
        g["alpha"] = alpha
    return g


def _mixed(rng, d=None):
    """[M12, RQ alpha = 0.5, RQ alpha = 2, RQ alpha = 50, M52, SE]"""
    return [_gp(rng, "matern12", d=d), _gp(rng, "rq", 0.5, d), _gp(rng, "rq", 2.0, d), _gp(rng, "rq", 50.0, d),
            _gp(rng, "matern52", d=d), _gp(rng, "se", d=d)]


def _orth(rng, p, m):
    U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
    return np.ascontiguousarray(U), S


def _inputs(rng, case, n):
    """d = 1 sorted (separable Matern12 path), d = 1 unsorted over > 40 lengthscales (its per-element fallback), d = 3 (the d <= 8
    tile path), d = 12 (generic tiles)."""
    if case == "d1sorted":
        return np.sort(rng.uniform(0.0, 0.02 * n, n))
    if case == "d1spread":
        return rng.uniform(0.0, 80.0, n)
    d = {"d3": 3, "d12": 12}[case]
    return rng.uniform(0.0, 3.0, size=(d, n))


def _dim(x):
    return 1 if np.ndim(x) == 1 else x.shape[0]


# ---------------------------------------------------------------------------------------------------
# 1. values: mixed latents through every Gram path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [70, 1000, 2100])
@pytest.mark.parametrize("case", ["d1sorted", "d1spread", "d3", "d12"])
def test_mixed_latents_oilmm_logpdf(lmm, case, n):
    rng = np.random.default_rng(3000 + n + len(case))
    p = 7
    x = _inputs(rng, case, n)
    gps = _mixed(rng)
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    assert got == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)


# ---------------------------------------------------------------------------------------------------
# 2. RQ latents that differ only in alpha: the batched Gram and the dense-H decoupled shortcut must keep them apart
# ---------------------------------------------------------------------------------------------------
def test_rq_alpha_is_per_latent(lmm):
    from lmm_amd import _lib as L
    lib = lmm.load()
    rng = np.random.default_rng(3100)
    n, p = 150, 3
    x = rng.uniform(0.0, 4.0, size=(2, n))
    base = {"kind": "rq", "variance": 1.1, "lengthscale": 0.9, "mean": 0.2}
    gps = [dict(base, alpha=0.5), dict(base, alpha=6.0)]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))        # one batched Gram launch for both latents
    assert lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y) == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-10)
    H = rng.uniform(size=(p, 2))
    xc = np.asfortranarray(x).ravel(order="F")

    def logpdf_ex(g):
        arr = L.gps_array(g)
        val, path = C.c_double(), C.c_int(-1)
        L.check(lib.lmm_ilmm_logpdf_ex(xc.ctypes.data_as(DP), 2, n, np.ascontiguousarray(y).ctypes.data_as(DP), p,
                                       L.Arr(L.colmajor(H)).ptr, 2, C.c_double(0.1), arr, None, 1, C.byref(path), C.byref(val)))
        return val.value, path.value
    val, path = logpdf_ex(gps)
    assert path == 0                                            # the shortcut needs one shared kernel: not taken
    assert val == pytest.approx(O.ilmm_logpdf(gps, H, x, 0.1, y), rel=1e-9)
    same = [dict(base, alpha=0.5), dict(base, alpha=0.5)]
    val, path = logpdf_ex(same)
    assert path == 1                                            # equal alphas: still taken
    assert val == pytest.approx(O.ilmm_logpdf(same, H, x, 0.1, y), rel=1e-8)


# ---------------------------------------------------------------------------------------------------
# 3. the other verbs with Matern12 and RQ latents
# ---------------------------------------------------------------------------------------------------
def test_verbs_matern12_rq(lmm):
    rng = np.random.default_rng(3200)
    d, n, n2, ns, p = 2, 140, 60, 30, 4
    x, x2, xs = (rng.uniform(0.0, 3.0, size=(d, k)) for k in (n, n2, ns))
    gps = [_gp(rng, "matern12"), _gp(rng, "rq", 0.7), _gp(rng, "rq", 3.0)]
    m = len(gps)
    U, S = _orth(rng, p, m)
    H = O.orthogonal_dense(U, S)
    y, y2, ys = rng.standard_normal(n * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    post = lmm.posterior(fx, y)
    po = O.oilmm_posterior(gps, U, S, x, 0.1, y)
    pox = post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1)
    mo, vo = O.oilmm_mean_var(po, U, S, xs, 0.1)
    mu, v = lmm.mean_and_var(pox)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    np.testing.assert_allclose(lmm.mean(pox), mo, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(lmm.marginals(pox).sigma, np.sqrt(vo), rtol=1e-8)
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
    # sequential conditioning
    po2 = lmm.posterior(post(lmm.MOInputIsotopicByOutputs(x2, p), 0.3), y2)
    ro = O.oilmm_posterior(po, U, S, x2, 0.3, y2)
    mu, v = lmm.mean_and_var(po2(lmm.MOInputIsotopicByOutputs(xs, p), 0.2))
    mo, vo = O.oilmm_mean_var(ro, U, S, xs, 0.2)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)
    # lmm_mogp_cross_cov, prior and posterior
    fm = _model(lmm, gps)
    ym = rng.standard_normal(n * m)
    xa, xb = lmm.MOInputIsotopicByOutputs(xs, m), lmm.MOInputIsotopicByOutputs(x2[:, :20], m)
    np.testing.assert_allclose(lmm.cov(fm, xa, xb), O.mogp_cross_cov(gps, xs, x2[:, :20]), rtol=1e-12, atol=1e-13)
    pm = lmm.posterior(fm(lmm.MOInputIsotopicByOutputs(x, m), 0.2), ym)
    rm = O.mogp_posterior(gps, x, 0.2, ym)
    np.testing.assert_allclose(lmm.cov(pm, xa, xb), O.mogp_cross_cov(rm, xs, x2[:, :20]), rtol=1e-8, atol=1e-10)
    # dense-H ILMM: logpdf, mean_and_cov, sequential conditioning
    Hd = rng.uniform(size=(p, m))
    fd = lmm.ILMM(_model(lmm, gps), Hd)
    fdx = fd(lmm.MOInputIsotopicByOutputs(x[:, :60], p), 0.1)
    yd = y[: 60 * p]
    assert lmm.logpdf(fdx, yd) == pytest.approx(O.ilmm_logpdf(gps, Hd, x[:, :60], 0.1, yd), rel=1e-8)
    pd = lmm.posterior(fdx, yd)
    rd = O.ilmm_posterior(gps, Hd, x[:, :60], 0.1, yd)
    xsi = lmm.MOInputIsotopicByOutputs(xs[:, :12], p)
    M, Cm = lmm.mean_and_cov(pd(xsi, 0.1))
    Mr, Cr = O.ilmm_mean_cov(rd, Hd, xs[:, :12], 0.1)
    np.testing.assert_allclose(M, Mr, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(Cm, Cr, rtol=1e-7, atol=1e-9)
    pd2 = lmm.posterior(pd(lmm.MOInputIsotopicByOutputs(x2[:, :30], p), 0.25), y2[: 30 * p])
    rd2 = O.ilmm_posterior_condition(rd, Hd, x2[:, :30], 0.25, y2[: 30 * p])
    mu, v = lmm.mean_and_var(pd2(xsi, 0.1))
    mo, vo = O.ilmm_mean_var(rd2, Hd, xs[:, :12], 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-7, atol=1e-9); np.testing.assert_allclose(v, vo, rtol=1e-7)


# ---------------------------------------------------------------------------------------------------
# 4. per-dimension lengthscales with Matern12 and RQ; the d = 1 fold keeps alpha
# ---------------------------------------------------------------------------------------------------
def test_ard_matern12_rq_and_fold(lmm):
    rng = np.random.default_rng(3300)
    n, p = 160, 3
    x = rng.uniform(0.0, 3.0, size=(3, n))
    gps = [_gp(rng, "matern12", d=3), _gp(rng, "rq", 0.8, d=3), _gp(rng, "rq", 4.0)]
    U, S = _orth(rng, p, 3)
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    assert lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y) == pytest.approx(O.oilmm_logpdf(gps, U, S, x, 0.1, y), rel=1e-9)
    Hd = rng.uniform(size=(p, 3))
    xd = x[:, :50]
    assert (lmm.logpdf(lmm.ILMM(_model(lmm, gps), Hd)(lmm.MOInputIsotopicByOutputs(xd, p), 0.1), y[: 50 * p])
            == pytest.approx(O.ilmm_logpdf(gps, Hd, xd, 0.1, y[: 50 * p]), rel=1e-8))
    # d = 1: a length-1 vector folds into the isotropic latent, alpha included
    x1 = np.sort(rng.uniform(0.0, 6.0, n))
    iso = [_gp(rng, "rq", 0.5), _gp(rng, "matern12")]
    ard = [dict(g, lengthscale=np.array([g["lengthscale"]])) for g in iso]
    U2, S2 = _orth(rng, p, 2)
    xin = lmm.MOInputIsotopicByOutputs(x1, p)
    vals = [lmm.logpdf(lmm.ILMM(_model(lmm, g), lmm.Orthogonal(U2, S2))(xin, 0.1), y) for g in (iso, ard)]
    assert vals[1] == pytest.approx(vals[0], rel=1e-12)
    assert vals[0] == pytest.approx(O.oilmm_logpdf(iso, U2, S2, x1, 0.1, y), rel=1e-9)
    other = [dict(ard[0], alpha=2.0), ard[1]]
    assert lmm.logpdf(lmm.ILMM(_model(lmm, other), lmm.Orthogonal(U2, S2))(xin, 0.1), y) != pytest.approx(vals[0], rel=1e-6)


# ---------------------------------------------------------------------------------------------------
# 5. gradients against central finite differences of the patched oracle
# ---------------------------------------------------------------------------------------------------
H_FD = 1e-6


def _fd(fun, gps, l, key, k=None):
    def at(t):
        g2 = [dict(g) for g in gps]
        if k is None:
            g2[l][key] = g2[l][key] + t
        else:
            v = np.array(g2[l][key], dtype=np.float64)
            v[k] += t
            g2[l][key] = v
        return fun(g2)
    return (at(H_FD) - at(-H_FD)) / (2 * H_FD)


def _check_grads(G, gps, fun, rel=2e-5, abs_=1e-6):
    for l, g in enumerate(gps):
        Gl = G["gps"][l]
        assert ("alpha" in Gl) == (g["kind"] == "rq"), l
        keys = ["variance", "mean"] + (["alpha"] if g["kind"] == "rq" else [])
        for key in keys:
            assert Gl[key] == pytest.approx(_fd(fun, gps, l, key), rel=rel, abs=abs_), (l, key)
        if np.ndim(g["lengthscale"]) == 0:
            assert Gl["lengthscale"] == pytest.approx(_fd(fun, gps, l, "lengthscale"), rel=rel, abs=abs_), (l, "lengthscale")
        else:
            for k in range(len(g["lengthscale"])):
                assert Gl["lengthscale"][k] == pytest.approx(_fd(fun, gps, l, "lengthscale", k), rel=rel, abs=abs_), (l, k)


def _fd_s2(fun_s2, s2):
    return (fun_s2(s2 + H_FD) - fun_s2(s2 - H_FD)) / (2 * H_FD)


@pytest.mark.parametrize("d", [1, 3])
def test_gradient_oilmm_prior(lmm, d):
    rng = np.random.default_rng(3400 + d)
    n, p = 120, 4
    x = rng.uniform(0.0, 3.0, size=(d, n)) if d > 1 else np.sort(rng.uniform(0.0, 5.0, n))
    gps = [_gp(rng, "matern12", d=d if d > 1 else None), _gp(rng, "rq", 0.6, d=d if d > 1 else None), _gp(rng, "rq", 3.0),
           _gp(rng, "matern52")]
    U, S = _orth(rng, p, len(gps))
    y = rng.standard_normal(n * p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    assert G["sigma2"] == pytest.approx(_fd_s2(lambda s: O.oilmm_logpdf(gps, U, S, x, s, y), 0.2), rel=2e-5, abs=1e-6)


def test_gradient_oilmm_predictive_two_batches(lmm):
    rng = np.random.default_rng(3500)
    d, n1, n2, ns, p = 2, 50, 40, 20, 3
    x1, x2, xs = (rng.uniform(0.0, 3.0, size=(d, k)) for k in (n1, n2, ns))
    gps = [_gp(rng, "rq", 1.5, d=d), _gp(rng, "matern12")]
    U, S = _orth(rng, p, 2)
    y1, y2, ys = rng.standard_normal(n1 * p), rng.standard_normal(n2 * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    po = lmm.posterior(lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x1, p), 0.2), y1)(lmm.MOInputIsotopicByOutputs(x2, p), 0.2), y2)
    G = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.15), ys)

    def fun(g2):
        ro = O.oilmm_posterior(O.oilmm_posterior(g2, U, S, x1, 0.2, y1), U, S, x2, 0.2, y2)
        return O.oilmm_logpdf(ro, U, S, xs, 0.15, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_grads(G, gps, fun)


def test_gradient_dense_prior_and_predictive(lmm):
    rng = np.random.default_rng(3600)
    d, n, ns, p = 3, 45, 15, 3
    x, xs = rng.uniform(0.0, 3.0, size=(d, n)), rng.uniform(0.0, 3.0, size=(d, ns))
    gps = [_gp(rng, "rq", 0.9, d=d), _gp(rng, "matern12"), _gp(rng, "rq", 2.5)]
    H = rng.uniform(size=(p, 3))
    y, ys = rng.standard_normal(n * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), H)
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    fun = lambda g2: O.ilmm_logpdf(g2, H, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)
    assert G["sigma2"] == pytest.approx(_fd_s2(lambda s: O.ilmm_logpdf(gps, H, x, s, y), 0.2), rel=2e-5, abs=1e-6)
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    G = lmm.logpdf_and_gradient(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys)
    fun = lambda g2: O.ilmm_logpdf(O.ilmm_posterior(g2, H, x, 0.2, y), H, xs, 0.2, ys)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-8)
    _check_grads(G, gps, fun)


def test_gradient_matern12_ard_coincident_inputs(lmm):
    """r = 0 between distinct points: the per-dimension Matern12 factor e^{-r}/r is guarded, the pair contributes 0."""
    rng = np.random.default_rng(3700)
    d, n, p = 3, 80, 3
    x = rng.uniform(0.0, 3.0, size=(d, n))
    x[:, 40:50] = x[:, 0:10]                                    # ten duplicated input rows
    gps = [_gp(rng, "matern12", d=d), _gp(rng, "rq", 1.2, d=d)]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.2), y)
    for Gl in G["gps"]:
        assert all(np.all(np.isfinite(v)) for v in Gl.values())
    fun = lambda g2: O.oilmm_logpdf(g2, U, S, x, 0.2, y)
    assert G["value"] == pytest.approx(fun(gps), rel=1e-9)
    _check_grads(G, gps, fun)


# ---------------------------------------------------------------------------------------------------
# 6. fp32 compute mode, handle lifetime, production shape
# ---------------------------------------------------------------------------------------------------
def test_f32_mode_matern12_rq(lmm):
    rng = np.random.default_rng(3800)
    n, p = 1000, 4
    x = np.sort(rng.uniform(0.0, 20.0, n))
    gps = [_gp(rng, "matern12"), _gp(rng, "rq", 0.7), _gp(rng, "rq", 2.0)]
    U, S = _orth(rng, p, 3)
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
    assert v32 == pytest.approx(ref, rel=RTOL32)
    for l in range(3):                                          # kernel parameters: rtol 2e-3 + 1e-2 absolute
        for key in G64["gps"][l]:
            assert G32["gps"][l][key] == pytest.approx(G64["gps"][l][key], rel=2e-3, abs=1e-2), (l, key)


def test_handle_outlives_rq_tag(lmm):
    rng = np.random.default_rng(3900)
    d, n, p = 2, 90, 3
    x, xs = rng.uniform(0.0, 3.0, size=(d, n)), rng.uniform(0.0, 3.0, size=(d, 25))
    gps = [_gp(rng, "rq", 0.4), _gp(rng, "rq", 9.0, d=d)]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    post = lmm.posterior(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y)
    gc.collect()                                                # the mirror destroyed the tags once posterior() returned
    mu, v = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, p), 0.1))
    mo, vo = O.oilmm_mean_var(O.oilmm_posterior(gps, U, S, x, 0.1, y), U, S, xs, 0.1)
    np.testing.assert_allclose(mu, mo, rtol=1e-8, atol=1e-10); np.testing.assert_allclose(v, vo, rtol=1e-8)


def _latent_lml(kappa_fn, x, t, noise):
    r = np.abs(x[:, None] - x[None, :])
    K = kappa_fn(r)
    K[np.diag_indices_from(K)] += noise
    Lc = np.linalg.cholesky(K)
    del K
    a = np.linalg.solve(Lc, t)
    return -0.5 * (a @ a) - np.sum(np.log(np.diag(Lc))) - 0.5 * len(x) * math.log(2 * math.pi)


@pytest.mark.parametrize("lead", ["matern12", "rq"])
def test_production_shape_latent0_vs_numpy_cholesky(lmm, lead):
    """configs[2]'s n = 16384 with one Matern12 and one RQ latent, d = 1 sorted: latent 0 (the `lead` kind) by hand."""
    rng = np.random.default_rng(4000)
    n, p = 16384, 4
    x = np.sort(rng.uniform(0.0, 400.0, n))
    m12 = {"kind": "matern12", "variance": 1.2, "lengthscale": 1.5, "mean": 0.0}
    rq = {"kind": "rq", "variance": 0.9, "lengthscale": 0.8, "alpha": 0.75, "mean": 0.0}
    gps = [m12, rq] if lead == "matern12" else [rq, m12]
    U, S = _orth(rng, p, 2)
    y = rng.standard_normal(n * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S), shard=(0, 1))
    got = lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, with_regulariser=False)
    T, ST = O.project_orthogonal(U, S, 0.1)
    t = (T @ y.reshape(p, n))[0]
    g = gps[0]
    if lead == "matern12":
        kap = lambda r: g["variance"] * np.exp(-r / g["lengthscale"])
    else:
        kap = lambda r: g["variance"] * (1.0 + (r / g["lengthscale"]) ** 2 / (2 * g["alpha"])) ** (-g["alpha"])
    assert got == pytest.approx(_latent_lml(kap, x, t, ST[0]), rel=1e-9)
