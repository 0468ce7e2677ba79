"""-m gpu: gradients of logpdf with respect to the input locations (include/lmm_hip.h lmm_*_grad_x; logpdf_and_gradient(inputs=True)).
References: central finite differences of the CPU oracle, and the analytic formula
    d logpdf / d x_ik = -(1 / l_k^2) sum_{j != i} w_ij h(r_ij) (x_ik - x_jk),   w = alpha alpha' - K^-1,
evaluated in NumPy from np.linalg.inv.  The oracle's kernelmatrix is extended inside this file to Matern12, RQ and per-dimension
lengthscales (direct differences), so every kind reaches the finite differences."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def _r2(a, b, ls):
    a, b = O._as_cols(a), O._as_cols(b)
    s = np.asarray(ls, dtype=np.float64).reshape(-1, 1) if np.ndim(ls) else float(ls)
    a, b = a / s, b / s
    r2 = np.zeros((a.shape[1], b.shape[1]))
    for k in range(a.shape[0]):
        t = a[k][:, None] - b[k][None, :]
        r2 += t * t
    return r2


def _kappa_h(g, r2):
    """kappa(r) and h(r) (d kappa / d x_ik = -h t_k / l_k) of a latent; Matern12's h is 0 at r = 0 (the library's convention)."""
    v, kind = float(g["variance"]), g["kind"]
    r = np.sqrt(r2)
    if kind == "se":
        k = v * np.exp(-0.5 * r2); return k, k
    if kind == "matern32":
        s = np.sqrt(3.0) * r; e = np.exp(-s); return v * (1 + s) * e, 3.0 * v * e
    if kind == "matern52":
        s = np.sqrt(5.0) * r; e = np.exp(-s); return v * (1 + s + 5.0 / 3.0 * r2) * e, 5.0 / 3.0 * v * (1 + s) * e
    if kind == "matern12":
        k = v * np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(r2 > 0, k / np.where(r2 > 0, r, 1.0), 0.0)
        return k, h
    al = float(g.get("alpha", 2.0))
    u = r2 / (2.0 * al)
    k = v * np.exp(-al * np.log1p(u))
    return k, k / (1.0 + u)


@pytest.fixture(autouse=True)
def family_oracle(monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", lambda gp, x, x2=None: _kappa_h(gp, _r2(x, x if x2 is None else x2, gp.get("lengthscale", 1.0)))[0])


def _kernel(lmm, g):
    if g["kind"] == "rq":
        return lmm.RationalQuadraticKernel(g["variance"], g["lengthscale"], alpha=g.get("alpha", 2.0))
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel, "matern12": lmm.Matern12Kernel}
    return K[g["kind"]](g["variance"], g["lengthscale"])


def _model(lmm, gps):
    return lmm.independent_mogp([lmm.GP(g["mean"], _kernel(lmm, g)) for g in gps])


def _gp(rng, kind, d=None, alpha=None):
    g = {"kind": kind, "variance": float(rng.uniform(0.6, 1.6)), "mean": float(rng.normal()),
         "lengthscale": rng.uniform(0.6, 2.5, d) if d else float(rng.uniform(0.7, 1.8))}
    if alpha is not None:
        g["alpha"] = alpha
    return g


def _mixed(rng, d=None):
    return [_gp(rng, "se", d), _gp(rng, "matern32", d), _gp(rng, "matern52", d), _gp(rng, "matern12", d), _gp(rng, "rq", d, 0.7)]


def _orth(rng, p, m):
    U, S, _ = np.linalg.svd(rng.uniform(size=(p, m)), full_matrices=False)
    return np.ascontiguousarray(U), np.linspace(2.0, 1.0, m)


def _inputs(rng, d, n, scale=4.0):
    """d = 1: unsorted points at least 0.02 apart (finite differences of Matern12 must not step across a neighbour)."""
    if d == 1:
        return rng.permutation(np.cumsum(rng.uniform(0.02, 0.06, n))) * (scale / 4.0)
    return rng.uniform(0.0, scale, size=(d, n))


def _fd_x(F, x, h=1e-5):
    """Central differences of F with respect to every coordinate of x ((n,) or (d, n))."""
    g = np.zeros_like(x)
    for idx in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h; xm[idx] -= h
        g[idx] = (F(xp) - F(xm)) / (2 * h)
    return g


def _close(got, ref, rtol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * np.abs(ref).max())


def _host_grad_x(g, x, noise, z):
    """The analytic input gradient of one latent's logpdf at projected data z with (scalar or per-point) noise, from np.linalg.inv."""
    X = O._as_cols(x)
    ls = g["lengthscale"]
    r2 = _r2(X, X, ls)
    K, Hm = _kappa_h(g, r2)
    K = K + np.diag(np.broadcast_to(noise, (X.shape[1],)))
    Ki = np.linalg.inv(K)
    a = Ki @ (z - g["mean"])
    WH = (np.outer(a, a) - Ki) * Hm
    np.fill_diagonal(WH, 0.0)
    il2 = (1.0 / np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[0],)) ** 2)[:, None]
    return -il2 * (X * WH.sum(axis=1)[None, :] - X @ WH)      # (d, n)


# ---------------------------------------------------------------------------------------------------
# 1. prior OILMM and IndependentMOGP against finite differences of the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 130])
@pytest.mark.parametrize("d,ard", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("model", ["oilmm", "mogp"])
def test_prior_input_gradient_vs_finite_differences(lmm, model, d, ard, n):
    rng = np.random.default_rng(7000 + 10 * n + d + 2 * ard + (model == "mogp"))
    gps = _mixed(rng, d if ard else None)
    m = len(gps)
    x = _inputs(rng, d, n)
    if model == "oilmm":
        p = m + 2
        U, S = _orth(rng, p, m)
        f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
        F = lambda xx: O.oilmm_logpdf(gps, U, S, xx, 0.1, y)
    else:
        p = m
        f = _model(lmm, gps)
        F = lambda xx: O.mogp_logpdf(gps, xx, 0.1, y)
    y = rng.standard_normal(n * p)
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, inputs=True)
    assert G["x"].shape == x.shape and isinstance(G["x"], np.ndarray)
    _close(G["x"], _fd_x(F, x), 1e-5)


# the 4 < d <= 8 and d > 8 instantiations of grad_x_kernel (d = 1 and d <= 4 are above): the same comparison, same tolerance
@pytest.mark.parametrize("d,ard", [(6, False), (12, True)])
def test_prior_input_gradient_wide_inputs(lmm, d, ard):
    test_prior_input_gradient_vs_finite_differences(lmm, "oilmm", d, ard, 37)


# ---------------------------------------------------------------------------------------------------
# 2. analytic host reference at size: 47 ragged tiles (3 chunks), and 128 tiles (8 chunks) on one latent
# ---------------------------------------------------------------------------------------------------
def test_input_gradient_analytic_n3000(lmm):
    rng = np.random.default_rng(7100)
    n, d, p = 3000, 4, 3
    gps = [_gp(rng, "matern52", d), _gp(rng, "rq", d, 1.5)]
    U, S = _orth(rng, p, 2)
    x = _inputs(rng, d, n, 10.0)
    y = rng.standard_normal(n * p)
    G = lmm.logpdf_and_gradient(lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, inputs=True)
    T, ST = O.project_orthogonal(U, S, 0.1)
    Ty = T @ y.reshape(p, n)
    ref = sum(_host_grad_x(g, x, ST[l], Ty[l]) for l, g in enumerate(gps))
    assert np.linalg.norm(G["x"] - ref) <= 1e-8 * np.linalg.norm(ref)


def test_input_gradient_analytic_multichunk_latent0(lmm):
    rng = np.random.default_rng(7101)
    n, d = 8192, 2
    g = _gp(rng, "matern32", d)
    x = _inputs(rng, d, n, 30.0)
    y = rng.standard_normal(n)
    G = lmm.logpdf_and_gradient(_model(lmm, [g])(lmm.MOInputIsotopicByOutputs(x, 1), 0.1), y, inputs=True)
    ref = _host_grad_x(g, x, 0.1, y)
    assert np.linalg.norm(G["x"] - ref) <= 1e-8 * np.linalg.norm(ref)


# ---------------------------------------------------------------------------------------------------
# 3. translation invariance at configs[2]'s n: the gradients sum to 0 over the points (prior) and over train + test (predictive)
# ---------------------------------------------------------------------------------------------------
def test_translation_invariance_large(lmm):
    import torch
    rng = np.random.default_rng(7200)
    n, m, d, p = 16384, 2, 2, 3
    gps = [_gp(rng, "matern52"), _gp(rng, "se", d)]
    U, S = _orth(rng, p, m)
    x = torch.tensor(_inputs(rng, d, n, 200.0), device="cuda")
    y = torch.tensor(rng.standard_normal(n * p), device="cuda")
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    G = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, p), 0.1), y, inputs=True)
    gx = G["x"]
    assert torch.is_tensor(gx) and gx.is_cuda and tuple(gx.shape) == (d, n)
    gx = gx.cpu().numpy()
    assert np.all(np.isfinite(gx)) and np.abs(gx).sum() > 0
    assert np.all(np.abs(gx.sum(axis=1)) <= 1e-9 * np.abs(gx).sum(axis=1))
    nt = 12000
    post = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x[:, :nt], p), 0.1), y.reshape(p, n)[:, :nt].reshape(-1))
    ys = y.reshape(p, n)[:, nt:].reshape(-1)
    P = lmm.logpdf_and_gradient(post(lmm.MOInputIsotopicByOutputs(x[:, nt:], p), 0.2), ys, inputs=True)
    gs, gt = P["x"].cpu().numpy(), P["x_train"].cpu().numpy()
    assert gs.shape == (d, n - nt) and gt.shape == (d, nt)
    tot = np.abs(gs).sum(axis=1) + np.abs(gt).sum(axis=1)
    assert np.all(np.abs(gs.sum(axis=1) + gt.sum(axis=1)) <= 1e-9 * tot)


# ---------------------------------------------------------------------------------------------------
# 4. predictive OILMM: one batch, and two batches with different noise
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,noises", [((40,), (0.1,)), ((30, 25), (0.3, 0.12))])
def test_predictive_oilmm_input_gradient(lmm, sizes, noises):
    rng = np.random.default_rng(7300 + len(sizes))
    d, ns, p = 2, 20, 4
    gps = [_gp(rng, "matern52"), _gp(rng, "matern12", d), _gp(rng, "rq", None, 2.0)]
    m = len(gps)
    U, S = _orth(rng, p, m)
    xb = [_inputs(rng, d, nb) for nb in sizes]
    yb = [rng.standard_normal(nb * p) for nb in sizes]
    xs = _inputs(rng, d, ns)
    ys = rng.standard_normal(ns * p)

    def F(xbs=xb, xss=xs):
        po = O.oilmm_posterior(gps, U, S, xbs[0], noises[0], yb[0])
        for x_, s_, y_ in zip(xbs[1:], noises[1:], yb[1:]):
            po = O.oilmm_posterior(po, U, S, x_, s_, y_)
        return O.oilmm_logpdf(po, U, S, xss, 0.2, ys)

    po = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    for x_, s_, y_ in zip(xb, noises, yb):
        po = lmm.posterior(po(lmm.MOInputIsotopicByOutputs(x_, p), s_), y_)
    G = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys, inputs=True)
    assert G["value"] == pytest.approx(F(), rel=1e-8)
    _close(G["x"], _fd_x(lambda z: F(xss=z), xs), 1e-5)
    xtr = G["x_train"] if len(sizes) > 1 else [G["x_train"]]
    assert len(xtr) == len(sizes)
    for b in range(len(sizes)):
        def Fb(z, b=b):
            xx = list(xb); xx[b] = z
            return F(xbs=xx)
        _close(xtr[b], _fd_x(Fb, xb[b]), 1e-5)


# ---------------------------------------------------------------------------------------------------
# 5. dense H: prior, predictive, and the latent view of a dense-H posterior
# ---------------------------------------------------------------------------------------------------
def test_dense_h_input_gradient(lmm):
    rng = np.random.default_rng(7400)
    d, n, ns, p = 2, 30, 12, 3
    gps = [_gp(rng, "matern32", d), _gp(rng, "rq", None, 0.8)]
    m = len(gps)
    H = rng.uniform(0.2, 1.0, size=(p, m))
    x, xs = _inputs(rng, d, n), _inputs(rng, d, ns)
    y, ys, zs = rng.standard_normal(n * p), rng.standard_normal(ns * p), rng.standard_normal(ns * m)
    f = lmm.ILMM(_model(lmm, gps), H)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    G = lmm.logpdf_and_gradient(fx, y, inputs=True)
    _close(G["x"], _fd_x(lambda z: O.ilmm_logpdf(gps, H, z, 0.1, y), x), 1e-5)
    po = lmm.posterior(fx, y)
    P = lmm.logpdf_and_gradient(po(lmm.MOInputIsotopicByOutputs(xs, p), 0.2), ys, inputs=True)
    Fp = lambda xt, xq: O.ilmm_logpdf(O.ilmm_posterior(gps, H, xt, 0.1, y), H, xq, 0.2, ys)
    _close(P["x"], _fd_x(lambda z: Fp(x, z), xs), 1e-5)
    _close(P["x_train"], _fd_x(lambda z: Fp(z, xs), x), 1e-5)

    def Fl(xt, xq):
        mo, Co = O._ilmm_latent_joint(O.ilmm_posterior(gps, H, xt, 0.1, y), xq)
        return O.gaussian_logpdf(mo, Co + 0.07 * np.eye(m * ns), zs)
    Lg = lmm.logpdf_and_gradient(lmm.get_latent_gp(po)(lmm.MOInputIsotopicByOutputs(xs, m), 0.07), zs, inputs=True)
    _close(Lg["x"], _fd_x(lambda z: Fl(x, z), xs), 1e-5)
    _close(Lg["x_train"], _fd_x(lambda z: Fl(z, xs), x), 1e-5)


# ---------------------------------------------------------------------------------------------------
# 6. shards add up; 7. nothing changes when the input gradient is not asked for
# ---------------------------------------------------------------------------------------------------
def test_shards_sum_to_whole(lmm):
    rng = np.random.default_rng(7500)
    d, n, p = 3, 300, 7
    gps = _mixed(rng)
    m = len(gps)
    U, S = _orth(rng, p, m)
    x, y = _inputs(rng, d, n), rng.standard_normal(n * p)
    fx = lambda sh: lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S), shard=sh)(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    whole = lmm.logpdf_and_gradient(fx(None), y, inputs=True)["x"]
    parts = [lmm.logpdf_and_gradient(fx(sh), y, inputs=True)["x"] for sh in [(0, 2), (2, m)]]
    assert np.linalg.norm(parts[0] + parts[1] - whole) <= 1e-12 * np.linalg.norm(whole)


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + "/" + k)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{path}[{i}]")
    else:
        u, v = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert np.all(np.abs(u - v) <= 1e-12 * np.maximum(np.abs(v), np.abs(v).max() if v.size else 0)), path


def test_other_outputs_unchanged(lmm):
    from lmm_amd import _lib as L
    rng = np.random.default_rng(7600)
    d, n, ns, p = 2, 120, 30, 4
    gps = [_gp(rng, "se", d), _gp(rng, "matern12"), _gp(rng, "rq", None, 3.0)]
    m = len(gps)
    U, S = _orth(rng, p, m)
    x, xs, y, ys = _inputs(rng, d, n), _inputs(rng, d, ns), rng.standard_normal(n * p), rng.standard_normal(ns * p)
    f = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    pox = lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(xs, p), 0.2)
    H = rng.uniform(0.2, 1.0, size=(p, m))
    fd = lmm.ILMM(_model(lmm, gps), H)(lmm.MOInputIsotopicByOutputs(x[:, :40], p), 0.1)
    for fxx, yy in [(fx, y), (pox, ys), (fd, y[:40 * p])]:
        a = lmm.logpdf_and_gradient(fxx, yy, inputs=True)
        b = lmm.logpdf_and_gradient(fxx, yy)
        assert "x" in a and "x" not in b and "x_train" not in b
        a.pop("x"); a.pop("x_train", None)
        _same(a, b)
    # the _x entry point with grad_x = NULL is the old entry point
    lib = lmm.load()
    xc = np.ascontiguousarray(x.T).ravel()
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    outs = []
    for fn, extra in [(lib.lmm_oilmm_logpdf_grad, ()), (lib.lmm_oilmm_logpdf_grad_x, (None,))]:
        val, gs2 = C.c_double(), C.c_double()
        gy, gS, gU, gg, ga = np.empty(n * p), np.empty(m), np.empty(p * m), (L.GpGradT * m)(), L.gps_array([dict(g) for g in gps])
        L.check(fn(L.Arr(xc).ptr, d, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(0.1), ga, 0, m, 1, C.byref(val),
                   L.Arr(gy, True).ptr, C.byref(gs2), L.Arr(gS, True).ptr, L.Arr(gU, True).ptr, gg, *extra))
        outs.append([val.value, gs2.value, gy, gS, gU, [(g.variance, g.lengthscale, g.mean) for g in gg]])
    _same(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------
# 8. fp32 compute mode; 9. Matern12 at coincident points; 10. the dimension limit
# ---------------------------------------------------------------------------------------------------
def test_f32_input_gradient(lmm):
    rng = np.random.default_rng(7700)
    n, p, d = 900, 5, 2
    gps = [_gp(rng, "se"), _gp(rng, "matern32"), _gp(rng, "matern52", d)]
    U, S = _orth(rng, p, 3)
    x, y = _inputs(rng, d, n, 30.0), rng.standard_normal(n * p)
    fx = lmm.ILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    R = lmm.logpdf_and_gradient(fx, y, inputs=True)["x"]
    lmm.set_compute_dtype("f32")
    try:
        G = lmm.logpdf_and_gradient(fx, y, inputs=True)["x"]
    finally:
        lmm.set_compute_dtype("f64")
    np.testing.assert_allclose(G, R, rtol=2e-3, atol=1e-2)


@pytest.mark.parametrize("d", [1, 2])
def test_matern12_coincident_points(lmm, d):
    rng = np.random.default_rng(7800 + d)
    n = 90
    x = _inputs(rng, d, n)
    x[..., 10:20] = x[..., 0:10]              # duplicated points
    x[..., 40] = x[..., 41]
    g = _gp(rng, "matern12")
    y = rng.standard_normal(n)
    G = lmm.logpdf_and_gradient(_model(lmm, [g])(lmm.MOInputIsotopicByOutputs(x, 1), 0.1), y, inputs=True)["x"]
    assert np.all(np.isfinite(G))
    ref = _host_grad_x(g, x, 0.1, y)
    _close(G, ref.reshape(G.shape), 1e-9)


def test_dimension_limit(lmm):
    rng = np.random.default_rng(7900)
    n, p, d = 50, 2, 33
    x, y = _inputs(rng, d, n), rng.standard_normal(n * p)
    fx = _model(lmm, [_gp(rng, "se"), _gp(rng, "matern52")])(lmm.MOInputIsotopicByOutputs(x, p), 0.1)
    with pytest.raises(NotImplementedError):
        lmm.logpdf_and_gradient(fx, y, inputs=True)
    G = lmm.logpdf_and_gradient(fx, y)
    assert "x" not in G and np.isfinite(G["value"])
