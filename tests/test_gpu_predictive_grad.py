"""-m gpu: gradients of the predictive marginals with respect to the test inputs (include/lmm_hip.h lmm_oilmm_mean_and_var_grad_xs;
lmm_amd.mean_and_var_vjp).  References: central finite differences of the library's own mean_and_var, and the analytic formula
    d/d xs_sk = -(1 / l_k) sum_j (mbar_s alpha_j - 2 vbar_s W[s, j]) h(r_sj) t_k,   W = K(xs, x) K^-1,  t_k = (xs_sk - x_jk) / l_k,
evaluated in NumPy from a Cholesky factorisation of each latent's noisy training Gram."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu
KINDS = ["se", "matern32", "matern52", "matern12", "rq"]


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def _cols(x):
    return np.asarray(x, dtype=np.float64).reshape(1, -1) if np.ndim(x) == 1 else np.asarray(x, dtype=np.float64)


def _kappa_h(g, r2):
    """kappa(r) and h(r) (d kappa / d xs_k = -h t_k / l_k); Matern12's h is 0 at r = 0 (the library's convention)."""
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
        h = np.where(r2 > 0, k / np.where(r2 > 0, r, 1.0), 0.0)
        return k, h
    al = float(g.get("alpha", 2.0))
    u = r2 / (2.0 * al)
    k = v * np.exp(-al * np.log1p(u))
    return k, k / (1.0 + u)


def _scaled_diffs(g, a, b):
    """t[k] = (a_k - b_k) / l_k for every pair (difference first) and r^2."""
    a, b = _cols(a), _cols(b)
    ls = np.broadcast_to(np.asarray(g["lengthscale"], dtype=np.float64), (a.shape[0],))
    t = np.stack([(a[k][:, None] - b[k][None, :]) / ls[k] for k in range(a.shape[0])])
    return t, (t * t).sum(0), ls


def _latent_ref(g, x, noise, yl, xs, mbar, vbar):
    """d/d xs (d x ns) of sum_s mbar_s mean(xs_s) + vbar_s var(xs_s) for one posterior latent (data yl, noise variance `noise`)."""
    _, r2 = _scaled_diffs(g, x, x)[:2]
    K = _kappa_h(g, r2)[0] + noise * np.eye(r2.shape[0])
    cf = cho_factor(K, lower=True)
    solve = lambda B: cho_solve(cf, B)
    alpha = solve(yl - g["mean"])
    t, r2s, ls = _scaled_diffs(g, xs, x)
    Kx, h = _kappa_h(g, r2s)
    c = mbar[:, None] * alpha[None, :]
    if vbar is not None:
        c = c - 2.0 * vbar[:, None] * solve(Kx.T).T
    return np.stack([-(c * h * t[k]).sum(1) / ls[k] for k in range(t.shape[0])])


def _kernel(lmm, g):
    if g["kind"] == "rq":
        return lmm.RationalQuadraticKernel(g["variance"], g["lengthscale"], alpha=g.get("alpha", 2.0))
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel, "matern12": lmm.Matern12Kernel}
    return K[g["kind"]](g["variance"], g["lengthscale"])


def _model(lmm, gps):
    return lmm.independent_mogp([lmm.GP(g["mean"], _kernel(lmm, g)) for g in gps])


def _gp(rng, kind, d=None):
    g = {"kind": kind, "variance": float(rng.uniform(0.6, 1.6)), "mean": float(rng.normal()),
         "lengthscale": rng.uniform(0.6, 2.5, d) if d else float(rng.uniform(0.7, 1.8))}
    if kind == "rq":
        g["alpha"] = 0.7
    return g


def _inputs(rng, n, d):
    return rng.uniform(0.0, 6.0, n) if d == 1 else rng.uniform(0.0, 4.0, (d, n))


def _orth(rng, p, m):
    U, _, _ = np.linalg.svd(rng.uniform(0.0, 1.0, (p, m)), full_matrices=False)
    return np.ascontiguousarray(U), np.linspace(2.0, 1.0, m)


def _oilmm_post(lmm, gps, U, S, x, s2, y, shard=None):
    p = U.shape[0]
    kw = {} if shard is None else {"shard": shard}
    f = lmm.OILMM(_model(lmm, gps), lmm.Orthogonal(U, S), **kw)
    return lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, p), s2), y)


def _oilmm_ref(gps, U, S, x, s2, y, xs, dmean, dvar):
    n, ns, p = _cols(x).shape[1], _cols(xs).shape[1], U.shape[0]
    T, ST = O.project_orthogonal(U, S, s2)
    Ty = T @ y.reshape(p, n)
    H = U * np.sqrt(S)[None, :]
    mbar = H.T @ dmean.reshape(p, ns)
    vbar = None if dvar is None else (H * H).T @ dvar.reshape(p, ns)
    return sum(_latent_ref(g, x, ST[l], Ty[l], xs, mbar[l], None if vbar is None else vbar[l]) for l, g in enumerate(gps))


def _flat(g):
    return np.asarray(g, dtype=np.float64).reshape(-1, np.asarray(g).shape[-1]) if np.ndim(g) > 1 else np.asarray(g).reshape(1, -1)


def _close(a, b, rtol):
    a, b = _flat(a), _flat(b)
    scale = np.abs(b).max()
    assert np.all(np.isfinite(a))
    assert np.abs(a - b).max() <= rtol * scale, (np.abs(a - b).max(), scale)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_finite_differences(lmm, kind, d):
    rng = np.random.default_rng(11 + KINDS.index(kind) + 7 * d)
    n, ns, p, m, s2 = 200, 50, 3, 2, 0.1
    gps = [_gp(rng, kind, d if d > 1 else None) for _ in range(m)]
    U, S = _orth(rng, p, m)
    x, xs = _inputs(rng, n, d), _inputs(rng, ns, d)
    po = _oilmm_post(lmm, gps, U, S, x, s2, rng.standard_normal(n * p))
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    got = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)
    assert got["x"].shape == np.shape(xs)
    assert got["sigma2"] == pytest.approx(dvar.sum(), rel=1e-12)

    def per_point(xv):                      # each test point's output depends on its own input only
        mu, v = lmm.mean_and_var(po(lmm.MOInputIsotopicByOutputs(xv, p), s2))
        return (dmean * mu + dvar * v).reshape(p, ns).sum(0)

    fd = np.zeros((d, ns))
    X = _cols(xs)
    for k in range(d):
        eps = 1e-5 * max(1.0, np.abs(X[k]).max())
        Xp, Xm = X.copy(), X.copy()
        Xp[k] += eps; Xm[k] -= eps
        shape = lambda A: A[0].copy() if d == 1 else A
        fd[k] = (per_point(shape(Xp)) - per_point(shape(Xm))) / (2 * eps)
    _close(got["x"], fd if d > 1 else fd[0], 1e-6)


@pytest.mark.parametrize("d", [1, 3])
def test_analytic_oilmm_n1000(lmm, d):
    rng = np.random.default_rng(5 + d)
    n, ns, p, s2 = 1000, 77, 4, 0.05
    gps = [_gp(rng, k, d if d > 1 else None) for k in ["matern52", "se", "rq"]]
    U, S = _orth(rng, p, len(gps))
    x, xs, y = _inputs(rng, n, d), _inputs(rng, ns, d), rng.standard_normal(n * p)
    po = _oilmm_post(lmm, gps, U, S, x, s2, y)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    got = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]
    _close(got, _oilmm_ref(gps, U, S, x, s2, y, xs, dmean, dvar), 1e-9)
    got_m = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean)["x"]
    _close(got_m, _oilmm_ref(gps, U, S, x, s2, y, xs, dmean, None), 1e-9)


# the 4 < d <= 8 and d > 8 instantiations of pred_grad_x_kernel, with and without the variance cotangent: the analytic reference and
# tolerance of test_analytic_oilmm_n1000 at n = 130, ns = 70
@pytest.mark.parametrize("d", [6, 12])
def test_analytic_oilmm_wide_inputs(lmm, d):
    rng = np.random.default_rng(50 + d)
    n, ns, p, s2 = 130, 70, 4, 0.05
    gps = [_gp(rng, k, d) for k in ["matern52", "se", "rq"]]
    U, S = _orth(rng, p, len(gps))
    x, xs, y = _inputs(rng, n, d), _inputs(rng, ns, d), rng.standard_normal(n * p)
    fx = _oilmm_post(lmm, gps, U, S, x, s2, y)(lmm.MOInputIsotopicByOutputs(xs, p), s2)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    _close(lmm.mean_and_var_vjp(fx, dmean, dvar)["x"], _oilmm_ref(gps, U, S, x, s2, y, xs, dmean, dvar), 1e-9)
    _close(lmm.mean_and_var_vjp(fx, dmean)["x"], _oilmm_ref(gps, U, S, x, s2, y, xs, dmean, None), 1e-9)


def test_analytic_mogp_n8192_deep_recursion(lmm):
    rng = np.random.default_rng(3)
    n, ns, m, s2 = 8192, 1024, 2, 0.1
    gps = [_gp(rng, "matern52"), _gp(rng, "se")]
    x, xs, y = rng.uniform(0.0, 40.0, n), rng.uniform(0.0, 40.0, ns), rng.standard_normal(n * m)
    f = _model(lmm, gps)
    po = lmm.posterior(f(lmm.MOInputIsotopicByOutputs(x, m), s2), y)
    dmean, dvar = rng.standard_normal(ns * m), rng.standard_normal(ns * m)
    got = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, m), s2), dmean, dvar)
    ref = sum(_latent_ref(g, x, s2, y.reshape(m, n)[l], xs, dmean.reshape(m, ns)[l], dvar.reshape(m, ns)[l]) for l, g in enumerate(gps))
    _close(got["x"], ref[0], 1e-9)
    assert got["sigma2"] == pytest.approx(dvar.sum(), rel=1e-12)


def test_mean_only_equals_zero_dvar(lmm):
    rng = np.random.default_rng(21)
    n, ns, p, s2 = 300, 90, 3, 0.1
    gps = [_gp(rng, k, 2) for k in ["matern32", "matern12"]]
    U, S = _orth(rng, p, 2)
    x, xs = _inputs(rng, n, 2), _inputs(rng, ns, 2)
    po = _oilmm_post(lmm, gps, U, S, x, s2, rng.standard_normal(n * p))
    fx = po(lmm.MOInputIsotopicByOutputs(xs, p), s2)
    dmean = rng.standard_normal(ns * p)
    a = lmm.mean_and_var_vjp(fx, dmean)
    b = lmm.mean_and_var_vjp(fx, dmean, np.zeros(ns * p))
    _close(a["x"], b["x"], 1e-12)
    assert a["sigma2"] == 0.0 and b["sigma2"] == 0.0
    z = lmm.mean_and_var_vjp(fx)
    assert np.array_equal(z["x"], np.zeros_like(z["x"]))


def test_priors_give_zeros(lmm):
    rng = np.random.default_rng(4)
    ns, p, m, s2 = 40, 3, 2, 0.2
    gps = [_gp(rng, "se"), _gp(rng, "rq")]
    xs = _inputs(rng, ns, 1)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    U, S = _orth(rng, p, m)
    priors = [lmm.OILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(xs, p), s2),
              lmm.ILMM(_model(lmm, gps), rng.uniform(0.0, 1.0, (p, m)))(lmm.MOInputIsotopicByOutputs(xs, p), s2)]
    for fx in priors:
        g = lmm.mean_and_var_vjp(fx, dmean, dvar)
        assert np.array_equal(g["x"], np.zeros(ns)) and g["sigma2"] == pytest.approx(dvar.sum())
    gm = lmm.mean_and_var_vjp(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(xs, m), s2), dmean[:ns * m], dvar[:ns * m])
    assert np.array_equal(gm["x"], np.zeros(ns))


def test_sequential_conditioning(lmm):
    rng = np.random.default_rng(8)
    n1, n2, ns, p, s2 = 150, 130, 60, 3, 0.1
    gps = [_gp(rng, "matern52", 2), _gp(rng, "se", 2)]
    U, S = _orth(rng, p, 2)
    x1, x2, xs = _inputs(rng, n1, 2), _inputs(rng, n2, 2), _inputs(rng, ns, 2)
    y1, y2 = rng.standard_normal(n1 * p), rng.standard_normal(n2 * p)
    po1 = _oilmm_post(lmm, gps, U, S, x1, s2, y1)
    po2 = lmm.posterior(po1(lmm.MOInputIsotopicByOutputs(x2, p), s2), y2)
    x12 = np.concatenate([x1, x2], axis=1)
    y12 = np.concatenate([y1.reshape(p, n1), y2.reshape(p, n2)], axis=1).reshape(-1)
    po12 = _oilmm_post(lmm, gps, U, S, x12, s2, y12)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    a = lmm.mean_and_var_vjp(po2(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]
    b = lmm.mean_and_var_vjp(po12(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]
    _close(a, b, 1e-9)


def test_mogp_by_outputs_and_features(lmm):
    rng = np.random.default_rng(9)
    n, ns, m, s2 = 400, 70, 3, 0.1
    gps = [_gp(rng, k, 2) for k in ["se", "matern12", "rq"]]
    x, xs, y = _inputs(rng, n, 2), _inputs(rng, ns, 2), rng.standard_normal(n * m)
    po = lmm.posterior(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(x, m), s2), y)
    dmean, dvar = rng.standard_normal(ns * m), rng.standard_normal(ns * m)
    ref = sum(_latent_ref(g, x, s2, y.reshape(m, n)[l], xs, dmean.reshape(m, ns)[l], dvar.reshape(m, ns)[l]) for l, g in enumerate(gps))
    go = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, m), s2), dmean, dvar)
    _close(go["x"], ref, 1e-9)
    assert go["sigma2"] == pytest.approx(dvar.sum(), rel=1e-12)
    idx = lmm.indices_which_reorder_outputs_to_features(lmm.MOInputIsotopicByOutputs(xs, m)) - 1
    gf = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByFeatures(xs, m), s2), dmean[idx], dvar[idx])
    _close(gf["x"], ref, 1e-9)


def test_shards_sum_to_whole(lmm):
    rng = np.random.default_rng(12)
    n, ns, p, m, s2 = 260, 45, 6, 5, 0.1
    gps = [_gp(rng, KINDS[l]) for l in range(m)]
    U, S = _orth(rng, p, m)
    x, xs, y = _inputs(rng, n, 1), _inputs(rng, ns, 1), rng.standard_normal(n * p)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    whole = lmm.mean_and_var_vjp(_oilmm_post(lmm, gps, U, S, x, s2, y)(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]
    parts = [lmm.mean_and_var_vjp(_oilmm_post(lmm, gps, U, S, x, s2, y, sh)(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)["x"]
             for sh in [(0, 2), (2, 3), (3, 5)]]
    _close(parts[0] + parts[1] + parts[2], whole, 1e-12)


def test_deterministic(lmm):
    rng = np.random.default_rng(13)
    n, ns, p, s2 = 1100, 300, 6, 0.1
    gps = [_gp(rng, k) for k in KINDS]
    U, S = _orth(rng, p, len(gps))
    x, xs = _inputs(rng, n, 1), _inputs(rng, ns, 1)
    fx = _oilmm_post(lmm, gps, U, S, x, s2, rng.standard_normal(n * p))(lmm.MOInputIsotopicByOutputs(xs, p), s2)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    a = lmm.mean_and_var_vjp(fx, dmean, dvar)["x"]
    b = lmm.mean_and_var_vjp(fx, dmean, dvar)["x"]
    assert np.array_equal(a, b)


def test_matern12_coincident_points(lmm):
    rng = np.random.default_rng(14)
    n, m, s2 = 200, 2, 0.1
    gps = [_gp(rng, "matern12", 2), _gp(rng, "matern12")]
    x, y = _inputs(rng, n, 2), rng.standard_normal(n * m)
    po = lmm.posterior(_model(lmm, gps)(lmm.MOInputIsotopicByOutputs(x, m), s2), y)
    dmean, dvar = rng.standard_normal(n * m), rng.standard_normal(n * m)
    got = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(x.copy(), m), s2), dmean, dvar)["x"]
    ref = sum(_latent_ref(g, x, s2, y.reshape(m, n)[l], x, dmean.reshape(m, n)[l], dvar.reshape(m, n)[l]) for l, g in enumerate(gps))
    _close(got, ref, 1e-9)


def test_errors(lmm):
    from lmm_amd import _lib as L
    rng = np.random.default_rng(15)
    n, ns, p, m, s2 = 120, 30, 3, 2, 0.1
    gps = [_gp(rng, "se"), _gp(rng, "matern32")]
    x, xs, y = _inputs(rng, n, 1), _inputs(rng, ns, 1), rng.standard_normal(n * p)
    H = rng.uniform(0.0, 1.0, (p, m))
    dpo = lmm.posterior(lmm.ILMM(_model(lmm, gps), H)(lmm.MOInputIsotopicByOutputs(x, p), s2), y)
    dfx = dpo(lmm.MOInputIsotopicByOutputs(xs, p), s2)
    with pytest.raises(NotImplementedError):
        lmm.mean_and_var_vjp(dfx, np.ones(ns * p), np.ones(ns * p))
    with pytest.raises(NotImplementedError):
        lmm.mean_and_var_vjp(lmm.get_latent_gp(dpo)(lmm.MOInputIsotopicByOutputs(xs, m), s2), np.ones(ns * m))
    lib = L.load()
    gpsa = L.gps_array([g.desc() for g in _model(lmm, gps).fs])
    Hc = np.asfortranarray(H)
    out = np.zeros(33 * ns)
    xsa, dm = np.ascontiguousarray(xs), np.ones(ns * p)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.lmm_oilmm_mean_and_var_grad_xs(dpo.f._post.ptr, gpsa, ptr(Hc), None, p, m, 0, m, ptr(xsa), 1, ns, ptr(dm), None, ptr(out))
    assert rc == L.LMM_ERR_UNSUPPORTED
    U, S = _orth(rng, p, m)
    po = _oilmm_post(lmm, gps, U, S, x, s2, y)
    x33 = rng.uniform(0.0, 1.0, 33 * ns)
    rc = lib.lmm_oilmm_mean_and_var_grad_xs(po.f._post.ptr, gpsa, ptr(U), ptr(S), p, m, 0, m, ptr(x33), 33, ns, ptr(dm), None, ptr(out))
    assert rc == L.LMM_ERR_UNSUPPORTED
    x2 = rng.uniform(0.0, 1.0, 2 * ns)
    rc = lib.lmm_oilmm_mean_and_var_grad_xs(po.f._post.ptr, gpsa, ptr(U), ptr(S), p, m, 0, m, ptr(x2), 2, ns, ptr(dm), None, ptr(out))
    assert rc == L.LMM_ERR_DIM
    lmm.set_compute_dtype("f32")
    try:
        with pytest.raises(NotImplementedError):
            lmm.mean_and_var_vjp(lmm.OILMM(_model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(xs, p), s2), dm)
    finally:
        lmm.set_compute_dtype("f64")


def test_torch_device_inputs(lmm):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(16)
    n, ns, p, s2 = 180, 40, 3, 0.1
    gps = [_gp(rng, "matern52", 2), _gp(rng, "rq", 2)]
    U, S = _orth(rng, p, 2)
    x, xs = _inputs(rng, n, 2), _inputs(rng, ns, 2)
    po = _oilmm_post(lmm, gps, U, S, x, s2, rng.standard_normal(n * p))
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    ref = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(xs, p), s2), dmean, dvar)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    got = lmm.mean_and_var_vjp(po(lmm.MOInputIsotopicByOutputs(dev(xs), p), s2), dev(dmean), dev(dvar))
    assert torch.is_tensor(got["x"]) and got["x"].is_cuda and tuple(got["x"].shape) == xs.shape
    _close(got["x"].cpu().numpy(), ref["x"], 1e-12)
    assert got["sigma2"] == pytest.approx(ref["sigma2"], rel=1e-12)
