"""Host-only checks of the gradients of the state-space logpdf (include/lmm_hip.h "state space"): the two entry points
are declared, exported and bound with matching arity, the refusals of the Python mirror come before any library call, and the NumPy
restatement of the gradient agrees with the dense analytic gradient, which is itself checked by central finite differences.  The
largest disagreement delta_grad() fixes the GPU tolerances of tests/test_gpu_statespace_grad.py, max(1e-10, 100 delta_grad()), which
imports the restatement from here.  No GPU and no lmm_init needed.

The restatement, per latent with C = K + diag(w) over the observed points:
  d lml / d r_t = -alpha_t, alpha_t = (r_t - mu_t) / w_t, and d lml / d w_t = (alpha_t^2 - c_t) / 2, c_t = (w_t - P_t) / w_t^2, from the
  smoothed first-component mean mu and variance P of test_statespace_abi.statespace_reference;
  d lml / d variance and d lml / d lengthscale by a sequential tangent filter: the Kalman filter on test_statespace_abi's ss_model / ss_AQ
  carried on value + i h tangent with h = 1e-30 (the complex step: h^2 is below every rounding, so the imaginary part over h is the
  forward-mode tangent, with no subtraction).

`python tests/test_statespace_grad_abi.py` prints the disagreements."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lmm_amd
from lmm_amd import _lib as L

import test_statespace_abi as T

SYMS = ("lmm_oilmm_logpdf_grad_statespace", "lmm_dev_statespace_grad")
STEP = 1e-30


# ---- the gradient, restated ----------------------------------------------------------------------------------------------------
def tangent_filter(kind, v, ell, x, w, r):
    """(d lml / d variance, d lml / d lengthscale) by the sequential filter on (value, tangent)."""
    out = []
    for vv, ll in ((v + 1j * STEP, ell + 0j), (v + 0j, ell + 1j * STEP)):
        model = T.ss_model(kind, vv, ll)
        D = model[1].shape[0]
        m, P = np.zeros(D, dtype=complex), model[2].astype(complex)
        val = 0.0 + 0j
        for t in range(len(x)):
            if t > 0:
                A, Q = T.ss_AQ(model, x[t] - x[t - 1])
                m, P = A @ m, A @ P @ A.T + Q
            if np.isfinite(w[t]):
                S = P[0, 0] + w[t]
                K = P[:, 0] / S
                e = r[t] - m[0]
                m, P = m + K * e, P - np.outer(K, P[0, :])
                val += -0.5 * (T.LOG2PI + np.log(S) + e * e / S)
        out.append(float(val.imag / STEP))
    return out[0], out[1]


def point_gradients(w, r, sm, sv):
    """(d lml / d r, d lml / d w) from the smoothed marginals; 0 at the unobserved points."""
    obs = np.isfinite(w)
    ws = np.where(obs, w, 1.0)
    alpha = np.where(obs, (r - sm) / ws, 0.0)
    c = np.where(obs, (ws - sv) / (ws * ws), 0.0)
    return -alpha, np.where(obs, 0.5 * (alpha * alpha - c), 0.0)


def statespace_grad_reference(kind, v, ell, x, w, r):
    """(value, grad_r, grad_w, d/d variance, d/d lengthscale) of the restatement."""
    val, _, _, sm, sv = T.statespace_reference(kind, v, ell, x, w, r)
    gr, gw = point_gradients(w, r, sm, sv)
    gv, gl = tangent_filter(kind, v, ell, x, w, r)
    return val, gr, gw, gv, gl


# ---- the dense analytic gradient it is compared with -----------------------------------------------------------------------------
def matern_dK_dell(kind, v, ell, x):
    d = T.O.pairwise_dist(x)
    if kind == "matern12":
        return v * np.exp(-d / ell) * d / (ell * ell)
    return T.O.kernel_dlengthscale(kind, v, ell, d)


def dense_grad_reference(kind, v, ell, x, w, r):
    """The same five quantities from C = K + diag(w) over the observed points: alpha = C^-1 r, alpha' K_theta alpha / 2 -
    tr(C^-1 K_theta) / 2, (alpha^2 - diag C^-1) / 2."""
    n = len(x)
    obs = np.flatnonzero(np.isfinite(w))
    gr, gw = np.zeros(n), np.zeros(n)
    if len(obs) == 0:
        return 0.0, gr, gw, 0.0, 0.0
    K = T.matern_K(kind, v, ell, x[obs])
    Ci = np.linalg.inv(K + np.diag(w[obs]))
    Ci = 0.5 * (Ci + Ci.T)
    alpha = Ci @ r[obs]
    A = np.outer(alpha, alpha) - Ci
    gr[obs], gw[obs] = -alpha, 0.5 * np.diag(A)
    val = T.dense_reference(kind, v, ell, x, w, r)[0]
    return val, gr, gw, 0.5 * np.sum(A * K) / v, 0.5 * np.sum(A * matern_dK_dell(kind, v, ell, x[obs]))


def equal_case(kind):
    """Complete data with runs of equal inputs (test_statespace_abi.test_equal_points_and_complete_data)."""
    v, ell, x, w, r = T.case(kind, 65, unobserved=False)
    x[10:14] = x[10]
    x[40] = x[39]
    return v, ell, x, w, r


def cases(kind):
    return [((kind, n), T.case(kind, n)) for n in T.CPU_N] + [((kind, "equal"), equal_case(kind))]


def grad_err(got, ref):
    """Largest relative disagreement per array: of max|ref| for grad_r and grad_w, relative for the two scalars."""
    return (T.arr_err(got[1], ref[1]) if np.abs(ref[1]).max() > 0 else float(np.abs(got[1]).max()),
            T.arr_err(got[2], ref[2]) if np.abs(ref[2]).max() > 0 else float(np.abs(got[2]).max()),
            T.rel(got[3], ref[3]), T.rel(got[4], ref[4]))


_DELTA = {}


def deltas_grad():
    """{(kind, n or "equal"): (grad_r, grad_w, d/d variance, d/d lengthscale)} disagreements of the restatement with the dense gradient."""
    if not _DELTA:
        for kind in T.KINDS:
            for key, (v, ell, x, w, r) in cases(kind):
                _DELTA[key] = grad_err(statespace_grad_reference(kind, v, ell, x, w, r), dense_grad_reference(kind, v, ell, x, w, r))
    return _DELTA


def delta_grad():
    """The largest disagreement over every case and array: the DELTA of the GPU tolerances."""
    return max(max(d) for d in deltas_grad().values())


@pytest.mark.parametrize("kind", T.KINDS)
def test_dense_gradient_agrees_with_finite_differences(kind):
    """Central differences of dense_reference's value in variance, lengthscale and a few r_t and w_t (step 1e-5 of a smooth function of
    size ~ n: truncation ~ 1e-10 relative, rounding ~ eps |value| / step ~ 1e-9 absolute)."""
    for key, (v, ell, x, w, r) in [c for c in cases(kind) if c[0][1] in (5, 65, "equal")]:
        ref = dense_grad_reference(kind, v, ell, x, w, r)
        f = lambda v_=v, ell_=ell, w_=w, r_=r: T.dense_reference(kind, v_, ell_, x, w_, r_)[0]
        h = 1e-5
        fd_v = (f(v_=v + h) - f(v_=v - h)) / (2 * h)
        fd_l = (f(ell_=ell + h) - f(ell_=ell - h)) / (2 * h)
        assert abs(fd_v - ref[3]) <= 1e-6 * max(1.0, abs(ref[3])), (key, fd_v, ref[3])
        assert abs(fd_l - ref[4]) <= 1e-6 * max(1.0, abs(ref[4])), (key, fd_l, ref[4])
        obs = np.flatnonzero(np.isfinite(w))
        for t in obs[:: max(1, len(obs) // 5)]:
            e = np.zeros(len(x)); e[t] = h
            fd_r = (f(r_=r + e) - f(r_=r - e)) / (2 * h)
            fd_w = (f(w_=w + e) - f(w_=w - e)) / (2 * h)
            assert abs(fd_r - ref[1][t]) <= 1e-6 * max(1.0, abs(ref[1][t])), (key, t)
            assert abs(fd_w - ref[2][t]) <= 1e-6 * max(1.0, abs(ref[2][t])), (key, t)
        unobs = np.flatnonzero(~np.isfinite(w))
        assert (ref[1][unobs] == 0).all() and (ref[2][unobs] == 0).all()


@pytest.mark.parametrize("kind", T.KINDS)
def test_gradient_restatement_agrees_with_dense(kind):
    for key, _ in cases(kind):
        d = deltas_grad()[key]
        print(f"{key}: grad_r {d[0]:.2e} grad_w {d[1]:.2e} variance {d[2]:.2e} lengthscale {d[3]:.2e}")
        assert max(d) <= 1e-10, (key, d)


def scaling_identity(v, w, r, gr, gw, gv):
    """lml(s v, s w, sqrt(s) r) = lml(v, w, r) - (n_obs / 2) log s, differentiated at s = 1: (left side, the terms' absolute sum, -n_obs / 2)."""
    obs = np.isfinite(w)
    terms = np.concatenate([[v * gv], w[obs] * gw[obs], 0.5 * r[obs] * gr[obs]])
    return float(terms.sum()), float(np.abs(terms).sum()), -0.5 * int(obs.sum())


@pytest.mark.parametrize("kind", T.KINDS)
def test_scaling_identity_on_the_restatement(kind):
    for key, (v, ell, x, w, r) in cases(kind):
        _, gr, gw, gv, _ = statespace_grad_reference(kind, v, ell, x, w, r)
        lhs, mag, rhs = scaling_identity(v, w, r, gr, gw, gv)
        assert abs(lhs - rhs) <= 1e-11 * max(mag, 1.0), (key, lhs, rhs)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_statespace_grad_symbols_declared_exported_and_bound():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(T.HEADER).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert proto, s
        params = [a.strip() for a in proto.group(1).split(",")]
        types = L.STATESPACE_ARGTYPES[s]
        assert len(params) == len(types), (s, len(params), len(types))
        assert getattr(lib, s).argtypes == types
        for a, t in zip(params, types):
            want = L._P if ("*" in a or "[" in a) else (L._D if a.startswith("double") else L._I)
            assert t is want, (s, a)
    proto = re.search(r"int\s+lmm_oilmm_logpdf_grad_statespace\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "with_regulariser", "out_logpdf",
                     "grad_y", "grad_sigma2", "grad_S", "grad_U", "grad_gps"]
    proto = re.search(r"int\s+lmm_dev_statespace_grad\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "n", "gp", "w", "r", "chunk", "lml", "grad_r", "grad_w", "grad_theta"]
    assert "statespace_logpdf_and_gradient" in lmm_amd.__all__


def test_gradient_refusals_come_before_any_library_call():
    fs, x, H = T._models()
    y = np.zeros(8)
    M = lmm_amd.model
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    sharded = lmm_amd.ILMM(fs, H, shard=(0, 0))(x, 0.1)
    post = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._PostHandle(None, 0, 1)), H)(x, 0.1)
    sparse = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._SparsePostHandle(None, 0, 1)), H)(x, 0.1)
    features = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), lmm_amd.MOInputIsotopicByFeatures(np.arange(4.0), 2), 0.1)
    perpoint = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), x, np.full(8, 0.1))
    d2 = lmm_amd.ILMM(fs, H)(lmm_amd.MOInputIsotopicByOutputs(np.zeros((2, 4)), 2), 0.1)

    def with_kernel(k):
        return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(k)]), H)(x, 0.1)

    se = with_kernel(lmm_amd.SEKernel())
    rq = with_kernel(lmm_amd.RationalQuadraticKernel())
    per = with_kernel(lmm_amd.PeriodicKernel())
    lp = with_kernel(lmm_amd.LocallyPeriodicKernel())
    ksum = with_kernel(lmm_amd.KernelSum(lmm_amd.Matern32Kernel(), lmm_amd.Matern52Kernel()))
    ard = with_kernel(lmm_amd.Matern52Kernel(1.0, np.array([0.5])))
    saved = L.ensure_init
    L.ensure_init = T._no_library
    try:
        fn = lmm_amd.statespace_logpdf_and_gradient
        for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                             (sparse, y, "posterior model"), (oilmm, np.zeros((8, 2)), "matrix Y"), (sharded, y, "sharded"),
                             (features, y, "MOInputIsotopicByOutputs"), (perpoint, y, "scalar noise"), (d2, y, "d = 2"),
                             (se, y, "latent 0"), (rq, y, "latent 0"), (per, y, "latent 0"), (lp, y, "latent 0"),
                             (ksum, y, "latent 0"), (ard, y, "latent 0")):
            with pytest.raises(NotImplementedError, match=what):
                fn(fx, yy)
        with pytest.raises(ValueError, match="length"):
            fn(oilmm, np.zeros(7))
        with pytest.raises(AssertionError, match="the library was reached"):      # a valid call gets as far as the library
            fn(oilmm, y)
        # data with NaN: the mirror never asks the library for "S" and "U"; the dict refuses them by itself
        g = M._NoStateSpaceMixingGradient({"value": 0.0, "y": y, "sigma2": 0.0, "gps": []})
        for key in ("S", "U"):
            with pytest.raises(NotImplementedError, match="NaN"):
                g[key]
        with pytest.raises(KeyError):
            g["x"]
        assert g["sigma2"] == 0.0
    finally:
        L.ensure_init = saved


if __name__ == "__main__":
    for key, d in deltas_grad().items():
        print(f"{key[0]:9s} {str(key[1]):>6s}  grad_r {d[0]:.2e}  grad_w {d[1]:.2e}  variance {d[2]:.2e}  lengthscale {d[3]:.2e}")
    print(f"delta_grad = {delta_grad():.2e}")
