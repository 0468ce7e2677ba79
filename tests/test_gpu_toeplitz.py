"""The Toeplitz path on the GPU: the value and every gradient key against dense Gaussians built in NumPy (per latent
n x n; kernels and complex-step derivatives of test_toeplitz_abi), the building blocks against a dense Cholesky solve, the library's
dense path, reproducibility, refusals.  n = 1, 2, 3, 1023, 1025, 2049: the one / two / three rows per thread boundaries of the
1024-thread workgroup; the building blocks also at five rows and at the cap.  Tolerance 1e-10 of max |reference| (CPU deltas < 1e-11)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_toeplitz_abi import LATENTS, dense_latent, row, toeplitz

pytestmark = pytest.mark.gpu
P_OUT, S2, TOL, H = 4, 0.2, 1e-10, 0.01
SIZES = (1, 2, 3, 1023, 1025, 2049)
MIXES = (("se", "rq", "periodic"), ("lp", "matern52", "sum"), ("sho", "matern12", "matern32"))
CTOR = {"se": lmm.SEKernel, "rq": lmm.RationalQuadraticKernel, "periodic": lmm.PeriodicKernel, "lp": lmm.LocallyPeriodicKernel,
        "matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel, "sho": lmm.SHOKernel}
SHAPE = {"variance": 0, "lengthscale": 1, "alpha": 2, "r": 2, "quality": 2, "decay": 3}


def problem(names, n):
    rng = np.random.default_rng(n)
    x = 0.5 + H * np.arange(n)
    U = np.linalg.qr(rng.standard_normal((P_OUT, len(names))))[0]
    S = np.array([1.0, 1.6, 0.7])
    y = rng.standard_normal(n * P_OUT)
    ks = [CTOR[LATENTS[k][0][0]](*LATENTS[k][0][1:]) if len(LATENTS[k]) == 1 else lmm.KernelSum(*[CTOR[t[0]](*t[1:]) for t in LATENTS[k]])
          for k in names]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, S))
    return f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), x, y, U, S


def dense_gaussian(names, n, y, U, S):
    """The OILMM log density and its gradient from per-latent dense Gaussians: r_l = S_l^-1/2 U_l' Y, noise S2 / S_l, plus the
    regulariser -n/2 (sum log S + (p - m) log(2 pi S2)) - |(I - U U') Y|^2 / (2 S2).  gps[l][(c, j)]: parameter j of term c."""
    Y, m, lags = y.reshape(P_OUT, n), len(names), (0.5 + H * np.arange(n)) - 0.5      # the actual x_d - x_0
    P = np.eye(P_OUT) - U @ U.T
    PY, M = P @ Y, Y @ Y.T
    out = {"value": -0.5 * n * (np.log(S).sum() + (P_OUT - m) * np.log(2 * np.pi * S2)) - 0.5 * np.sum(PY * PY) / S2,
           "y": -PY / S2, "sigma2": -0.5 * n * (P_OUT - m) / S2 + 0.5 * np.sum(PY * PY) / S2 ** 2, "S": -0.5 * n / S,
           "U": (P @ M @ U + M @ P @ U) / S2, "gps": []}
    for l, k in enumerate(names):
        Ty = U[:, l] @ Y / np.sqrt(S[l])
        lml, alpha, gw, gth, _, _ = dense_latent(LATENTS[k], lags, S2 / S[l], Ty)
        out["value"] += lml
        out["y"] -= np.outer(U[:, l] / np.sqrt(S[l]), alpha)
        out["sigma2"] += gw / S[l]
        out["S"][l] += -gw * S2 / S[l] ** 2 + 0.5 * (alpha @ Ty) / S[l]
        out["U"][:, l] -= Y @ alpha / np.sqrt(S[l])
        out["gps"].append(dict(gth, mean=alpha.sum()))
    out["y"] = out["y"].reshape(-1)
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("names", MIXES)
def test_value_and_gradient_against_dense_gaussian(names, n):
    fx, x, y, U, S = problem(names, n)
    ref, got = dense_gaussian(names, n, y, U, S), lmm.toeplitz_logpdf_and_gradient(fx, y)
    again = lmm.toeplitz_logpdf_and_gradient(fx, y)      # two calls are bitwise equal, and the value is the value call's
    assert got["value"] == lmm.toeplitz_logpdf(fx, y) == again["value"] and repr(got["gps"]) == repr(again["gps"])
    assert all(np.array_equal(got[k], again[k]) for k in ("y", "sigma2", "S", "U"))
    for key in ("value", "y", "sigma2", "S", "U"):
        assert np.abs(np.asarray(got[key]) - ref[key]).max() <= TOL * np.abs(ref[key]).max(), key
    scale = max(abs(v) for g in ref["gps"] for v in g.values())
    for k, g, rg in zip(names, got["gps"], ref["gps"]):
        terms = LATENTS[k]
        pairs = [(g["mean"], rg["mean"])]
        if len(terms) == 1:
            assert set(g) >= {"variance", "lengthscale", *{"rq": ["alpha"], "periodic": ["r"], "lp": ["r", "decay"], "sho": ["quality"]}.get(k, [])}
            pairs += [(g[s], rg[(0, SHAPE[s])]) for s in g if s != "mean"]
        else:      # the whole sum's variance and lengthscale are 1: d/dv0 = sum v_c d/dV_c, d/ds0 = sum l_c d/dE_c
            pairs += [(g["variance"], sum(t[1] * rg[(c, 0)] for c, t in enumerate(terms))), (g["lengthscale"], sum(t[2] * rg[(c, 1)] for c, t in enumerate(terms)))]
            pairs += [(gt[s], rg[(c, SHAPE[s])]) for c, gt in enumerate(g["terms"]) for s in gt]
        assert max(abs(a - b) for a, b in pairs) <= TOL * scale, k


@pytest.mark.parametrize("names", MIXES)
def test_agrees_with_the_dense_path(names):
    fx, x, y, U, S = problem(names, 1025)
    got, ref = lmm.toeplitz_logpdf_and_gradient(fx, y), lmm.logpdf_and_gradient(fx, y)
    assert abs(lmm.toeplitz_logpdf(fx, y) - lmm.logpdf(fx, y)) <= TOL * abs(ref["value"])
    for key in ("y", "sigma2", "S", "U"):
        assert np.abs(np.asarray(got[key]) - np.asarray(ref[key])).max() <= TOL * np.abs(ref[key]).max(), key
    assert [sorted(g) for g in got["gps"]] == [sorted(g) for g in ref["gps"]]
    for g, rg in zip(got["gps"], ref["gps"]):
        assert all(abs(g[s] - rg[s]) <= TOL * max(abs(v) for q in ref["gps"] for v in q.values() if np.isscalar(v)) for s in g if s != "terms")


@pytest.mark.parametrize("n", SIZES + (4097, 8192))
def test_building_blocks_against_dense_solve(n):
    import torch
    lmm.init(0)
    lib = lmm.load()
    assert lib.lmm_toeplitz_max_n() == 8192
    t = row(LATENTS["lp"] + LATENTS["matern52"], 0.013 * np.arange(n)); t[0] += 0.05
    r = np.random.default_rng(7 * n).standard_normal(n)
    cf = scipy.linalg.cho_factor(toeplitz(t), lower=True)
    alpha, logdet = scipy.linalg.cho_solve(cf, r), 2.0 * np.log(np.diag(cf[0])).sum()
    td, rd = torch.tensor(t, device="cuda"), torch.tensor(r, device="cuda")
    pd, qd, ad = torch.empty_like(td), torch.empty_like(td), torch.empty_like(td)
    ld, qu = C.c_double(), C.c_double()
    L.check(lib.lmm_dev_toeplitz_factor(td.data_ptr(), rd.data_ptr(), n, C.byref(ld), C.byref(qu), pd.data_ptr(), qd.data_ptr()))
    L.check(lib.lmm_dev_toeplitz_solve(pd.data_ptr(), qd.data_ptr(), rd.data_ptr(), n, ad.data_ptr()))
    assert abs(ld.value - logdet) <= TOL * max(1.0, abs(logdet))
    assert abs(qu.value - r @ alpha) <= TOL * abs(r @ alpha)
    assert np.abs(ad.cpu().numpy() - alpha).max() <= TOL * np.abs(alpha).max()


def test_refusals():
    import torch
    fx, x, y, U, S = problem(MIXES[0], 65)
    td = torch.tensor([1.0, 1.2, 0.3, 0.1, 0.0], device="cuda", dtype=torch.float64)      # not positive definite: refused by value
    o = torch.empty_like(td)
    with pytest.raises(lmm.PosDefException, match="latent 0"):
        L.check(lmm.load().lmm_dev_toeplitz_factor(td.data_ptr(), td.data_ptr(), 5, None, None, o.data_ptr(), o.data_ptr()))
    bad_y = y.copy(); bad_y[70] = np.nan
    with pytest.raises(NotImplementedError, match="point 5 has a NaN"):
        lmm.toeplitz_logpdf(fx, bad_y)
    xb = x.copy(); xb[9] += 1e-3
    with pytest.raises(ValueError, match=r"x\[9\]"):
        lmm.toeplitz_logpdf(fx.f(lmm.MOInputIsotopicByOutputs(xb, P_OUT), S2), y)
    lib = lmm.load()
    out = C.c_double()
    rc = lib.lmm_oilmm_logpdf_toeplitz(L.Arr(xb).ptr, 65, L.Arr(y).ptr, P_OUT, L.Arr(L.colmajor(U)).ptr, L.Arr(S).ptr, 3, S2,
                                       L.gps_array([g.desc() for g in fx.f.f.fs]), 0, 3, 1, C.byref(out))
    with pytest.raises(ValueError, match=r"x\[9\] is off the grid"):
        L.check(rc)
    fc, xc, yc, _, _ = problem(MIXES[0], lib.lmm_toeplitz_max_n() + 1)
    with pytest.raises(NotImplementedError, match="lmm_toeplitz_max_n"):
        lmm.toeplitz_logpdf(fc, yc)
