"""The blocked schedule of the Toeplitz path (DESIGN.md 4.22 "Blocked schedule") on the GPU.  With J steps per launch and R rows per
workgroup (lmm_toeplitz_blocked_shape) the sizes sit on the kernel's boundaries: 1, 2, 3 (no full block), J, J + 1, 2 J + 1 (the last
block with J - 1, 0 and 0 rotations), R, R + 1, R + J + 1, 2 R + J + 3 (one, two and three workgroups on a side), 4097, and 8193, one
past the unblocked cap.  References and the tolerance 1e-10 of max |reference| are those of test_gpu_toeplitz.py: the arithmetic per
row and step is the unblocked kernel's."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_toeplitz import H, MIXES, P_OUT, S2, SHAPE, TOL, dense_gaussian, problem
from test_gpu_toeplitz_posterior import check
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_posterior_abi import Q, queries

pytestmark = pytest.mark.gpu


def _shape():
    j, r = C.c_int(), C.c_int()
    L.check(lmm.load().lmm_toeplitz_blocked_shape(C.byref(j), C.byref(r)))
    return j.value, r.value


J, R = _shape()


def factor(t, r, blocked=True):
    """log det, r' K^-1 r and the device generators p, q of one matrix"""
    import torch
    lmm.init(0)
    lib, n = lmm.load(), len(t)
    td, rd = torch.tensor(t, device="cuda"), torch.tensor(r, device="cuda")
    pd, qd = torch.empty_like(td), torch.empty_like(td)
    ld, qu = C.c_double(), C.c_double()
    fn = lib.lmm_dev_toeplitz_factor_blocked if blocked else lib.lmm_dev_toeplitz_factor
    L.check(fn(td.data_ptr(), rd.data_ptr(), n, C.byref(ld), C.byref(qu), pd.data_ptr(), qd.data_ptr()))
    return ld.value, qu.value, pd, qd, rd


@pytest.mark.parametrize("n", (1, 2, 3, J, J + 1, 2 * J + 1, R, R + 1, R + J + 1, 2 * R + J + 3, 4097, 8193))
def test_building_block_against_dense_cholesky(n):
    import torch
    t = row(LATENTS["lp"] + LATENTS["matern52"], 0.013 * np.arange(n)); t[0] += 0.05
    r = np.random.default_rng(7 * n).standard_normal(n)
    cf = scipy.linalg.cho_factor(toeplitz(t), lower=True)
    alpha, logdet = scipy.linalg.cho_solve(cf, r), 2.0 * np.log(np.diag(cf[0])).sum()
    ld, qu, pd, qd, rd = factor(t, r)
    ld2, qu2, pd2, qd2, _ = factor(t, r)
    assert (ld, qu) == (ld2, qu2) and torch.equal(pd, pd2) and torch.equal(qd, qd2)      # two calls are bitwise equal
    print(f"n={n}: log det {abs(ld - logdet) / max(1.0, abs(logdet)):.2e}, quad {abs(qu - r @ alpha) / abs(r @ alpha):.2e}")
    assert abs(ld - logdet) <= TOL * max(1.0, abs(logdet))
    assert abs(qu - r @ alpha) <= TOL * abs(r @ alpha)
    if n != 8193:      # alpha at the cap belongs to the Gohberg-Semencul products (1.2e-10 at 8192), which are not the recursion's
        ad = torch.empty_like(pd)
        L.check(lmm.load().lmm_dev_toeplitz_solve(pd.data_ptr(), qd.data_ptr(), rd.data_ptr(), n, ad.data_ptr()))
        assert np.abs(ad.cpu().numpy() - alpha).max() <= TOL * np.abs(alpha).max()


@pytest.mark.parametrize("n", (2 * J + 1, R + J + 1))
@pytest.mark.parametrize("names", MIXES)
def test_value_and_gradient_against_dense_gaussian(names, n):
    fx, x, y, U, S = problem(names, n)
    ref, got = dense_gaussian(names, n, y, U, S), lmm.toeplitz_logpdf_and_gradient(fx, y, blocked=True)
    assert got["value"] == lmm.toeplitz_logpdf(fx, y, blocked=True)
    for key in ("value", "y", "sigma2", "S", "U"):
        assert np.abs(np.asarray(got[key]) - ref[key]).max() <= TOL * np.abs(ref[key]).max(), key
    scale = max(abs(v) for g in ref["gps"] for v in g.values())
    for k, g, rg in zip(names, got["gps"], ref["gps"]):
        terms = LATENTS[k]
        pairs = [(g["mean"], rg["mean"])]
        if len(terms) == 1:
            pairs += [(g[s], rg[(0, SHAPE[s])]) for s in g if s != "mean"]
        else:      # the whole sum's variance and lengthscale are 1: d/dv0 = sum v_c d/dV_c, d/ds0 = sum l_c d/dE_c
            pairs += [(g["variance"], sum(t[1] * rg[(c, 0)] for c, t in enumerate(terms))), (g["lengthscale"], sum(t[2] * rg[(c, 1)] for c, t in enumerate(terms)))]
            pairs += [(gt[s], rg[(c, SHAPE[s])]) for c, gt in enumerate(g["terms"]) for s in gt]
        assert max(abs(a - b) for a, b in pairs) <= TOL * scale, k


def test_posterior_against_the_dense_posterior():
    names, n = MIXES[1], R + J + 1
    fx, x, y, U, S = problem(names, n)
    xs = queries(0.5, H, n, Q + 1)
    dm, dv = lmm.mean_and_var(lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2))
    prior = ((U * np.sqrt(S)) ** 2 @ np.array([row(LATENTS[k], 0.0) for k in names])).max() + S2
    with lmm.toeplitz_posterior(fx, y, blocked=True) as post:
        assert post.logpdf == lmm.toeplitz_logpdf(fx, y, blocked=True)      # bitwise
        check(post.mean_and_var(xs), (dm, dv, prior), f"{names} blocked against the dense posterior")


@pytest.mark.parametrize("d", (3, J + 5, 2 * J + R // 2))
def test_failing_pivot_is_reported_as_the_unblocked_kernel_reports_it(d):
    t = np.zeros(d + R); t[0], t[d] = 1.0, 1.5      # positive definite through size d, indefinite at d + 1
    with pytest.raises(lmm.PosDefException) as want:
        factor(t, np.ones(len(t)), blocked=False)
    assert "latent 0, step" in str(want.value)
    with pytest.raises(lmm.PosDefException) as got:
        factor(t, np.ones(len(t)))
    assert str(got.value) == str(want.value)


def test_refusals():
    n = lmm.load().lmm_toeplitz_blocked_max_n() + 1
    f = problem(MIXES[0], 1)[0].f
    with pytest.raises(NotImplementedError, match="lmm_toeplitz_blocked_max_n"):
        lmm.toeplitz_logpdf(f(lmm.MOInputIsotopicByOutputs(0.5 + 0.01 * np.arange(n), P_OUT), S2), np.zeros(n * P_OUT), blocked=True)
    fx, x, y, U, S = problem(MIXES[0], 65)
    bad_y = y.copy(); bad_y[70] = np.nan
    xb = x.copy(); xb[9] += 1e-3
    for fn in (lmm.toeplitz_logpdf, lmm.toeplitz_logpdf_and_gradient, lmm.toeplitz_posterior):
        with pytest.raises(NotImplementedError, match="point 5 has a NaN"):
            fn(fx, bad_y, blocked=True)
        with pytest.raises(ValueError, match=r"x\[9\]"):
            fn(fx.f(lmm.MOInputIsotopicByOutputs(xb, P_OUT), S2), y, blocked=True)
