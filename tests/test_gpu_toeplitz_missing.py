"""Missing observations on the Toeplitz path (DESIGN.md 4.22 "Missing observations") on the GPU: the inverse block against
np.linalg.inv(T)[S][:, S] with k around the 128-wide tile, the value against the dense Gaussian of the observed points built from the
front end's definition.  Tolerance: 100 x the CPU delta where that exceeds 1e-11, else 1e-10; the block relative to max |T^-1|."""
import functools

import numpy as np
import pytest

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_missing import flat_orthogonal, restatement
from test_gpu_toeplitz import CTOR
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_missing_abi import delta_toeplitz_missing

pytestmark = pytest.mark.gpu
TOL = 100.0 * delta_toeplitz_missing() if delta_toeplitz_missing() > 1e-11 else 1e-10
P_OUT, S2, SV, H = 5, 0.1, np.array([1.0, 1.6, 0.7]), 0.01                      # S2 / SV: 0.1, 0.0625, 0.143
MIX = (LATENTS["se"], LATENTS["matern52"] + LATENTS["lp"], LATENTS["rq"])       # SE, Matern52 + SE x Periodic, RQ


@functools.lru_cache(maxsize=None)
def factored(kind, n):
    """T^-1 in NumPy and the generators of lmm_dev_toeplitz_factor on the device"""
    import torch
    lmm.init(0)
    t = row(LATENTS[kind], 0.05 * np.arange(n)); t[0] += 0.1
    td = torch.tensor(t, device="cuda")
    pd, qd = torch.empty_like(td), torch.empty_like(td)
    L.check(lmm.load().lmm_dev_toeplitz_factor(td.data_ptr(), torch.zeros_like(td).data_ptr(), n, None, None, pd.data_ptr(), qd.data_ptr()))
    return np.linalg.inv(toeplitz(t)), pd, qd


def indices(shape, n, k):
    if shape == "run":
        return n // 3 - k // 3 + np.arange(k)
    if shape == "scattered":
        return np.sort(np.random.default_rng(k).choice(n, k, replace=False))
    return np.unique(np.concatenate([[0, n - 1], 1 + (n - k) // 2 + np.arange(k - 2)]))[:k]


@pytest.mark.parametrize("shape", ("run", "scattered", "run+ends"))
@pytest.mark.parametrize("n, k", [(n, k) for n in (129, 1025) for k in (1, 127, 129, 300) if k <= n])
@pytest.mark.parametrize("kind", ("se", "matern52"))
def test_inverse_block_against_dense_inverse(kind, n, k, shape):
    import torch
    Ti, pd, qd = factored(kind, n)
    S = indices(shape, n, k)
    k, idx = len(S), torch.tensor(S, device="cuda", dtype=torch.int32)

    def block():
        out = torch.full((k, k + 3), np.nan, device="cuda", dtype=torch.float64)
        L.check(lmm.load().lmm_dev_toeplitz_inverse_block(pd.data_ptr(), qd.data_ptr(), n, idx.data_ptr(), k, out.data_ptr(), k + 3))
        return out.cpu().numpy().T

    got, lo = block(), np.tril_indices(k)
    err = np.abs(got[lo] - Ti[np.ix_(S, S)][lo]).max() / np.abs(Ti).max()
    print(f"{kind} n={n} k={k} {shape}: {err:.2e}")
    assert err <= TOL
    assert np.isnan(got[:k][np.triu_indices(k, 1)]).all() and np.isnan(got[k:]).all()      # the triangle and nothing else
    assert np.array_equal(got, block(), equal_nan=True)                                    # two calls are bitwise equal


def problem(n, gaps, seed=0):
    """fx, Y (P_OUT x n), U; "partial": 40 scattered points miss one or two outputs; "all": also an outage of 130 points and both ends"""
    rng = np.random.default_rng(n + seed)
    U, Y = flat_orthogonal(rng, P_OUT, len(MIX)), rng.standard_normal((P_OUT, n))
    if gaps != "none":
        for t in rng.choice(np.arange(1, n - 1), 40, replace=False):
            Y[rng.choice(P_OUT, int(rng.integers(1, 3)), replace=False), t] = np.nan
    if gaps == "all":
        Y[:, [0, n - 1]] = np.nan
        Y[:, n // 2:n // 2 + 130] = np.nan
    ks = [CTOR[t[0][0]](*t[0][1:]) if len(t) == 1 else lmm.KernelSum(*[CTOR[c[0]](*c[1:]) for c in t]) for t in MIX]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, SV))
    return f(lmm.MOInputIsotopicByOutputs(0.5 + H * np.arange(n), P_OUT), S2), Y, U


def dense_gaussian(Y, U, n):
    """sum over the points with data of r_t, plus per latent the Gaussian of z over those points with noise S2 (G_t^-1)_ll"""
    ob = ~np.isnan(Y).all(axis=0)
    z, noise, ref, cond = restatement(Y[:, ob], U * np.sqrt(SV), S2)
    assert cond <= 1e3
    for l, terms in enumerate(MIX):
        A = toeplitz(row(terms, H * np.arange(n)))[np.ix_(ob, ob)] + np.diag(noise[:, l])
        ref += -0.5 * (z[:, l] @ np.linalg.solve(A, z[:, l]) + np.linalg.slogdet(A)[1] + ob.sum() * np.log(2 * np.pi))
    return ref


@pytest.mark.parametrize("n, blocked", ((1025, False), (1793, True)))      # 1793: two workgroups per latent, 29 launches of 64 steps
def test_value_against_dense_gaussian_of_observed_points(n, blocked):
    fx, Y, U = problem(n, "all")
    ref, got = dense_gaussian(Y, U, n), lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1), blocked)
    print(f"n={n} blocked={blocked}: {abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= TOL * abs(ref)
    assert got == lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1), blocked)                  # two calls are bitwise equal


@pytest.mark.parametrize("blocked", (False, True))
def test_complete_data_is_bitwise_toeplitz_logpdf_and_partial_data_agrees_with_the_dense_missing_path(blocked):
    fx, Y, _ = problem(1025, "none")
    assert lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1), blocked) == lmm.toeplitz_logpdf(fx, Y.reshape(-1), blocked=blocked)
    fx, Y, _ = problem(1025, "partial")                                                    # no point without data: the dense path drops those
    ref = lmm.logpdf(fx, Y.reshape(-1))
    assert abs(lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1), blocked) - ref) <= TOL * abs(ref)


def test_refusals():
    cap = lmm.load().lmm_toeplitz_missing_max_k()
    fx, Y, _ = problem(cap + 9, "none")
    Y[0, :cap + 1] = np.nan
    with pytest.raises(NotImplementedError, match=f"lmm_toeplitz_missing_max_k; k = {cap + 1}"):
        lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1))
    fx, Y, _ = problem(65, "none")
    Y[:3, 17] = np.nan
    with pytest.raises(NotImplementedError, match="point 17 observes 2 outputs"):
        lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1))
    Y[:] = np.nan
    with pytest.raises(ValueError, match="no point has an observed output"):
        lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1))
    lmm.set_compute_dtype("f32")
    try:
        with pytest.raises(NotImplementedError, match="Float64 only"):
            lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1))
    finally:
        lmm.set_compute_dtype("f64")
