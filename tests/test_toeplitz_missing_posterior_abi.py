"""The posterior for gappy grids on the Toeplitz path without a GPU (DESIGN.md 4.22 "Posterior handle for gappy grids"): a NumPy
restatement of  mean = k*' alpha-hat, alpha-hat = alpha - T^-1 J_S (d o M^-1 a),  var = kappa(0) - k*' T^-1 k* + |L_M^-1 (d o V[:, *])|^2,
V = (T^-1 K*)[S, :] = L(q)[S, :] Uq - L(p)[S, :] Up  against the dense Gaussian of the observed points; symbols."""
import functools
import os

import numpy as np

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_missing_abi import H, KINDS, NOISE, SIZES, generators, inverse_block, pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lmm_oilmm_toeplitz_posterior_create_missing", "lmm_toeplitz_post_gap_k", "lmm_dev_toeplitz_inverse_rows",
        "lmm_toeplitz_missing_post_last_ms")


def queries(n, gone, e, S):
    """inside the outage, on partially observed points (the one with e = 0 among them), between grid points, on either side of the grid"""
    part = S[~gone[S]]
    zero = part[e[part] == 0.0][:1]
    return H * np.concatenate([n // 3 + np.array([0.0, 7.0, 17.5, 34.0]), part[:3], zero, [3.5, n - 2.25], [-2.0, -0.3, n - 1 + 0.4, n + 3.0]])


@functools.lru_cache(maxsize=None)
def deltas():
    """largest errors over kinds and sizes: mean over max |reference|, variance over kappa(0), V over max |T^-1 K*|"""
    dm = dv = dV = 0.0
    for kind in KINDS:
        for n in SIZES:
            rng = np.random.default_rng(n)
            x = H * np.arange(n)
            t = row(LATENTS[kind], x); k0 = t[0]; t[0] += NOISE
            T = toeplitz(t)
            Ti = np.linalg.inv(T)
            p, q = generators(Ti)
            gone, e, S = pattern(n, rng)
            z = np.where(gone, 0.0, rng.standard_normal(n))
            xs = queries(n, gone, e, S)
            Ks = row(LATENTS[kind], np.abs(x[:, None] - xs[None, :]))
            d, f = np.where(gone[S], 1.0, np.sqrt(e[S])), np.where(gone[S], 0.0, 1.0)
            LM = np.linalg.cholesky(d[:, None] * inverse_block(p, q, S) * d[None, :] + np.diag(f))
            solve_M = lambda b: np.linalg.solve(LM.T, np.linalg.solve(LM, b))
            alpha = np.linalg.solve(T, z)
            rhs = np.zeros(n); rhs[S] = d * solve_M(d * alpha[S])
            mean = Ks.T @ (alpha - np.linalg.solve(T, rhs))
            Lq, Lp = np.tril(toeplitz(q)), np.tril(toeplitz(p))
            Uq, Up = Lq.T @ Ks, Lp.T @ Ks
            V = Lq[S] @ Uq - Lp[S] @ Up
            var = k0 - (Uq * Uq).sum(0) + (Up * Up).sum(0) + (np.linalg.solve(LM, d[:, None] * V) ** 2).sum(0)
            ob = ~gone
            C = (T + np.diag(e))[np.ix_(ob, ob)]
            mref = Ks[ob].T @ np.linalg.solve(C, z[ob])
            vref = k0 - (Ks[ob] * np.linalg.solve(C, Ks[ob])).sum(0)
            TK = Ti @ Ks
            dm = max(dm, np.abs(mean - mref).max() / np.abs(mref).max())
            dv = max(dv, np.abs(var - vref).max() / k0)
            dV = max(dV, np.abs(V - TK[S]).max() / np.abs(TK).max())
    return dm, dv, dV


def delta_toeplitz_missing_posterior():
    return max(deltas())


def test_restatement_matches_dense_gaussian_of_observed_points():
    dm, dv, dV = deltas()
    print(f"mean {dm:.2e}; variance {dv:.2e}; V {dV:.2e}")
    assert delta_toeplitz_missing_posterior() <= 1e-11


def test_symbols_and_prototypes():
    hdr, lib = open(os.path.join(ROOT, "include", "lmm_hip.h")).read(), lmm.load()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr and hasattr(lib, s)
    assert "toeplitz_posterior_missing" in lmm.__all__
