"""The Toeplitz posterior handle without a GPU (DESIGN.md 4.22 "Posterior handle"): a NumPy restatement of what the library computes per
latent -- var = kappa(0) - (|L(q)' k*|^2 - |L(p)' k*|^2) from the recursion's generators, mean = k*' alpha with alpha by the
Gohberg-Semencul products -- against the dense solve, at exactly the sizes the GPU test uses; symbols; the mirror's refusals."""
import functools
import os

import numpy as np
import pytest

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, _fx, row, schur, toeplitz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lmm_oilmm_toeplitz_posterior_create", "lmm_toeplitz_post_destroy", "lmm_oilmm_toeplitz_post_mean_and_var", "lmm_dev_toeplitz_predict")
R, Q = 256, 32                                  # toep_predict_kernel's row-block height and query-block width
SIZES = (1, 2, 3, R - 1, R + 1, 1025)           # the GPU test's
GRIDS = ((0.01, 0.125), (0.05, 0.05))           # (h, noise)


def queries(x0, h, n, ns):
    """ns queries, unsorted: before x_0, beyond x_{n-1}, exactly on grid points and between them"""
    rng = np.random.default_rng(ns)
    on = x0 + h * rng.integers(0, n, size=ns)
    xs = np.where(np.arange(ns) % 2 == 0, on, x0 + h * (n - 1) * rng.random(ns))
    xs[0], xs[ns // 2] = x0 + h * (n - 1) + 2.3 * h, x0 - 1.7 * h
    return xs


@functools.lru_cache(maxsize=None)
def deltas():
    """largest errors over kinds, grids and sizes: of var relative to kappa(0), as the sum of (u_q - u_p)(u_q + u_p) and as the
    difference of the two sums of squares, and of the mean relative to max |reference mean|"""
    dprod = dtwo = dmean = 0.0
    for terms in LATENTS.values():
        k0 = row(terms, 0.0)
        for h, w in GRIDS:
            for n in SIZES:
                x, r = 0.5 + h * np.arange(n), np.random.default_rng(n).standard_normal(n)
                xs = queries(0.5, h, n, Q + 1)
                t = row(terms, x - x[0]); t[0] += w
                Ks = row(terms, np.abs(x[:, None] - xs[None, :]))
                sol = np.linalg.solve(toeplitz(t), np.column_stack([Ks, r]))
                ref_var, ref_mean = k0 - np.sum(Ks * sol[:, :-1], axis=0), Ks.T @ sol[:, -1]
                _, _, p, q = schur(t, r)
                Lq, Lp = np.tril(toeplitz(q)), np.tril(toeplitz(p))
                uq, up = Lq.T @ Ks, Lp.T @ Ks
                alpha = Lq @ (Lq.T @ r) - Lp @ (Lp.T @ r)
                dprod = max(dprod, np.abs(k0 - np.sum((uq - up) * (uq + up), axis=0) - ref_var).max() / k0)
                dtwo = max(dtwo, np.abs(k0 - (np.sum(uq * uq, axis=0) - np.sum(up * up, axis=0)) - ref_var).max() / k0)
                dmean = max(dmean, np.abs(Ks.T @ alpha - ref_mean).max() / np.abs(ref_mean).max())
    return dprod, dtwo, dmean


def delta_toeplitz_posterior_var():
    return deltas()[0]


def delta_toeplitz_posterior_mean():
    return deltas()[2]


def test_restatement_matches_dense_solve():
    dprod, dtwo, dmean = deltas()
    print(f"var, product form {dprod:.2e}; var, two sums {dtwo:.2e}; mean {dmean:.2e}")
    assert dprod <= 1e-10 and dmean <= 1e-10      # measured: 2.4e-11 (as two sums: 2.8e-11) and 3.0e-11


def test_symbols_and_prototypes():
    hdr = open(os.path.join(ROOT, "include", "lmm_hip.h")).read()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr


def test_mirror_refusals_reach_no_library_call():
    x = np.linspace(0.0, 1.0, 9)
    with pytest.raises(ValueError, match=r"x\[4\]"):
        xb = x.copy(); xb[4] += 1e-6
        lmm.toeplitz_posterior(_fx(xb), np.zeros(27))
    with pytest.raises(ValueError, match="length"):
        lmm.toeplitz_posterior(_fx(x), np.zeros(26))
    with pytest.raises(NotImplementedError, match="matrix Y"):
        lmm.toeplitz_posterior(_fx(x), np.zeros((27, 2)))
    post = lmm.ToeplitzPosterior(object(), 9, 3, 0.0)      # a handle that no library call may reach
    try:
        with pytest.raises(ValueError, match=r"\(ns,\)"):
            post.mean_and_var(np.zeros((2, 2)))
        with pytest.raises(ValueError, match="finite"):
            post.mean(np.array([0.0, np.inf]))
        assert post.var(np.zeros(0)).shape == (0,)
    finally:
        post._ptr = None
    with pytest.raises(ValueError, match="closed"):
        post.mean_and_var(x)
