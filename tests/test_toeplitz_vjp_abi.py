"""ToeplitzPosterior.mean_and_var_vjp without a GPU (DESIGN.md 4.22 "Gradients with respect to the queries"): a NumPy restatement of what
the library computes per latent -- d var / d xs = -2 (u_q . u'_q - u_p . u'_p) from the recursion's generators, d mean / d xs = k*' . alpha
-- against the dense solve at the sizes the GPU test uses; symbols; the mirror's refusals.  d kappa / d xs is a complex step through
test_toeplitz_abi.row, so no derivative formula is shared with the library."""
import functools
import os

import numpy as np
import pytest

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, ROOT, row, schur, toeplitz
from test_toeplitz_posterior_abi import GRIDS, SIZES, queries

SYMS = ("lmm_oilmm_toeplitz_post_mean_and_var_grad_xs", "lmm_dev_toeplitz_predict_grad")
NS = 33


def drow(terms, delta):
    """d kappa(xs - x) / d xs at delta = xs - x; a coincident pair gives exactly 0 (sign(0) = 0)"""
    return np.sign(delta) * row(terms, np.abs(delta) + 1e-30j).imag / 1e-30


@functools.lru_cache(maxsize=None)
def deltas():
    """largest errors over kinds, grids and sizes: of d var / d xs relative to max |d K* / d xs| in the three summation forms (the sum of
    u_q u'_q - u_p u'_p, the difference of the two sums, the half-sum of the mixed products), and of d mean / d xs relative to max |reference|"""
    dvar, dmean = np.zeros(3), 0.0
    for terms in LATENTS.values():
        for h, w in GRIDS:
            for n in SIZES:
                x, r = 0.5 + h * np.arange(n), np.random.default_rng(n).standard_normal(n)
                dl = queries(0.5, h, n, NS)[None, :] - x[:, None]
                t = row(terms, x - x[0]); t[0] += w
                Ks, dKs = row(terms, np.abs(dl)), drow(terms, dl)
                sol = np.linalg.solve(toeplitz(t), np.column_stack([Ks, r]))
                ref_dv, ref_dm = -2.0 * np.sum(dKs * sol[:, :-1], axis=0), dKs.T @ sol[:, -1]
                _, _, p, q = schur(t, r)
                Lq, Lp = np.tril(toeplitz(q)), np.tril(toeplitz(p))
                uq, up, vq, vp = Lq.T @ Ks, Lp.T @ Ks, Lq.T @ dKs, Lp.T @ dKs
                alpha = Lq @ (Lq.T @ r) - Lp @ (Lp.T @ r)
                forms = (np.sum(uq * vq - up * vp, axis=0), np.sum(uq * vq, axis=0) - np.sum(up * vp, axis=0),
                         0.5 * np.sum((uq - up) * (vq + vp) + (uq + up) * (vq - vp), axis=0))
                dvar = np.maximum(dvar, [np.abs(-2.0 * f - ref_dv).max() / np.abs(dKs).max() for f in forms])
                dmean = max(dmean, np.abs(dKs.T @ alpha - ref_dm).max() / np.abs(ref_dm).max())
    return tuple(dvar), dmean


def delta_toeplitz_vjp_var():
    return deltas()[0][0]           # the form toep_predict_grad_kernel sums


def delta_toeplitz_vjp_mean():
    return deltas()[1]


def test_restatement_matches_dense_solve():
    dvar, dmean = deltas()
    print(f"d var, sum of differences {dvar[0]:.2e}; two sums {dvar[1]:.2e}; mixed products {dvar[2]:.2e}; d mean {dmean:.2e}")
    assert delta_toeplitz_vjp_var() <= 1e-10 and delta_toeplitz_vjp_mean() <= 1e-10


def test_symbols_and_prototypes():
    hdr, lib = open(os.path.join(ROOT, "include", "lmm_hip.h")).read(), lmm.load()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr and hasattr(lib, s)


def test_mirror_refusals_reach_no_library_call():
    post = lmm.ToeplitzPosterior(object(), 9, 3, 0.0)      # a handle that no library call may reach
    try:
        for xs, kw, match in ((np.zeros((2, 2)), {"dmean": np.zeros(12)}, r"\(ns,\)"), (np.array([0.0, np.inf]), {"dvar": np.zeros(6)}, "finite"),
                              (np.zeros(2), {}, "both None"), (np.zeros(2), {"dvar": np.zeros(5)}, r"dvar holds ns \* p = 6"),
                              (np.zeros(2), {"dmean": np.zeros((2, 3))}, r"dmean holds ns \* p = 6")):
            with pytest.raises(ValueError, match=match):
                post.mean_and_var_vjp(xs, **kw)
        assert post.mean_and_var_vjp(np.zeros(0), np.zeros(0))["x"].shape == (0,)
    finally:
        post._ptr = None
    with pytest.raises(ValueError, match="closed"):
        post.mean_and_var_vjp(np.zeros(2), np.zeros(6))
