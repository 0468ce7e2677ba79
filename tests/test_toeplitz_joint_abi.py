"""The joint predictive of the Toeplitz posterior handle without a GPU (DESIGN.md 4.22 "Joint predictive"): a NumPy restatement of
C = K** - (Uq' Uq - Up' Up), Uq = L(q)' K*, Up = L(p)' K*, from the recursion's generators against K** - K*' solve(K, K*), and of the
log density and the paths built on it; the mirror's refusals.  The rand delta is taken at well-separated queries and at the
jitter JITTER kappa(0): a Cholesky factor amplifies the error of C by about kappa(0) / (d + lambda_min(C)); at 1e-3 kappa(0): 1.7e-9."""
import functools

import numpy as np
import pytest

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, row, schur, toeplitz
from test_toeplitz_posterior_abi import GRIDS, Q, SIZES, queries

JOINT_SIZES = SIZES[:-1] + (513,)               # the GPU test's (1025 there is 513 here: three row blocks)
JITTER = 1e-2                                   # of kappa(0): the diagonal term of the rand tests
RAND_NS = 9


def rand_queries(x0, h, n, ns=RAND_NS):
    """ns well-separated queries from a quarter of the grid's span before it to a quarter beyond it, off the grid points"""
    return x0 + h * (n - 1) * np.linspace(-0.25, 1.25, ns) + 0.37 * h


def gauss(A, v):
    return -0.5 * (v @ np.linalg.solve(A, v) + np.linalg.slogdet(A)[1] + len(v) * np.log(2.0 * np.pi))


@functools.lru_cache(maxsize=None)
def deltas():
    """largest errors over kinds, grids and sizes: of C relative to kappa(0), as two Grams and in the product form
    1/2 (D' S + S' D), D = Uq - Up, S = Uq + Up; of the predictive log density relative to |log N(train + held-out) - log N(train)|;
    of the paths mu* + chol(C + JITTER kappa(0) I) zeta relative to max |the same from the reference C|"""
    dtwo = dprod = dlog = drand = 0.0
    for terms in LATENTS.values():
        k0 = row(terms, 0.0)
        for h, w in GRIDS:
            for n in JOINT_SIZES:
                x, r = 0.5 + h * np.arange(n), np.random.default_rng(n).standard_normal(n)
                t = row(terms, x - x[0]); t[0] += w
                K = toeplitz(t)
                _, _, p, q = schur(t, r)
                Lq, Lp = np.tril(toeplitz(q)), np.tril(toeplitz(p))
                for xs in (queries(0.5, h, n, Q + 1), rand_queries(0.5, h, n)):
                    ns = len(xs)
                    Ks, Kss = row(terms, np.abs(x[:, None] - xs[None, :])), row(terms, np.abs(xs[:, None] - xs[None, :]))
                    sol = np.linalg.solve(K, np.column_stack([Ks, r]))
                    ref, mu = Kss - Ks.T @ sol[:, :-1], Ks.T @ sol[:, -1]
                    ref = 0.5 * (ref + ref.T)
                    uq, up = Lq.T @ Ks, Lp.T @ Ks
                    C = Kss - (uq.T @ uq - up.T @ up)
                    if ns == Q + 1:
                        D, S = uq - up, uq + up
                        dtwo = max(dtwo, np.abs(C - ref).max() / k0)
                        dprod = max(dprod, np.abs(Kss - 0.5 * (D.T @ S + S.T @ D) - ref).max() / k0)
                        ys = np.random.default_rng(n + 1).standard_normal(ns)
                        want = gauss(np.block([[K, Ks], [Ks.T, Kss + w * np.eye(ns)]]), np.concatenate([r, ys])) - gauss(K, r)
                        dlog = max(dlog, abs(gauss(C + w * np.eye(ns), ys - mu) - want) / abs(want))
                    else:
                        z, d = np.random.default_rng(n + 2).standard_normal(ns), JITTER * k0 * np.eye(ns)
                        a, b = mu + np.linalg.cholesky(C + d) @ z, mu + np.linalg.cholesky(ref + d) @ z
                        drand = max(drand, np.abs(a - b).max() / np.abs(b).max())
    return dtwo, dprod, dlog, drand


def delta_toeplitz_joint_cov():
    return deltas()[0]


def delta_toeplitz_predictive():
    return deltas()[2]


def delta_toeplitz_joint_rand():
    return deltas()[3]


def test_restatement_matches_dense_solve():
    dtwo, dprod, dlog, drand = deltas()
    print(f"C, two Grams {dtwo:.2e}; C, product form {dprod:.2e}; predictive {dlog:.2e}; rand {drand:.2e}")
    # measured: 8.2e-12 (product form 7.3e-12, at twice the MFMAs: the kernel takes the two Grams), 1.4e-10, 6.0e-10
    assert dtwo <= 1e-10 and dlog <= 1e-9 and drand <= 1e-9


def test_mirror_refusals_never_use_the_handle():
    post, rng = lmm.ToeplitzPosterior(object(), 9, 3, 0.0, 2), np.random.default_rng(0)      # a handle that no library call could take
    calls = (lambda xs, **kw: post.predictive_logpdf(xs, np.zeros(6), **kw), lambda xs, **kw: post.rand(rng, xs=xs, **kw))
    try:
        for call in calls:
            with pytest.raises(ValueError, match=r"\(ns,\)"):
                call(np.zeros((2, 1)))
            with pytest.raises(ValueError, match="finite"):
                call(np.array([0.0, np.nan]))
        for kw, msg in ((dict(horizon=1), "horizon must be 0"), (dict(N=0), "N is None or")):
            with pytest.raises(ValueError, match=msg):
                calls[1](np.zeros(2), **kw)
        with pytest.raises(ValueError, match=r"ns \* p = 6"):
            post.predictive_logpdf(np.zeros(2), np.zeros(5))
        with pytest.raises(ValueError, match="sigma2 must be finite and > 0"):
            calls[0](np.zeros(2), sigma2=0.0)
        assert post.predictive_logpdf(np.zeros(0), np.zeros(0)) == 0.0
    finally:
        post._ptr = None
