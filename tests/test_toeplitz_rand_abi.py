"""Sampling on the Toeplitz path without a GPU (DESIGN.md 4.22 "Sampling"): the sampling recursion and the conditioning formula in NumPy
against dense NumPy (cholesky(K + jitter I) @ zeta, the dense Matheron expression, the dense Gaussian posterior over grid + horizon);
symbols; the mirror's refusals.  Every matrix whose Cholesky factor the reference takes has condition number <= 1e5 (asserted): SE
at h = its lengthscale, the periodic kinds with an explicit jitter (their Grams have a numerical rank of a few dozen whatever h is)."""
import os

import numpy as np
import pytest

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, ROOT, _fx, row, schur, toeplitz

SYMS = ("lmm_oilmm_rand_toeplitz", "lmm_oilmm_toeplitz_post_rand", "lmm_toeplitz_rand_last_ms", "lmm_dev_toeplitz_sample")
H_GRID, W = 0.7, 0.15
CASES = (("se", 1e-18), ("matern52", 1e-18), ("periodic", 1e-2), ("lp", 1e-3), ("sum", 1e-2))      # kind, jitter of the prior
SHAPES = ((1, 0), (2, 1), (3, 0), (65, 7), (130, 3))      # n, horizon


def schur_sample(t, Z):
    """F = L Z with L L' = Toeplitz(t), as toep_schur_sample_kernel runs it: before step k shifts it, a is column k of L"""
    n, s = len(t), np.sqrt(t[0])
    a = t / s
    a[0] = s
    b, F = a.copy(), np.zeros_like(Z)
    for k in range(n):
        assert a[k] > 0.0
        F[k:] += np.outer(a[k:], Z[k])
        if k == n - 1:
            break
        a[k + 1:] = a[k:-1].copy()
        rho = b[k + 1] / a[k + 1]
        assert abs(rho) < 1.0
        c = np.sqrt((1.0 - rho) * (1.0 + rho))
        an = (a[k + 1:] - rho * b[k + 1:]) / c
        b[k + 1:] = c * b[k + 1:] - rho * an
        a[k + 1:] = an
    return F


def condition(t0, n, w, p, q, alpha, mu, f, xi):
    """The handle's pathwise conditioning: mu + f + T(t0) g, g = alpha - (K + w I)^-1 (f[0:n] + sqrt(w) xi) by the generators p, q"""
    Lq, Lp, Lt = np.tril(toeplitz(q)), np.tril(toeplitz(p)), np.tril(toeplitz(t0))
    d = f[:n] + np.sqrt(w) * xi
    g = np.zeros(len(t0))
    g[:n] = alpha - (Lq @ (Lq.T @ d) - Lp @ (Lp.T @ d))
    return mu + f + Lt @ g + Lt.T @ g - t0[0] * g


def _chol(A):
    assert np.linalg.cond(A) <= 1e5
    return np.linalg.cholesky(A)


def _deltas():
    """largest errors relative to max |reference|: of the prior path; of the posterior path and its implied mean and covariance"""
    dp = dq = 0.0
    for (name, jitter), (n, hz) in ((c, s) for c in CASES for s in SHAPES):
        nt, rng = n + hz, np.random.default_rng(n)
        t0 = row(LATENTS[name], H_GRID * np.arange(nt))
        K, tj = toeplitz(t0), t0 + jitter * (np.arange(nt) == 0)
        Z, xi, r, mu = rng.standard_normal((nt, 2)), rng.standard_normal(n), rng.standard_normal(n), 0.3
        ref = _chol(K + jitter * np.eye(nt)) @ Z
        F = schur_sample(tj, Z)
        dp = max(dp, np.abs(F - ref).max() / np.abs(ref).max())
        Kw = K[:n, :n] + W * np.eye(n)
        cf = _chol(Kw)
        solve = lambda v: np.linalg.solve(cf.T, np.linalg.solve(cf, v))
        tw = t0[:n].copy(); tw[0] += W
        _, _, p, q = schur(tw, r)
        alpha, G = solve(r), K[:, :n] @ np.linalg.inv(Kw)
        got = condition(t0, n, W, p, q, alpha, mu, F[:, 0], xi)
        want = mu + ref[:, 0] + G @ (r - ref[:n, 0] - np.sqrt(W) * xi)      # the dense Matheron expression
        dq = max(dq, np.abs(got - want).max() / np.abs(want).max())
        # the path is affine in (zeta, xi): its mean from zero normals, its covariance from unit normals
        m0 = condition(t0, n, W, p, q, alpha, mu, np.zeros(nt), np.zeros(n))
        Fe = schur_sample(tj, np.eye(nt))
        A = np.array([condition(t0, n, W, p, q, alpha, mu, Fe[:, j], np.zeros(n)) - m0 for j in range(nt)] +
                     [condition(t0, n, W, p, q, alpha, mu, np.zeros(nt), e) - m0 for e in np.eye(n)]).T
        M = np.eye(nt); M[:, :n] -= G      # the dense Gaussian posterior of a prior K + jitter I conditioned through cov(f, f_x) = K
        cov = M @ (K + jitter * np.eye(nt)) @ M.T + W * G @ G.T
        dq = max(dq, np.abs(m0 - (mu + K[:, :n] @ alpha)).max() / np.abs(mu + K[:, :n] @ alpha).max(), np.abs(A @ A.T - cov).max() / np.abs(cov).max())
    return dp, dq


def delta_toeplitz_rand():
    return _deltas()[0]


def delta_toeplitz_post_rand():
    return _deltas()[1]


def test_sampling_recursion_and_conditioning_match_dense():
    dp, dq = _deltas()
    print(f"delta_toeplitz_rand {dp:.2e}, delta_toeplitz_post_rand {dq:.2e}")
    assert max(dp, dq) <= 1e-11


def test_symbols_and_prototypes():
    hdr = open(os.path.join(ROOT, "include", "lmm_hip.h")).read()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr
    assert "toeplitz_rand" in lmm.__all__ and hasattr(lmm.ToeplitzPosterior, "rand")


@pytest.mark.parametrize("kw, err, match", (
    (dict(horizon=-1), ValueError, "horizon"), (dict(horizon=1.5), ValueError, "horizon"), (dict(N=0), ValueError, "N is None"),
    (dict(jitter=-1e-3), ValueError, "jitter"), (dict(jitter=np.inf), ValueError, "jitter"),
    (dict(horizon=lmm.load().lmm_toeplitz_blocked_max_n()), NotImplementedError, "n \\+ horizon")))
def test_mirror_refusals_reach_no_library_call(kw, err, match):
    x, rng = np.linspace(0.0, 1.0, 9), np.random.default_rng(0)
    post = lmm.ToeplitzPosterior(1, 9, 3, 0.0, 2)      # never dereferenced: every refusal comes first
    try:
        for call in (lambda: lmm.toeplitz_rand(rng, _fx(x), **kw), lambda: lmm.toeplitz_rand(rng, _fx(x), np.zeros(27), **kw),
                     lambda: post.rand(rng, **kw)):
            with pytest.raises(err, match=match):
                call()
        with pytest.raises(ValueError, match=r"x\[4\]"):
            xb = x.copy(); xb[4] += 1e-6
            lmm.toeplitz_rand(rng, _fx(xb))
    finally:
        post._ptr = None
    with pytest.raises(ValueError, match="closed"):
        post.rand(rng)
