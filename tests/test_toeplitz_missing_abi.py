"""Missing observations on the Toeplitz path without a GPU (DESIGN.md 4.22 "Missing observations"): a NumPy restatement of
log N = -1/2 [z' alpha - a' M^-1 a + log det T + log det M + n_obs log 2 pi], M = D B D + F, B = (T^-1)[S, S] from the generators, against
the dense Gaussian of the observed points; symbols.  The generators come from the first column of inv(T) (Gohberg-Semencul)."""
import functools
import os

import numpy as np

import lmm_amd as lmm
from test_toeplitz_abi import LATENTS, row, toeplitz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lmm_toeplitz_missing_max_k", "lmm_oilmm_logpdf_toeplitz_missing", "lmm_dev_toeplitz_inverse_block", "lmm_toeplitz_missing_last_ms")
KINDS, SIZES, NOISE, H = ("se", "matern52", "lp"), (129, 1025), 0.1, 0.05


def generators(Ti):
    """p, q with T^-1 = L(q) L(q)' - L(p) L(p)' from the first column of T^-1"""
    c = Ti[:, 0]
    return np.concatenate([[0.0], c[:0:-1]]) / np.sqrt(c[0]), c / np.sqrt(c[0])


def inverse_block(p, q, S):
    """B[i][j] = sum_{c <= min(s_i, s_j)} q[s_i - c] q[s_j - c] - p[s_i - c] p[s_j - c]"""
    Aq, Ap = np.tril(toeplitz(q))[S], np.tril(toeplitz(p))[S]
    return Aq @ Aq.T - Ap @ Ap.T


def pattern(n, rng):
    """(gone, e): a run of 35 points without data plus points 0 and n - 1; 32 points with extra noise e_t, one of them with e = 0"""
    gone = np.zeros(n, bool)
    gone[[0, n - 1]] = True
    gone[n // 3:n // 3 + 35] = True
    part = rng.choice(np.flatnonzero(~gone), 32, replace=False)
    e = np.zeros(n)
    e[part] = rng.uniform(0.01, 0.3, 32)
    e[part[0]] = 0.0
    return gone, e, np.sort(np.concatenate([np.flatnonzero(gone), part]))


@functools.lru_cache(maxsize=None)
def deltas():
    """largest errors over kinds and sizes: of the block relative to max |T^-1|, of the value relative to |reference|"""
    db = dv = 0.0
    for kind in KINDS:
        for n in SIZES:
            rng = np.random.default_rng(n)
            t = row(LATENTS[kind], H * np.arange(n)); t[0] += NOISE
            T = toeplitz(t)
            Ti = np.linalg.inv(T)
            p, q = generators(Ti)
            gone, e, S = pattern(n, rng)
            z = np.where(gone, 0.0, rng.standard_normal(n))
            B = inverse_block(p, q, S)
            db = max(db, np.abs(B - Ti[np.ix_(S, S)]).max() / np.abs(Ti).max())
            d, f = np.where(gone[S], 1.0, np.sqrt(e[S])), np.where(gone[S], 0.0, 1.0)
            M = d[:, None] * B * d[None, :] + np.diag(f)
            alpha = np.linalg.solve(T, z)
            a = d * alpha[S]
            ob = ~gone
            got = -0.5 * (z @ alpha - a @ np.linalg.solve(M, a) + np.linalg.slogdet(T)[1] + np.linalg.slogdet(M)[1] + ob.sum() * np.log(2 * np.pi))
            C = (T + np.diag(e))[np.ix_(ob, ob)]
            ref = -0.5 * (z[ob] @ np.linalg.solve(C, z[ob]) + np.linalg.slogdet(C)[1] + ob.sum() * np.log(2 * np.pi))
            dv = max(dv, abs(got - ref) / abs(ref))
    return db, dv


def delta_toeplitz_missing():
    return max(deltas())


def test_restatement_matches_dense_gaussian_of_observed_points():
    db, dv = deltas()
    print(f"block {db:.2e}; value {dv:.2e}")
    assert delta_toeplitz_missing() <= 1e-11      # measured: block 6.9e-15, value 3.1e-15


def test_symbols_and_prototypes():
    hdr, lib = open(os.path.join(ROOT, "include", "lmm_hip.h")).read(), lmm.load()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr and hasattr(lib, s)
    assert "toeplitz_logpdf_missing" in lmm.__all__
