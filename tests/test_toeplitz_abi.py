"""The Toeplitz path without a GPU: the Schur recursion and its gradient formulas in NumPy against the dense Gaussian
(slogdet, solve, inv) and the dense analytic gradient 1/2 tr((alpha alpha' - K^-1) dK); symbols; the mirror's refusals.  dK / d theta
is the complex-step derivative of the kernel formula below (exact to rounding), so no derivative code is shared with the library."""
import os

import numpy as np
import pytest

import lmm_amd as lmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lmm_toeplitz_max_n", "lmm_oilmm_logpdf_toeplitz", "lmm_oilmm_logpdf_grad_toeplitz", "lmm_dev_toeplitz_factor", "lmm_dev_toeplitz_solve")
SIZES = (1, 2, 3, 65, 257)
# a latent: its terms (kind, variance, lengthscale or period, shape: RQ alpha / periodic r / SHO quality, locally periodic decay)
LATENTS = {
    "se": [("se", 1.0, 0.7)], "rq": [("rq", 1.3, 0.9, 1.5)], "periodic": [("periodic", 1.0, 1.7, 0.8)], "lp": [("lp", 0.9, 1.1, 1.2, 2.5)],
    "matern52": [("matern52", 1.0, 1.4)], "sum": [("se", 1.0, 0.7), ("periodic", 1.0, 1.7, 0.8)],
    "sho": [("sho", 1.1, 1.9, 2.0)], "matern12": [("matern12", 0.8, 1.2)], "matern32": [("matern32", 1.2, 0.6)],
}
ISSUE_KINDS = ("se", "rq", "periodic", "lp", "matern52", "sum")


def row(terms, d, eps=None):
    """t_d = sum over the terms of kappa(d); eps = (c, j): parameter j of term c carries the complex step"""
    out = 0.0
    for c, (kind, *par) in enumerate(terms):
        par = [complex(v, 1e-30) if eps == (c, j) else v for j, v in enumerate(par)] + [1.0, 1.0]
        v, l, s, dc = par[:4]
        u = d / l
        if kind == "se":
            k = np.exp(-0.5 * u * u)
        elif kind == "rq":
            k = (1.0 + u * u / (2.0 * s)) ** (-s)
        elif kind in ("periodic", "lp"):
            k = np.exp(-np.sin(np.pi * u) ** 2 / (2.0 * s * s) - (d * d / (2.0 * dc * dc) if kind == "lp" else 0.0))
        elif kind == "sho":
            h = np.sqrt(1.0 - 1.0 / (4.0 * s * s))
            k = np.exp(-np.pi * u / s) * (np.cos(2 * np.pi * h * u) + np.sin(2 * np.pi * h * u) / (2.0 * h * s))
        else:
            q = np.sqrt({"matern12": 1.0, "matern32": 3.0, "matern52": 5.0}[kind]) * u
            k = {"matern12": 1.0, "matern32": 1.0 + q, "matern52": 1.0 + q + q * q / 3.0}[kind] * np.exp(-q)
        out = out + v * k
    return out


def toeplitz(t):
    n = len(t)
    return t[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])]


def dense_latent(terms, lags, w, r):
    """One latent's dense Gaussian: lml, alpha, d lml / d w, {(c, j): d lml / d theta}"""
    n, K = len(r), toeplitz(row(terms, lags)) + w * np.eye(len(r))
    Ki, alpha = np.linalg.inv(K), np.linalg.solve(K, r)
    W = np.outer(alpha, alpha) - Ki
    lml = -0.5 * (r @ alpha + np.linalg.slogdet(K)[1] + n * np.log(2 * np.pi))
    return lml, alpha, 0.5 * np.trace(W), {(c, j): 0.5 * np.sum(W * toeplitz(row(terms, lags, (c, j)).imag / 1e-30)) for c, t in enumerate(terms) for j in range(len(t) - 1)}, K, Ki


def schur(t, r):
    """The recursion as toep_schur_kernel runs it: log det, r' K^-1 r and the generators p, q of K^-1"""
    n, s = len(t), np.sqrt(t[0])
    a = t / s
    b = a.copy(); b[0] = 0.0
    p = np.zeros(n); p[0] = 1.0 / s
    q, r = p.copy(), r.copy()
    logdet = quad = 0.0
    for k in range(n):
        assert a[k] > 0.0
        logdet += 2.0 * np.log(a[k])
        z = r[k] / a[k]
        quad += z * z
        r[k + 1:] -= a[k + 1:] * z
        p[1:] = p[:-1].copy(); p[0] = 0.0
        if k == n - 1:
            break
        a[k + 1:] = a[k:-1].copy()
        rho = b[k + 1] / a[k + 1]
        assert abs(rho) < 1.0
        c = np.sqrt((1.0 - rho) * (1.0 + rho))
        an = (a[k + 1:] - rho * b[k + 1:]) / c
        b[k + 1:] = c * b[k + 1:] - rho * an
        a[k + 1:] = an
        pn = (p[:k + 2] - rho * q[:k + 2]) / c
        q[:k + 2] = c * q[:k + 2] - rho * pn
        p[:k + 2] = pn
    return logdet, quad, p, q


def _deltas():
    """largest errors relative to max |reference| over kinds and sizes: of (log det, r' K^-1 r, alpha, the diagonal sums of K^-1), and
    of the gradient (d lml / d theta by the lag contraction, d lml / d w) against the dense analytic one"""
    dv = dg = 0.0
    for name in ISSUE_KINDS:
        terms = LATENTS[name]
        for n in SIZES:
            lags, r = 0.05 * np.arange(n), np.random.default_rng(n).standard_normal(n)
            t = row(terms, lags); t[0] += 0.05
            _, alpha, gw, gth, K, Ki = dense_latent(terms, lags, 0.05, r)
            assert np.linalg.cond(K) <= 1e5, (name, n)
            logdet, quad, p, q = schur(t, r)
            Lq, Lp = np.tril(toeplitz(q)), np.tril(toeplitz(p))
            al = Lq @ (Lq.T @ r) - Lp @ (Lp.T @ r)
            sd = np.array([sum((n - d - j) * (q[j] * q[j + d] - p[j] * p[j + d]) for j in range(n - d)) for d in range(n)])
            ad = np.array([al[:n - d] @ al[d:] for d in range(n)])
            ref_sd, ref_ld = np.array([np.trace(Ki, d) for d in range(n)]), np.linalg.slogdet(K)[1]
            dv = max(dv, abs(logdet - ref_ld) / max(1.0, abs(ref_ld)), abs(quad - r @ alpha) / abs(r @ alpha),
                     np.abs(al - alpha).max() / np.abs(alpha).max(), np.abs(sd - ref_sd).max() / np.abs(ref_sd).max())
            m = np.where(np.arange(n) == 0, 1.0, 2.0)
            got = [0.5 * np.sum(m * (ad - sd) * row(terms, lags, cj).imag / 1e-30) for cj in gth] + [0.5 * (ad[0] - sd[0])]
            ref = np.array(list(gth.values()) + [gw])
            dg = max(dg, np.abs(np.array(got) - ref).max() / np.abs(ref).max())
    return dv, dg


def delta_toeplitz():
    return _deltas()[0]


def delta_toeplitz_grad():
    return _deltas()[1]


def test_recursion_and_gradient_match_dense_gaussian():
    assert max(_deltas()) <= 1e-11      # measured: 7.8e-14 and 1.6e-14


def test_symbols_and_prototypes():
    hdr = open(os.path.join(ROOT, "include", "lmm_hip.h")).read()
    for s in SYMS:
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr


def _fx(x, sigma2=0.1, p=3):
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.SEKernel()), lmm.GP(lmm.PeriodicKernel())]), lmm.Orthogonal(np.eye(p)[:, :2], np.array([1.0, 2.0])))
    return f(lmm.MOInputIsotopicByOutputs(x, p), sigma2)


@pytest.mark.parametrize("fn", (lmm.toeplitz_logpdf, lmm.toeplitz_logpdf_and_gradient))
def test_mirror_refusals_reach_no_library_call(fn):
    x = np.linspace(0.0, 1.0, 9)
    with pytest.raises(ValueError, match=r"x\[4\]"):
        xb = x.copy(); xb[4] += 1e-6
        fn(_fx(xb), np.zeros(27))
    with pytest.raises(ValueError, match="length"):
        fn(_fx(x), np.zeros(26))
    with pytest.raises(NotImplementedError, match="matrix Y"):
        fn(_fx(x), np.zeros((27, 2)))
    with pytest.raises(NotImplementedError, match="IndependentMOGP"):
        f = lmm.independent_mogp([lmm.GP(lmm.SEKernel())])
        fn(f(lmm.MOInputIsotopicByOutputs(x, 1), 0.1), np.zeros(9))
