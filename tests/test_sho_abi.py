"""Host-only checks of SHO (damped-oscillator) latents (include/lmm_hip.h LMM_KERNEL_SHO and "state space"): the
kernel, its closed-form derivatives and the oscillator's state-space model restated in NumPy; the sequential Kalman filter / RTS
smoother on that model against the dense Gaussian of the kernel (value, filtered and smoothed marginals) and its tangent filter
against the dense analytic gradient; the Python mirror (SHOKernel, descriptors, tags), the header / mirror constants and prototypes,
tag misuse and the refusals, which come before any library call.  No GPU and no lmm_init needed.

delta() and delta_grad() are the largest disagreements of the restatement with the dense Gaussian over Q in {0.51, 2, 50}, with ties
in x and unobserved points; they fix the GPU tolerances of tests/test_gpu_sho.py, max(1e-10, 100 delta), which imports the restatement
from here.

`python tests/test_sho_abi.py` prints the disagreements."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lmm_amd
from lmm_amd import _lib as L

import test_statespace_abi as T

HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SHIM = os.path.join(ROOT, "linearmixingmodels.jl_amd", "julia", "LinearMixingModelsHIP.jl")
QS = (0.51, 2.0, 50.0)
CPU_N = (1, 2, 3, 63, 257)
LOG2PI = T.LOG2PI
STEP = 1e-30


# ---- the kernel, restated -------------------------------------------------------------------------------------------------------
def sho_consts(P, Q):
    """(w0, a, eta): w0 = 2 pi / P, a = w0 / (2 Q), eta = w0 sqrt(1 - 1 / (4 Q^2)) (real or complex P, Q)."""
    w0 = 2.0 * np.pi / P
    return w0, w0 / (2.0 * Q), w0 * np.sqrt((2.0 * Q - 1.0) * (2.0 * Q + 1.0)) / (2.0 * Q)


def k_sho(v, P, Q, tau):
    """k(tau) = v exp(-a tau) (cos(eta tau) + (a / eta) sin(eta tau)), tau >= 0."""
    _, a, eta = sho_consts(P, Q)
    return v * np.exp(-a * tau) * (np.cos(eta * tau) + (a / eta) * np.sin(eta * tau))


def dk_sho(v, P, Q, tau):
    """(dk / dv, dk / dP, dk / dQ) in closed form.  With c = a / eta = 1 / (2 Q s), s = sqrt(1 - 1 / (4 Q^2)): a and eta scale with w0
    and c does not, so dk / dw0 = -tau w0 v exp(-a tau) sin(eta tau) / eta (the cosine terms cancel through eta c = a and a c + eta =
    w0^2 / eta) and dk / dP = -(w0 / P) dk / dw0; in Q, a_Q = -a / Q, eta_Q = w0 / (4 Q^3 s), c_Q = -(2 s + 1 / (2 Q^2 s)) / (2 Q s)^2."""
    w0, a, eta = sho_consts(P, Q)
    s = eta / w0
    c = a / eta
    e, cs, sn = np.exp(-a * tau), np.cos(eta * tau), np.sin(eta * tau)
    dP = tau * w0 * w0 * v * e * sn / (eta * P)
    aQ, etaQ = -a / Q, w0 / (4.0 * Q ** 3 * s)
    cQ = -(2.0 * s + 1.0 / (2.0 * Q * Q * s)) / (2.0 * Q * s) ** 2
    dQ = v * e * (-aQ * tau * (cs + c * sn) + etaQ * tau * (c * cs - sn) + cQ * sn)
    return e * (cs + c * sn), dP, dQ


def sho_K(v, P, Q, x, x2=None):
    x2 = x if x2 is None else x2
    return k_sho(v, P, Q, np.abs(np.asarray(x)[:, None] - np.asarray(x2)[None, :]))


# ---- the state-space models: the oscillator, and the Matern ones of test_statespace_abi behind the same interface -----------------
class Model:
    """D, Pinf and AQ(dt) -> (A(dt), Q(dt) = Pinf - A Pinf A') of one latent; K(x, x2) its kernel matrix."""

    def __init__(self, kind, v, ell, quality=None):
        self.kind, self.v, self.ell, self.quality = kind, v, ell, quality
        if kind == "sho":
            w0, a, eta = sho_consts(ell, quality)
            self.a, self.eta = a, eta
            self.N = np.array([[a, 1.0], [-w0 * w0, -a]])                 # F + a I, F = [0 1; -w0^2 -w0 / Q]; N^2 = -eta^2 I
            self.Pinf = np.array([[v, 0.0], [0.0, w0 * w0 * v]])
        else:
            self.matern = T.ss_model(kind, v, ell)
            self.Pinf = self.matern[2]
        self.D = self.Pinf.shape[0]

    def AQ(self, dt):
        if self.kind != "sho":
            return T.ss_AQ(self.matern, dt)
        A = np.exp(-self.a * dt) * (np.cos(self.eta * dt) * np.eye(2) + np.sin(self.eta * dt) / self.eta * self.N)
        return A, self.Pinf - A @ self.Pinf @ A.T

    def K(self, x, x2=None):
        if self.kind == "sho":
            return sho_K(self.v, self.ell, self.quality, x, x2)
        return T.matern_K(self.kind, self.v, self.ell, np.asarray(x), None if x2 is None else np.asarray(x2))

    def desc(self, mean=0.0):
        d = {"kind": self.kind, "variance": self.v, "lengthscale": self.ell, "mean": mean}
        if self.kind == "sho":
            d["quality"] = self.quality
        return d


def sho(v, P, Q):
    return Model("sho", v, P, Q)


def kalman_filter(model, x, w, r):
    """The sequential filter: (value, filtered first-component mean, variance, states m (n, D), P (n, D, D)).  w = +inf: unobserved.
    Complex parameters carry a tangent (the complex step)."""
    D, n = model.D, len(x)
    dtype = model.Pinf.dtype
    m, P = np.zeros(D, dtype=dtype), model.Pinf.copy()
    ms, Ps = np.zeros((n, D), dtype=dtype), np.zeros((n, D, D), dtype=dtype)
    val = 0.0
    for t in range(n):
        if t > 0:
            A, Q = model.AQ(x[t] - x[t - 1])
            m, P = A @ m, A @ P @ A.T + Q
        if np.isfinite(w[t]):
            S = P[0, 0] + w[t]
            K = P[:, 0] / S
            e = r[t] - m[0]
            m, P = m + K * e, P - np.outer(K, P[0, :])
            val = val + -0.5 * (LOG2PI + np.log(S) + e * e / S)
        ms[t], Ps[t] = m, P
    return val, ms[:, 0].copy(), Ps[:, 0, 0].copy(), ms, Ps


def rts_smoother(model, x, ms, Ps):
    """Smoothed first-component mean and variance by the sequential Rauch-Tung-Striebel recursion."""
    n = len(x)
    g, Lm = ms[-1].copy(), Ps[-1].copy()
    sm, sv = np.zeros(n), np.zeros(n)
    sm[-1], sv[-1] = g[0], Lm[0, 0]
    for t in range(n - 2, -1, -1):
        A, Q = model.AQ(x[t + 1] - x[t])
        Pp = A @ Ps[t] @ A.T + Q
        E = np.linalg.solve(Pp, A @ Ps[t]).T if np.abs(Pp).max() > 0 else np.zeros_like(Pp)
        g = ms[t] + E @ (g - A @ ms[t])
        Lm = Ps[t] + E @ (Lm - Pp) @ E.T
        sm[t], sv[t] = g[0], Lm[0, 0]
    return sm, sv


def statespace_reference(model, x, w, r):
    """(value, filtered mean, filtered variance, smoothed mean, smoothed variance) of the restatement."""
    val, fm, fv, ms, Ps = kalman_filter(model, x, w, r)
    sm, sv = rts_smoother(model, x, ms, Ps)
    return val, fm, fv, sm, sv


def dense_reference(model, x, w, r):
    """The same five quantities from K + diag(w) over the observed points (test_statespace_abi.dense_reference for any model)."""
    import scipy.linalg as sla
    n, v = len(x), model.v
    obs = np.flatnonzero(np.isfinite(w))
    if len(obs) == 0:
        return 0.0, np.zeros(n), np.full(n, v), np.zeros(n), np.full(n, v)
    Lc = np.linalg.cholesky(model.K(x[obs]) + np.diag(w[obs]))
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    V = sla.solve_triangular(Lc, model.K(x[obs], x), lower=True)
    val = -0.5 * (len(obs) * LOG2PI + 2.0 * np.log(np.diag(Lc)).sum() + u @ u)
    cm = np.vstack([np.zeros(n), np.cumsum(V * u[:, None], axis=0)])
    cv = np.vstack([np.zeros(n), np.cumsum(V * V, axis=0)])
    seen = np.cumsum(np.isfinite(w))
    t = np.arange(n)
    return val, cm[seen, t], v - cv[seen, t], cm[-1], v - cv[-1]


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def tangent_filter(v, P, Q, x, w, r):
    """(d lml / d variance, d lml / d period, d lml / d quality) by the sequential filter on value + i h tangent (the complex step of
    test_statespace_grad_abi: no subtraction)."""
    out = []
    for k in range(3):
        th = [v + 0j, P + 0j, Q + 0j]
        th[k] += 1j * STEP
        out.append(float(kalman_filter(sho(*th), x, w, r)[0].imag / STEP))
    return tuple(out)


def point_gradients(w, r, sm, sv):
    import test_statespace_grad_abi as TG
    return TG.point_gradients(w, r, sm, sv)


def statespace_grad_reference(v, P, Q, x, w, r):
    """(value, grad_r, grad_w, d / d variance, d / d period, d / d quality) of the restatement."""
    val, _, _, sm, sv = statespace_reference(sho(v, P, Q), x, w, r)
    gr, gw = point_gradients(w, r, sm, sv)
    return (val, gr, gw) + tangent_filter(v, P, Q, x, w, r)


def dense_grad_reference(v, P, Q, x, w, r):
    """The same six quantities from C = K + diag(w) over the observed points: alpha = C^-1 r, (alpha' K_theta alpha - tr(C^-1
    K_theta)) / 2 with K_theta from dk_sho, (alpha^2 - diag C^-1) / 2."""
    n = len(x)
    obs = np.flatnonzero(np.isfinite(w))
    gr, gw = np.zeros(n), np.zeros(n)
    if len(obs) == 0:
        return 0.0, gr, gw, 0.0, 0.0, 0.0
    tau = np.abs(x[obs][:, None] - x[obs][None, :])
    Ci = np.linalg.inv(k_sho(v, P, Q, tau) + np.diag(w[obs]))
    Ci = 0.5 * (Ci + Ci.T)
    alpha = Ci @ r[obs]
    A = np.outer(alpha, alpha) - Ci
    gr[obs], gw[obs] = -alpha, 0.5 * np.diag(A)
    val = dense_reference(sho(v, P, Q), x, w, r)[0]
    return (val, gr, gw) + tuple(0.5 * np.sum(A * dK) for dK in dk_sho(v, P, Q, tau))


# ---- sampling (test_statespace_rand_abi restated for any model) ------------------------------------------------------------------
def sho_t(v, P, Q, dt):
    """sho(v, P, Q) with every constant formed in the dtype dt (pi included)."""
    if dt is np.float64:
        return sho(v, P, Q)
    pi = dt(4) * np.arctan(dt(1))
    return sho(dt(v), dt(P) * (dt(np.pi) / pi), dt(Q))          # sho_consts multiplies by the float64 pi: P carries the correction


def prior_path(model, x, zeta, dt=np.float64):
    """The sequential prior path f_t = (s_t)_1: s_0 = chol(Pinf) zeta_0, s_t = A(dt_t) s_{t-1} + chol(Q(dt_t)) zeta_t.  zeta: (D, n)."""
    import test_statespace_rand_abi as R
    x, zeta = np.asarray(x, dtype=dt), np.asarray(zeta, dtype=dt)
    s = np.zeros(model.D, dtype=dt)
    f = np.zeros(len(x), dtype=dt)
    for t in range(len(x)):
        A, Qd = (np.zeros((model.D, model.D), dtype=dt), model.Pinf) if t == 0 else model.AQ(x[t] - x[t - 1])
        s = A @ s + R.chol_psd(Qd) @ zeta[:, t]
        f[t] = s[0]
    return f


def pathwise_posterior(model, x, w, r, zeta, xi):
    """Matheron's rule: prior path + smoothed mean of r - f - sqrt(w) xi at the observed points (w = +inf: unobserved, xi not read)."""
    f = prior_path(model, x, zeta)
    obs = np.isfinite(w)
    rp = np.array(r, dtype=np.float64)
    rp[obs] = r[obs] - f[obs] - np.sqrt(w[obs]) * np.asarray(xi)[obs]
    _, _, _, ms, Ps = kalman_filter(model, x, w, rp)
    return f + rts_smoother(model, x, ms, Ps)[0]


def dense_posterior(model, x, w, r):
    """(mean, covariance) of f at every point given the observed ones."""
    obs = np.flatnonzero(np.isfinite(w))
    K = model.K(x)
    if len(obs) == 0:
        return np.zeros(len(x)), K
    G = np.linalg.solve(K[np.ix_(obs, obs)] + np.diag(w[obs]), K[obs, :])
    return G.T @ r[obs], K - K[:, obs] @ G


RAND_V, RAND_P = 1.3, 0.7
LAW_SPACINGS = (1.0, 0.1, 0.01, 0.003)


def rand_case(Q, n, seed=0):
    """Well-separated inputs: spacings uniform in [0.5, 2] periods, 10 % exact duplicates, one gap of 1e4 periods (n > 2).  Returns
    (v, P, x, zeta (2, n))."""
    rng = np.random.default_rng([seed, n, int(round(100 * Q)), 77])
    d = RAND_P * rng.uniform(0.5, 2.0, n)
    d[rng.random(n) < 0.1] = 0.0
    if n > 2:
        d[n // 2] = 1e4 * RAND_P
    return RAND_V, RAND_P, np.cumsum(d) - 1.0, rng.standard_normal((2, n))


def law_case(spacing, n=8):
    """n points `spacing` periods apart, two of them duplicated."""
    d = np.full(n, spacing * RAND_P)
    d[[n // 3, n - 2]] = 0.0
    return np.cumsum(d)


def path_map(model, x):
    """M (n, 2 n): column i is the path of the i-th unit vector of normals (component-major, as the library's z)."""
    n = len(x)
    return np.stack([prior_path(model, x, e.reshape(2, n)) for e in np.eye(2 * n)], axis=1)


def posterior_map(model, x, w, r):
    """(the path with zero normals, B (n, 3 n)): B's columns are the path's linear part at the unit vectors of (zeta, xi)."""
    n = len(x)
    zero = pathwise_posterior(model, x, w, r, np.zeros((2, n)), np.zeros(n))
    B = np.stack([pathwise_posterior(model, x, w, r, e[:2 * n].reshape(2, n), e[2 * n:]) - zero for e in np.eye(3 * n)], axis=1)
    return zero, B


_DELTA_RAND = {}


def deltas_rand():
    """{Q: (path: max|float64 - longdouble| / sqrt(v) at the well-separated case, n = 200; law: max|M M' - K| / v over LAW_SPACINGS,
    n = 8 with duplicates; posterior mean and covariance of the pathwise restatement against the dense posterior, n = 24 of `case`)}."""
    if not _DELTA_RAND:
        for Q in QS:
            v, P, x, zeta = rand_case(Q, 200)
            a = prior_path(sho(v, P, Q), x, zeta)
            b = prior_path(sho_t(v, P, Q, np.longdouble), x, zeta, np.longdouble)
            path = float(np.abs(a - b).max() / np.sqrt(v))
            law = 0.0
            for sp in LAW_SPACINGS:
                xl = law_case(sp)
                M = path_map(sho(RAND_V, RAND_P, Q), xl)
                law = max(law, float(np.abs(M @ M.T - sho_K(RAND_V, RAND_P, Q, xl)).max() / RAND_V))
            v, P, x, w, r = case(Q, 24)
            zero, B = posterior_map(sho(v, P, Q), x, w, r)
            mu, Sg = dense_posterior(sho(v, P, Q), x, w, r)
            _DELTA_RAND[Q] = (path, law, T.arr_err(zero, mu), T.arr_err(B @ B.T, Sg))
    return _DELTA_RAND


def delta_rand():
    """The largest of them: DELTA of the sampling tests' GPU tolerance max(1e-10, 100 DELTA)."""
    return max(max(d) for d in deltas_rand().values())


# ---- cases and the measured disagreements ---------------------------------------------------------------------------------------
def case(Q, n, seed=0, unobserved=True, ties=True):
    """Spacings dt / P between about 0.01 and 1 (log-uniform), w in [0.05, 0.5], a quarter of the points unobserved (the first one
    among them), and (n >= 63) runs of equal inputs."""
    rng = np.random.default_rng([seed, n, int(round(100 * Q))])
    P, v = 0.7, 1.3
    x = np.cumsum(P * 10.0 ** rng.uniform(-2.0, 0.0, n)) - 1.0
    w = rng.uniform(0.05, 0.5, n)
    r = rng.standard_normal(n)
    if unobserved:
        miss = rng.random(n) < 0.25
        miss[0] = True
        w = np.where(miss, np.inf, w)
    if ties and n >= 63:
        x[10:14] = x[10]
        x[40] = x[39]
    return v, P, x, w, r


_DELTA, _DELTA_GRAD = {}, {}


def deltas():
    """{(Q, n): (value, filtered, smoothed)} disagreements of the restatement with the dense Gaussian."""
    if not _DELTA:
        for Q in QS:
            for n in CPU_N:
                v, P, x, w, r = case(Q, n)
                got, ref = statespace_reference(sho(v, P, Q), x, w, r), dense_reference(sho(v, P, Q), x, w, r)
                _DELTA[(Q, n)] = (T.rel(got[0], ref[0]), max(T.arr_err(got[1], ref[1]), T.arr_err(got[2], ref[2])),
                                  max(T.arr_err(got[3], ref[3]), T.arr_err(got[4], ref[4])))
    return _DELTA


def delta():
    """The largest disagreement over every case and quantity: DELTA of the GPU tolerances."""
    return max(max(d) for d in deltas().values())


def grad_err(got, ref):
    arr = lambda a, b: T.arr_err(a, b) if np.abs(b).max() > 0 else float(np.abs(a).max())
    return (arr(got[1], ref[1]), arr(got[2], ref[2])) + tuple(T.rel(got[k], ref[k]) for k in (3, 4, 5))


def deltas_grad():
    """{(Q, n): (grad_r, grad_w, d / d variance, d / d period, d / d quality)} disagreements with the dense analytic gradient."""
    if not _DELTA_GRAD:
        for Q in QS:
            for n in CPU_N:
                v, P, x, w, r = case(Q, n)
                _DELTA_GRAD[(Q, n)] = grad_err(statespace_grad_reference(v, P, Q, x, w, r), dense_grad_reference(v, P, Q, x, w, r))
    return _DELTA_GRAD


def delta_grad():
    return max(max(d) for d in deltas_grad().values())


# ---- tests of the mathematics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", QS + (0.7, 10.0))
def test_closed_form_derivatives_agree_with_central_differences(Q):
    """Step 1e-6 of smooth functions of size ~ 1: truncation ~ 1e-12, rounding ~ eps / step ~ 1e-10 (Q = 0.51: the derivative with
    respect to Q is of size ~ 1 / (2 Q - 1) and so is its rounding)."""
    v, P = 1.3, 0.7
    tau = np.concatenate([[0.0], 10.0 ** np.linspace(-3, 1, 41)])
    dv, dP, dQ = dk_sho(v, P, Q, tau)
    h = 1e-6
    tol = 1e-8 / min(1.0, 2.0 * Q - 1.0)
    assert np.abs((k_sho(v + h, P, Q, tau) - k_sho(v - h, P, Q, tau)) / (2 * h) - dv).max() <= tol
    assert np.abs((k_sho(v, P + h, Q, tau) - k_sho(v, P - h, Q, tau)) / (2 * h) - dP).max() <= tol * max(1.0, np.abs(dP).max())
    assert np.abs((k_sho(v, P, Q + h, tau) - k_sho(v, P, Q - h, tau)) / (2 * h) - dQ).max() <= tol * max(1.0, np.abs(dQ).max())
    assert k_sho(v, P, Q, 0.0) == v and dP[0] == 0.0 and dQ[0] == 0.0


@pytest.mark.parametrize("Q", QS)
def test_transition_reproduces_the_kernel(Q):
    """A(dt)[0, 0] v = k(dt); A(0) = I and Q(0) = 0 exactly; N^2 = -eta^2 I; Pinf is stationary (F Pinf + Pinf F' + L q L' = 0 has no
    [0, 0] and [0, 1] entries from the noise, which enters the velocity only)."""
    m = sho(1.3, 0.7, Q)
    for dt in (0.0, 1e-4, 0.03, 0.7, 5.0):
        A, Qd = m.AQ(dt)
        assert abs(A[0, 0] * m.v - k_sho(m.v, m.ell, Q, dt)) <= 1e-15 * m.v
        assert np.linalg.eigvalsh(0.5 * (Qd + Qd.T)).min() >= -1e-13 * np.abs(m.Pinf).max()
    A, Qd = m.AQ(0.0)
    assert (A == np.eye(2)).all() and (Qd == 0.0).all()
    assert np.abs(m.N @ m.N + m.eta ** 2 * np.eye(2)).max() <= 1e-12 * m.eta ** 2
    F = m.N - m.a * np.eye(2)
    lyap = F @ m.Pinf + m.Pinf @ F.T
    assert abs(lyap[0, 0]) <= 1e-12 * np.abs(lyap).max() and abs(lyap[0, 1]) <= 1e-12 * np.abs(lyap).max()
    A1, _ = m.AQ(0.11)
    A2, _ = m.AQ(0.23)
    assert np.abs(A1 @ A2 - m.AQ(0.34)[0]).max() <= 1e-13                       # a semigroup


def test_half_quality_limit_is_matern32():
    """Q -> 1/2 with sqrt(3) / l = 2 pi / P: k -> v (1 + lam tau) exp(-lam tau); at Q = 1/2 + 1e-9 the difference is O(2 Q - 1)."""
    v, P = 1.3, 0.7
    ell = np.sqrt(3.0) * P / (2.0 * np.pi)
    tau = np.linspace(0.0, 3.0, 31)
    ref = T.matern_K("matern32", v, ell, tau[:1], tau)[0]
    assert np.abs(k_sho(v, P, 0.5 + 1e-9, tau) - ref).max() <= 1e-7


@pytest.mark.parametrize("Q", QS)
def test_restatement_agrees_with_dense(Q):
    for n in CPU_N:
        d = deltas()[(Q, n)]
        print(f"Q={Q} n={n}: value {d[0]:.2e} filtered {d[1]:.2e} smoothed {d[2]:.2e}")
        assert max(d) <= 1e-12, (Q, n, d)


@pytest.mark.parametrize("Q", QS)
def test_dense_gradient_agrees_with_finite_differences(Q):
    """Central differences of dense_reference's value (step 1e-5; the bounds of test_statespace_grad_abi, with the 1 / (2 Q - 1) of the
    derivative with respect to Q near 1/2)."""
    v, P, x, w, r = case(Q, 63)
    ref = dense_grad_reference(v, P, Q, x, w, r)
    f = lambda v_=v, P_=P, Q_=Q, w_=w, r_=r: dense_reference(sho(v_, P_, Q_), x, w_, r_)[0]
    h = 1e-5 if Q > 0.6 else 1e-6
    fd = ((f(v_=v + h) - f(v_=v - h)) / (2 * h), (f(P_=P + h) - f(P_=P - h)) / (2 * h), (f(Q_=Q + h) - f(Q_=Q - h)) / (2 * h))
    for k in range(3):
        assert abs(fd[k] - ref[3 + k]) <= 1e-5 * max(1.0, abs(ref[3 + k])), (Q, k, fd[k], ref[3 + k])
    obs = np.flatnonzero(np.isfinite(w))
    for t in obs[:: max(1, len(obs) // 5)]:
        e = np.zeros(len(x)); e[t] = 1e-5
        assert abs((f(r_=r + e) - f(r_=r - e)) / 2e-5 - ref[1][t]) <= 1e-6 * max(1.0, abs(ref[1][t]))
        assert abs((f(w_=w + e) - f(w_=w - e)) / 2e-5 - ref[2][t]) <= 1e-6 * max(1.0, abs(ref[2][t]))
    unobs = np.flatnonzero(~np.isfinite(w))
    assert (ref[1][unobs] == 0).all() and (ref[2][unobs] == 0).all()


@pytest.mark.parametrize("Q", QS)
def test_gradient_restatement_agrees_with_dense(Q):
    for n in CPU_N:
        d = deltas_grad()[(Q, n)]
        print(f"Q={Q} n={n}: grad_r {d[0]:.2e} grad_w {d[1]:.2e} variance {d[2]:.2e} period {d[3]:.2e} quality {d[4]:.2e}")
        assert max(d) <= 1e-9, (Q, n, d)


@pytest.mark.parametrize("Q", QS)
def test_sampling_restatement(Q):
    """The float64 path against the longdouble one at separated inputs, the law M M' = K down to small spacings, and the pathwise
    posterior against the dense one."""
    d = deltas_rand()[Q]
    print(f"Q={Q}: path {d[0]:.2e} law {d[1]:.2e} posterior mean {d[2]:.2e} covariance {d[3]:.2e}")
    assert max(d) <= 1e-12, (Q, d)


# ---- the mirror -----------------------------------------------------------------------------------------------------------------
def test_shokernel_construction_and_descriptor():
    k = lmm_amd.SHOKernel(1.5, 0.7, 3.0)
    assert (k.variance, k.lengthscale, k.period, k.quality, k.kind) == (1.5, 0.7, 0.7, 3.0, "sho")
    assert lmm_amd.SHOKernel().quality == 1.0 and lmm_amd.SHOKernel().lengthscale == 1.0
    assert k.desc() == {"kind": "sho", "variance": 1.5, "lengthscale": 0.7, "quality": 3.0}
    assert repr(k) == "SHOKernel(variance=1.5, lengthscale=0.7, quality=3.0)"
    assert k == lmm_amd.SHOKernel(1.5, 0.7, 3.0) and k != lmm_amd.SHOKernel(1.5, 0.7, 3.5) and k != lmm_amd.Matern32Kernel(1.5, 0.7)
    assert k.key() != lmm_amd.SHOKernel(1.5, 0.7, 3.5).key()
    k.period = 0.9
    assert k.lengthscale == 0.9
    for bad in (0.5, 0.3, 0.0, -1.0, float("nan"), float("inf"), np.array([1.0, 2.0])):
        with pytest.raises(ValueError, match="quality"):
            lmm_amd.SHOKernel(1.0, 1.0, bad)
    with pytest.raises(ValueError, match="one scalar"):
        lmm_amd.SHOKernel(1.0, np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="one scalar"):
        k.period = np.array([1.0, 2.0])
    assert "SHOKernel" in lmm_amd.__all__ and lmm_amd.model.SHOKernel is lmm_amd.SHOKernel
    assert lmm_amd.GP(0.3, k).desc() == {"kind": "sho", "variance": 1.5, "lengthscale": 0.9, "quality": 3.0, "mean": 0.3}


def test_constants_header_and_mirror():
    src = open(HEADER).read()
    assert re.search(r"^#define LMM_KERNEL_SHO 12$", src, flags=re.M)
    enum = re.search(r"typedef enum \{([^}]*)\} lmm_kernel_kind;", src).group(1)
    assert "SHO" not in enum
    assert L.KERNEL_SHO == 12 and 12 not in L.KERNEL_KINDS.values() and "sho" not in L.KERNEL_KINDS


def test_symbols_declared_exported_and_bound():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "int lmm_kernel_tag_create_sho(double quality, int* tag);" in src
    assert "int lmm_kernel_tag_quality_grad(int tag, double* out);" in src
    types = dict(L.SHO_ARGTYPES, lmm_dev_statespace_grad_sho=L.STATESPACE_ARGTYPES["lmm_dev_statespace_grad_sho"])
    for s, want in types.items():
        assert hasattr(lib, s) and s in L.SYMBOLS, s
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert proto, s
        params = [a.strip() for a in proto.group(1).split(",")]
        assert len(params) == len(want) and getattr(lib, s).argtypes == want, s
        for a, t in zip(params, want):
            if "*" in a:
                assert t is L._P or issubclass(t, C._Pointer), (s, a)
            else:
                assert t is (L._D if a.startswith("double") else L._I), (s, a)
    # the two-parameter block keeps its prototype; the SHO one has the same arity and a three-value output
    assert L.STATESPACE_ARGTYPES["lmm_dev_statespace_grad_sho"] == L.STATESPACE_ARGTYPES["lmm_dev_statespace_grad"]


def test_gps_array_kind_word_and_tag():
    arr = L.gps_array([lmm_amd.GP(0.2, lmm_amd.SHOKernel(1.5, 0.7, 3.0)).desc(), {"kind": "sho", "variance": 2.0, "lengthscale": 0.4},
                       lmm_amd.GP(lmm_amd.Matern32Kernel()).desc()])
    assert arr[0].kind & L.KERNEL_BASE_MASK == L.KERNEL_SHO and arr[0].kind >> 8 == arr.ard.tags[0] > 0
    assert (arr[0].variance, arr[0].lengthscale, arr[0].mean) == (1.5, 0.7, 0.2)
    assert arr.ard.has_quality == [True, False, False] and not any(arr.ard.has_alpha) and not any(arr.ard.has_rho)
    assert arr[1].kind == L.KERNEL_SHO and arr.ard.tags[1] == 0                  # no "quality": no tag, Q = 1, no quality gradient
    assert arr[2].kind == L.KERNEL_KINDS["matern32"]
    g = C.c_double(-1.0)
    assert lmm_amd.load().lmm_kernel_tag_quality_grad(arr.ard.tags[0], C.byref(g)) == L.LMM_OK and g.value == 0.0
    assert arr.ard.quality_grad(0) == 0.0
    tag = arr.ard.tags[0]
    arr.ard.close()
    assert lmm_amd.load().lmm_kernel_tag_quality_grad(tag, C.byref(g)) == L.LMM_ERR_ARG
    with pytest.raises(ValueError, match="quality"):
        L.gps_array([{"kind": "sho", "quality": 0.5}])
    with pytest.raises(ValueError, match="one scalar"):
        L.gps_array([{"kind": "sho", "lengthscale": np.array([1.0, 2.0])}])


def test_tag_registry_and_misuse():
    lib = lmm_amd.load()
    t, g = C.c_int(), C.c_double()
    for bad in (0.5, 0.2, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.lmm_kernel_tag_create_sho(C.c_double(bad), C.byref(t)) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_create_sho(C.c_double(2.0), None) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_create_sho(C.c_double(0.51), C.byref(t)) == L.LMM_OK and t.value > 0
    tq = t.value
    try:
        assert lib.lmm_kernel_tag_quality_grad(tq, None) == L.LMM_ERR_ARG
        assert lib.lmm_kernel_tag_quality_grad(tq, C.byref(g)) == L.LMM_OK and g.value == 0.0
        for other in (lib.lmm_kernel_tag_alpha_grad, lib.lmm_kernel_tag_rho_grad, lib.lmm_kernel_tag_decay_grad):
            assert other(tq, C.byref(g)) == L.LMM_ERR_ARG
        ta, tr = C.c_int(), C.c_int()
        assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK
        assert lib.lmm_kernel_tag_create_periodic(0, None, C.c_double(1.2), C.byref(tr)) == L.LMM_OK
        for tt in (ta, tr):
            assert lib.lmm_kernel_tag_quality_grad(tt.value, C.byref(g)) == L.LMM_ERR_ARG
        # kind 12 is not a sum term, with or without its tag; a term of another kind cannot carry a quality
        tag_out = C.c_int()
        for kind in (L.KERNEL_SHO, L.KERNEL_SHO | tq << 8):
            terms = (L.GpT * 1)(L.GpT(kind, 1.0, 1.0, 0.0))
            assert lib.lmm_kernel_sum_create(1, terms, C.byref(tag_out)) == L.LMM_ERR_UNSUPPORTED
        terms = (L.GpT * 1)(L.GpT(L.KERNEL_KINDS["matern32"] | tq << 8, 1.0, 1.0, 0.0))
        assert lib.lmm_kernel_sum_create(1, terms, C.byref(tag_out)) == L.LMM_ERR_ARG
        for tt in (ta, tr):
            lib.lmm_ard_destroy(tt.value)
    finally:
        assert lib.lmm_ard_destroy(tq) == L.LMM_OK
    assert lib.lmm_kernel_tag_quality_grad(tq, C.byref(g)) == L.LMM_ERR_ARG


def test_julia_shim_maps_the_kernel():
    src = open(SHIM).read()
    assert "struct SHOKernel" in src and "LMM_KERNEL_SHO = 12" in src
    assert re.search(r"ccall\(\(:lmm_kernel_tag_create_sho,\s*liblmm\),\s*Cint,\s*\(Cdouble,\s*Ref\{Cint\}\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_quality_grad,\s*liblmm\),\s*Cint,\s*\(Cint,\s*Ref\{Cdouble\}\)", src)


# ---- refusals, all before any library call ----------------------------------------------------------------------------------------
def _no_library():
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    M = lmm_amd.model
    k = lmm_amd.SHOKernel(1.0, 0.7, 3.0)
    H = lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0]))
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2)
    y = np.zeros(8)

    def oilmm(kern, xin=x):
        return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(kern)]), H)(xin, 0.1)

    fx = oilmm(k)
    d2 = oilmm(k, lmm_amd.MOInputIsotopicByOutputs(np.zeros((2, 4)), 2))
    ksum = oilmm(lmm_amd.KernelSum(lmm_amd.Matern32Kernel(), k))
    dense = lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(k)]), np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = lmm_amd.independent_mogp([lmm_amd.GP(k)])(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    vfe = lmm_amd.VFE(np.linspace(0.0, 3.0, 3))
    rng = np.random.default_rng(0)
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        ss = (lambda f, yy: lmm_amd.statespace_logpdf(f, yy), lambda f, yy: lmm_amd.statespace_mean_and_var(f, yy),
              lambda f, yy: lmm_amd.statespace_logpdf_and_gradient(f, yy), lambda f, yy: lmm_amd.statespace_rand(rng, f, yy))
        for fn in ss:
            with pytest.raises(NotImplementedError, match="d = 2"):           # d > 1 on the state-space path
                fn(d2, y)
            with pytest.raises(NotImplementedError, match="latent 0"):        # an SHO term inside a sum
                fn(ksum, y)
            with pytest.raises(NotImplementedError, match="dense-H"):
                fn(dense, y)
            with pytest.raises(NotImplementedError, match="IndependentMOGP"):
                fn(mogp, y[:4])
        dense_verbs = (lambda f: lmm_amd.logpdf(f, y), lambda f: lmm_amd.logpdf_and_gradient(f, y), lambda f: lmm_amd.posterior(f, y),
                       lmm_amd.mean_and_var, lmm_amd.mean, lmm_amd.var, lmm_amd.marginals, lmm_amd.mean_and_cov, lmm_amd.cov,
                       lambda f: lmm_amd.rand(rng, f))
        unserved = (lambda f: lmm_amd.logpdf_and_gradient(f, y, inputs=True), lambda f: lmm_amd.mean_and_var_vjp(f, np.ones(8)),
                    lambda f: lmm_amd.elbo(vfe, f, y), lambda f: lmm_amd.dtc(vfe, f, y),
                    lambda f: lmm_amd.elbo_and_gradient(vfe, f, y), lambda f: lmm_amd.approx_posterior(vfe, f, y))
        for fn in dense_verbs:                                                 # served for d = 1 only, and not inside a sum
            with pytest.raises(NotImplementedError, match="d = 2"):
                fn(d2)
            with pytest.raises(NotImplementedError, match="KernelSum"):
                fn(ksum)
            with pytest.raises(AssertionError, match="the library was reached"):      # d = 1: served
                fn(fx)
        for fn in unserved:
            for f in (fx, d2, ksum, dense):
                with pytest.raises(NotImplementedError, match="SHO"):
                    fn(f)
        mogp2 = lmm_amd.independent_mogp([lmm_amd.GP(k)])
        with pytest.raises(NotImplementedError, match="d = 2"):
            lmm_amd.cov(mogp2, lmm_amd.MOInputIsotopicByOutputs(np.zeros((2, 4)), 1))
        # an SHO term of a sum never reaches lmm_kernel_sum_create
        with pytest.raises(NotImplementedError, match="SHO term"):
            L.gps_array([lmm_amd.KernelSum(lmm_amd.SEKernel(), k).desc()])
    finally:
        L.ensure_init = saved
    assert M._has_sho(k) and M._has_sho(lmm_amd.KernelSum(lmm_amd.SEKernel(), k)) and not M._has_sho(lmm_amd.Matern32Kernel())


if __name__ == "__main__":
    for (Q, n), d in deltas().items():
        print(f"Q={Q:5.2f} n={n:4d}  value {d[0]:.2e}  filtered {d[1]:.2e}  smoothed {d[2]:.2e}")
    for (Q, n), d in deltas_grad().items():
        print(f"Q={Q:5.2f} n={n:4d}  grad_r {d[0]:.2e}  grad_w {d[1]:.2e}  variance {d[2]:.2e}  period {d[3]:.2e}  quality {d[4]:.2e}")
    for Q, d in deltas_rand().items():
        print(f"Q={Q:5.2f}  path {d[0]:.2e}  law {d[1]:.2e}  posterior mean {d[2]:.2e}  covariance {d[3]:.2e}")
    print(f"DELTA = {delta():.2e}  DELTA_GRAD = {delta_grad():.2e}  DELTA_RAND = {delta_rand():.2e}")
