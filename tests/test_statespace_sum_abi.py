"""Host-only checks of sum latents on the state-space path (include/lmm_hip.h "State space: sum latents"; DESIGN.md 4.18 "Sum latents"):
the NumPy restatement of the mathematics in the transformed basis s' = T s (filter, RTS smoother, forward-mode gradient, prior and
posterior paths) against the dense Gaussian with K = K_a + K_b built from direct differences; ss_inv at D = 4 through a stand-alone host
build of csrc/lmm_statespace.h; the Python mirror with the library stubbed out; and the tag registry, which needs no GPU.  The largest
disagreements delta_sum(), delta_sum_grad() and delta_sum_rand() fix the tolerances of tests/test_gpu_statespace_sum.py, which imports
the restatement from here.  No GPU and no lmm_init needed.

`python tests/test_statespace_sum_abi.py` prints the disagreements."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lmm_amd
from lmm_amd import _lib as L

LOG2PI = float(np.log(2.0 * np.pi))
TERM_DIM = {"matern12": 1, "matern32": 2, "matern52": 3, "sho": 2}
# the seven pair models, in the library's order of the terms
PAIRS = (("matern12", "matern12"), ("matern12", "matern32"), ("matern12", "sho"), ("matern12", "matern52"), ("matern32", "matern32"),
         ("matern32", "sho"), ("sho", "sho"))
QUALITIES = (0.51, 2.0, 50.0)
CPU_N = (1, 2, 17, 257)


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
# A term is (kind, variance, lengthscale) or ("sho", variance, period, quality).  Every function below works in the arithmetic of its
# parameters: real, or complex with one parameter moved by i h -- the imaginary part of the result over h is then its forward-mode
# derivative (the complex step), the restatement of the kernels' dual numbers.
def term_model(term):
    """(D, Pinf, AQ) of one term's SDE, AQ(dt) -> (A, Q) with Q = Pinf - A Pinf A'."""
    kind, v, ell = term[:3]
    if kind == "sho":
        q = term[3]
        w0 = 2.0 * np.pi / ell
        a = w0 / (2.0 * q)
        eta = a * np.sqrt((2.0 * q - 1.0) * (2.0 * q + 1.0))
        N = np.array([[a, 1.0], [-w0 * w0, -a]])
        Pinf = np.array([[v, 0.0 * v], [0.0 * v, w0 * w0 * v]])

        def AQ(dt):
            A = np.exp(-a * dt) * (np.cos(eta * dt) * np.eye(2) + np.sin(eta * dt) / eta * N)
            return A, Pinf - A @ Pinf @ A.T
        return 2, Pinf, AQ
    D = TERM_DIM[kind]
    lam = np.sqrt(2.0 * D - 1.0) / ell
    if D == 1:
        F, Pinf = np.array([[-lam]]), np.array([[v]])
    elif D == 2:
        F, Pinf = np.array([[0.0, 1.0], [-lam ** 2, -2.0 * lam]]), np.array([[v, 0.0 * v], [0.0 * v, lam ** 2 * v]])
    else:
        F = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam ** 3, -3.0 * lam ** 2, -3.0 * lam]])
        k = lam ** 2 / 3.0
        Pinf = v * np.array([[1.0, 0.0, -k], [0.0, k, 0.0], [-k, 0.0, lam ** 4]])
    N = F + lam * np.eye(D)

    def AQ(dt):
        A = np.exp(-lam * dt) * (np.eye(D) + N * dt + (N @ N) * (dt * dt / 2.0 if D > 2 else 0.0))
        return A, Pinf - A @ Pinf @ A.T
    return D, Pinf, AQ


def blkdiag(Xa, Xb):
    Da, Db = Xa.shape[0], Xb.shape[0]
    X = np.zeros((Da + Db, Da + Db), dtype=np.result_type(Xa, Xb))
    X[:Da, :Da], X[Da:, Da:] = Xa, Xb
    return X


def sum_model(ta, tb):
    """(D, Pinf', AQ') of the sum of two terms in the basis s' = T s, T = I + e_1 e_{Da+1}': the first component is f_a + f_b, so the
    observation stays e_1'.  Pinf' = T blkdiag(Pinf_a, Pinf_b) T', A' = T blkdiag(A_a, A_b) T^-1, Q' = T blkdiag(Q_a, Q_b) T' (which is
    Pinf' - A' Pinf' A'')."""
    Da, Pa, AQa = term_model(ta)
    Db, Pb, AQb = term_model(tb)
    D = Da + Db
    T = np.eye(D)
    T[0, Da] = 1.0
    Ti = np.eye(D)
    Ti[0, Da] = -1.0
    Pinf = T @ blkdiag(Pa, Pb) @ T.T

    def AQ(dt):
        (Aa, Qa), (Ab, Qb) = AQa(dt), AQb(dt)
        return T @ blkdiag(Aa, Ab) @ Ti, T @ blkdiag(Qa, Qb) @ T.T
    return D, Pinf, AQ


def kalman_filter(model, x, w, r):
    """The sequential filter observed through e_1': (values, filtered first-component mean, variance, states m (n, D, k), P (n, D, D)).
    r is (n,) or (n, k): k data vectors share the covariances, and `values` has one entry per vector.  w = +inf: unobserved."""
    D, Pinf, AQ = model
    n = len(x)
    R = np.asarray(r).reshape(n, -1)
    k = R.shape[1]
    dt_ = np.result_type(Pinf, R, AQ(0.0)[0])
    m, P = np.zeros((D, k), dtype=dt_), Pinf.astype(dt_)
    ms, Ps = np.zeros((n, D, k), dtype=dt_), np.zeros((n, D, D), dtype=dt_)
    val = np.zeros(k, dtype=dt_)
    for t in range(n):
        if t > 0:
            A, Q = AQ(x[t] - x[t - 1])
            m, P = A @ m, A @ P @ A.T + Q
        if np.isfinite(w[t]):
            S = P[0, 0] + w[t]
            K = P[:, 0] / S
            e = R[t] - m[0]
            m, P = m + np.outer(K, e), P - np.outer(K, P[0, :])
            val = val - 0.5 * (LOG2PI + np.log(S) + e * e / S)
        ms[t], Ps[t] = m, P
    return val, ms[:, 0, :], Ps[:, 0, 0], ms, Ps


def rts_smoother(model, x, ms, Ps):
    """Smoothed first-component means (n, k) and variances (n,) from the filtered states."""
    D, Pinf, AQ = model
    n = len(x)
    sm, sP = ms[n - 1], Ps[n - 1]
    om, ov = np.zeros_like(ms[:, 0, :]), np.zeros_like(Ps[:, 0, 0])
    om[n - 1], ov[n - 1] = sm[0], sP[0, 0]
    for t in range(n - 2, -1, -1):
        A, Q = AQ(x[t + 1] - x[t])
        Pp = A @ Ps[t] @ A.T + Q
        E = Ps[t] @ A.T @ np.linalg.inv(Pp)
        sm = ms[t] + E @ (sm - A @ ms[t])
        sP = Ps[t] + E @ (sP - Pp) @ E.T
        om[t], ov[t] = sm[0], sP[0, 0]
    return om, ov


def chol_psd(X):
    """The lower factor with non-negative diagonal of a positive SEMI-definite X: a pivot that is not > 0 gives a zero column."""
    D = X.shape[0]
    Lo = np.zeros((D, D))
    for j in range(D):
        s = X[j, j] - Lo[j, :j] @ Lo[j, :j]
        if not s > 0.0:
            continue
        Lo[j, j] = np.sqrt(s)
        for i in range(j + 1, D):
            Lo[i, j] = (X[i, j] - Lo[i, :j] @ Lo[j, :j]) / Lo[j, j]
    return Lo


def prior_paths(model, x, Z):
    """f (n, k): the first component of s_0 = chol(Pinf) zeta_0, s_t = A s_{t-1} + chol(Q) zeta_t for k sets of normals Z (n, D, k)."""
    D, Pinf, AQ = model
    n = len(x)
    s = chol_psd(Pinf) @ Z[0]
    f = np.zeros((n, Z.shape[2]))
    f[0] = s[0]
    for t in range(1, n):
        A, Q = AQ(x[t] - x[t - 1])
        s = A @ s + chol_psd(Q) @ Z[t]
        f[t] = s[0]
    return f


def posterior_paths(model, x, w, r, Z, Xi):
    """Pathwise conditioning: the prior paths plus the smoothed mean of r - f - sqrt(w) xi over the observed points.  Xi: (n, k)."""
    f = prior_paths(model, x, Z)
    obs = np.isfinite(w)
    resid = np.where(obs[:, None], np.asarray(r).reshape(len(x), -1) - f - np.sqrt(np.where(obs, w, 0.0))[:, None] * Xi, 0.0)
    _, _, _, ms, Ps = kalman_filter(model, x, w, resid)
    return f + rts_smoother(model, x, ms, Ps)[0]


def with_step(terms, c, i, h):
    """The two terms with parameter i (1 = variance, 2 = lengthscale / period, 3 = quality) of term c moved by i h."""
    out = [tuple(t) for t in terms]
    t = list(out[c])
    t[i] = t[i] + 1j * h
    out[c] = tuple(t)
    return out


def term_params(term):
    return (1, 2, 3) if term[0] == "sho" else (1, 2)


def filter_gradient(terms, x, w, r, h=1e-30):
    """The forward-mode derivative of the filter's value with respect to every parameter of the two terms, in their order."""
    g = []
    for c in range(2):
        for i in term_params(terms[c]):
            g.append(kalman_filter(sum_model(*with_step(terms, c, i, h)), x, w, r)[0][0].imag / h)
    return np.array(g)


# ---- the dense Gaussian it is compared with -------------------------------------------------------------------------------------
def term_K(term, tau):
    """The term's covariance at the distances tau, from its closed form."""
    kind, v, ell = term[:3]
    if kind == "sho":
        q = term[3]
        w0 = 2.0 * np.pi / ell
        a = w0 / (2.0 * q)
        eta = w0 * np.sqrt(1.0 - 1.0 / (4.0 * q * q))
        return v * np.exp(-a * tau) * (np.cos(eta * tau) + a / eta * np.sin(eta * tau))
    if kind == "matern12":
        return v * np.exp(-tau / ell)
    if kind == "matern32":
        s = np.sqrt(3.0) * tau / ell
        return v * (1.0 + s) * np.exp(-s)
    s = np.sqrt(5.0) * tau / ell
    return v * (1.0 + s + s * s / 3.0) * np.exp(-s)


def sum_K(terms, x, x2=None):
    tau = np.abs(x[:, None] - (x if x2 is None else x2)[None, :])
    return term_K(terms[0], tau) + term_K(terms[1], tau)


def dense_reference(terms, x, w, r):
    """(value, filtered mean, filtered variance, smoothed mean, smoothed variance) from K + diag(w) over the observed points: with L
    its Cholesky factor (time order), u = L^-1 r and V = L^-1 K(obs, all), conditioning on the first j observations is a sum over the
    first j rows of V and u."""
    import scipy.linalg as sla
    n = len(x)
    v0 = float(terms[0][1] + terms[1][1])
    obs = np.flatnonzero(np.isfinite(w))
    if len(obs) == 0:
        return 0.0, np.zeros(n), np.full(n, v0), np.zeros(n), np.full(n, v0)
    Lc = np.linalg.cholesky(sum_K(terms, x[obs]) + np.diag(w[obs]))
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    V = sla.solve_triangular(Lc, sum_K(terms, x[obs], x), lower=True)
    val = -0.5 * (len(obs) * LOG2PI + 2.0 * np.log(np.diag(Lc)).sum() + u @ u)
    cm = np.vstack([np.zeros(n), np.cumsum(V * u[:, None], axis=0)])
    cv = np.vstack([np.zeros(n), np.cumsum(V * V, axis=0)])
    seen = np.cumsum(np.isfinite(w))
    t = np.arange(n)
    return val, cm[seen, t], v0 - cv[seen, t], cm[-1], v0 - cv[-1]


def dense_gradient(terms, x, w, r, h=1e-30):
    """d value / d parameter = (alpha' dK alpha - tr(C^-1 dK)) / 2 with C = K + diag(w) over the observed points and dK the
    derivative of the closed form (by the complex step, which is exact to rounding for an analytic expression)."""
    obs = np.flatnonzero(np.isfinite(w))
    if len(obs) == 0:
        return np.zeros(sum(len(term_params(t)) for t in terms))
    xo = x[obs]
    Ci = np.linalg.inv(sum_K(terms, xo) + np.diag(w[obs]))
    al = Ci @ r[obs]
    g = []
    for c in range(2):
        for i in term_params(terms[c]):
            dK = sum_K(with_step(terms, c, i, h), xo).imag / h
            g.append(0.5 * (al @ dK @ al - np.sum(Ci * dK)))
    return np.array(g)


def make_terms(pair, quality=2.0):
    """Two terms with different variances and scales, the second the longer one."""
    out = []
    for c, kind in enumerate(pair):
        v, ell = (1.3, 0.7) if c == 0 else (0.6, 2.9)
        out.append((kind, v, ell, quality) if kind == "sho" else (kind, v, ell))
    return out


def case(pair, n, quality=2.0, seed=0):
    """Inputs of the comparison: spacings 10^U(-2, 0) times the shorter lengthscale with some exact duplicates, w in [0.05, 0.5], about
    a fifth of the points unobserved (the first one among them when n > 1)."""
    rng = np.random.default_rng([seed, n, PAIRS.index(tuple(pair)), int(round(100 * quality))])
    terms = make_terms(pair, quality)
    dt = terms[0][2] * 10.0 ** rng.uniform(-2.0, 0.0, n)
    dt[rng.random(n) < 0.1] = 0.0
    x = np.cumsum(dt) - 1.0
    w = rng.uniform(0.05, 0.5, n)
    r = rng.standard_normal(n)
    miss = rng.random(n) < 0.2
    if n > 1:
        miss[0] = True
    return terms, x, np.where(miss, np.inf, w), r


def cases():
    for pair in PAIRS:
        for q in (QUALITIES if "sho" in pair else (2.0,)):
            for n in CPU_N:
                yield pair, q, n


def arr_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


_DELTA, _DELTA_GRAD, _DELTA_RAND = {}, {}, {}


def deltas_sum():
    """{(pair, quality, n): (value, filtered, smoothed)} disagreements of the restatement with the dense Gaussian."""
    if not _DELTA:
        for pair, q, n in cases():
            terms, x, w, r = case(pair, n, q)
            model = sum_model(*terms)
            val, fm, fv, ms, Ps = kalman_filter(model, x, w, r)
            sm, sv = rts_smoother(model, x, ms, Ps)
            dv, dfm, dfv, dsm, dsv = dense_reference(terms, x, w, r)
            _DELTA[(pair, q, n)] = (abs(val[0] - dv) / max(abs(dv), 1e-300) if val[0] != dv else 0.0,
                                    max(arr_err(fm[:, 0], dfm), arr_err(fv, dfv)), max(arr_err(sm[:, 0], dsm), arr_err(sv, dsv)))
    return _DELTA


def deltas_sum_grad():
    """{(pair, quality, n): the forward-mode gradient's largest error relative to the largest entry of the dense gradient}."""
    if not _DELTA_GRAD:
        for pair, q, n in cases():
            terms, x, w, r = case(pair, n, q)
            _DELTA_GRAD[(pair, q, n)] = arr_err(filter_gradient(terms, x, w, r), dense_gradient(terms, x, w, r))
    return _DELTA_GRAD


def path_maps(terms, x, w):
    """(M, Mp): the linear maps from the normals to the prior path (n x n D) and to the posterior path at r = 0 (n x (n D + n))."""
    model = sum_model(*terms)
    n, D = len(x), model[0]
    Z = np.eye(n * D).reshape(n, D, n * D)
    M = prior_paths(model, x, Z)
    Zp = np.concatenate([Z, np.zeros((n, D, n))], axis=2)
    Xi = np.concatenate([np.zeros((n, n * D)), np.eye(n)], axis=1)
    return M, posterior_paths(model, x, w, np.zeros(n), Zp, Xi)


def deltas_sum_rand():
    """{(pair, quality, n): (prior, posterior)}: M M' against K and against K - K(., obs) C^-1 K(obs, .), relative to max |K|."""
    if not _DELTA_RAND:
        for pair, q, n in cases():
            if n > 65:      # the maps are n x n D matrices: the law is checked at the small sizes, the recursion itself above at all
                continue
            terms, x, w, r = case(pair, n, q)
            M, Mp = path_maps(terms, x, w)
            K = sum_K(terms, x)
            obs = np.flatnonzero(np.isfinite(w))
            Kp = K - K[:, obs] @ np.linalg.solve(K[np.ix_(obs, obs)] + np.diag(w[obs]), K[obs, :]) if len(obs) else K
            sc = np.abs(K).max()
            _DELTA_RAND[(pair, q, n)] = (float(np.abs(M @ M.T - K).max() / sc), float(np.abs(Mp @ Mp.T - Kp).max() / sc))
    return _DELTA_RAND


def delta_sum():
    return max(max(d) for d in deltas_sum().values())


def delta_sum_grad():
    return max(deltas_sum_grad().values())


def delta_sum_rand():
    return max(max(d) for d in deltas_sum_rand().values())


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_restatement_agrees_with_dense(pair):
    for (pr, q, n), d in deltas_sum().items():
        if pr == pair:
            print(f"{'+'.join(pair)} Q={q} n={n}: value {d[0]:.2e} filtered {d[1]:.2e} smoothed {d[2]:.2e}")
            assert max(d) <= 1e-11, (pair, q, n, d)


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_forward_mode_gradient_agrees_with_dense(pair):
    for (pr, q, n), d in deltas_sum_grad().items():
        if pr == pair:
            print(f"{'+'.join(pair)} Q={q} n={n}: gradient {d:.2e}")
            assert d <= 1e-9, (pair, q, n, d)


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_path_law_agrees_with_dense(pair):
    for (pr, q, n), d in deltas_sum_rand().items():
        if pr == pair:
            print(f"{'+'.join(pair)} Q={q} n={n}: prior {d[0]:.2e} posterior {d[1]:.2e}")
            assert max(d) <= 1e-11, (pair, q, n, d)


def test_transformed_basis_identities():
    """First component f_a + f_b; Q' of the blocks is Pinf' - A' Pinf' A''; dt = 0 gives A' = I and Q' = 0 exactly."""
    for pair in PAIRS:
        terms = make_terms(pair)
        D, Pinf, AQ = sum_model(*terms)
        assert D == TERM_DIM[pair[0]] + TERM_DIM[pair[1]] <= 4
        assert Pinf[0, 0] == terms[0][1] + terms[1][1]
        A, Q = AQ(0.0)
        assert (A == np.eye(D)).all() and (Q == 0.0).all()
        for dt in (1e-3, 0.1, 3.0):
            A, Q = AQ(dt)
            assert np.abs(Q - (Pinf - A @ Pinf @ A.T)).max() <= 1e-14 * np.abs(Pinf).max()
            assert np.abs(Q - Q.T).max() <= 1e-16 * np.abs(Pinf).max()
            # the first component's transition: Cov(f(dt), f(0)) = (A' Pinf')_11 is K(dt)
            assert abs((A @ Pinf)[0, 0] - sum_K(terms, np.array([0.0]), np.array([dt]))[0, 0]) <= 1e-14 * Pinf[0, 0]


# ---- the dense OILMM the GPU tests compare with (tests/test_gpu_statespace_sum.py) -----------------------------------------------------
# A latent is {"mean", "v0", "s0", "terms": [(kind, v_c, l_c[, quality]), ..]}: the kernel v0 sum_c v_c kappa_c(tau / (s0 l_c)); a plain
# latent has one term and v0 = s0 = 1.  Data Y is (p, n) with NaN = missing; a point observes no output, or at least m of them.
def latent_K(lat, x, x2=None):
    tau = np.abs(x[:, None] - (x if x2 is None else x2)[None, :])
    return lat["v0"] * sum(term_K((t[0], t[1], lat["s0"] * t[2]) + tuple(t[3:]), tau) for t in lat["terms"])


def oilmm_front(U, S, s2, Y, means):
    """The missing-data projection, point by point: with H_t the observed rows of H = U sqrt(S) and G_t = H_t' H_t, the latents'
    pseudo-observations r[l, t] = (G_t^-1 H_t' y_t)_l - mean_l with noise w[l, t] = s2 (G_t^-1)_ll (+inf at a point without
    observations), and the regulariser sum_t -((p_t - m) log(2 pi s2) + logdet G_t + |y_t - H_t z_t|^2 / s2) / 2."""
    p, n = Y.shape
    m = U.shape[1]
    H = U * np.sqrt(S)[None, :]
    r, w, reg = np.zeros((m, n)), np.full((m, n), np.inf), 0.0
    proj = [None] * n
    for t in range(n):
        o = np.flatnonzero(~np.isnan(Y[:, t]))
        if len(o) == 0:
            continue
        Ht = H[o]
        Gi = np.linalg.inv(Ht.T @ Ht)
        z = Gi @ Ht.T @ Y[o, t]
        res = Y[o, t] - Ht @ z
        r[:, t], w[:, t] = z - means, s2 * np.diag(Gi)
        reg += -0.5 * ((len(o) - m) * np.log(2.0 * np.pi * s2) - np.log(np.linalg.det(Gi)) + res @ res / s2)
        proj[t] = (o, Ht, Gi, res)
    return r, w, reg, proj


def oilmm_dense(lats, U, S, x, s2, Y, with_reg=True, xs=None, add_noise=True, grad=False):
    """The OILMM's log density (the missing-data approximation: per latent, a dense Gaussian over its pseudo-observations) and, with
    xs, the by-outputs posterior mean and variance there; grad: the analytic gradient {"value", "y", "sigma2", "gps"} as well (the
    kernel parameters by the complex step on the closed forms, everything else in closed form)."""
    p, n = Y.shape
    m = len(lats)
    means = np.array([lat["mean"] for lat in lats])
    r, w, reg, proj = oilmm_front(U, S, s2, Y, means)
    H = U * np.sqrt(S)[None, :]
    val = reg if with_reg else 0.0
    out = {}
    if xs is not None:
        out["mean"], out["var"] = np.zeros((p, len(xs))), np.zeros((p, len(xs))) + (s2 if add_noise else 0.0)
    alpha, dw = np.zeros((m, n)), np.zeros((m, n))
    ggps = []
    for l, lat in enumerate(lats):
        obs = np.flatnonzero(np.isfinite(w[l]))
        xo = x[obs]
        Ci = np.linalg.inv(latent_K(lat, xo) + np.diag(w[l, obs])) if len(obs) else np.zeros((0, 0))
        al = Ci @ r[l, obs]
        if len(obs):
            val += -0.5 * (len(obs) * LOG2PI - np.linalg.slogdet(Ci)[1] + r[l, obs] @ al)
        if xs is not None:
            Ks = latent_K(lat, xs, xo)
            ml = lat["mean"] + Ks @ al
            vl = np.diag(latent_K(lat, xs)) - np.sum((Ks @ Ci) * Ks, axis=1)
            out["mean"] += np.outer(H[:, l], ml)
            out["var"] += np.outer(H[:, l] ** 2, vl)
        if grad:
            alpha[l, obs], dw[l, obs] = al, 0.5 * (al * al - np.diag(Ci))

            def dK(mod):
                return latent_K(mod, xo).imag / 1e-30

            def d(dKm):
                return 0.5 * (al @ dKm @ al - np.sum(Ci * dKm))
            g = {"mean": float(al.sum())}
            tg = []
            for c, t in enumerate(lat["terms"]):
                e = {}
                for i, name in ((1, "variance"), (2, "lengthscale"), (3, "quality"))[:len(t) - 1]:
                    tt = list(t)
                    tt[i] = tt[i] + 1e-30j
                    e[name] = d(dK(dict(lat, terms=lat["terms"][:c] + [tuple(tt)] + lat["terms"][c + 1:])))
                tg.append(e)
            if len(lat["terms"]) == 1 and lat["v0"] == 1.0 and lat["s0"] == 1.0:
                g.update(tg[0])
            else:
                g.update(variance=d(dK(dict(lat, v0=lat["v0"] + 1e-30j))), lengthscale=d(dK(dict(lat, s0=lat["s0"] + 1e-30j))), terms=tg)
            ggps.append(g)
    out["value"] = float(val)
    if grad:
        gy, gs2 = np.zeros((p, n)), 0.0
        for t in range(n):
            if proj[t] is None:
                continue
            o, Ht, Gi, res = proj[t]
            gy[o, t] = -Ht @ Gi @ alpha[:, t]
            gs2 += dw[:, t] @ np.diag(Gi)
            if with_reg:
                gy[o, t] += -res / s2
                gs2 += -0.5 * ((len(o) - m) / s2 - res @ res / (s2 * s2))
        out.update(y=gy.reshape(-1), sigma2=float(gs2), gps=ggps)
    return out


def test_dense_oilmm_gradient_is_the_derivative_of_its_value():
    """The analytic gradient of the reference against central differences of its own value, on a small problem with NaN."""
    rng = np.random.default_rng(5)
    p, m, n = 4, 2, 9
    lats = [{"mean": 0.3, "v0": 1.2, "s0": 0.9, "terms": [("matern32", 0.8, 1.1), ("sho", 0.5, 1.7, 2.5)]},
            {"mean": -0.1, "v0": 1.0, "s0": 1.0, "terms": [("matern52", 1.4, 0.6)]}]
    U, S = np.linalg.qr(rng.standard_normal((p, m)))[0], rng.uniform(0.5, 2.0, m)
    x, Y = np.sort(rng.uniform(0.0, 4.0, n)), rng.standard_normal((p, n))
    Y[0, 2] = Y[3, 5] = np.nan
    Y[:, 7] = np.nan
    s2 = 0.2
    for with_reg in (True, False):
        G = oilmm_dense(lats, U, S, x, s2, Y, with_reg, grad=True)
        f = lambda **kw: oilmm_dense(kw.get("lats", lats), U, S, x, kw.get("s2", s2), kw.get("Y", Y), with_reg)["value"]
        h = 1e-6
        assert abs((f(s2=s2 + h) - f(s2=s2 - h)) / (2 * h) - G["sigma2"]) <= 1e-6 * max(1.0, abs(G["sigma2"]))
        gy = G["y"].reshape(p, n)
        assert (gy[np.isnan(Y)] == 0.0).all()
        for o, t in ((1, 0), (2, 2), (0, 5)):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[o, t] += h
            Ym[o, t] -= h
            assert abs((f(Y=Yp) - f(Y=Ym)) / (2 * h) - gy[o, t]) <= 1e-6 * max(1.0, abs(gy[o, t]))

        def moved(l, key, c, i, dh):
            new = [dict(lat) for lat in lats]
            if c is None:
                new[l][key] = new[l][key] + dh
            else:
                tt = list(new[l]["terms"][c])
                tt[i] += dh
                new[l]["terms"] = new[l]["terms"][:c] + [tuple(tt)] + new[l]["terms"][c + 1:]
            return new
        checks = [(0, "mean", None, 0, G["gps"][0]["mean"]), (0, "v0", None, 0, G["gps"][0]["variance"]),
                  (0, "s0", None, 0, G["gps"][0]["lengthscale"]), (0, None, 0, 2, G["gps"][0]["terms"][0]["lengthscale"]),
                  (0, None, 1, 1, G["gps"][0]["terms"][1]["variance"]), (0, None, 1, 3, G["gps"][0]["terms"][1]["quality"]),
                  (1, None, 0, 2, G["gps"][1]["lengthscale"]), (1, "mean", None, 0, G["gps"][1]["mean"])]
        for l, key, c, i, got in checks:
            fd = (f(lats=moved(l, key, c, i, h)) - f(lats=moved(l, key, c, i, -h))) / (2 * h)
            assert abs(fd - got) <= 1e-6 * max(1.0, abs(got)), (l, key, c, i, fd, got)


# ---- ss_inv at D = 4: a stand-alone host build of the header ---------------------------------------------------------------------
SS_INV_PROGRAM = r"""
#include "lmm_statespace.h"
#include <cstdio>
// X = I + C J with C = S G1 G1' S and J = S^-1 G2 G2' S^-1 positive semi-definite and scaled like the covariances of (f, f', ..):
// X_ij ~ s_i / s_j.  The error of ss_inv against Gauss-Jordan with partial pivoting in long double, entry by entry in the scaled
// sense |Y_ij - Yref_ij| s_i / s_j, relative to the largest scaled entry of Yref.
static unsigned long long state = 88172645463325252ull;
static double unif() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0 - 0.5; }
template <int D> static double trial(const double s[D], int rank) {
  double G1[D][D], G2[D][D], Cm[D][D], Jm[D][D], X[D][D], Y[D][D];
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) { G1[i][j] = j < rank ? unif() : 0.0; G2[i][j] = j < rank ? unif() : 0.0; }
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
    double c = 0.0, q = 0.0;
    for (int k = 0; k < D; ++k) { c += G1[i][k] * G1[j][k]; q += G2[i][k] * G2[j][k]; }
    Cm[i][j] = 4.0 * s[i] * c * s[j]; Jm[i][j] = 4.0 * q / (s[i] * s[j]);
  }
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
    double t = i == j ? 1.0 : 0.0;
    for (int k = 0; k < D; ++k) t += Cm[i][k] * Jm[k][j];
    X[i][j] = t;
  }
  ss_inv<D>(X, Y);
  long double W[D][2 * D];
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) { W[i][j] = (long double)X[i][j] * s[j] / s[i]; W[i][D + j] = i == j ? 1.0L : 0.0L; }
  for (int c = 0; c < D; ++c) {
    int piv = c;
    for (int i = c + 1; i < D; ++i) if (fabsl(W[i][c]) > fabsl(W[piv][c])) piv = i;
    for (int j = 0; j < 2 * D; ++j) { long double t = W[c][j]; W[c][j] = W[piv][j]; W[piv][j] = t; }
    const long double d = W[c][c];
    for (int j = 0; j < 2 * D; ++j) W[c][j] /= d;
    for (int i = 0; i < D; ++i) if (i != c) { const long double f = W[i][c]; for (int j = 0; j < 2 * D; ++j) W[i][j] -= f * W[c][j]; }
  }
  long double err = 0.0L, big = 0.0L;
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
    const long double ref = W[i][D + j], got = (long double)Y[i][j] * s[j] / s[i];
    if (fabsl(got - ref) > err) err = fabsl(got - ref);
    if (fabsl(ref) > big) big = fabsl(ref);
  }
  return (double)(err / big);
}
int main() {
  double worst4 = 0.0, worst3 = 0.0;
  const double lams[4] = {1.0, 30.0, 1e3, 1e-2};
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) for (int rep = 0; rep < 50; ++rep) {
    const double la = lams[a], lb = lams[b];
    const double s22[4] = {1.0, la, 1.0, lb}, s13[4] = {1.0, 1.0, lb, lb * lb}, s3[3] = {1.0, la, la * la};
    for (int rank = 1; rank <= 4; ++rank) {
      const double e1 = trial<4>(s22, rank), e2 = trial<4>(s13, rank);
      worst4 = e1 > worst4 ? e1 : worst4; worst4 = e2 > worst4 ? e2 : worst4;
    }
    const double e3 = trial<3>(s3, 3);
    worst3 = e3 > worst3 ? e3 : worst3;
  }
  std::printf("%.3e %.3e\n", worst4, worst3);
  return 0;
}
"""


def test_ss_inv_d4_host(tmp_path):
    """ss_inv<4> on I + C J, scaled like (f, f', ..) with rate constants from 1e-2 to 1e3, against long-double Gauss-Jordan: the error
    in the scaled sense stays at rounding level whatever the scaling, as for the D = 3 cofactors beside it."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src, exe = tmp_path / "ss_inv_check.cpp", tmp_path / "ss_inv_check"
    src.write_text(SS_INV_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    worst4, worst3 = float(out[0]), float(out[1])
    print(f"ss_inv: D = 4 worst scaled error {worst4:.2e}, D = 3 {worst3:.2e}")
    assert worst4 <= 1e-12 and worst3 <= 1e-12


# ---- the Python mirror, with the library stubbed out ---------------------------------------------------------------------------------
def _no_library():
    raise AssertionError("the library was reached")


def _fx(kernel, n=4):
    fs = lmm_amd.independent_mogp([lmm_amd.GP(kernel)])
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(float(n)), 2)
    H = lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0]))
    return lmm_amd.ILMM(fs, H)(x, 0.1)


def _kernel(kind, quality=3.0):
    return {"matern12": lmm_amd.Matern12Kernel, "matern32": lmm_amd.Matern32Kernel, "matern52": lmm_amd.Matern52Kernel,
            "se": lmm_amd.SEKernel}[kind](0.8, 1.7) if kind != "sho" else lmm_amd.SHOKernel(0.8, 1.7, quality)


SERVED = PAIRS + (("sho", "matern12"), ("matern52", "matern12"))      # what the library serves: either order of the terms
# The Python state-space functions serve the Matern-only pairs.  A sum with an SHO term stays refused by them, naming the latent
# (tests/test_sho_abi.py pins that refusal); the C ABI serves it, which the registry test below and the GPU tests reach directly.
MIRROR_SERVED = tuple(p for p in SERVED if "sho" not in p)


@pytest.mark.parametrize("pair", MIRROR_SERVED, ids=["+".join(p) for p in MIRROR_SERVED])
def test_served_sums_reach_the_library(pair):
    fx = _fx(lmm_amd.KernelSum(_kernel(pair[0]), _kernel(pair[1]), variance=1.2, lengthscale=0.9))
    y = np.zeros(8)
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        for call in (lambda: lmm_amd.statespace_logpdf(fx, y), lambda: lmm_amd.statespace_mean_and_var(fx, y),
                     lambda: lmm_amd.statespace_logpdf_and_gradient(fx, y), lambda: lmm_amd.statespace_rand(np.random.default_rng(0), fx, y),
                     lambda: lmm_amd.statespace_rand(np.random.default_rng(0), fx), lambda: lmm_amd.statespace_posterior(fx, y)):
            with pytest.raises(AssertionError, match="the library was reached"):
                call()
    finally:
        L.ensure_init = saved


def test_out_of_scope_sums_are_refused_before_any_library_call():
    M32, M52, M12 = _kernel("matern32"), _kernel("matern52"), _kernel("matern12")
    bad = {"three terms": lmm_amd.KernelSum(M12, M12, M12), "Matern32 + Matern52": lmm_amd.KernelSum(M32, M52),
           "Matern52 + SHO": lmm_amd.KernelSum(M52, _kernel("sho")), "SE + Matern32": lmm_amd.KernelSum(_kernel("se"), M32),
           "an ARD term": lmm_amd.KernelSum(M12, lmm_amd.Matern32Kernel(1.0, np.array([0.5]))), "one term": lmm_amd.KernelSum(M32),
           "Matern32 + SHO": lmm_amd.KernelSum(M32, _kernel("sho")), "SHO + Matern12": lmm_amd.KernelSum(_kernel("sho"), M12)}
    y = np.zeros(8)
    bad = {name: _fx(k) for name, k in bad.items()}
    served = _fx(lmm_amd.KernelSum(M32, M12))
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    try:
        for name, fx in bad.items():
            for fn in (lmm_amd.statespace_logpdf, lmm_amd.statespace_mean_and_var, lmm_amd.statespace_logpdf_and_gradient,
                       lmm_amd.statespace_posterior):
                with pytest.raises(NotImplementedError, match="latent 0"):
                    fn(fx, y)
            with pytest.raises(NotImplementedError, match="latent 0"):
                lmm_amd.statespace_rand(np.random.default_rng(0), fx, y)
        with pytest.raises(NotImplementedError, match="latent 0"):
            lmm_amd.statespace_logpdf_and_gradient(served, y, inputs=True)
        fake = lmm_amd.model.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0, [3], 3.0, [0])
        try:
            with pytest.raises(NotImplementedError, match="latent 0"):
                fake.mean_and_var_vjp(np.zeros(3), dmean=np.zeros(6))
        finally:
            fake._ptr = None                                             # nothing to free
        # the dense path's array keeps refusing an SHO term, before any library call
        with pytest.raises(NotImplementedError, match="latent 0"):
            L.gps_array([lmm_amd.KernelSum(_kernel("se"), _kernel("sho")).desc()])
    finally:
        L.ensure_init, L.load = saved


def test_state_dimensions_of_the_mirror():
    M = lmm_amd.model
    for pair in PAIRS:
        want = None if "sho" in pair else TERM_DIM[pair[0]] + TERM_DIM[pair[1]]
        assert M._statespace_dim(lmm_amd.KernelSum(_kernel(pair[0]), _kernel(pair[1]))) == want
    assert M._statespace_dim(lmm_amd.KernelSum(_kernel("matern32"), _kernel("matern52"))) is None
    assert M._statespace_dim(_kernel("matern52")) == 3 and M._statespace_dim(_kernel("se")) is None


# ---- the tag registry (no GPU, no lmm_init) -----------------------------------------------------------------------------------------
KIND = {"matern12": 3, "matern32": 1, "matern52": 2, "se": 0, "sho": L.KERNEL_SHO}


def _terms(kinds, tags=None):
    arr = (L.GpT * len(kinds))()
    for c, k in enumerate(kinds):
        arr[c].kind = KIND[k] | ((tags[c] if tags else 0) << 8)
        arr[c].variance, arr[c].lengthscale, arr[c].mean = 1.0 + c, 0.5 + c, 0.0
    return arr


def test_sum_creators_without_a_gpu():
    lib = lmm_amd.load()
    made = []

    def create(fn, kinds, tags=None):
        t = C.c_int(0)
        rc = fn(len(kinds), _terms(kinds, tags), C.byref(t))
        if rc == L.LMM_OK:
            made.append(t.value)
        return rc

    new, old = lib.lmm_kernel_sum_create_statespace, lib.lmm_kernel_sum_create
    q = C.c_int(0)
    assert lib.lmm_kernel_tag_create_sho(C.c_double(3.0), C.byref(q)) == L.LMM_OK
    ard = C.c_int(0)
    one = (C.c_double * 1)(0.5)
    assert lib.lmm_ard_create(1, one, C.byref(ard)) == L.LMM_OK
    try:
        for pair in SERVED:
            assert create(new, pair) == L.LMM_OK, pair
            tags = [q.value if k == "sho" else 0 for k in pair]
            assert create(new, pair, tags) == L.LMM_OK, pair
        for kinds in (("matern12", "matern12", "matern12"), ("matern32",), ("matern32", "matern52"), ("matern52", "sho"),
                      ("matern52", "matern52"), ("se", "matern32")):
            assert create(new, kinds) == L.LMM_ERR_UNSUPPORTED, kinds
        assert create(new, ("matern12", "matern32"), [0, ard.value]) == L.LMM_ERR_UNSUPPORTED          # an ARD term
        assert create(new, ("matern12", "sho"), [0, ard.value]) == L.LMM_ERR_ARG                       # an SHO term's tag is a quality tag
        assert create(new, ("matern12", "sho"), [0, 1 << 20]) == L.LMM_ERR_ARG                         # an unknown tag
        t = C.c_int(0)
        assert new(0, _terms(("matern12",)), C.byref(t)) == L.LMM_ERR_ARG and new(2, None, C.byref(t)) == L.LMM_ERR_ARG
        bad = _terms(("matern12", "matern32"))
        bad[1].variance = -1.0
        assert new(2, bad, C.byref(t)) == L.LMM_ERR_ARG
        # the dense path's creator is as it was: kind 12 is refused, a Matern-only sum is taken
        assert create(old, ("matern32", "sho")) == L.LMM_ERR_UNSUPPORTED
        assert create(old, ("matern32", "matern12")) == L.LMM_OK
        g = (L.GpGradT * 2)()
        assert lib.lmm_kernel_sum_grad(made[0], g) == L.LMM_OK and g[0].variance == 0.0 and g[1].lengthscale == 0.0
    finally:
        for t in made + [q.value, ard.value]:
            lib.lmm_ard_destroy(t)


def test_new_symbols_declared_exported_and_bound():
    import re
    lib = lmm_amd.load()
    with open(os.path.join(ROOT, "include", "lmm_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for s in ("lmm_kernel_sum_create_statespace", "lmm_dev_statespace_grad_sum"):
        assert hasattr(lib, s) and s in L.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % s, src), s
    assert getattr(lib, "lmm_dev_statespace_grad_sum").argtypes == L.STATESPACE_ARGTYPES["lmm_dev_statespace_grad_sho"]


if __name__ == "__main__":
    for (pair, q, n), d in deltas_sum().items():
        g = deltas_sum_grad()[(pair, q, n)]
        rd = deltas_sum_rand().get((pair, q, n))
        law = "" if rd is None else f"  prior law {rd[0]:.2e}  posterior law {rd[1]:.2e}"
        print(f"{'+'.join(pair):18s} Q={q:5.2f} n={n:4d}  value {d[0]:.2e}  filtered {d[1]:.2e}  smoothed {d[2]:.2e}  gradient {g:.2e}{law}")
    print(f"delta_sum = {delta_sum():.2e}  delta_sum_grad = {delta_sum_grad():.2e}  delta_sum_rand = {delta_sum_rand():.2e}")
