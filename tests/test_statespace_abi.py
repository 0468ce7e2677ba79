"""Host-only checks of state-space inference for Matern latents (include/lmm_hip.h "state space"): the entry points are
declared, exported and bound with matching arity, every refusal of the Python mirror comes before any library call, sorting and
un-permuting is right, and the NumPy restatement of the mathematics (the Kalman filter, the scan elements with their combine, the
smoother) agrees with the dense Gaussian.  Their largest disagreement DELTA fixes the GPU tolerances of tests/test_gpu_statespace.py,
max(1e-10, 100 DELTA), which imports the restatement from here.  No GPU and no lmm_init needed.

`python tests/test_statespace_abi.py` prints the disagreements."""
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
from oracle import lmm_oracle as O

HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SYMS = ("lmm_oilmm_logpdf_statespace", "lmm_oilmm_mean_and_var_statespace", "lmm_dev_statespace_filter", "lmm_dev_statespace_smooth")
KINDS = ("matern12", "matern32", "matern52")
LOG2PI = float(np.log(2.0 * np.pi))


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def ss_model(kind, v, ell):
    """(lam, F, Pinf) of the SDE whose first component has the Matern covariance of oracle.kernel_eval (Matern12: v exp(-r / ell))."""
    if kind == "matern12":
        lam = 1.0 / ell
        return lam, np.array([[-lam]]), np.array([[v]])
    if kind == "matern32":
        lam = np.sqrt(3.0) / ell
        return lam, np.array([[0.0, 1.0], [-lam ** 2, -2.0 * lam]]), np.diag([v, lam ** 2 * v])
    if kind == "matern52":
        lam = np.sqrt(5.0) / ell
        F = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam ** 3, -3.0 * lam ** 2, -3.0 * lam]])
        k = lam ** 2 / 3.0
        return lam, F, v * np.array([[1.0, 0.0, -k], [0.0, k, 0.0], [-k, 0.0, lam ** 4]])
    raise ValueError(kind)


def ss_AQ(model, dt):
    """A(dt) = exp(-lam dt) (I + N dt + N^2 dt^2 / 2) with N = F + lam I nilpotent; Q(dt) = Pinf - A Pinf A'."""
    lam, F, Pinf = model
    D = F.shape[0]
    N = F + lam * np.eye(D)
    A = np.exp(-lam * dt) * (np.eye(D) + N * dt + (N @ N) * (dt * dt / 2.0 if D > 2 else 0.0))
    return A, Pinf - A @ Pinf @ A.T


def kalman_filter(kind, v, ell, x, w, r):
    """The sequential filter: (value, filtered first-component mean, variance, states m (n, D), P (n, D, D)).  w = +inf: unobserved."""
    model = ss_model(kind, v, ell)
    D = model[1].shape[0]
    n = len(x)
    m, P = np.zeros(D), model[2].copy()
    ms, Ps = np.zeros((n, D)), np.zeros((n, D, D))
    val = 0.0
    for t in range(n):
        if t > 0:
            A, Q = ss_AQ(model, x[t] - x[t - 1])
            m, P = A @ m, A @ P @ A.T + Q
        if np.isfinite(w[t]):
            S = P[0, 0] + w[t]
            K = P[:, 0] / S
            e = r[t] - m[0]
            m, P = m + K * e, P - np.outer(K, P[0, :])
            val += -0.5 * (LOG2PI + np.log(S) + e * e / S)
        ms[t], Ps[t] = m, P
    return val, ms[:, 0].copy(), Ps[:, 0, 0].copy(), ms, Ps


def fwd_element(model, first, dt, w, r):
    """(A, b, C, eta, J) of one point; the first point takes (0, Pinf) for (A, Q)."""
    D = model[1].shape[0]
    A, Q = (np.zeros((D, D)), model[2].copy()) if first else ss_AQ(model, dt)
    if not np.isfinite(w):
        return A, np.zeros(D), Q, np.zeros(D), np.zeros((D, D))
    S = Q[0, 0] + w
    K = Q[:, 0] / S
    IKh = np.eye(D)
    IKh[:, 0] -= K
    return IKh @ A, K * r, IKh @ Q, A[0, :] * r / S, np.outer(A[0, :], A[0, :]) / S


def fwd_combine(ei, ej):
    """ei before ej."""
    Ai, bi, Ci, hi, Ji = ei
    Aj, bj, Cj, hj, Jj = ej
    D = len(bi)
    M = Aj @ np.linalg.inv(np.eye(D) + Ci @ Jj)
    Mp = Ai.T @ np.linalg.inv(np.eye(D) + Jj @ Ci)
    return M @ Ai, M @ (bi + Ci @ hj) + bj, M @ Ci @ Aj.T + Cj, Mp @ (hj - Jj @ bi) + hi, Mp @ Jj @ Ai + Ji


def bwd_element(model, last, dt, m, P):
    D = len(m)
    if last:
        return np.zeros((D, D)), m.copy(), P.copy()
    A, Q = ss_AQ(model, dt)
    E = P @ A.T @ np.linalg.inv(A @ P @ A.T + Q)
    return E, m - E @ A @ m, P - E @ A @ P


def bwd_combine(ei, ej):
    Ei, gi, Li = ei
    Ej, gj, Lj = ej
    return Ei @ Ej, Ei @ gj + gi, Ei @ Lj @ Ei.T + Li


def chunked_scan(elems, combine, chunk, reverse=False):
    """The three-phase schedule on the host: fold runs of `chunk` elements, scan the aggregates, return the inclusive prefix (suffix)
    of every aggregate."""
    n = len(elems)
    aggs = []
    for t0 in range(0, n, chunk):
        acc = elems[t0]
        for t in range(t0 + 1, min(n, t0 + chunk)):
            acc = combine(acc, elems[t])
        aggs.append(acc)
    if reverse:
        for j in range(len(aggs) - 2, -1, -1):
            aggs[j] = combine(aggs[j], aggs[j + 1])
    else:
        for j in range(1, len(aggs)):
            aggs[j] = combine(aggs[j - 1], aggs[j])
    return aggs


def parallel_filter(kind, v, ell, x, w, r, chunk):
    """The filter through the scan: the prefix's (b, C) restarts the sequential recursion of each run."""
    model = ss_model(kind, v, ell)
    n = len(x)
    elems = [fwd_element(model, t == 0, 0.0 if t == 0 else x[t] - x[t - 1], w[t], r[t]) for t in range(n)]
    aggs = chunked_scan(elems, fwd_combine, chunk)
    fm, fv = np.zeros(n), np.zeros(n)
    for j, t0 in enumerate(range(0, n, chunk)):
        t1 = min(n, t0 + chunk)
        _, b, C, _, _ = aggs[j]           # the filtered state at the run's last point
        fm[t1 - 1], fv[t1 - 1] = b[0], C[0, 0]
    # every point: fold the elements one by one (the prefix of a run of length 1)
    acc = elems[0]
    full_m, full_v = [acc[1][0]], [acc[2][0, 0]]
    for t in range(1, n):
        acc = fwd_combine(acc, elems[t])
        full_m.append(acc[1][0]); full_v.append(acc[2][0, 0])
    return np.array(full_m), np.array(full_v), fm, fv


def rts_smoother(kind, v, ell, x, ms, Ps, chunk=7):
    """Smoothed first-component mean and variance from the filtered states, through the backward elements and a chunked suffix scan."""
    model = ss_model(kind, v, ell)
    n = len(x)
    elems = [bwd_element(model, t == n - 1, 0.0 if t == n - 1 else x[t + 1] - x[t], ms[t], Ps[t]) for t in range(n)]
    aggs = chunked_scan(elems, bwd_combine, chunk, reverse=True)
    sm, sv = np.zeros(n), np.zeros(n)
    for j, t0 in enumerate(range(0, n, chunk)):
        t1 = min(n, t0 + chunk)
        if t1 < n:
            _, g, Lm = aggs[j + 1]
        else:
            g, Lm = np.zeros(len(ms[0])), np.zeros_like(Ps[0])
        for t in range(t1 - 1, t0 - 1, -1):
            E, ge, Le = elems[t]
            g, Lm = E @ g + ge, E @ Lm @ E.T + Le
            sm[t], sv[t] = g[0], Lm[0, 0]
    return sm, sv


def statespace_reference(kind, v, ell, x, w, r):
    """(value, filtered mean, filtered variance, smoothed mean, smoothed variance) of the restatement."""
    val, fm, fv, ms, Ps = kalman_filter(kind, v, ell, x, w, r)
    sm, sv = rts_smoother(kind, v, ell, x, ms, Ps)
    return val, fm, fv, sm, sv


# ---- the dense Gaussian it is compared with -------------------------------------------------------------------------------------
def matern_K(kind, v, ell, x, x2=None):
    if kind == "matern12":
        return v * np.exp(-O.pairwise_dist(x, x2) / ell)
    return O.kernelmatrix({"kind": kind, "variance": v, "lengthscale": ell}, x, x2)


def dense_reference(kind, v, ell, x, w, r):
    """The same five quantities from K + diag(w) over the observed points: with L its Cholesky factor (time order), u = L^-1 r and
    V = L^-1 K(obs, all), conditioning on the first j observations is a sum over the first j rows of V and u."""
    import scipy.linalg as sla
    n = len(x)
    obs = np.flatnonzero(np.isfinite(w))
    if len(obs) == 0:
        return 0.0, np.zeros(n), np.full(n, v), np.zeros(n), np.full(n, v)
    Lc = np.linalg.cholesky(matern_K(kind, v, ell, x[obs]) + np.diag(w[obs]))
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    V = sla.solve_triangular(Lc, matern_K(kind, v, ell, x[obs], x), lower=True)
    val = -0.5 * (len(obs) * LOG2PI + 2.0 * np.log(np.diag(Lc)).sum() + u @ u)
    cm = np.vstack([np.zeros(n), np.cumsum(V * u[:, None], axis=0)])
    cv = np.vstack([np.zeros(n), np.cumsum(V * V, axis=0)])
    seen = np.cumsum(np.isfinite(w))                   # observations at or before each point
    t = np.arange(n)
    return val, cm[seen, t], v - cv[seen, t], cm[-1], v - cv[-1]


def case(kind, n, seed=0, unobserved=True):
    """Inputs of the comparison: spacings dt / ell between about 0.01 and 1 (log-uniform), w in [0.05, 0.5], a quarter of the points
    unobserved (the first one among them)."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    ell, v = 0.7, 1.3
    x = np.cumsum(ell * 10.0 ** rng.uniform(-2.0, 0.0, n)) - 1.0
    w = rng.uniform(0.05, 0.5, n)
    r = rng.standard_normal(n)
    if unobserved:
        miss = rng.random(n) < 0.25
        miss[0] = True
        w = np.where(miss, np.inf, w)
    return v, ell, x, w, r


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300) if a != b else 0.0


def arr_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


CPU_N = (1, 2, 5, 65, 257, 1000)
_DELTA = {}


def deltas():
    """{(kind, n): (value, filtered, smoothed, parallel filter)} disagreements of the restatement with the dense Gaussian."""
    if not _DELTA:
        for kind in KINDS:
            for n in CPU_N:
                v, ell, x, w, r = case(kind, n)
                val, fm, fv, sm, sv = statespace_reference(kind, v, ell, x, w, r)
                dv, dfm, dfv, dsm, dsv = dense_reference(kind, v, ell, x, w, r)
                pm, pv, _, _ = parallel_filter(kind, v, ell, x, w, r, 7)
                _DELTA[(kind, n)] = (rel(val, dv), max(arr_err(fm, dfm), arr_err(fv, dfv)), max(arr_err(sm, dsm), arr_err(sv, dsv)),
                                     max(arr_err(pm, dfm), arr_err(pv, dfv)))
    return _DELTA


def delta():
    """The largest disagreement over every case and quantity: DELTA of the GPU tolerances."""
    return max(max(d) for d in deltas().values())


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_agrees_with_dense(kind):
    for n in CPU_N:
        d = deltas()[(kind, n)]
        print(f"{kind} n={n}: value {d[0]:.2e} filtered {d[1]:.2e} smoothed {d[2]:.2e} scan {d[3]:.2e}")
        assert max(d) <= 1e-12, (kind, n, d)


@pytest.mark.parametrize("kind", KINDS)
def test_chunked_schedule_agrees_with_sequential_filter(kind):
    v, ell, x, w, r = case(kind, 65)
    _, fm, fv, ms, Ps = kalman_filter(kind, v, ell, x, w, r)
    for chunk in (1, 7, 64, 65):
        _, _, cm, cv = parallel_filter(kind, v, ell, x, w, r, chunk)
        ends = [min(65, t0 + chunk) - 1 for t0 in range(0, 65, chunk)]
        assert np.abs(cm[ends] - fm[ends]).max() <= 1e-12 and np.abs(cv[ends] - fv[ends]).max() <= 1e-12
        sm, sv = rts_smoother(kind, v, ell, x, ms, Ps, chunk)
        sm1, sv1 = rts_smoother(kind, v, ell, x, ms, Ps, 65)
        assert np.abs(sm - sm1).max() <= 1e-12 and np.abs(sv - sv1).max() <= 1e-12


def test_equal_points_and_complete_data():
    for kind in KINDS:
        v, ell, x, w, r = case(kind, 65, unobserved=False)
        x[10:14] = x[10]
        x[40] = x[39]
        got, ref = statespace_reference(kind, v, ell, x, w, r), dense_reference(kind, v, ell, x, w, r)
        assert rel(got[0], ref[0]) <= 1e-12
        for a, b in zip(got[1:], ref[1:]):
            assert arr_err(a, b) <= 1e-12


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_statespace_symbols_declared_exported_and_bound():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert proto, s
        params = [a.strip() for a in proto.group(1).split(",")]
        types = L.STATESPACE_ARGTYPES[s]
        assert len(params) == len(types), (s, len(params), len(types))
        assert getattr(lib, s).argtypes == types
        for a, t in zip(params, types):
            want = L._P if ("*" in a or "[" in a) else (L._D if a.startswith("double") else L._I)
            assert t is want, (s, a)
    proto = re.search(r"int\s+lmm_oilmm_logpdf_statespace\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "with_regulariser", "out"]
    assert "statespace_logpdf" in lmm_amd.__all__ and "statespace_mean_and_var" in lmm_amd.__all__


def _no_library():
    raise AssertionError("the library was reached")


def _models():
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel())])
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2)
    H = lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0]))
    return fs, x, H


def test_refusals_come_before_any_library_call():
    fs, x, H = _models()
    y = np.zeros(8)
    M = lmm_amd.model
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    sharded = lmm_amd.ILMM(fs, H, shard=(0, 0))(x, 0.1)
    post = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._PostHandle(None, 0, 1)), H)(x, 0.1)
    sparse = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._SparsePostHandle(None, 0, 1)), H)(x, 0.1)
    features = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), lmm_amd.MOInputIsotopicByFeatures(np.arange(4.0), 2), 0.1)
    perpoint = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), x, np.full(8, 0.1))
    d2 = lmm_amd.ILMM(fs, H)(lmm_amd.MOInputIsotopicByOutputs(np.zeros((2, 4)), 2), 0.1)

    def with_kernel(k):
        return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(k)]), H)(x, 0.1)

    se = with_kernel(lmm_amd.SEKernel())
    rq = with_kernel(lmm_amd.RationalQuadraticKernel())
    per = with_kernel(lmm_amd.PeriodicKernel())
    lp = with_kernel(lmm_amd.LocallyPeriodicKernel())
    ksum = with_kernel(lmm_amd.KernelSum(lmm_amd.Matern32Kernel(), lmm_amd.Matern52Kernel()))
    ard = with_kernel(lmm_amd.Matern52Kernel(1.0, np.array([0.5])))
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        for fn in (lmm_amd.statespace_logpdf, lmm_amd.statespace_mean_and_var):
            for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                                 (sparse, y, "posterior model"), (oilmm, np.zeros((8, 2)), "matrix Y"), (sharded, y, "sharded"),
                                 (features, y, "MOInputIsotopicByOutputs"), (perpoint, y, "scalar noise"), (d2, y, "d = 2"),
                                 (se, y, "latent 0"), (rq, y, "latent 0"), (per, y, "latent 0"), (lp, y, "latent 0"),
                                 (ksum, y, "latent 0"), (ard, y, "latent 0")):
                with pytest.raises(NotImplementedError, match=what):
                    fn(fx, yy)
            with pytest.raises(ValueError, match="length"):
                fn(oilmm, np.zeros(7))
        with pytest.raises(ValueError, match="xs"):
            lmm_amd.statespace_mean_and_var(oilmm, y, xs=np.zeros((2, 3)))
    finally:
        L.ensure_init = saved


def test_sorting_and_unpermuting_on_the_host():
    M = lmm_amd.model
    rng = np.random.default_rng(3)
    n, p, ns = 9, 3, 4
    x = rng.permutation(np.arange(n, dtype=np.float64))
    x[2] = x[5]                                           # a tie: the stable sort keeps their order
    y = rng.standard_normal(n * p)
    xs = rng.uniform(0, n, ns)
    for xt in (None, xs):
        xx, yy, perm, n0 = M._statespace_sorted(x, y, p, xt)
        N = n + (0 if xt is None else ns)
        assert xx.shape == (N,) and yy.shape == (N * p,) and n0 == n
        assert (np.diff(xx) >= 0).all()
        allx = x if xt is None else np.concatenate([x, xs])
        assert (xx == allx[perm]).all()
        assert list(perm[np.flatnonzero(xx == x[2])]) == sorted(perm[np.flatnonzero(xx == x[2])])
        Y = yy.reshape(p, N)
        back = M._statespace_unsorted(yy, perm, p, n0, xt is not None)
        if xt is None:
            assert (back == y).all()
        else:
            assert np.isnan(back).all() and back.shape == (ns * p,)
            assert (Y[:, np.argsort(perm, kind="stable")][:, :n].reshape(-1) == y).all()
    try:
        import torch
    except ImportError:
        return
    xx, yy, perm, n0 = M._statespace_sorted(torch.as_tensor(x), torch.as_tensor(y), p, None)
    assert (xx.numpy() == np.sort(x, kind="stable")).all()
    assert (M._statespace_unsorted(yy, perm, p, n0, False).numpy() == y).all()


if __name__ == "__main__":
    for (kind, n), d in deltas().items():
        print(f"{kind:9s} n={n:5d}  value {d[0]:.2e}  filtered {d[1]:.2e}  smoothed {d[2]:.2e}  scan {d[3]:.2e}")
    print(f"DELTA = {delta():.2e}")
