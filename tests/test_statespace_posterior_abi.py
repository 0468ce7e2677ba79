"""Host-only checks of the state-space posterior object (include/lmm_hip.h "state space: the posterior object"; DESIGN.md 4.18
"Posterior object"): the NumPy restatement of the full-state smoother and of the interpolation at new inputs agrees with the dense
Gaussian posterior, the entry points are declared, exported and bound with matching arity, and every refusal of the Python mirror
comes before any library call.  The restatement is built from the functions of tests/test_statespace_abi.py (the Matern models, its
`case`) and the model interface of tests/test_sho_abi.py (which serves the Matern kinds and the oscillator alike);
tests/test_gpu_statespace_posterior.py imports it from here.  No GPU and no lmm_init needed.

delta_posterior(), the largest disagreement between the restated interpolation and the dense Gaussian over every case below, was
measured at 1.7e-13 (the Matern kinds alone: 8.9e-15; the largest is the mean of the SHO latent with Q = 50 at n = 257);
test_statespace_abi.delta() is 7.6e-15.  The GPU tolerance is max(1e-10, 100 max(delta(), delta_posterior())) = 1e-10.

`python tests/test_statespace_posterior_abi.py` prints the disagreements."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmm_amd
from lmm_amd import _lib as L

import test_sho_abi as S
import test_statespace_abi as T

HEADER = T.HEADER
SYMS = ("lmm_oilmm_statespace_posterior_create", "lmm_statespace_post_destroy", "lmm_oilmm_statespace_post_mean_and_var",
        "lmm_dev_statespace_states", "lmm_dev_statespace_interp", "lmm_dev_statespace_interp_layout")


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def model_of(kind, v, ell, quality=None):
    """test_sho_abi.Model: D, Pinf, AQ(dt) and K(x, x2) of a Matern latent (through test_statespace_abi.ss_model / ss_AQ) or of an
    oscillator."""
    return S.Model(kind, v, ell, quality)


def bwd_element(model, dt, m, P):
    """test_statespace_abi.bwd_element (not the last point) for any model: (E, g, L) of a state (m, P) whose successor lies dt
    further."""
    A, Q = model.AQ(dt)
    E = P @ A.T @ np.linalg.inv(A @ P @ A.T + Q)
    return E, m - E @ A @ m, P - E @ A @ P


def full_states(model, x, w, r):
    """(fm (n, D), fP (n, D, D), sm, sP): the filtered states of the sequential filter and the FULL smoothed states of the sequential
    Rauch-Tung-Striebel recursion over the backward elements."""
    _, _, _, fm, fP = S.kalman_filter(model, x, w, r)
    n = len(x)
    sm, sP = np.zeros_like(fm), np.zeros_like(fP)
    g, Lm = fm[-1].copy(), fP[-1].copy()
    sm[-1], sP[-1] = g, Lm
    for t in range(n - 2, -1, -1):
        E, ge, Le = bwd_element(model, x[t + 1] - x[t], fm[t], fP[t])
        g, Lm = E @ g + ge, E @ Lm @ E.T + Le
        sm[t], sP[t] = g, Lm
    return fm, fP, sm, sP


def interp_state(model, x, fm, fP, sm, sP, s):
    """The posterior state (m, P) at the input s: k = #{t : x_t <= s}; the filtered state of point k - 1 predicted over s - x_{k-1}
    (the prior when k = 0), then one RTS step back from the smoothed state of point k over x_k - s (none when k = n)."""
    n = len(x)
    k = int(np.searchsorted(x, s, side="right"))
    if k == 0:
        m, P = np.zeros(model.D), model.Pinf.copy()
    else:
        A, Q = model.AQ(s - x[k - 1])
        m, P = A @ fm[k - 1], A @ fP[k - 1] @ A.T + Q
    if k < n:
        E, g, Lm = bwd_element(model, x[k] - s, m, P)
        m, P = E @ sm[k] + g, E @ sP[k] @ E.T + Lm
    return m, P


def interp_reference(model, x, states, xs):
    """(mean, var): the zero-mean first-component marginals at the queries xs from the stored states."""
    out = [interp_state(model, x, *states, s) for s in xs]
    return np.array([m[0] for m, _ in out]), np.array([P[0, 0] for _, P in out])


def dense_posterior(model, x, w, r, xs):
    """The same from K + diag(w) over the observed points."""
    obs = np.flatnonzero(np.isfinite(w))
    xs = np.asarray(xs)
    if len(obs) == 0:
        return np.zeros(len(xs)), np.full(len(xs), model.v)
    import scipy.linalg as sla
    Lc = np.linalg.cholesky(model.K(x[obs]) + np.diag(w[obs]))
    V = sla.solve_triangular(Lc, model.K(x[obs], xs), lower=True)
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    return V.T @ u, model.v - (V * V).sum(axis=0)


def queries(x, seed=0):
    """Q(x): 40 uniform draws on [x_0 - 2, x_{n-1} + 2], 5 training inputs, both ends, 1e-9 beyond either end; shuffled."""
    rng = np.random.default_rng([seed, len(x)])
    q = np.concatenate([rng.uniform(x[0] - 2.0, x[-1] + 2.0, 40), rng.choice(x, 5), [x[0], x[-1], x[0] - 1e-9, x[-1] + 1e-9]])
    return rng.permutation(q)


CPU_N = T.CPU_N
_DELTA = {}


def cases():
    """(label, model, (x, w, r)) of every comparison: the three Matern kinds on test_statespace_abi.case at CPU_N, the oscillator on
    test_sho_abi.case (ties included) at its qualities and sizes."""
    for kind in T.KINDS:
        for n in CPU_N:
            v, ell, x, w, r = T.case(kind, n)
            yield (kind, n), model_of(kind, v, ell), (x, w, r)
    for Q in S.QS:
        for n in S.CPU_N:
            v, P, x, w, r = S.case(Q, n)
            yield ("sho Q=%g" % Q, n), S.sho(v, P, Q), (x, w, r)


def deltas():
    """{(label, n): (mean, var)} disagreements of the restated interpolation with the dense Gaussian posterior at Q(x)."""
    if not _DELTA:
        for key, model, (x, w, r) in cases():
            xs = queries(x)
            gm, gv = interp_reference(model, x, full_states(model, x, w, r), xs)
            dm, dv = dense_posterior(model, x, w, r, xs)
            _DELTA[key] = (T.arr_err(gm, dm) if np.abs(dm).max() > 0 else float(np.abs(gm).max()), T.arr_err(gv, dv))
    return _DELTA


def delta_posterior():
    """The largest disagreement over every case: with test_statespace_abi.delta(), the DELTA of the GPU tolerances."""
    return max(max(d) for d in deltas().values())


def test_restated_interpolation_agrees_with_dense_posterior():
    for key, d in deltas().items():
        print(f"{key[0]} n={key[1]}: mean {d[0]:.2e} var {d[1]:.2e}")
        assert max(d) <= 1e-12, (key, d)
    print(f"delta_posterior = {delta_posterior():.2e}")


@pytest.mark.parametrize("kind", T.KINDS)
def test_full_smoother_restates_the_first_component_smoother(kind):
    """The full-state recursion's first component is test_statespace_abi's smoother, and its elements are test_statespace_abi's."""
    v, ell, x, w, r = T.case(kind, 65)
    model = model_of(kind, v, ell)
    fm, fP, sm, sP = full_states(model, x, w, r)
    _, _, _, ms, Ps = T.kalman_filter(kind, v, ell, x, w, r)
    assert np.abs(fm - ms).max() <= 1e-14 and np.abs(fP - Ps).max() <= 1e-14
    rm, rv = T.rts_smoother(kind, v, ell, x, ms, Ps, 65)
    assert np.abs(sm[:, 0] - rm).max() <= 1e-12 and np.abs(sP[:, 0, 0] - rv).max() <= 1e-12
    for a, b in zip(bwd_element(model, 0.3, fm[7], fP[7]), T.bwd_element(T.ss_model(kind, v, ell), False, 0.3, ms[7], Ps[7])):
        assert np.abs(a - b).max() <= 1e-14


def test_tie_rule_and_the_ends():
    """A query on a training input (duplicated or not) returns that input's smoothed marginal; in front of the data with nothing
    observed the prior; far behind the data the prior as well."""
    for model, (x, w, r) in ((S.sho(*S.case(2.0, 63)[:2], 2.0), S.case(2.0, 63)[2:]),
                             (model_of("matern52", *T.case("matern52", 65)[:2]), T.case("matern52", 65)[2:])):
        x = x.copy()
        x[20:23] = x[20]
        st = full_states(model, x, w, r)
        for t in (0, 5, 20, 21, 22, len(x) - 1):
            m, P = interp_state(model, x, *st, x[t])
            last = np.flatnonzero(x == x[t]).max()
            assert np.abs(m - st[2][last]).max() <= 1e-12 and np.abs(P - st[3][last]).max() <= 1e-12
            sm1, sv1 = S.statespace_reference(model, x, w, r)[3:]
            assert abs(m[0] - sm1[t]) <= 1e-11 and abs(P[0, 0] - sv1[t]) <= 1e-11          # every copy of a tie has one marginal
        m, P = interp_state(model, x, *st, x[-1] + 1e6)
        assert np.abs(m).max() <= 1e-12 and np.abs(P - model.Pinf).max() <= 1e-9 * np.abs(model.Pinf).max()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_posterior_symbols_declared_exported_and_bound():
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
    proto = re.search(r"int\s+lmm_oilmm_statespace_posterior_create\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "out", "out_logpdf"]
    assert "typedef struct lmm_ss_post lmm_ss_post_t;" in src


def test_exports():
    assert "statespace_posterior" in lmm_amd.__all__ and "StateSpacePosterior" in lmm_amd.__all__
    assert lmm_amd.statespace_posterior is lmm_amd.model.statespace_posterior
    assert lmm_amd.StateSpacePosterior is lmm_amd.model.StateSpacePosterior


def _no_library(*a, **k):
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    fs, x, H = T._models()
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
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    fake = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0)          # never reaches the library: every call below is refused first
    try:
        fn = lmm_amd.statespace_posterior
        for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                             (sparse, y, "posterior model"), (oilmm, np.zeros((8, 2)), "matrix Y"), (sharded, y, "sharded"),
                             (features, y, "MOInputIsotopicByOutputs"), (perpoint, y, "scalar noise"), (d2, y, "d = 2"),
                             (se, y, "latent 0"), (rq, y, "latent 0"), (per, y, "latent 0"), (lp, y, "latent 0"),
                             (ksum, y, "latent 0"), (ard, y, "latent 0")):
            with pytest.raises(NotImplementedError, match=what):
                fn(fx, yy)
        with pytest.raises(ValueError, match="length"):
            fn(oilmm, np.zeros(7))
        # bad xs: another shape, NaN, +-Inf
        for call in (fake.mean_and_var, fake.mean, fake.var, fake.marginals):
            with pytest.raises(ValueError, match="xs"):
                call(np.zeros((2, 3)))
            for bad in (np.nan, np.inf, -np.inf):
                with pytest.raises(ValueError, match="finite"):
                    call(np.array([0.0, bad, 1.0]))
        # no queries: empty arrays, no library call
        m0, v0 = fake.mean_and_var(np.zeros(0))
        assert m0.shape == (0,) and v0.shape == (0,)
        assert fake.n == 4 and fake.p == 2 and fake.logpdf == 0.0
        # a closed handle
        closed = M.StateSpacePosterior(None, 4, 2, 0.0)
        closed.close()                                               # closing twice is fine
        for call in (closed.mean_and_var, closed.mean, closed.var, closed.marginals):
            with pytest.raises(ValueError, match="closed"):
                call(np.zeros(3))
        with M.StateSpacePosterior(None, 4, 2, 0.0) as ctx:
            assert isinstance(ctx, M.StateSpacePosterior)
    finally:
        fake._ptr = None                                             # nothing to free
        L.ensure_init, L.load = saved


if __name__ == "__main__":
    for key, d in deltas().items():
        print(f"{key[0]:12s} n={key[1]:5d}  mean {d[0]:.2e}  var {d[1]:.2e}")
    print(f"delta_posterior = {delta_posterior():.2e}   (test_statespace_abi.delta() = {T.delta():.2e})")
