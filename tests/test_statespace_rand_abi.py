"""Host-only checks of state-space sampling (include/lmm_hip.h "state space", lmm_oilmm_rand_statespace; DESIGN.md 4.18 "Sampling"):
the NumPy restatement of the prior path and of the pathwise posterior, generic over the dtype, and what fixes the GPU tolerance of
tests/test_gpu_statespace_rand.py, max(1e-10, 100 delta) with three deltas, each asserted <= 1e-12 here:
  delta_rand : float64 against np.longdouble paths for FIXED normals at well-separated inputs (spacings 0.5 - 2 lengthscales, exact
               duplicates, one huge gap), in units of sqrt(variance).  The path is ill-conditioned in small spacings (Q's small pivots
               come out of a cancellation), so paths are compared only there;
  delta_law  : max|M M' - K| / variance for the linear map M from normals to path, down to spacings of 0.003 lengthscales: the law
               is not affected by that ill-conditioning;
  delta_post : the pathwise posterior against the dense Gaussian: its mean with zero normals, its covariance from unit-vector normals.
Also: the chunked affine scan against the sequential path, the symbols, the mirror's refusals, draw order and un-permuting.  No GPU
and no lmm_init needed.

`python tests/test_statespace_rand_abi.py` prints the deltas."""
import contextlib
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
SYMS = ("lmm_oilmm_rand_statespace", "lmm_dev_statespace_sample", "lmm_dev_statespace_sample_posterior")
KINDS = T.KINDS
DIM = {"matern12": 1, "matern32": 2, "matern52": 3}
ELL, VAR = 0.7, 1.3


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def ss_model_t(kind, v, ell, dt=np.float64):
    """T.ss_model with every constant formed in the dtype dt."""
    v, ell = dt(v), dt(ell)
    D = DIM[kind]
    lam = np.sqrt(dt(2 * D - 1)) / ell
    if D == 1:
        return lam, np.array([[-lam]], dtype=dt), np.array([[v]], dtype=dt)
    if D == 2:
        return lam, np.array([[0, 1], [-lam ** 2, -2 * lam]], dtype=dt), np.array([[v, 0], [0, lam ** 2 * v]], dtype=dt)
    F = np.array([[0, 1, 0], [0, 0, 1], [-lam ** 3, -3 * lam ** 2, -3 * lam]], dtype=dt)
    k = lam ** 2 / dt(3)
    return lam, F, v * np.array([[1, 0, -k], [0, k, 0], [-k, 0, lam ** 4]], dtype=dt)


def chol_psd(X):
    """Lower factor with non-negative diagonal; a pivot that is not > 0 gives a zero column."""
    D = X.shape[0]
    Lc = np.zeros_like(X)
    for j in range(D):
        s = X[j, j] - (Lc[j, :j] * Lc[j, :j]).sum()
        if not s > 0:
            continue
        Lc[j, j] = np.sqrt(s)
        for i in range(j + 1, D):
            Lc[i, j] = (X[i, j] - (Lc[i, :j] * Lc[j, :j]).sum()) / Lc[j, j]
    return Lc


def aff_elements(kind, v, ell, x, zeta, dt=np.float64):
    """[(A_t, c_t)]: s_t = A_t s_{t-1} + c_t with c_t = chol(Q_t) zeta_t; the first is (0, chol(Pinf) zeta_0).  zeta: (D, n)."""
    model = ss_model_t(kind, v, ell, dt)
    D = DIM[kind]
    x, zeta = np.asarray(x, dtype=dt), np.asarray(zeta, dtype=dt)
    out = []
    for t in range(len(x)):
        A, Q = (np.zeros((D, D), dtype=dt), model[2]) if t == 0 else T.ss_AQ(model, x[t] - x[t - 1])
        out.append((A, chol_psd(Q) @ zeta[:, t]))
    return out


def aff_combine(ei, ej):
    """ei before ej."""
    return ej[0] @ ei[0], ej[0] @ ei[1] + ej[1]


def prior_path(kind, v, ell, x, zeta, dt=np.float64):
    """The sequential prior path f_t = (s_t)_1, in the dtype dt."""
    s = np.zeros(DIM[kind], dtype=dt)
    f = np.zeros(len(x), dtype=dt)
    for t, (A, c) in enumerate(aff_elements(kind, v, ell, x, zeta, dt)):
        s = A @ s + c
        f[t] = s[0]
    return f


def scanned_path(kind, v, ell, x, zeta, chunk):
    """The three-phase schedule: fold, scan the aggregates, restart every run from its prefix state."""
    elems = aff_elements(kind, v, ell, x, zeta)
    aggs = T.chunked_scan(elems, aff_combine, chunk)
    n = len(x)
    f = np.zeros(n)
    for j, t0 in enumerate(range(0, n, chunk)):
        s = aggs[j - 1][1] if j else np.zeros(DIM[kind])
        for t in range(t0, min(n, t0 + chunk)):
            s = elems[t][0] @ s + elems[t][1]
            f[t] = s[0]
    return f


def pathwise_posterior(kind, v, ell, x, w, r, zeta, xi, dt=np.float64):
    """Matheron's rule: prior path + smoothed mean of r - f - sqrt(w) xi at the observed points (w = +inf: unobserved, xi not read).
    The prior path runs in dt; the filter and smoother are those of test_statespace_abi (float64)."""
    f = np.asarray(prior_path(kind, v, ell, x, zeta, dt), dtype=np.float64)
    obs = np.isfinite(w)
    rp = np.array(r, dtype=np.float64)
    rp[obs] = r[obs] - f[obs] - np.sqrt(w[obs]) * np.asarray(xi)[obs]
    _, _, _, ms, Ps = T.kalman_filter(kind, v, ell, x, w, rp)
    sm, _ = T.rts_smoother(kind, v, ell, x, ms, Ps)
    return f + sm


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def rand_case(kind, n, seed=0):
    """Well-separated inputs: spacings uniform in [0.5, 2] lengthscales, 10 % exact duplicates, one gap of 1e4 lengthscales (n > 2).
    Returns (v, ell, x, zeta (D, n))."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind), 77])
    d = ELL * rng.uniform(0.5, 2.0, n)
    d[rng.random(n) < 0.1] = 0.0
    if n > 2:
        d[n // 2] = 1e4 * ELL
    return VAR, ELL, np.cumsum(d) - 1.0, rng.standard_normal((DIM[kind], n))


LAW_SPACINGS = (1.0, 0.1, 0.01, 0.003)


def law_case(spacing, n=8):
    """n points `spacing` lengthscales apart, two of them duplicated."""
    d = np.full(n, spacing * ELL)
    d[[n // 3, n - 2]] = 0.0
    return np.cumsum(d)


def path_map(kind, v, ell, x):
    """M (n, D n): column i is the path of the i-th unit vector of normals (component-major, as the library's z)."""
    D, n = DIM[kind], len(x)
    M = np.zeros((n, D * n))
    for i in range(D * n):
        e = np.zeros(D * n)
        e[i] = 1.0
        M[:, i] = prior_path(kind, v, ell, x, e.reshape(D, n))
    return M


def dense_posterior(kind, v, ell, x, w, r):
    """(mean, covariance) of f at every point given the observed ones."""
    obs = np.flatnonzero(np.isfinite(w))
    K = T.matern_K(kind, v, ell, x)
    if len(obs) == 0:
        return np.zeros(len(x)), K
    G = np.linalg.solve(K[np.ix_(obs, obs)] + np.diag(w[obs]), K[obs, :])
    return G.T @ r[obs], K - K[:, obs] @ G


def posterior_map(kind, v, ell, x, w, r):
    """(the path with zero normals, B (n, D n + n)): B's columns are the path's linear part at the unit vectors of (zeta, xi)."""
    D, n = DIM[kind], len(x)
    zero = pathwise_posterior(kind, v, ell, x, w, r, np.zeros((D, n)), np.zeros(n))
    B = np.zeros((n, D * n + n))
    for i in range(D * n + n):
        e = np.zeros(D * n + n)
        e[i] = 1.0
        B[:, i] = pathwise_posterior(kind, v, ell, x, w, r, e[:D * n].reshape(D, n), e[D * n:]) - zero
    return zero, B


_CACHE = {}


def delta_rand():
    """{kind: max|float64 - longdouble| / sqrt(v)} of the prior path at the well-separated case, n = 200."""
    if "rand" not in _CACHE:
        out = {}
        for kind in KINDS:
            v, ell, x, zeta = rand_case(kind, 200)
            a = prior_path(kind, v, ell, x, zeta)
            b = prior_path(kind, v, ell, x, zeta, np.longdouble)
            out[kind] = float(np.abs(a - b).max() / np.sqrt(v))
        _CACHE["rand"] = out
    return _CACHE["rand"]


def delta_law():
    """{(kind, spacing): max|M M' - K| / v}, n = 8 with duplicates."""
    if "law" not in _CACHE:
        out = {}
        for kind in KINDS:
            for sp in LAW_SPACINGS:
                x = law_case(sp)
                M = path_map(kind, VAR, ELL, x)
                out[(kind, sp)] = float(np.abs(M @ M.T - T.matern_K(kind, VAR, ELL, x)).max() / VAR)
        _CACHE["law"] = out
    return _CACHE["law"]


POST_N = 24


def delta_post():
    """{kind: (mean, covariance)} disagreements of the pathwise restatement with the dense posterior, relative to the largest entry;
    the inputs of test_statespace_abi.case (spacings 0.01 - 1 lengthscales, a quarter of the points unobserved)."""
    if "post" not in _CACHE:
        out = {}
        for kind in KINDS:
            v, ell, x, w, r = T.case(kind, POST_N)
            zero, B = posterior_map(kind, v, ell, x, w, r)
            mu, Sg = dense_posterior(kind, v, ell, x, w, r)
            out[kind] = (T.arr_err(zero, mu), T.arr_err(B @ B.T, Sg))
        _CACHE["post"] = out
    return _CACHE["post"]


def delta():
    """The largest of the three: DELTA of the GPU tolerance max(1e-10, 100 DELTA)."""
    return max(max(delta_rand().values()), max(delta_law().values()), max(max(d) for d in delta_post().values()))


def test_float64_path_agrees_with_longdouble_at_separated_inputs():
    for kind, d in delta_rand().items():
        print(f"delta_rand {kind}: {d:.2e}")
        assert d <= 1e-12, (kind, d)


def test_law_of_the_prior_path_down_to_small_spacings():
    for key, d in delta_law().items():
        print(f"delta_law {key}: {d:.2e}")
        assert d <= 1e-12, (key, d)


def test_pathwise_posterior_agrees_with_dense():
    for kind, d in delta_post().items():
        print(f"delta_post {kind}: mean {d[0]:.2e} cov {d[1]:.2e}")
        assert max(d) <= 1e-12, (kind, d)


def test_chol_psd_clamps():
    assert (chol_psd(np.zeros((3, 3))) == 0).all()
    X = np.array([[4.0, 2.0, 2.0], [2.0, 1.0, 1.0], [2.0, 1.0, 5.0]])          # rank 2: the second pivot is exactly 0
    Lc = chol_psd(X)
    assert (Lc[:, 1] == 0).all() and np.abs(Lc @ Lc.T - X).max() <= 1e-15
    assert (np.diag(chol_psd(np.array([[1.0, 0.0], [0.0, -1e-20]]))) == [1.0, 0.0]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_chunked_affine_scan_agrees_with_sequential_path(kind):
    v, ell, x, zeta = rand_case(kind, 65)
    f = prior_path(kind, v, ell, x, zeta)
    for chunk in (1, 7, 64):
        assert np.abs(scanned_path(kind, v, ell, x, zeta, chunk) - f).max() <= 1e-12 * np.sqrt(v), chunk
    xd = x.copy()                                       # a duplicated point repeats the state
    xd[5] = xd[4]
    fd = prior_path(kind, v, ell, xd, zeta)
    assert fd[5] == fd[4]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_rand_symbols_declared_exported_and_bound():
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
    proto = re.search(r"int\s+lmm_oilmm_rand_statespace\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "add_noise", "nsamples", "z", "xi",
                     "eps", "out"]


def test_mirror_is_exported():
    assert callable(lmm_amd.statespace_rand) and "statespace_rand" in lmm_amd.__all__


def test_header_no_longer_lists_rand_as_missing():
    src = open(HEADER).read()
    block = src[src.index("---- state space"):src.index("int lmm_oilmm_logpdf_statespace(")]
    assert "sums of Matern terms, rand" not in block and "lmm_oilmm_rand_statespace" in block


def test_refusals_come_before_any_library_call():
    fs, x, H = T._models()
    y = np.zeros(8)
    M = lmm_amd.model
    rng = np.random.default_rng(0)
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    sharded = lmm_amd.ILMM(fs, H, shard=(0, 0))(x, 0.1)
    post = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._PostHandle(None, 0, 1)), H)(x, 0.1)
    features = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), lmm_amd.MOInputIsotopicByFeatures(np.arange(4.0), 2), 0.1)
    perpoint = lmm_amd.FiniteGP(lmm_amd.ILMM(fs, H), x, np.full(8, 0.1))
    d2 = lmm_amd.ILMM(fs, H)(lmm_amd.MOInputIsotopicByOutputs(np.zeros((2, 4)), 2), 0.1)

    def with_kernel(k):
        return lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(k)]), H)(x, 0.1)

    se = with_kernel(lmm_amd.SEKernel())
    ksum = with_kernel(lmm_amd.KernelSum(lmm_amd.Matern32Kernel(), lmm_amd.Matern52Kernel()))
    ard = with_kernel(lmm_amd.Matern52Kernel(1.0, np.array([0.5])))
    saved = L.ensure_init
    L.ensure_init = T._no_library
    try:
        for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                             (oilmm, np.zeros((8, 2)), "matrix Y"), (sharded, y, "sharded"), (features, y, "MOInputIsotopicByOutputs"),
                             (perpoint, y, "scalar noise"), (d2, y, "d = 2"), (se, y, "latent 0"), (ksum, y, "latent 0"),
                             (ard, y, "latent 0")):
            with pytest.raises(NotImplementedError, match=what):
                lmm_amd.statespace_rand(rng, fx, yy)
            if what != "matrix Y":                          # the prior sample takes the same checks
                with pytest.raises(NotImplementedError, match=what):
                    lmm_amd.statespace_rand(rng, fx)
        with pytest.raises(ValueError, match="length"):
            lmm_amd.statespace_rand(rng, oilmm, np.zeros(7))
        with pytest.raises(ValueError, match="xs"):
            lmm_amd.statespace_rand(rng, oilmm, xs=np.zeros(3))
        with pytest.raises(ValueError, match="xs"):
            lmm_amd.statespace_rand(rng, oilmm, y, xs=np.zeros((2, 3)))
        with pytest.raises(ValueError, match="N is"):
            lmm_amd.statespace_rand(rng, oilmm, y, N=0)
    finally:
        L.ensure_init = saved


class RecordingRng:
    """Counts every draw; the k-th draw is filled with k + (position in the draw) / 1e6."""

    def __init__(self):
        self.counts = []

    def standard_normal(self, count):
        self.counts.append(int(count))
        return len(self.counts) + np.arange(count) / 1e6


class FakeLib:
    """Stands in for the library: records the call and writes out[q][o][t] = 100 q + 10 o + x_sorted[t]."""

    def __init__(self):
        self.calls = []

    def lmm_oilmm_rand_statespace(self, x, n, y, p, U, S, m, s2, gps, l0, l1, add_noise, nsamples, z, xi, eps, out):
        own = lambda a: None if a is None else np.array(a._owner, copy=True)
        self.calls.append(dict(x=own(x), n=n, y=own(y), p=p, m=m, l0=l0, l1=l1, add_noise=add_noise, nsamples=nsamples, z=own(z), xi=own(xi),
                               eps=own(eps)))
        o = out._owner.reshape(nsamples, p, n)
        o[...] = 100.0 * np.arange(nsamples)[:, None, None] + 10.0 * np.arange(p)[None, :, None] + x._owner[None, None, :]
        return L.LMM_OK


@contextlib.contextmanager
def fake_library():
    saved = (L.ensure_init, L.load)
    fake = FakeLib()
    L.ensure_init = lambda: None
    L.load = lambda: fake
    try:
        yield fake
    finally:
        L.ensure_init, L.load = saved


def _three_kinds(n, p=4):
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern12Kernel()), lmm_amd.GP(lmm_amd.Matern52Kernel()),
                                   lmm_amd.GP(lmm_amd.Matern32Kernel())])
    U = np.linalg.qr(np.random.default_rng(1).standard_normal((p, 3)))[0]
    x = np.random.default_rng(2).permutation(n).astype(np.float64) / 10.0
    return lmm_amd.ILMM(fs, lmm_amd.Orthogonal(U, np.array([1.0, 2.0, 0.5])))(lmm_amd.MOInputIsotopicByOutputs(x, p), 0.1), x


def test_draw_order_counts_and_unpermuting():
    n, p, ns = 6, 4, 3
    fx, x = _three_kinds(n, p)                      # built with the real library (Orthogonal validates its fields)
    with fake_library() as fake_lib:
        _draw_order_checks(fake_lib, fx, x, n, p, ns)


def _draw_order_checks(fake_lib, fx, x, n, p, ns):
    xs = np.array([0.25, -1.0, 0.05])
    y = np.arange(n * p, dtype=np.float64)
    # prior, one sample
    rng = RecordingRng()
    out = lmm_amd.statespace_rand(rng, fx)
    assert rng.counts == [1 * n, 3 * n, 2 * n, n * p]
    c = fake_lib.calls[-1]
    assert c["y"] is None and c["xi"] is None and c["nsamples"] == 1 and c["add_noise"] == 1 and (c["l0"], c["l1"]) == (0, 3)
    assert (c["x"] == np.sort(x)).all()
    assert c["z"].shape == (1, 6 * n) and (np.floor(c["z"][0]) == np.repeat([1, 2, 3], [n, 3 * n, 2 * n])).all()
    assert (np.floor(c["eps"][0]) == 4).all()
    assert out.shape == (n * p,) and (out.reshape(p, n) == 10.0 * np.arange(p)[:, None] + x[None, :]).all()      # the callers' order
    # prior without noise: no noise draw, no eps
    rng = RecordingRng()
    lmm_amd.statespace_rand(rng, fx, add_noise=False)
    assert rng.counts == [n, 3 * n, 2 * n] and fake_lib.calls[-1]["eps"] is None and fake_lib.calls[-1]["add_noise"] == 0
    # posterior at new inputs, N = 2: per sample latents, xi, eps, over n + ns points; only the new rows come back
    rng = RecordingRng()
    na = n + ns
    out = lmm_amd.statespace_rand(rng, fx, y, N=2, xs=xs)
    assert rng.counts == [na, 3 * na, 2 * na, 3 * na, na * p] * 2
    c = fake_lib.calls[-1]
    assert c["n"] == na and c["nsamples"] == 2 and c["xi"].shape == (2, 3 * na) and c["eps"].shape == (2, na * p)
    assert (np.floor(c["xi"][0]) == 4).all() and (np.floor(c["eps"][1]) == 10).all() and (np.floor(c["z"][1][:na]) == 6).all()
    xall = np.concatenate([x, xs])
    perm = np.argsort(xall, kind="stable")
    assert (c["x"] == xall[perm]).all()
    Y = c["y"].reshape(p, na)
    assert (Y[:, np.argsort(perm)][:, :n].reshape(-1) == y).all() and np.isnan(Y[:, np.argsort(perm)][:, n:]).all()
    assert out.shape == (ns * p, 2)
    for q in range(2):
        assert (out[:, q].reshape(p, ns) == 100.0 * q + 10.0 * np.arange(p)[:, None] + xs[None, :]).all()
    # posterior at the training inputs, N = None
    out = lmm_amd.statespace_rand(RecordingRng(), fx, y, add_noise=False)
    assert out.shape == (n * p,) and (out.reshape(p, n) == 10.0 * np.arange(p)[:, None] + x[None, :]).all()


if __name__ == "__main__":
    for k, d in delta_rand().items():
        print(f"delta_rand {k:9s} {d:.2e}")
    for k, d in delta_law().items():
        print(f"delta_law  {k[0]:9s} spacing {k[1]:<6g} {d:.2e}")
    for k, d in delta_post().items():
        print(f"delta_post {k:9s} mean {d[0]:.2e} cov {d[1]:.2e}")
    print(f"DELTA = {delta():.2e}")
