"""Host-only checks of sampling from the state-space posterior object (include/lmm_hip.h "state space: sampling from the posterior
object"; DESIGN.md 4.18 "Sampling from the posterior object"): the NumPy restatement of the backward recursion over the window of the
queries has the mean and the covariance of the dense Gaussian joint posterior, the window positions are a stable merge, the entry
points are declared, exported and bound with matching arity, and every refusal of the Python mirror comes before any library call.
Built on tests/test_statespace_posterior_abi.py (the full states, `cases`, `queries`) and tests/test_sho_abi.py (the models);
tests/test_gpu_statespace_post_rand.py imports the restatement from here.  No GPU and no lmm_init needed.

A sample is mean + M zeta for the window's normals zeta, so its law is N(mean, M M'); both are compared with the dense posterior at the
queries: the mean relative to max|mean|, the covariance as max|M M' - Sigma| / v (v the latent's variance).  delta_post_rand(), the
largest of the two over every case of test_statespace_posterior_abi.cases() and the query sets of `query_sets`, was measured at
5.2e-13 (the mean of the SHO latent with Q = 50 at n = 257; the Matern kinds alone 4.5e-14; the largest law disagreement is 9.5e-15,
SHO with Q = 50 at n = 63).  With queries 1e-9, 1e-12 and 1e-5 lengthscales beside training inputs and on them (tiny_case) the law
disagrees by at most 9.4e-15 with the upper factor (Matern52: 2.4e-15); the lower factor of ss_chol_psd gives 6.1e-5 on the Matern52
case and the same as the upper one on the others.  The GPU tolerance is max(1e-10, 100 delta_post_rand()) = 1e-10.

`python tests/test_statespace_post_rand_abi.py` prints the disagreements."""
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
import test_statespace_posterior_abi as PA

HEADER = T.HEADER
SYMS = ("lmm_statespace_post_window", "lmm_oilmm_statespace_post_rand", "lmm_dev_statespace_post_sample")


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def chol_upper(X):
    """U upper triangular, U U' = X, eliminating component D first; a pivot that is not > 0 gives a zero column."""
    D = X.shape[0]
    U = np.zeros((D, D))
    for j in range(D - 1, -1, -1):
        s = X[j, j] - U[j, j + 1:] @ U[j, j + 1:]
        if not s > 0.0:
            continue
        U[j, j] = np.sqrt(s)
        for i in range(j):
            U[i, j] = (X[i, j] - U[i, j + 1:] @ U[j, j + 1:]) / U[j, j]
    return U


def chol_lower(X):
    """ss_chol_psd: the lower factor, eliminating component 1 first, with the same rule for a pivot that is not > 0."""
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


def window(x, q):
    """(a, b, src) of the sorted queries q: a = #{x_t <= q_0}, b = #{x_t <= q_-1}; src[j] = t >= 0 for training point t, -1 - i for
    query i, by the position formulas (no merge pass): training point t at (t - a) + #{i : q_i < x_t}, query i at
    i + #{t : x_t <= q_i} - a."""
    a, b = int(np.searchsorted(x, q[0], side="right")), int(np.searchsorted(x, q[-1], side="right"))
    W = len(q) + b - a
    src = np.full(W, np.iinfo(np.int64).min)
    for t in range(a, b):
        pos = (t - a) + int(np.searchsorted(q, x[t], side="left"))
        assert src[pos] == np.iinfo(np.int64).min
        src[pos] = t
    for i in range(len(q)):
        pos = i + int(np.searchsorted(x, q[i], side="right")) - a
        assert src[pos] == np.iinfo(np.int64).min
        src[pos] = -1 - i
    return a, b, src


def window_inputs(x, q, src):
    return np.array([x[s] if s >= 0 else q[-1 - s] for s in src])


def filtered_at(model, x, fm, fP, s):
    """The filtered state at the query s: that of training point k - 1, k = #{t : x_t <= s}, predicted over s - x_{k-1}; the prior
    when k = 0."""
    k = int(np.searchsorted(x, s, side="right"))
    if k == 0:
        return np.zeros(model.D), model.Pinf.copy()
    A, Q = model.AQ(s - x[k - 1])
    return A @ fm[k - 1], A @ fP[k - 1] @ A.T + Q


def elements(model, x, states, q, factor=chol_upper):
    """[(E_j, g_j, U_j)] of the window's points and src: s_j = E_j s_{j+1} + g_j + U_j zeta_j, the last one (0, m*, U(P*)) with
    (m*, P*) the posterior state at the largest query."""
    fm, fP, sm, sP = states
    a, b, src = window(x, q)
    xin = window_inputs(x, q, src)
    W = len(src)
    out = []
    for j in range(W):
        m, P = (fm[src[j]], fP[src[j]]) if src[j] >= 0 else filtered_at(model, x, fm, fP, xin[j])
        if j == W - 1:
            ms, Ps = PA.interp_state(model, x, fm, fP, sm, sP, xin[j])
            out.append((np.zeros((model.D, model.D)), ms, factor(Ps)))
        else:
            E, g, Lm = PA.bwd_element(model, xin[j + 1] - xin[j], m, P)
            out.append((E, g, factor(0.5 * (Lm + Lm.T))))
    return out, src


def sample_paths(model, x, states, q, zeta, factor=chol_upper):
    """The sequential recursion on fixed normals: zeta (N, D W), component i of window point j at i W + j -> f (N, ns), zero-mean,
    in the order of the sorted queries q."""
    els, src = elements(model, x, states, q, factor)
    W, D = len(src), model.D
    Z = np.asarray(zeta).reshape(-1, D, W)
    f = np.zeros((Z.shape[0], len(q)))
    for n_ in range(Z.shape[0]):
        s = np.zeros(D)
        for j in range(W - 1, -1, -1):
            E, g, U = els[j]
            s = E @ s + g + U @ Z[n_, :, j]
            if src[j] < 0:
                f[n_, -1 - src[j]] = s[0]
    return f


def sample_map(model, x, states, q, factor=chol_upper):
    """(mean (ns,), M (ns, D W)): a sample at the sorted queries is mean + M zeta."""
    els, src = elements(model, x, states, q, factor)
    W, D = len(src), model.D
    mean, M = np.zeros(len(q)), np.zeros((len(q), D * W))
    s, Sm = np.zeros(D), np.zeros((D, D * W))
    for j in range(W - 1, -1, -1):
        E, g, U = els[j]
        s, Sm = E @ s + g, E @ Sm
        Sm[:, j::W] += U
        if src[j] < 0:
            mean[-1 - src[j]], M[-1 - src[j]] = s[0], Sm[0]
    return mean, M


def dense_joint(model, x, w, r, q):
    """(mean, Sigma) of the zero-mean latent at the queries given the data, from K + diag(w) over the observed points."""
    obs = np.flatnonzero(np.isfinite(w))
    q = np.asarray(q)
    Kss = model.K(q)
    if len(obs) == 0:
        return np.zeros(len(q)), Kss
    import scipy.linalg as sla
    Lc = np.linalg.cholesky(model.K(x[obs]) + np.diag(w[obs]))
    V = sla.solve_triangular(Lc, model.K(x[obs], q), lower=True)
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    return V.T @ u, Kss - V.T @ V


def query_sets(x, ell):
    """{label: sorted queries}: all of test_statespace_posterior_abi.queries(x); 12 behind the data; 12 in front; one point; 9 inside a
    stretch of 6 training points (n >= 8)."""
    rng = np.random.default_rng([7, len(x)])
    sets = {"all": PA.queries(x), "behind": x[-1] + np.cumsum(rng.uniform(0.05, 0.5, 12) * ell),
            "front": x[0] - np.cumsum(rng.uniform(0.05, 0.5, 12) * ell), "one": np.array([0.5 * (x[0] + x[-1]) + 0.013])}
    if len(x) >= 8:
        i0 = len(x) // 3
        sets["inside"] = rng.uniform(x[i0], x[i0 + 5], 9)
    return {k: np.sort(v, kind="stable") for k, v in sets.items()}


def law_errors(model, x, w, r, q, states=None, factor=chol_upper):
    """(mean, law): |mean - dense mean| / max|dense mean| and max|M M' - Sigma| / v at the sorted queries q."""
    states = PA.full_states(model, x, w, r) if states is None else states
    mean, M = sample_map(model, x, states, q, factor)
    dm, dS = dense_joint(model, x, w, r, q)
    em = T.arr_err(mean, dm) if np.abs(dm).max() > 0 else float(np.abs(mean).max())
    return em, float(np.abs(M @ M.T - dS).max() / model.v)


_DELTA = {}


def deltas():
    """{(label, n, set): (mean, law)} over every case of test_statespace_posterior_abi.cases() and every query set."""
    if not _DELTA:
        for key, model, (x, w, r) in PA.cases():
            states = PA.full_states(model, x, w, r)
            for name, q in query_sets(x, model.ell).items():
                _DELTA[key + (name,)] = law_errors(model, x, w, r, q, states)
    return _DELTA


def delta_post_rand():
    """The largest disagreement over every case: the DELTA of the GPU tolerance."""
    return max(max(d) for d in deltas().values())


def tiny_case(model, x):
    """Queries close to training inputs, the normal case of this feature: 400 uniform ones, x[:10] + 1e-9, x[20:30] - 1e-12, x[30:40]
    exactly, x[40:45] + 1e-5 lengthscales."""
    rng = np.random.default_rng([11, len(x)])
    q = np.concatenate([rng.uniform(x[0] - 2.0, x[-1] + 2.0, 400), x[:10] + 1e-9, x[20:30] - 1e-12, x[30:40], x[40:45] + 1e-5 * model.ell])
    return np.sort(q, kind="stable")


def tiny_cases():
    for key, model, data in PA.cases():
        if key[1] in (63, 65):
            yield key, model, data


def test_restated_sampler_has_the_dense_posterior_law():
    for key, d in deltas().items():
        print(f"{key[0]} n={key[1]} {key[2]}: mean {d[0]:.2e} law {d[1]:.2e}")
        assert max(d) <= 1e-12, (key, d)
    print(f"delta_post_rand = {delta_post_rand():.2e}")


def test_tiny_spacings_keep_the_law_with_the_upper_factor():
    seen = 0
    for key, model, (x, w, r) in tiny_cases():
        q = tiny_case(model, x)
        em, el = law_errors(model, x, w, r, q)
        print(f"{key[0]} n={key[1]}: mean {em:.2e} law {el:.2e}")
        assert el <= 1e-12, (key, el)
        seen += 1
    assert seen == len(T.KINDS) + len(S.QS)


def test_upper_factor():
    rng = np.random.default_rng(3)
    for D in (1, 2, 3):
        B = rng.standard_normal((D, D))
        X = B @ B.T
        U = chol_upper(X)
        assert np.abs(np.tril(U, -1)).max() == 0.0 and (np.diag(U) > 0).all()
        assert np.abs(U @ U.T - X).max() <= 1e-14 * np.abs(X).max()
        assert np.abs(chol_upper(np.zeros((D, D)))).max() == 0.0
    # a first entry that is rounding noise (negative here) spoils nothing: the column of component 1 is zero, the rest is exact
    X = np.array([[-1e-20, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 1.0, 3.0]])
    U = chol_upper(X)
    assert (U[:, 0] == 0.0).all() and np.abs((U @ U.T)[1:, 1:] - X[1:, 1:]).max() <= 1e-15


def test_fixed_normals_paths_follow_the_map():
    """sample_paths (the recursion the kernels run) and sample_map (the linear map the law is read from) agree."""
    model, (x, w, r) = PA.model_of("matern52", *T.case("matern52", 65)[:2]), T.case("matern52", 65)[2:]
    st = PA.full_states(model, x, w, r)
    q = query_sets(x, model.ell)["all"]
    mean, M = sample_map(model, x, st, q)
    zeta = np.random.default_rng(0).standard_normal((3, M.shape[1]))
    f = sample_paths(model, x, st, q, zeta)
    assert np.abs(f - (mean + zeta @ M.T)).max() <= 1e-12 * np.abs(f).max()
    assert np.abs(sample_paths(model, x, st, q, np.zeros((1, M.shape[1])))[0] - PA.interp_reference(model, x, st, q)[0]).max() <= 1e-12


def test_window_positions_are_a_stable_merge():
    """The position formulas against a stable host sort of (training points, then queries): ties between a training point and a
    query put the training point first, equal queries keep their order, and the last window point is the largest query."""
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 10.0, 40))
    x[10:13] = x[10]
    x[25] = x[26]
    sets = [np.sort(rng.uniform(-1.0, 11.0, 30)), np.sort(np.concatenate([x[[3, 10, 11, 25, 39]], x[[3, 3, 10]], [x[0], x[-1]]])),
            np.array([x[-1] + 1.0, x[-1] + 2.0]), np.array([x[0] - 2.0, x[0] - 1.0]), np.array([x[17]]), np.array([4.0, 4.0, 4.0]),
            np.array([x[0] - 1.0, x[-1] + 1.0]), np.array([0.5 * (x[5] + x[6])] * 2)]
    for q in sets:
        a, b, src = window(x, q)
        assert a == (x <= q[0]).sum() and b == (x <= q[-1]).sum() and len(src) == len(q) + b - a
        keys = np.concatenate([x[a:b], q])
        ids = np.concatenate([np.arange(a, b), -1 - np.arange(len(q))])
        assert (src == ids[np.argsort(keys, kind="stable")]).all()
        assert src[-1] == -len(q)
        assert (np.diff(window_inputs(x, q, src)) >= 0).all()
    a, b, src = window(x, np.array([x[-1] + 1.0, x[-1] + 2.0]))
    assert (a, b) == (40, 40) and (src == [-1, -2]).all()
    a, b, src = window(x, np.array([x[0] - 2.0, x[0] - 1.0]))
    assert (a, b) == (0, 0)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_post_rand_symbols_declared_exported_and_bound():
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
    order = {s: [re.sub(r".*[\s*]", "", a.strip()) for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % s, src).group(1).split(",")] for s in SYMS}
    assert order["lmm_statespace_post_window"] == ["post", "lo", "hi", "first", "count"]
    assert order["lmm_oilmm_statespace_post_rand"] == ["post", "xs", "ns", "z", "eps", "nsamples", "add_noise", "out"]
    assert order["lmm_dev_statespace_post_sample"] == ["x", "n", "gp", "fstate", "sstate", "xs", "ns", "z", "nsamples", "chunk", "f"]


def _no_library(*a, **k):
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    M = lmm_amd.model
    rng = np.random.default_rng(0)
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    fake = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0, [3])      # never reaches the library: every call below is refused first
    try:
        for call in (lambda xs: fake.rand(rng, xs), lambda xs: fake.rand(rng, xs, 3), fake.window):
            with pytest.raises(ValueError, match="xs"):
                call(np.zeros((2, 3)))
            for bad in (np.nan, np.inf, -np.inf):
                with pytest.raises(ValueError, match="finite"):
                    call(np.array([0.0, bad, 1.0]))
        for N in (0, -1, 1.5):
            with pytest.raises(ValueError, match="N is None or"):
                fake.rand(rng, np.zeros(3), N)
        # no queries: empty results, no library call, no draw
        state = rng.bit_generator.state
        assert fake.rand(rng, np.zeros(0)).shape == (0,)
        assert fake.rand(rng, np.zeros(0), 3).shape == (0, 3)
        assert fake.rand(rng, np.zeros(0), add_noise=False).shape == (0,)
        assert fake.window(np.zeros(0)) == (0, 0)
        assert rng.bit_generator.state == state
        # the four positional arguments still build a handle; it answers queries but cannot size rand's normals
        old = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0)
        assert old.n == 4 and old.p == 2 and old.logpdf == 0.0
        with pytest.raises(ValueError, match="state dimensions"):
            old.rand(rng, np.zeros(3))
        old._ptr = None
        # a closed handle
        closed = M.StateSpacePosterior(None, 4, 2, 0.0, [3])
        closed.close()
        for call in (lambda: closed.rand(rng, np.zeros(3)), lambda: closed.rand(rng, np.zeros(3), 2), lambda: closed.window(np.zeros(3)),
                     lambda: closed.rand(rng, np.zeros(0))):
            with pytest.raises(ValueError, match="closed"):
                call()
    finally:
        fake._ptr = None                                             # nothing to free
        L.ensure_init, L.load = saved


if __name__ == "__main__":
    for key, d in deltas().items():
        print(f"{key[0]:12s} n={key[1]:5d} {key[2]:7s} mean {d[0]:.2e}  law {d[1]:.2e}")
    print(f"delta_post_rand = {delta_post_rand():.2e}")
    for key, model, (x, w, r) in tiny_cases():
        q = tiny_case(model, x)
        up, lo = law_errors(model, x, w, r, q), law_errors(model, x, w, r, q, factor=chol_lower)
        print(f"tiny {key[0]:12s} n={key[1]:3d}  upper: mean {up[0]:.2e} law {up[1]:.2e}   lower: mean {lo[0]:.2e} law {lo[1]:.2e}")
