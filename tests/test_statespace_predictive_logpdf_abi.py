"""Host-only checks of the predictive log density of the state-space posterior object (include/lmm_hip.h "state space: predictive
log density"; DESIGN.md 4.18 "Predictive log density from the posterior object"): the NumPy restatement of "a Kalman filter over the
window's backward chain, run from the largest query down to the smallest" agrees with the dense Gaussian, log N(train and held-out)
- log N(train), and, for forecasts, with the filter continued from the last stored state (test_statespace_append_abi.filter_from); the
new entry points are declared, exported and bound with matching arity, and every refusal of the Python mirror comes before any library
call.  tests/test_gpu_statespace_predictive_logpdf.py imports the restatement from here.  No GPU and no lmm_init needed.

delta_predictive(), the largest disagreement with the dense Gaussian relative to max(1, |reference|) over every case of
test_statespace_posterior_abi.cases() and the four query sets of query_sets() (the whole range with one unobserved query; forecasts
with a tie with the last input and a repeated query; one query on a training input; queries in front of all the data), was measured
at 2.0e-13 (Matern12 at n = 1000 with the one query on a training input, where the dense reference is the difference of two values
near 1e3 and the result is of order 1; the SHO latent with Q = 50 at n = 257: 1.4e-13; an earlier scratch restatement on its own
draws gave 9.5e-14).  It is asserted below 1e-12, so that with delta() = 7.6e-15,
delta_posterior() = 1.7e-13, delta_post_rand() and delta_append() = 1.4e-13 the GPU tolerance stays max(1e-10, 100 DELTA) = 1e-10.

`python tests/test_statespace_predictive_logpdf_abi.py` prints the disagreements."""
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
import test_statespace_append_abi as AP
import test_statespace_posterior_abi as PA
from test_statespace_posterior_abi import bwd_element, full_states, interp_state

HEADER = T.HEADER
SYMS = ("lmm_oilmm_statespace_post_logpdf", "lmm_dev_statespace_post_logpdf")
LOG2PI = float(np.log(2.0 * np.pi))


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def window_points(x, q):
    """The window of the sorted queries q: [(input, t)] with t >= 0 a training point and t = -1 - i query i, the training points
    first .. first + count - 1 (first = #{t : x_t <= q_0}, first + count = #{t : x_t <= q_last}) merged with the queries by input, a
    training point before an equal query and equal queries in their order."""
    first, end = int(np.searchsorted(x, q[0], side="right")), int(np.searchsorted(x, q[-1], side="right"))
    pts = [(x[t], 0, t, t) for t in range(first, end)] + [(q[i], 1, i, -1 - i) for i in range(len(q))]
    pts.sort(key=lambda a: a[:3])
    return [(a[0], a[3]) for a in pts]


def filtered_state(model, x, fm, fP, s, t):
    """The filtered state of a window point: the stored one of training point t >= 0; for a query at s the stored one of point k - 1,
    k = #{t : x_t <= s}, predicted over s - x_{k-1}, and the prior when k = 0."""
    if t >= 0:
        return fm[t], fP[t]
    k = int(np.searchsorted(x, s, side="right"))
    if k == 0:
        return np.zeros(model.D), model.Pinf.copy()
    A, Q = model.AQ(s - x[k - 1])
    return A @ fm[k - 1], A @ fP[k - 1] @ A.T + Q


def observe(m, P, w, r):
    """The filter's update through h = e_1' with noise w: (m, P, log-density term); w = +inf: nothing."""
    if not np.isfinite(w):
        return m, P, 0.0
    Sv = P[0, 0] + w
    K = P[:, 0] / Sv
    e = r - m[0]
    return m + K * e, P - np.outer(K, P[0, :]), -0.5 * (LOG2PI + np.log(Sv) + e * e / Sv)


def window_logpdf(model, x, states, xs, ws, rs):
    """log p(rs at xs | the training data) of one zero-mean latent from its stored states (fm, fP, sm, sP) alone.  Given the data
    the states at the window's points are a Markov chain that runs backwards, s_j | s_{j+1}, y ~ N(E_j s_{j+1} + g_j, L_j) with
    (E_j, g_j, L_j) = bwd_element of the FILTERED state of point j; observing rs (noise ws, +inf: unobserved) at the queries of that
    chain is a Kalman filter from the last window point, which starts at its posterior state (interp_state), down to the first with
    the affine transitions m <- E m + g, P <- E P E' + L.  Training points of the window are unobserved steps.  xs in any order."""
    fm, fP, sm, sP = states
    order = np.argsort(np.asarray(xs), kind="stable")
    q, ws, rs = np.asarray(xs)[order], np.asarray(ws)[order], np.asarray(rs)[order]
    pts = window_points(x, q)
    s_last, t_last = pts[-1]
    m, P = interp_state(model, x, fm, fP, sm, sP, s_last)
    m, P, val = observe(m, P, ws[-1 - t_last], rs[-1 - t_last]) if t_last < 0 else (m, P, 0.0)
    for j in range(len(pts) - 2, -1, -1):
        s, t = pts[j]
        E, g, Lm = bwd_element(model, pts[j + 1][0] - s, *filtered_state(model, x, fm, fP, s, t))
        m, P = E @ m + g, E @ P @ E.T + Lm
        if t < 0:
            m, P, term = observe(m, P, ws[-1 - t], rs[-1 - t])
            val += term
    return val


def dense_predictive(model, x, w, r, xs, ws, rs):
    """The same from dense Gaussians: log N over the training and the held-out points minus log N over the training points."""
    xa, wa, ra = np.concatenate([x, xs]), np.concatenate([w, ws]), np.concatenate([r, rs])
    return S.dense_reference(model, xa, wa, ra)[0] - S.dense_reference(model, x, w, r)[0]


def held_out(xs, seed, unobserved=()):
    """Noise and data of the queries xs: w uniform on [0.05, 0.5], r standard normal; the queries listed are unobserved."""
    rng = np.random.default_rng([seed, len(xs)])
    ws, rs = rng.uniform(0.05, 0.5, len(xs)), rng.standard_normal(len(xs))
    for i in unobserved:
        ws[i], rs[i] = np.inf, 0.0
    return ws, rs


def query_sets(x):
    """{label: (xs, ws, rs)}: test_statespace_posterior_abi.queries(x) (the whole range, ties with training inputs, both ends) with
    one unobserved query; forecasts with a tie with the last input and a repeated query; one query equal to a training input;
    queries in front of all the data."""
    n = len(x)
    whole = PA.queries(x)
    fore = np.array([x[-1], x[-1] + 0.3, x[-1] + 0.3, x[-1] + 1e-9, x[-1] + 2.5])
    front = x[0] - np.array([0.7, 1e-9, 0.2, 3.0])
    return {"whole": (whole,) + held_out(whole, 1, unobserved=(7,)),
            "forecasts": (fore,) + held_out(fore, 2),
            "one": (x[[n // 2]],) + held_out(x[[n // 2]], 3),
            "front": (front,) + held_out(front, 4)}


def rel1(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


_DELTA = {}


def deltas():
    """{(label, n, query set): disagreement of the restatement with the dense Gaussian, relative to max(1, |reference|)}."""
    if not _DELTA:
        for key, model, (x, w, r) in PA.cases():
            st = full_states(model, x, w, r)
            for name, (xs, ws, rs) in query_sets(x).items():
                _DELTA[key + (name,)] = rel1(window_logpdf(model, x, st, xs, ws, rs), dense_predictive(model, x, w, r, xs, ws, rs))
    return _DELTA


def delta_predictive():
    """The largest disagreement over every case: with the deltas of the neighbouring files, the DELTA of the GPU tolerances."""
    return max(deltas().values())


def test_restated_window_filter_agrees_with_the_dense_gaussian():
    for key, d in deltas().items():
        print(f"{key[0]} n={key[1]} {key[2]}: {d:.2e}")
    print(f"delta_predictive = {delta_predictive():.2e}")
    assert delta_predictive() < 1e-12, max(deltas().items(), key=lambda kv: kv[1])


def test_forecasts_are_the_filter_continued_from_the_last_state():
    """For queries at or behind the last input the window holds no training point, and the restatement equals
    test_statespace_append_abi.filter_from's value from the last filtered state."""
    for key, model, (x, w, r) in PA.cases():
        st = full_states(model, x, w, r)
        xs, ws, rs = query_sets(x)["forecasts"]
        order = np.argsort(xs, kind="stable")
        ref = AP.filter_from(model, st[0][-1], st[1][-1], x[-1], xs[order], ws[order], rs[order])[0]
        got = window_logpdf(model, x, st, xs, ws, rs)
        assert rel1(got, ref) < 1e-12, (key, got, ref)


def test_unobserved_queries_contribute_nothing_and_order_does_not_matter():
    model, (x, w, r) = [(m, c) for k, m, c in PA.cases() if k == ("matern52", 65)][0]
    st = full_states(model, x, w, r)
    xs, ws, rs = query_sets(x)["whole"]
    ref = window_logpdf(model, x, st, xs, ws, rs)
    keep = np.isfinite(ws)
    assert rel1(window_logpdf(model, x, st, xs[keep], ws[keep], rs[keep]), ref) < 1e-12
    perm = np.random.default_rng(0).permutation(len(xs))
    assert rel1(window_logpdf(model, x, st, xs[perm], ws[perm], rs[perm]), ref) < 1e-12
    assert window_logpdf(model, x, st, xs, np.full(len(xs), np.inf), rs) == 0.0


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_predictive_logpdf_symbols_declared_exported_and_bound():
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
    proto = re.search(r"int\s+lmm_oilmm_statespace_post_logpdf\s*\(([^)]*)\)", src).group(1)
    assert [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")] == ["post", "xs", "ns", "ys", "sigma2", "out"]
    assert re.search(r"int\s+lmm_oilmm_statespace_post_logpdf\s*\(const lmm_ss_post_t\* post", src)      # the handle is const
    proto = re.search(r"int\s+lmm_dev_statespace_post_logpdf\s*\(([^)]*)\)", src).group(1)
    assert [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")] == ["x", "n", "gp", "fstate", "sstate", "xs", "ns", "w", "r",
                                                                             "chunk", "out"]
    assert "state space: predictive log density" in open(HEADER).read()


def test_python_surface():
    assert callable(lmm_amd.StateSpacePosterior.predictive_logpdf)


def _no_library(*a, **k):
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    M = lmm_amd.model
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    fake = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0, [2], 3.0)   # never reaches the library: every call below is refused first
    try:
        with pytest.raises(ValueError, match="xs"):
            fake.predictive_logpdf(np.zeros((2, 2)), np.zeros(8))
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="finite"):
                fake.predictive_logpdf(np.array([4.0, bad, 1.0]), np.zeros(6))
        for ybad in (np.zeros(5), np.zeros((3, 2)), np.zeros(3)):       # ns * p = 6
            with pytest.raises(ValueError, match="ns \\* p"):
                fake.predictive_logpdf(np.array([3.0, 4.0, 5.0]), ybad)
        for s2 in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(ValueError, match="sigma2"):
                fake.predictive_logpdf(np.array([3.0]), np.zeros(2), sigma2=s2)
        assert fake.predictive_logpdf(np.zeros(0), np.zeros(0)) == 0.0  # no queries: no library call
        assert fake.predictive_logpdf(np.zeros(0), np.zeros(0), sigma2=0.3) == 0.0
        assert fake.n == 4 and fake.logpdf == 0.0
        closed = M.StateSpacePosterior(None, 4, 2, 0.0, [2], 3.0)
        with pytest.raises(ValueError, match="closed"):
            closed.predictive_logpdf(np.array([4.0]), np.zeros(2))
    finally:
        fake._ptr = None                                                # nothing to free
        L.ensure_init, L.load = saved


if __name__ == "__main__":
    for key, d in deltas().items():
        print(f"{key[0]:12s} n={key[1]:5d} {key[2]:10s} {d:.2e}")
    print(f"delta_predictive = {delta_predictive():.2e}")
