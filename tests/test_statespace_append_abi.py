"""Host-only checks of appending observations to the state-space posterior object (include/lmm_hip.h "state space: appending
observations"; DESIGN.md 4.18 "Appending observations"): the NumPy restatement of "filter continued from a stored state, then the RTS
recursion over the kept filtered states" agrees with the one-shot restatement (test_statespace_posterior_abi.full_states) and with the
dense Gaussian, the new entry points are declared, exported and bound with matching arity, and every refusal of the Python mirror comes
before any library call.  tests/test_gpu_statespace_append.py imports the restatement from here.  No GPU and no lmm_init needed.

delta_append(), the largest disagreement over every case below (all four models, SHO at test_sho_abi.QS; splits n0 + k of 1 + 1,
40 + 17 and 300 + 40; unobserved points, ties in x and a first new point at spacing 0 from the last old one), was measured at 1.4e-13
(against the one-shot restatement 8.1e-16, stored states component by component: the two run the same recursion; against the dense
Gaussian 1.4e-13, the largest being the SHO latent with Q = 50 at 300 + 40).  With delta() = 7.6e-15, delta_posterior() = 1.7e-13 and
delta_post_rand() the GPU tolerance stays max(1e-10, 100 DELTA) = 1e-10.

`python tests/test_statespace_append_abi.py` prints the disagreements."""
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
SYMS = ("lmm_oilmm_statespace_post_append", "lmm_statespace_post_smooth", "lmm_statespace_post_reserve", "lmm_statespace_post_size",
        "lmm_dev_statespace_filter_from")
SPLITS = ((1, 1), (40, 17), (300, 40))
LOG2PI = float(np.log(2.0 * np.pi))


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def filter_from(model, m0, P0, x0, x, w, r):
    """The sequential filter over the points (x, w, r) whose predecessor is the state (m0, P0) at the input x0 <= x[0], not the
    prior: (log p(r | state), states m (k, D), P (k, D, D))."""
    k, D = len(x), model.D
    m, P = np.array(m0, dtype=float), np.array(P0, dtype=float)
    ms, Ps = np.zeros((k, D)), np.zeros((k, D, D))
    val, xp = 0.0, x0
    for t in range(k):
        A, Q = model.AQ(x[t] - xp)
        m, P = A @ m, A @ P @ A.T + Q
        xp = x[t]
        if np.isfinite(w[t]):
            Sv = P[0, 0] + w[t]
            K = P[:, 0] / Sv
            e = r[t] - m[0]
            m, P = m + K * e, P - np.outer(K, P[0, :])
            val += -0.5 * (LOG2PI + np.log(Sv) + e * e / Sv)
        ms[t], Ps[t] = m, P
    return val, ms, Ps


def smooth_kept(model, x, fm, fP):
    """The full smoothed states from kept filtered states and the inputs alone (test_statespace_posterior_abi.full_states' recursion;
    the data is not an argument)."""
    n = len(x)
    sm, sP = np.zeros_like(fm), np.zeros_like(fP)
    g, Lm = fm[-1].copy(), fP[-1].copy()
    sm[-1], sP[-1] = g, Lm
    for t in range(n - 2, -1, -1):
        E, ge, Le = PA.bwd_element(model, x[t + 1] - x[t], fm[t], fP[t])
        g, Lm = E @ g + ge, E @ Lm @ E.T + Le
        sm[t], sP[t] = g, Lm
    return sm, sP


def appended_states(model, x, w, r, n0):
    """(value of the first n0 points, increment, (fm, fP, sm, sP)): the filter over the first n0 points, continued from its last state
    over the rest, then the smoother over the kept states."""
    v0, _, _, fm0, fP0 = S.kalman_filter(model, x[:n0], w[:n0], r[:n0])
    inc, fm1, fP1 = filter_from(model, fm0[-1], fP0[-1], x[n0 - 1], x[n0:], w[n0:], r[n0:])
    fm, fP = np.concatenate([fm0, fm1]), np.concatenate([fP0, fP1])
    return v0, inc, (fm, fP) + smooth_kept(model, x, fm, fP)


def state_err(got, ref):
    """Stored states compared component by component: the largest |got - ref| / max |ref| over the components of an (n, D) or
    (n, D, D) array (a component that is zero throughout must be reproduced to 1e-300)."""
    g, f = got.reshape(len(got), -1), ref.reshape(len(ref), -1)
    return float(max(np.abs(g[:, c] - f[:, c]).max() / max(np.abs(f[:, c]).max(), 1e-300) for c in range(g.shape[1])))


def append_case(model_key, n0, k):
    """(model, x, w, r) of n0 + k points: the cases of the one-shot tests, with the first new point unobserved and at spacing 0 from
    the last old one for the 40 + 17 split (so every split but one starts on an observed point), and runs of equal inputs on either
    side of the join from 40 points on."""
    n = n0 + k
    if model_key[0] == "sho":
        v, P, x, w, r = S.case(model_key[1], n)
        model = S.sho(v, P, model_key[1])
    else:
        v, ell, x, w, r = T.case(model_key[0], n)
        model = PA.model_of(model_key[0], v, ell)
    x, w, r = x.copy(), w.copy(), r.copy()
    if n >= 40:
        x[5:8] = x[5]
        x[n0 + 3:n0 + 6] = x[n0 + 3]
        w[n0 - 1] = 0.2                        # the state the append starts from has seen its own observation
    if n0 == 40:
        x[n0] = x[n0 - 1]                      # spacing 0 across the join
        w[n0] = np.inf                         # and the first new point unobserved
    if n0 == 300:
        x[n0] = x[n0 - 1]                      # spacing 0 across the join, observed on both sides
        w[n0] = 0.1
    return model, x, w, r


MODEL_KEYS = tuple((kind, None) for kind in T.KINDS) + tuple(("sho", Q) for Q in S.QS)
_DELTA = {}


def deltas():
    """{(model key, n0, k): (against the one-shot restatement, against the dense Gaussian)}."""
    if not _DELTA:
        for key in MODEL_KEYS:
            for n0, k in SPLITS:
                model, x, w, r = append_case(key, n0, k)
                v0, inc, st = appended_states(model, x, w, r, n0)
                ref = PA.full_states(model, x, w, r)
                vall = S.kalman_filter(model, x, w, r)[0]
                one = max([state_err(a, b) for a, b in zip(st, ref)] + [T.rel(v0 + inc, vall)])
                xs = PA.queries(x)
                gm, gv = PA.interp_reference(model, x, st, xs)
                dm, dv = PA.dense_posterior(model, x, w, r, xs)
                dense = max(T.arr_err(gm, dm) if np.abs(dm).max() > 0 else float(np.abs(gm).max()), T.arr_err(gv, dv),
                            T.rel(v0 + inc, S.dense_reference(model, x, w, r)[0]))
                _DELTA[(key, n0, k)] = (one, dense)
    return _DELTA


def delta_append():
    """The largest disagreement over every case: with delta(), delta_posterior() and delta_post_rand(), the DELTA of the GPU tolerances."""
    return max(max(d) for d in deltas().values())


def test_restated_append_agrees_with_one_shot_and_dense():
    for key, d in deltas().items():
        print(f"{key}: one-shot {d[0]:.2e} dense {d[1]:.2e}")
        assert max(d) <= 1e-12, (key, d)
    print(f"delta_append = {delta_append():.2e}")


def test_zero_spacing_is_exact_and_unobserved_points_predict():
    """A new point at spacing 0 that is unobserved keeps the stored state bit for bit and adds nothing to the value."""
    model, x, w, r = append_case(("matern52", None), 40, 17)
    _, _, _, fm0, fP0 = S.kalman_filter(model, x[:40], w[:40], r[:40])
    inc, fm, fP = filter_from(model, fm0[-1], fP0[-1], x[39], x[40:41], w[40:41], r[40:41])
    assert inc == 0.0 and np.array_equal(fm[0], fm0[-1]) and np.array_equal(fP[0], fP0[-1])


def test_increments_add_up():
    """Appending in several pieces gives the states of appending at once (the same sequential recursion) and the value of all data."""
    model, x, w, r = append_case(("sho", 2.0), 40, 17)
    v0, inc, st = appended_states(model, x, w, r, 40)
    _, _, _, fm, fP = S.kalman_filter(model, x[:40], w[:40], r[:40])
    tot = v0
    for a, b in ((40, 41), (41, 50), (50, 57)):
        i, m1, P1 = filter_from(model, fm[-1], fP[-1], x[a - 1], x[a:b], w[a:b], r[a:b])
        fm, fP, tot = np.concatenate([fm, m1]), np.concatenate([fP, P1]), tot + i
    assert np.array_equal(fm, st[0]) and np.array_equal(fP, st[1])
    assert abs(tot - (v0 + inc)) <= 1e-12 * abs(v0 + inc)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_append_symbols_declared_exported_and_bound():
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
    proto = re.search(r"int\s+lmm_oilmm_statespace_post_append\s*\(([^)]*)\)", src).group(1)
    assert [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")] == ["post", "x_new", "k", "y_new", "out_increment"]
    # the query entry points keep their const handle
    for s in ("lmm_oilmm_statespace_post_mean_and_var", "lmm_oilmm_statespace_post_mean_and_var_grad_xs", "lmm_statespace_post_window",
              "lmm_oilmm_statespace_post_rand"):
        assert re.search(r"int\s+%s\s*\(const lmm_ss_post_t\* post" % s, src), s


def test_python_surface():
    P = lmm_amd.StateSpacePosterior
    for name in ("append", "smooth", "reserve"):
        assert callable(getattr(P, name))
    assert isinstance(P.smoothed, property) and P.smoothed.fset is None


def _no_library(*a, **k):
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    M = lmm_amd.model
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    fake = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0, [2], 3.0)   # never reaches the library: every call below is refused first
    try:
        with pytest.raises(ValueError, match="x_new"):
            fake.append(np.zeros((2, 2)), np.zeros(8))
        for ybad in (np.zeros(5), np.zeros((3, 2)), np.zeros(3)):       # k * p = 6
            with pytest.raises(ValueError, match="k \\* p"):
                fake.append(np.array([3.0, 4.0, 5.0]), ybad)
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="finite"):
                fake.append(np.array([4.0, bad]), np.zeros(4))
        with pytest.raises(ValueError, match="at or behind the last input"):
            fake.append(np.array([5.0, 3.0 - 1e-12]), np.zeros(4))      # any order: the smallest decides
        assert fake.append(np.zeros(0), np.zeros(0)) == 0.0             # nothing to append: no library call
        assert fake.n == 4 and fake.logpdf == 0.0
        with pytest.raises(ValueError, match="n_total"):
            fake.reserve(-1)
        with pytest.raises(ValueError, match="n_total"):
            fake.reserve(2 ** 31)
        old = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0)           # a handle built without its last input
        with pytest.raises(ValueError, match="last input"):
            old.append(np.array([9.0]), np.zeros(2))
        old._ptr = None
        closed = M.StateSpacePosterior(None, 4, 2, 0.0, [2], 3.0)
        for call in (lambda: closed.append(np.array([4.0]), np.zeros(2)), closed.smooth, lambda: closed.reserve(10),
                     lambda: closed.smoothed):
            with pytest.raises(ValueError, match="closed"):
                call()
    finally:
        fake._ptr = None                                                # nothing to free
        L.ensure_init, L.load = saved


if __name__ == "__main__":
    for key, d in deltas().items():
        print(f"{str(key):32s} one-shot {d[0]:.2e}  dense {d[1]:.2e}")
    print(f"delta_append = {delta_append():.2e}   one-shot {max(d[0] for d in deltas().values()):.2e}   "
          f"dense {max(d[1] for d in deltas().values()):.2e}")
