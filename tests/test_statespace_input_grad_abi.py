"""Host-only checks of the gradients with respect to locations on the state-space path (include/lmm_hip.h,
lmm_oilmm_logpdf_grad_statespace_x and lmm_oilmm_statespace_post_mean_and_var_grad_xs; DESIGN.md 4.18 "Gradients with respect to
locations"): the entry points are declared, exported and bound with matching arity, the refusals of the Python mirror come before any
library call, and the NumPy restatement of the mathematics agrees with the dense Gaussian:
  training inputs  g_t = d lml / d (x_t - x_{t-1}) from the filtered state of point t - 1 and the smoothed state of point t, and
                   d lml / d x_t = g_t - g_{t+1}, against sum_j (alpha alpha' - C^-1)_tj k'(x_t - x_j) with C = K + diag(w);
  queries          d mean / d s = m[1] and d var / d s = 2 P[0][1] of the interpolated state (Matern12: the closed form of its
                   predict-then-smooth step), against the derivative of the dense Gaussian posterior.
The restatement is built from tests/test_statespace_abi.py (its `case`), tests/test_sho_abi.py (the model interface) and
tests/test_statespace_posterior_abi.py (the full-state smoother, the interpolation, its queries);
tests/test_gpu_statespace_input_grad.py imports it from here.  No GPU and no lmm_init needed.

Cases: Matern12 / 32 / 52 and SHO with Q in {0.51, 2, 50} at n in {63, 333}, on the inputs of test_statespace_abi.case (spacings 0.01 - 1
lengthscales, a quarter of the points unobserved; an SHO latent takes those of its D = 2 sibling Matern32, its period the lengthscale)
and on one set per kind whose spacings go down to 1e-4 lengthscales.  Measured here, each the largest error relative to max|reference|:
  delta_input_grad() = 1.65e-13   (the Matern kinds and SHO Q <= 2: 2.1e-14 at the most; the largest is SHO Q = 50 at n = 333);
  delta_query_grad() = 2.74e-13   (the Matern kinds and SHO Q <= 2: 1.2e-14 at the most; the largest is the mean of SHO Q = 50 at
                                   n = 333).
They are asserted under ten times that, INPUT_BOUND and QUERY_BOUND.  The GPU tolerance is max(1e-10, 100 delta).

`python tests/test_statespace_input_grad_abi.py` prints the disagreements."""
import ctypes as C
import inspect
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
SYMS = ("lmm_oilmm_logpdf_grad_statespace_x", "lmm_dev_statespace_grad_x", "lmm_oilmm_statespace_post_mean_and_var_grad_xs")
CPU_N = (63, 333)
INPUT_BOUND = 1.65e-12         # ten times the measured delta_input_grad()
QUERY_BOUND = 2.74e-12         # ten times the measured delta_query_grad()


# ---- the mathematics, restated ------------------------------------------------------------------------------------------------
def drift(model):
    """F of the model's SDE, dA / dt = F A: the companion matrix of a Matern latent, N - a I of an oscillator."""
    return model.N - model.a * np.eye(2) if model.kind == "sho" else model.matern[1]


def spacing_grads(model, x, w, r, states=None):
    """g (n,): g_t = d lml / d (x_t - x_{t-1}) for t >= 1 and g_0 = 0.  With (mp, Pp) the filtered state of point t - 1 pushed through
    A(dt), Q(dt), (ms, Ps) the smoothed state of point t and delta = ms - mp:
    g_t = (Pp^-1 delta)' F mp + tr(Pp^-1 (delta delta' + Ps - Pp) Pp^-1 F (Pp - Pinf))."""
    fm, fP, sm, sP = PA.full_states(model, x, w, r) if states is None else states
    F = drift(model)
    g = np.zeros(len(x))
    for t in range(1, len(x)):
        A, Q = model.AQ(x[t] - x[t - 1])
        mp, Pp = A @ fm[t - 1], A @ fP[t - 1] @ A.T + Q
        Pi = np.linalg.inv(Pp)
        d = sm[t] - mp
        g[t] = (Pi @ d) @ (F @ mp) + np.trace(Pi @ (np.outer(d, d) + sP[t] - Pp) @ Pi @ F @ (Pp - model.Pinf))
    return g


def input_grad(model, x, w, r):
    """d lml / d x_t = g_t - g_{t+1} (g_n = 0), exactly 0 at an unobserved point."""
    g = np.append(spacing_grads(model, x, w, r), 0.0)
    return np.where(np.isfinite(w), g[:-1] - g[1:], 0.0)


def query_grad(model, x, states, xs):
    """(d mean / d s, d var / d s) of the zero-mean first-component marginals at the queries xs from the stored states."""
    fm, fP, sm, sP = states
    n = len(x)
    dmu, dv = np.zeros(len(xs)), np.zeros(len(xs))
    for q, s in enumerate(xs):
        if model.D >= 2:
            m, P = PA.interp_state(model, x, fm, fP, sm, sP, s)
            dmu[q], dv[q] = m[1], 2.0 * P[0, 1]
            continue
        # Matern12: mp = e1 m, Pp = v + e1^2 (P - v); the prediction (mn, Pn) of point k does not depend on s
        k = int(np.searchsorted(x, s, side="right"))
        v, lam = model.Pinf[0, 0], model.matern[0]
        mp, Pp = 0.0, v
        if k > 0:
            e1 = np.exp(-lam * (s - x[k - 1]))
            mp, Pp = e1 * fm[k - 1, 0], v + e1 * e1 * (fP[k - 1, 0, 0] - v)
        dmp, dPp = -lam * mp, -2.0 * lam * (Pp - v)
        if k == n:
            dmu[q], dv[q] = dmp, dPp
            continue
        e2 = np.exp(-lam * (x[k] - s))
        mn, Pn = e2 * mp, v + e2 * e2 * (Pp - v)
        E, dE = Pp * e2 / Pn, (dPp + lam * Pp) * e2 / Pn
        dmu[q], dv[q] = dmp + dE * (sm[k, 0] - mn), dPp + 2.0 * E * dE * (sP[k, 0, 0] - Pn)
    return dmu, dv


# ---- the dense Gaussian they are compared with -------------------------------------------------------------------------------------
def dk(model, tau, at_zero=0.0):
    """k'(tau) of the stationary kernel for signed tau (k is even: sign(tau) dk / d|tau|); at_zero: the sign taken at tau = 0, which
    only Matern12 (a kink) looks at."""
    r = np.abs(tau)
    sg = np.where(tau == 0.0, at_zero, np.sign(tau))
    v = model.v
    if model.kind == "sho":
        w0, a, eta = S.sho_consts(model.ell, model.quality)
        return sg * (-v * w0 * w0 / eta * np.exp(-a * r) * np.sin(eta * r))
    lam = model.matern[0]
    e = np.exp(-lam * r)
    if model.kind == "matern12":
        return sg * (-v * lam * e)
    if model.kind == "matern32":
        return sg * (-v * lam * lam * r * e)
    return sg * (-v * lam * lam * r / 3.0 * (1.0 + lam * r) * e)


def dense_input_grad(model, x, w, r):
    """sum_j (alpha alpha' - C^-1)_tj k'(x_t - x_j) over the observed points, 0 at the others."""
    obs = np.flatnonzero(np.isfinite(w))
    out = np.zeros(len(x))
    if len(obs) == 0:
        return out
    Ci = np.linalg.inv(model.K(x[obs]) + np.diag(w[obs]))
    Ci = 0.5 * (Ci + Ci.T)
    alpha = Ci @ r[obs]
    out[obs] = ((np.outer(alpha, alpha) - Ci) * dk(model, x[obs][:, None] - x[obs][None, :])).sum(axis=1)
    return out


def dense_query_grad(model, x, w, r, xs):
    """d / d s of k(s, X) alpha and of v - k(s, X) C^-1 k(X, s); at a query equal to a training input the derivative from the right
    (the side the search sorts the query to)."""
    obs = np.flatnonzero(np.isfinite(w))
    xs = np.asarray(xs)
    if len(obs) == 0:
        return np.zeros(len(xs)), np.zeros(len(xs))
    Ci = np.linalg.inv(model.K(x[obs]) + np.diag(w[obs]))
    Ci = 0.5 * (Ci + Ci.T)
    Ks = model.K(xs, x[obs])
    dKs = dk(model, xs[:, None] - x[obs][None, :], at_zero=1.0)
    return dKs @ (Ci @ r[obs]), -2.0 * np.einsum("qi,ij,qj->q", dKs, Ci, Ks)


# ---- cases and the measured disagreements ---------------------------------------------------------------------------------------
LABELS = tuple(T.KINDS) + tuple("sho Q=%g" % Q for Q in S.QS)


def model_and_inputs(label, n, fine=False):
    """(model, (x, w, r)): the inputs of test_statespace_abi.case (an SHO latent: those of Matern32); fine: their spacings redrawn
    log-uniformly between 1e-4 and 1 lengthscales."""
    kind = label if label in T.KINDS else "matern32"
    v, ell, x, w, r = T.case(kind, n)
    if fine:
        rng = np.random.default_rng([7, n, LABELS.index(label)])
        x = np.cumsum(ell * 10.0 ** rng.uniform(-4.0, 0.0, n)) - 1.0
    model = PA.model_of(kind, v, ell) if label in T.KINDS else S.sho(v, ell, float(label.split("=")[1]))
    return model, (x, w, r)


def cases():
    for label in LABELS:
        for n in CPU_N:
            yield (label, n, "case"), model_and_inputs(label, n)
        yield (label, CPU_N[-1], "fine"), model_and_inputs(label, CPU_N[-1], fine=True)


def err(got, ref):
    return T.arr_err(got, ref) if np.abs(ref).max() > 0 else float(np.abs(got).max())


_DIN, _DQ = {}, {}


def deltas_input_grad():
    if not _DIN:
        for key, (model, (x, w, r)) in cases():
            got, ref = input_grad(model, x, w, r), dense_input_grad(model, x, w, r)
            _DIN[key] = err(got, ref)
    return _DIN


def deltas_query_grad():
    if not _DQ:
        for key, (model, (x, w, r)) in cases():
            xs = PA.queries(x)
            got = query_grad(model, x, PA.full_states(model, x, w, r), xs)
            ref = dense_query_grad(model, x, w, r, xs)
            _DQ[key] = (err(got[0], ref[0]), err(got[1], ref[1]))
    return _DQ


def delta_input_grad():
    """The largest error of the restated d lml / d x relative to max|dense gradient| over every case."""
    return max(deltas_input_grad().values())


def delta_query_grad():
    """The largest error of the restated query derivatives relative to max|dense derivative| over every case."""
    return max(max(d) for d in deltas_query_grad().values())


def test_restated_input_gradient_agrees_with_dense():
    for key, d in deltas_input_grad().items():
        print(f"{key}: {d:.2e}")
    print(f"delta_input_grad = {delta_input_grad():.2e}")
    assert delta_input_grad() <= INPUT_BOUND, deltas_input_grad()


def test_restated_query_derivatives_agree_with_dense_posterior():
    for key, d in deltas_query_grad().items():
        print(f"{key}: mean {d[0]:.2e} var {d[1]:.2e}")
    print(f"delta_query_grad = {delta_query_grad():.2e}")
    assert delta_query_grad() <= QUERY_BOUND, deltas_query_grad()


def test_gradient_is_exactly_zero_at_unobserved_points():
    for label in LABELS:
        model, (x, w, r) = model_and_inputs(label, 63)
        g = input_grad(model, x, w, r)
        assert (g[~np.isfinite(w)] == 0.0).all() and np.abs(g[np.isfinite(w)]).min() > 0
        # the spacings' derivatives telescope there: g_t = g_{t+1} up to rounding
        gd = np.append(spacing_grads(model, x, w, r), 0.0)
        un = np.flatnonzero(~np.isfinite(w))
        assert np.abs(gd[un] - gd[un + 1]).max() <= 1e-11 * np.abs(gd).max()


@pytest.mark.parametrize("label", LABELS)
def test_restatement_agrees_with_central_differences_of_the_restated_lml(label):
    """Through the restated filter's value at x_t +- h, h = 1e-6 lengthscales.  The difference quotient carries a rounding error of
    about eps |lml| / h (|lml| <= 100 here, h = 7e-7: 3e-8) and a truncation error of about h^2 |lml'''| / 6 <= (h / dt_min)^2 |lml'|
    (the smallest spacing is 0.01 lengthscales: 1e-8 |lml'|).  Relative to max|gradient|, which is above 1 in every case, the two stay
    under 1e-6, the tolerance."""
    model, (x, w, r) = model_and_inputs(label, 63)
    got = input_grad(model, x, w, r)
    h = 1e-6 * model.ell
    fd = np.zeros(len(x))
    for t in range(len(x)):
        xp, xm = x.copy(), x.copy()
        xp[t] += h
        xm[t] -= h
        fd[t] = (S.kalman_filter(model, xp, w, r)[0] - S.kalman_filter(model, xm, w, r)[0]) / (2.0 * h)
    assert np.abs(fd).max() > 1.0
    e = err(got, fd)
    print(f"{label}: {e:.2e}")
    assert e <= 1e-6, (label, e)


@pytest.mark.parametrize("label", LABELS)
def test_query_derivatives_agree_with_central_differences_of_the_interpolation(label):
    """Away from the training inputs (Matern12 has a kink there) and by more than the step: h = 1e-6 lengthscales against values of
    order 1 leaves eps / h = 3e-10 of rounding and (h / dt)^2 <= 1e-8 of truncation; the tolerance is 1e-6."""
    model, (x, w, r) = model_and_inputs(label, 63)
    st = PA.full_states(model, x, w, r)
    rng = np.random.default_rng(5)
    xs = np.concatenate([0.5 * (x[:-1] + x[1:])[::3], [x[0] - 0.3, x[-1] + 0.4], rng.uniform(x[0], x[-1], 10)])
    h = 1e-6 * model.ell
    xs = xs[np.abs(xs[:, None] - x[None, :]).min(axis=1) > 10 * h]
    dmu, dv = query_grad(model, x, st, xs)
    mp, vp = PA.interp_reference(model, x, st, xs + h)
    mm, vm = PA.interp_reference(model, x, st, xs - h)
    e = max(err(dmu, (mp - mm) / (2 * h)), err(dv, (vp - vm) / (2 * h)))
    print(f"{label}: {e:.2e}")
    assert e <= 1e-6, (label, e)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
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

    def order(sym):
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % sym, src).group(1)
        return [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]

    # the `_x` convention: the arguments of the entry point it extends, then the trailing output
    assert order("lmm_oilmm_logpdf_grad_statespace_x") == order("lmm_oilmm_logpdf_grad_statespace") + ["grad_x"]
    assert order("lmm_oilmm_statespace_post_mean_and_var_grad_xs") == ["post", "xs", "ns", "dmean", "dvar", "grad_xs"]
    assert order("lmm_dev_statespace_grad_x") == ["x", "n", "gp", "w", "r", "chunk", "grad_x"]


def test_mirror_signatures():
    sig = inspect.signature(lmm_amd.statespace_logpdf_and_gradient)
    assert list(sig.parameters) == ["fx", "y", "with_regulariser", "inputs"]
    assert sig.parameters["inputs"].default is False and sig.parameters["with_regulariser"].default is True
    sig = inspect.signature(lmm_amd.StateSpacePosterior.mean_and_var_vjp)
    assert list(sig.parameters) == ["self", "xs", "dmean", "dvar"]
    assert sig.parameters["dmean"].default is None and sig.parameters["dvar"].default is None
    assert "inputs" in lmm_amd.statespace_logpdf_and_gradient.__doc__
    assert "no gradient with respect to the inputs" not in lmm_amd.statespace_logpdf_and_gradient.__doc__
    assert "sigma2" in lmm_amd.StateSpacePosterior.mean_and_var_vjp.__doc__


def _no_library(*a, **k):
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    M = lmm_amd.model
    fs, x, H = T._models()
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    saved = L.ensure_init, L.load
    L.ensure_init = L.load = _no_library
    fake = M.StateSpacePosterior(C.c_void_p(1), 4, 2, 0.0)          # never reaches the library: every call below is refused first
    try:
        ones = np.ones(6)
        with pytest.raises(ValueError, match="xs"):
            fake.mean_and_var_vjp(np.zeros((2, 3)), ones)
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="finite"):
                fake.mean_and_var_vjp(np.array([0.0, bad, 1.0]), ones)
        with pytest.raises(ValueError, match="both None"):
            fake.mean_and_var_vjp(np.zeros(3))
        for kw in ({"dmean": np.ones(5)}, {"dvar": np.ones(7)}, {"dmean": ones, "dvar": np.ones(3)}, {"dmean": np.ones((3, 2))}):
            with pytest.raises(ValueError, match="ns \\* p = 6"):
                fake.mean_and_var_vjp(np.zeros(3), **kw)
        out = fake.mean_and_var_vjp(np.zeros(0), np.zeros(0))        # no queries: an empty array, no library call
        assert set(out) == {"x"} and out["x"].shape == (0,)
        closed = M.StateSpacePosterior(None, 4, 2, 0.0)
        with pytest.raises(ValueError, match="closed"):
            closed.mean_and_var_vjp(np.zeros(3), ones)
        # the training-input gradient goes through the checks of statespace_logpdf_and_gradient
        with pytest.raises(NotImplementedError, match="dense-H"):
            lmm_amd.statespace_logpdf_and_gradient(dense, np.zeros(8), inputs=True)
        with pytest.raises(ValueError, match="length"):
            lmm_amd.statespace_logpdf_and_gradient(oilmm, np.zeros(7), inputs=True)
    finally:
        fake._ptr = None                                             # nothing to free
        L.ensure_init, L.load = saved


if __name__ == "__main__":
    for key, d in deltas_input_grad().items():
        print(f"{str(key):32s} input {d:.2e}")
    for key, d in deltas_query_grad().items():
        print(f"{str(key):32s} query mean {d[0]:.2e} var {d[1]:.2e}")
    print(f"delta_input_grad = {delta_input_grad():.2e}   delta_query_grad = {delta_query_grad():.2e}")
