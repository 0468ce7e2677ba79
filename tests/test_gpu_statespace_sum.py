"""-m gpu: sum latents on the state-space path (include/lmm_hip.h "State space: sum latents"; DESIGN.md 4.18 "Sum latents"): the filter
and smoother building blocks for the seven pair models, the OILMM entry points on a model that mixes sum and plain latents, the
gradient, sampling, the posterior handle and the refusals.  The Python state-space functions serve Matern-only sums; a sum with an
SHO term is reached through the C ABI (the building blocks, and test_sho_sums_through_the_c_abi end to end).  Every reference is a dense Gaussian built in NumPy
(tests/test_statespace_sum_abi.py: K = K_a + K_b from the closed forms), never the code under test; the Matern-only problem is compared
with the library's own dense path as well.

Tolerance: 1e-10 of max|reference| per array, and relative for a scalar -- the project's figure, which holds where the matching
disagreement of the NumPy restatement with the dense Gaussian is <= 1e-11 (else 100 times that disagreement):
test_statespace_sum_abi.delta_sum() = 2.4e-13, delta_sum_grad() = 2.7e-12, delta_sum_rand() = 1.2e-15, so it is 1e-10 throughout."""
import ctypes as C

import numpy as np
import pytest

import test_statespace_sum_abi as T

pytestmark = pytest.mark.gpu

BLOCK_N = (1, 2, 17, 257, 2100)
# every quality of the restatement is met once
PAIR_Q = {("matern12", "sho"): 0.51, ("matern32", "sho"): 2.0, ("sho", "sho"): 50.0}
V0, S0 = 1.25, 0.8      # the sum's own variance and lengthscale, which fold into the terms


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def rule(delta):
    return 1e-10 if delta <= 1e-11 else 100.0 * delta


@pytest.fixture(scope="module")
def tol():
    return rule(T.delta_sum())


@pytest.fixture(scope="module")
def tol_grad():
    return rule(T.delta_sum_grad())


@pytest.fixture(scope="module")
def tol_rand():
    return rule(T.delta_sum_rand())


def close(got, ref, tol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"error {err / max(scale, 1e-300):.2e} of max|reference| (tolerance {tol:.0e})")
    assert err <= tol * scale, (err, scale)


def close_value(got, ref, tol):
    print(f"value {got!r} reference {ref!r} relative error {abs(got - ref) / max(abs(ref), 1e-300):.2e} (tolerance {tol:.0e})")
    assert np.isfinite(got) and abs(got - ref) <= tol * abs(ref), (got, ref)


def close_difference(got, a, b, tol):
    """got against a - b, two dense log densities: the reference carries the rounding of both, so the tolerance is of the larger."""
    print(f"value {got!r} reference {a - b!r} error {abs(got - (a - b)):.2e} (tolerance {tol:.0e} of {max(abs(a), abs(b)):.3g})")
    assert np.isfinite(got) and abs(got - (a - b)) <= tol * max(abs(a), abs(b)), (got, a, b)


def term_desc(t, v0=1.0, s0=1.0):
    """The descriptor of a term whose EFFECTIVE parameters are t = (kind, v, ell[, quality]) inside a sum scaled by (v0, s0)."""
    d = {"kind": t[0], "variance": t[1] / v0, "lengthscale": t[2] / s0}
    if t[0] == "sho":
        d["quality"] = t[3]
    return d


def sum_desc(terms, swap=False, mean=0.0):
    ts = [term_desc(t, V0, S0) for t in (terms[::-1] if swap else terms)]
    return {"kind": "sum", "variance": V0, "lengthscale": S0, "mean": mean, "terms": ts}


# ---------------------------------------------------------------------------------------------------
# 1. the building blocks
# ---------------------------------------------------------------------------------------------------
_REF = {}


def block_reference(pair, n):
    if (pair, n) not in _REF:
        terms, x, w, r = T.case(pair, n, PAIR_Q.get(pair, 2.0))
        _REF[(pair, n)] = ((terms, x, w, r), T.dense_reference(terms, x, w, r))
    return _REF[(pair, n)]


def gpu_blocks(lmm, desc, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, wd, rd = dev(x), dev(w), dev(r)
    out = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]
    lml = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gp = L.statespace_gps_array([desc])
    lib = lmm.load()
    L.check(lib.lmm_dev_statespace_filter(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[0].data_ptr(),
                                          out[1].data_ptr(), lml.data_ptr()))
    L.check(lib.lmm_dev_statespace_smooth(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[2].data_ptr(),
                                          out[3].data_ptr()))
    return (float(lml.cpu()[0]),) + tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("pair", T.PAIRS, ids=["+".join(p) for p in T.PAIRS])
def test_filter_and_smoother_blocks(lmm, tol, pair, n):
    """chunk 1, 16 and n against the dense Gaussian; n = 2100 with chunk 16 is 132 aggregates, two workgroups of the scan at width 128.
    The mean of the descriptor (0.7) is not read.  The terms go in in the other order at n = 17: the library has one order."""
    (terms, x, w, r), ref = block_reference(pair, n)
    desc = sum_desc(terms, swap=n == 17, mean=0.7)
    for chunk in (1, 16, n):
        got = gpu_blocks(lmm, desc, x, w, r, chunk)
        if np.isfinite(w).any():
            close_value(got[0], ref[0], tol)
        else:
            assert got[0] == 0.0
        for a, b in zip(got[1:], ref[1:]):
            close(a, b, tol)
    if n == 257:
        one, two = gpu_blocks(lmm, desc, x, w, r, 16), gpu_blocks(lmm, desc, x, w, r, 16)
        assert one[0] == two[0] and all((a == b).all() for a, b in zip(one[1:], two[1:]))      # bitwise


@pytest.mark.parametrize("pair,swap", [(("matern12", "matern52"), True), (("matern32", "sho"), False), (("sho", "sho"), True)],
                         ids=["matern52+matern12", "matern32+sho", "sho+sho"])
def test_gradient_block_of_a_sum(lmm, tol_grad, pair, swap):
    """lmm_dev_statespace_grad_sum: six slots, the seeds of the first term in the library's order (whatever order the caller's terms
    come in), then the second's, zeros behind; against the dense analytic gradient, term by term.  n = 257 at chunk 16: 17 aggregates
    per seed.  The two- and three-value blocks refuse a sum latent, naming it."""
    import torch
    from lmm_amd import _lib as L
    (terms, x, w, r), ref = block_reference(pair, 257)
    n = len(x)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, wd, rd = dev(x), dev(w), dev(r)
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")
    gr, gw, lml, gth = nan(n), nan(n), nan(1), nan(6)
    torch.cuda.synchronize()
    gp = L.statespace_gps_array([sum_desc(terms, swap=swap, mean=0.7)])
    lib = lmm.load()
    L.check(lib.lmm_dev_statespace_grad_sum(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), 16, lml.data_ptr(), gr.data_ptr(),
                                            gw.data_ptr(), gth.data_ptr()))
    order = terms[::-1] if swap and pair[0] == pair[1] else terms      # two terms of one kind keep the caller's order
    got, want = gth.cpu().numpy(), T.dense_gradient(order, x, w, r)
    assert float(lml.cpu()[0]) == gpu_blocks(lmm, sum_desc(terms, swap=swap), x, w, r, 16)[0]      # the filter's value, bitwise
    na = len(T.term_params(order[0]))
    close(got[:na], want[:na], tol_grad); close(got[na:len(want)], want[na:], tol_grad)
    assert (got[len(want):] == 0.0).all()
    lat, info = C.c_int(), C.c_int()
    for fn in (lib.lmm_dev_statespace_grad, lib.lmm_dev_statespace_grad_sho):
        assert fn(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), 16, lml.data_ptr(), gr.data_ptr(), gw.data_ptr(),
                  gth.data_ptr()) == L.LMM_ERR_UNSUPPORTED
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        assert lat.value == 0 and b"latent 0" in lib.lmm_last_error_string()


# ---------------------------------------------------------------------------------------------------
# the OILMM problem: p = 5, m = 3, a sum beside plain latents (mixed launches)
# ---------------------------------------------------------------------------------------------------
P_OUT, S2 = 5, 0.15
LATS = [{"mean": 0.3, "v0": 1.2, "s0": 0.9, "terms": [("matern32", 0.8, 1.1), ("matern32", 0.5, 1.9)]},
        {"mean": 0.0, "v0": 1.0, "s0": 1.0, "terms": [("matern52", 1.4, 0.6)]},
        {"mean": -0.2, "v0": 0.7, "s0": 1.3, "terms": [("matern12", 1.1, 0.5), ("matern32", 0.6, 2.0)]}]
LATS_MATERN = LATS      # Matern-only sums: the dense verbs serve the same gps
# the first latent a Matern32 + SHO sum: the C ABI serves it (test_sho_sums_through_the_c_abi)
LATS_SHO = [dict(LATS[0], terms=[("matern32", 0.8, 1.1), ("sho", 0.5, 1.9, 3.0)]), LATS[1], LATS[2]]


def kernel_of(lmm, t):
    K = {"matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    return lmm.SHOKernel(t[1], t[2], t[3]) if t[0] == "sho" else K[t[0]](t[1], t[2])


def model(lmm, U, S, lats):
    gps = []
    for lat in lats:
        ks = [kernel_of(lmm, t) for t in lat["terms"]]
        k = ks[0] if len(ks) == 1 else lmm.KernelSum(*ks, variance=lat["v0"], lengthscale=lat["s0"])
        gps.append(lmm.GP(lat["mean"], k))
    return lmm.ILMM(lmm.independent_mogp(gps), lmm.Orthogonal(U, S))


_PROBLEM = {}


def problem(n, seed=0):
    """Unsorted inputs with one duplicate, NaN in y with every row observing at least m outputs, and some all-NaN rows."""
    if (n, seed) not in _PROBLEM:
        rng = np.random.default_rng([seed, n])
        m = 3
        x = rng.uniform(0.0, 6.0, n)
        if n > 3:
            x[3] = x[1]
        U, S = np.linalg.qr(rng.standard_normal((P_OUT, m)))[0], rng.uniform(0.5, 2.0, m)
        Y = rng.standard_normal((P_OUT, n))
        for t in range(n):
            u = rng.random()
            if u < 0.3:
                Y[rng.choice(P_OUT, rng.integers(1, P_OUT - m + 1), replace=False), t] = np.nan
            elif u < 0.4:
                Y[:, t] = np.nan
        if n > 2:                                  # at least one NaN in an observed row, whatever the draw
            Y[:, 2] = rng.standard_normal(P_OUT)
            Y[0, 2] = np.nan
        assert all(k == 0 or k >= m for k in (~np.isnan(Y)).sum(axis=0))
        _PROBLEM[(n, seed)] = (x, U, S, Y)
    return _PROBLEM[(n, seed)]


def dense(lats, x, U, S, Y, **kw):
    """T.oilmm_dense over the SORTED points (the reference takes any order: it is dense); results in the callers' order."""
    return T.oilmm_dense(lats, U, S, x, S2, Y, **kw)


# ---------------------------------------------------------------------------------------------------
# 2. end to end
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 40, 300])
def test_logpdf_and_mean_and_var_against_dense(lmm, tol, n):
    x, U, S, Y = problem(n)
    y = Y.reshape(-1)
    xs = np.concatenate([[x.min() - 0.7, x.max() + 0.9, x[0]], np.linspace(x.min(), x.max(), 7)[1:-1] + 0.013])
    fx = model(lmm, U, S, LATS)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    for with_reg in (True, False):
        close_value(lmm.statespace_logpdf(fx, y, with_reg), dense(LATS, x, U, S, Y, with_reg=with_reg)["value"], tol)
    for add_noise in (True, False):
        ref = dense(LATS, x, U, S, Y, xs=xs, add_noise=add_noise)
        gm, gv = lmm.statespace_mean_and_var(fx, y, add_noise, xs=xs)
        close(gm, ref["mean"].reshape(-1), tol); close(gv, ref["var"].reshape(-1), tol)
        ref = dense(LATS, x, U, S, Y, xs=x, add_noise=add_noise)
        gm, gv = lmm.statespace_mean_and_var(fx, y, add_noise)
        close(gm, ref["mean"].reshape(-1), tol); close(gv, ref["var"].reshape(-1), tol)


def test_matern_only_sums_against_the_dense_path_of_the_library(lmm, tol):
    """The same gps run on the dense verbs: logpdf, and posterior -> mean_and_var at the training and at new inputs."""
    x, U, S, Y = problem(300)
    y = Y.reshape(-1)
    f = model(lmm, U, S, LATS_MATERN)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    fx = f(xin, S2)
    for with_reg in (True, False):
        got = lmm.statespace_logpdf(fx, y, with_reg)
        close_value(got, dense(LATS_MATERN, x, U, S, Y, with_reg=with_reg)["value"], tol)
        close_value(got, lmm.logpdf(fx, y, with_reg), tol)
    xs = np.linspace(x.min() - 0.5, x.max() + 0.5, 9)
    post = lmm.posterior(fx, y)
    rm, rv = lmm.mean_and_var(post(xin, S2))
    gm, gv = lmm.statespace_mean_and_var(fx, y)
    close(gm, rm, tol); close(gv, rv, tol)
    rm, rv = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2))
    gm, gv = lmm.statespace_mean_and_var(fx, y, xs=xs)
    close(gm, rm, tol); close(gv, rv, tol)


# ---------------------------------------------------------------------------------------------------
# 3. the gradient
# ---------------------------------------------------------------------------------------------------
def check_gradient(got, ref, tol):
    """Every key.  A latent's own entries (variance, lengthscale, mean, quality) are one group and each term's entries another: the
    tolerance is of the largest reference entry of the group, so a term's small entry is not measured against another term's."""
    close_value(got["value"], ref["value"], tol)
    close(got["y"], ref["y"], tol)
    close_value(got["sigma2"], ref["sigma2"], tol)
    assert len(got["gps"]) == len(ref["gps"])
    for a, b in zip(got["gps"], ref["gps"]):
        assert set(a) == set(b), (set(a), set(b))
        keys = sorted(k for k in b if k != "terms")
        close(np.array([a[k] for k in keys]), np.array([b[k] for k in keys]), tol)
        if "terms" in b:
            assert len(a["terms"]) == len(b["terms"])
            for ta, tb in zip(a["terms"], b["terms"]):
                assert set(ta) == set(tb), (set(ta), set(tb))
                close(np.array([ta[k] for k in sorted(tb)]), np.array([tb[k] for k in sorted(tb)]), tol)


@pytest.mark.parametrize("n", [40, 1100])
def test_gradient_against_the_dense_analytic_gradient(lmm, tol_grad, n):
    """Every key, per-term entries included; n = 1100: 69 aggregates per seed at chunk 16, two workgroups of the dual
    scan at width 64."""
    x, U, S, Y = problem(n)
    y = Y.reshape(-1)
    fx = model(lmm, U, S, LATS)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    for with_reg in ((True, False) if n == 40 else (True,)):
        got = lmm.statespace_logpdf_and_gradient(fx, y, with_reg)
        assert set(got) == {"value", "y", "sigma2", "gps"}
        with pytest.raises(NotImplementedError):
            got["S"]
        assert got["value"] == lmm.statespace_logpdf(fx, y, with_reg)                        # bitwise
        assert (got["y"][np.isnan(y)] == 0.0).all()
        check_gradient(got, dense(LATS, x, U, S, Y, with_reg=with_reg, grad=True), tol_grad)


def test_gradient_of_matern_only_sums_against_the_dense_path_of_the_library(lmm, tol_grad):
    x, U, S, Y = problem(40)
    y = Y.reshape(-1)
    fx = model(lmm, U, S, LATS_MATERN)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    got, ref = lmm.statespace_logpdf_and_gradient(fx, y), lmm.logpdf_and_gradient(fx, y)
    check_gradient(got, {k: ref[k] for k in ("value", "y", "sigma2", "gps")}, tol_grad)
    check_gradient(got, dense(LATS_MATERN, x, U, S, Y, grad=True), tol_grad)
    # complete data: "S" and "U" as well
    Yc = np.where(np.isnan(Y), 0.25, Y)
    got, ref = lmm.statespace_logpdf_and_gradient(fx, Yc.reshape(-1)), lmm.logpdf_and_gradient(fx, Yc.reshape(-1))
    check_gradient(got, {k: ref[k] for k in ("value", "y", "sigma2", "gps")}, tol_grad)
    close(got["S"], ref["S"], tol_grad); close(got["U"], ref["U"], tol_grad)


def abi_descs(lats):
    out = []
    for lat in lats:
        if len(lat["terms"]) == 1:
            out.append(dict(term_desc(lat["terms"][0]), mean=lat["mean"]))
        else:
            out.append({"kind": "sum", "variance": lat["v0"], "lengthscale": lat["s0"], "mean": lat["mean"],
                        "terms": [term_desc(t) for t in lat["terms"]]})
    return out


@pytest.mark.parametrize("n", [40, 1100])
def test_sho_sums_through_the_c_abi(lmm, tol, tol_grad, n):
    """[Matern32 + SHO, Matern52, Matern12 + Matern32] end to end through the entry points themselves (the tag of the SHO sum from
    lmm_kernel_sum_create_statespace): value, marginals, and every key of the gradient with the SHO term's "quality", against the
    dense Gaussian.  n = 1100: the dual scan of the five-seed D = 4 model crosses a workgroup at width 64."""
    from lmm_amd import _lib as L
    x, U, S, Y = problem(n)
    order = np.argsort(x, kind="stable")
    x, Y = np.ascontiguousarray(x[order]), np.ascontiguousarray(Y[:, order])
    y = Y.reshape(-1)
    lib, ga = lmm.load(), L.statespace_gps_array(abi_descs(LATS_SHO))
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    ref = dense(LATS_SHO, x, U, S, Y, xs=x, grad=True)
    out = C.c_double()
    L.check(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, ga, 0, 3, 1, C.byref(out)))
    close_value(out.value, ref["value"], tol)
    mo, vo = np.empty(n * P_OUT), np.empty(n * P_OUT)
    L.check(lib.lmm_oilmm_mean_and_var_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, ga, 0, 3, 1,
                                                  L.Arr(mo, True).ptr, L.Arr(vo, True).ptr))
    close(mo, ref["mean"].reshape(-1), tol); close(vo, ref["var"].reshape(-1), tol)
    gg = (L.GpGradT * 3)()
    gy, val, gs2 = np.empty(n * P_OUT), C.c_double(), C.c_double()
    L.check(lib.lmm_oilmm_logpdf_grad_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, ga, 0, 3, 1, C.byref(val),
                                                 L.Arr(gy, True).ptr, C.byref(gs2), None, None, gg))
    assert val.value == out.value                                                            # bitwise
    got = {"value": val.value, "y": gy, "sigma2": gs2.value, "gps": lmm.model._gps_grads(gg, ga, 3, 1)}
    assert "quality" in got["gps"][0]["terms"][1]
    check_gradient(got, ref, tol_grad)


# ---------------------------------------------------------------------------------------------------
# 4. sampling
# ---------------------------------------------------------------------------------------------------
class UnitNormals:
    """A generator whose q-th sample of a call is the q-th unit vector of the call's normals: the samples are then the columns of the
    linear map from the normals to the result (plus its constant part, which an all-zero sample gives)."""

    def __init__(self, per_sample):
        self.per_sample, self.drawn = per_sample, 0

    def standard_normal(self, count):
        q, off = divmod(self.drawn, self.per_sample)
        self.drawn += count
        out = np.zeros(count)
        if off <= q < off + count:
            out[q - off] = 1.0
        return out


def latent_cov(lats, U, S, x, post_of=None):
    """Cov of the by-outputs vector H f(x) (+ nothing): sum_l H_l H_l' (x) K_l, with K_l the prior covariance or (post_of = (Y,)) the
    posterior one given the pseudo-observations of the front end."""
    H = U * np.sqrt(S)[None, :]
    n = len(x)
    cov = np.zeros((P_OUT * n, P_OUT * n))
    mean = np.zeros(P_OUT * n)
    if post_of is not None:
        r, w, _, _ = T.oilmm_front(U, S, S2, post_of, np.array([lat["mean"] for lat in lats]))
    for l, lat in enumerate(lats):
        K = T.latent_K(lat, x)
        ml = np.full(n, lat["mean"])
        if post_of is not None:
            obs = np.flatnonzero(np.isfinite(w[l]))
            Ci = np.linalg.inv(K[np.ix_(obs, obs)] + np.diag(w[l, obs]))
            ml = ml + K[:, obs] @ Ci @ r[l, obs]
            K = K - K[:, obs] @ Ci @ K[obs, :]
        cov += np.kron(np.outer(H[:, l], H[:, l]), K)
        mean += np.kron(H[:, l], ml)
    return mean, cov


def has_sho(lats):
    return any(t[0] == "sho" for lat in lats for t in lat["terms"])


def sorted_problem(x, Y):
    order = np.argsort(x, kind="stable")
    return np.ascontiguousarray(x[order]), np.ascontiguousarray(Y[:, order])


def posterior_of(lmm, lats, x, U, S, Y):
    """The handle of (lats, x, Y): statespace_posterior, or for a sum with an SHO term, which the Python functions refuse, the
    same object around lmm_oilmm_statespace_posterior_create on the sorted points."""
    from lmm_amd import _lib as L
    if not has_sho(lats):
        return lmm.statespace_posterior(model(lmm, U, S, lats)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), Y.reshape(-1))
    xa, Ya = sorted_problem(x, Y)
    ga = L.statespace_gps_array(abi_descs(lats))
    ptr, out = C.c_void_p(), C.c_double()
    L.check(lmm.load().lmm_oilmm_statespace_posterior_create(L.Arr(xa).ptr, len(xa), L.Arr(Ya.reshape(-1)).ptr, P_OUT,
                                                             L.Arr(L.colmajor(U)).ptr, L.Arr(S).ptr, 3, S2, ga, 0, 3,
                                                             C.byref(ptr), C.byref(out)))
    dims = [sum(T.TERM_DIM[t[0]] for t in lat["terms"]) for lat in lats]
    return lmm.model.StateSpacePosterior(ptr, len(xa), P_OUT, out.value, dims, float(xa[-1]), [l for l, lat in enumerate(lats) if len(lat["terms"]) > 1])


def rand_map(lmm, lats, x, U, S, Y, per):
    """(n p, per + 1): the samples of per unit normals and one of zeros, in the callers' order of points."""
    from lmm_amd import _lib as L
    n = len(x)
    if not has_sho(lats):
        fx = model(lmm, U, S, lats)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
        return lmm.statespace_rand(UnitNormals(per), fx, None if Y is None else Y.reshape(-1), N=per + 1)
    order = np.argsort(x, kind="stable")
    xa = np.ascontiguousarray(x[order])
    E = np.vstack([np.eye(per), np.zeros((1, per))])
    zl = per - n * P_OUT - (3 * n if Y is not None else 0)
    z, eps = np.ascontiguousarray(E[:, :zl]), np.ascontiguousarray(E[:, per - n * P_OUT:])
    xi = np.ascontiguousarray(E[:, zl:zl + 3 * n]) if Y is not None else None
    ya = None if Y is None else np.ascontiguousarray(Y[:, order]).reshape(-1)
    out = np.full((per + 1, n * P_OUT), np.nan)
    ga = L.statespace_gps_array(abi_descs(lats))
    L.check(lmm.load().lmm_oilmm_rand_statespace(L.Arr(xa).ptr, n, None if ya is None else L.Arr(ya).ptr, P_OUT, L.Arr(L.colmajor(U)).ptr,
                                                 L.Arr(S).ptr, 3, S2, ga, 0, 3, 1, per + 1, L.Arr(z).ptr,
                                                 None if xi is None else L.Arr(xi).ptr, L.Arr(eps).ptr, L.Arr(out, True).ptr))
    back = np.empty_like(out.reshape(per + 1, P_OUT, n))
    back[:, :, order] = out.reshape(per + 1, P_OUT, n)
    return back.reshape(per + 1, n * P_OUT).T


@pytest.mark.parametrize("lats", [LATS, LATS_SHO], ids=["matern", "sho"])
@pytest.mark.parametrize("posterior", [False, True])
def test_rand_has_the_law_of_the_dense_gaussian(lmm, tol_rand, posterior, lats):
    """n = 64: the map from the normals to the samples, recovered by unit normals in ONE call of as many samples as there are
    normals (plus one of zeros: the mean), has M M' = the dense covariance + sigma2 I and the dense mean.  The model with an SHO
    sum goes through lmm_oilmm_rand_statespace itself."""
    n = 64
    x, U, S, Y = problem(n, seed=1)
    dims = [4, 3, 3]                     # Matern32 + Matern32 (or SHO), Matern52, Matern12 + Matern32
    per = sum(dims) * n + (3 * n if posterior else 0) + n * P_OUT
    out = rand_map(lmm, lats, x, U, S, Y if posterior else None, per)
    assert out.shape == (n * P_OUT, per + 1)
    mean, M = out[:, per], out[:, :per] - out[:, per:per + 1]
    rmean, rcov = latent_cov(lats, U, S, x, Y if posterior else None)
    rcov = rcov + S2 * np.eye(n * P_OUT)
    close(mean, rmean, tol_rand)
    close(M @ M.T, rcov, tol_rand)


def test_rand_columns_are_the_single_sample_calls(lmm):
    n = 64
    x, U, S, Y = problem(n, seed=1)
    y = Y.reshape(-1)
    fx = model(lmm, U, S, LATS)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    xs = np.array([x.min() - 0.3, 2.5, x.max() + 0.1])
    for yy, kw in ((None, {}), (y, {}), (y, {"xs": xs})):
        three = lmm.statespace_rand(np.random.default_rng(7), fx, yy, N=3, **kw)
        rng = np.random.default_rng(7)
        for q in range(3):
            assert np.array_equal(three[:, q], lmm.statespace_rand(rng, fx, yy, **kw)), q      # bitwise, and the documented draw order


@pytest.mark.parametrize("lats", [LATS, LATS_SHO], ids=["matern", "sho"])
def test_post_rand_on_a_window_has_the_law_of_the_dense_posterior(lmm, tol_rand, lats):
    n = 64
    x, U, S, Y = problem(n, seed=1)
    xs = np.array([2.1, 2.6, np.sort(x)[30], 3.3, 2.9])          # inside the data, unsorted, one equal to a training input
    with posterior_of(lmm, lats, x, U, S, Y) as post:
        first, count = post.window(xs)
        W = len(xs) + count
        assert 0 < count < n - 5                                  # a window, not the whole data
        per = 10 * W + len(xs) * P_OUT
        out = post.rand(UnitNormals(per), xs, N=per + 1)
        three = post.rand(np.random.default_rng(3), xs, N=3)
        rng = np.random.default_rng(3)
        for q in range(3):
            assert np.array_equal(three[:, q], post.rand(rng, xs))
    mean, M = out[:, per], out[:, :per] - out[:, per:per + 1]
    xa = np.concatenate([x, xs])
    Ya = np.concatenate([Y, np.full((P_OUT, len(xs)), np.nan)], axis=1)
    rmean, rcov = latent_cov(lats, U, S, xa, Ya)
    sel = (np.arange(P_OUT)[:, None] * len(xa) + n + np.arange(len(xs))[None, :]).reshape(-1)
    close(mean, rmean[sel], tol_rand)
    close(M @ M.T, rcov[np.ix_(sel, sel)] + S2 * np.eye(len(sel)), tol_rand)


# ---------------------------------------------------------------------------------------------------
# 5. the posterior handle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lats", [LATS, LATS_SHO], ids=["matern", "sho"])
def test_handle_queries_append_and_predictive_logpdf(lmm, tol, lats):
    LATS = lats
    n, k1, k2 = 120, 1, 40
    x, U, S, Y = problem(n + k1 + k2, seed=2)
    order = np.argsort(x, kind="stable")
    x, Y = x[order], Y[:, order]
    perm = np.random.default_rng(0).permutation(n)               # the training inputs go in unsorted
    xt, Yt = x[:n][perm], Y[:, :n][:, perm]
    xs = np.array([x[0] - 0.4, 0.5 * (x[10] + x[11]), x[20], x[n - 1] + 0.2, x[n - 1] + 3.0])

    def value():
        """statespace_logpdf of the training data; through lmm_oilmm_logpdf_statespace for the model with an SHO sum"""
        from lmm_amd import _lib as L
        if not has_sho(lats):
            return lmm.statespace_logpdf(model(lmm, U, S, lats)(lmm.MOInputIsotopicByOutputs(xt, P_OUT), S2), Yt.reshape(-1))
        xa, Ya = sorted_problem(xt, Yt)
        out = C.c_double()
        L.check(lmm.load().lmm_oilmm_logpdf_statespace(L.Arr(xa).ptr, n, L.Arr(Ya.reshape(-1)).ptr, P_OUT, L.Arr(L.colmajor(U)).ptr,
                                                       L.Arr(S).ptr, 3, S2, L.statespace_gps_array(abi_descs(lats)), 0, 3, 1, C.byref(out)))
        return out.value

    with posterior_of(lmm, lats, xt, U, S, Yt) as post:
        assert post.logpdf == value()                                                        # bitwise
        ref = dense(LATS, xt, U, S, Yt, xs=xs)
        close_value(post.logpdf, ref["value"], tol)
        gm, gv = post.mean_and_var(xs)
        close(gm, ref["mean"].reshape(-1), tol); close(gv, ref["var"].reshape(-1), tol)
        # held-out data: log N(train u held-out) - log N(train)
        hx, hY = x[n:n + 12], Y[:, n:n + 12]
        both = dense(LATS, np.concatenate([xt, hx]), U, S, np.concatenate([Yt, hY], axis=1))["value"]
        close_difference(post.predictive_logpdf(hx, hY.reshape(-1)), both, ref["value"], tol)
        hq = np.array([x[5] + 1e-3, x[50] - 2e-3, x[n - 1] + 0.5])                               # inside the data too
        hYq = np.random.default_rng(4).standard_normal((P_OUT, 3))
        both = dense(LATS, np.concatenate([xt, hq]), U, S, np.concatenate([Yt, hYq], axis=1))["value"]
        close_difference(post.predictive_logpdf(hq, hYq.reshape(-1)), both, ref["value"], tol)
        assert post.n == n and post.logpdf == value()                                             # the handle is as it was
        # appending k = 1 and k = 40 against conditioning on everything at once
        total = post.logpdf
        for a, b in ((n, n + k1), (n + k1, n + k1 + k2)):
            total += post.append(x[a:b], Y[:, a:b].reshape(-1))
            one_shot = dense(LATS, x[:b], U, S, Y[:, :b], xs=xs)
            close_value(post.logpdf, one_shot["value"], tol)
            close_value(total, one_shot["value"], tol)
            assert post.n == b
            gm, gv = post.mean_and_var(xs)
            close(gm, one_shot["mean"].reshape(-1), tol); close(gv, one_shot["var"].reshape(-1), tol)


# ---------------------------------------------------------------------------------------------------
# 6. refusals through the C ABI
# ---------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(lmm, tol):
    import torch
    from lmm_amd import _lib as L
    n = 40
    x, U, S, Y = problem(n)
    order = np.argsort(x, kind="stable")
    x, Y = np.ascontiguousarray(x[order]), np.ascontiguousarray(Y[:, order])
    y = Y.reshape(-1)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    sho_sum = {"kind": "sum", "variance": 1.2, "lengthscale": 0.9, "mean": 0.3,
               "terms": [term_desc(("matern32", 0.8, 1.1)), term_desc(("sho", 0.5, 1.9, 3.0))]}
    plain = [{"kind": "matern52", "variance": 1.4, "lengthscale": 0.6, "mean": 0.0}, {"kind": "matern12", "variance": 1.0, "lengthscale": 0.5, "mean": 0.0}]
    gps = L.statespace_gps_array([plain[0], sho_sum, plain[1]])
    fx = model(lmm, U, S, LATS)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)

    def refused(rc, l):
        assert rc == L.LMM_ERR_UNSUPPORTED, rc
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        assert lat.value == l and b"latent %d" % l in lib.lmm_last_error_string(), lib.lmm_last_error_string()

    with lmm.statespace_posterior(fx, y) as post:
        xq = np.array([1.0, 2.5, 7.0])
        before = post.mean_and_var(xq)

        def handle_unchanged():
            after = post.mean_and_var(xq)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

        out = C.c_double()
        # the state-space entry point takes the array; the dense entry points refuse the tag of the new creator, naming the latent
        L.check(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, gps, 0, 3, 1, C.byref(out)))
        Yc = np.where(np.isnan(Y), 0.5, Y).reshape(-1)
        refused(lib.lmm_oilmm_logpdf(L.Arr(x).ptr, 1, n, L.Arr(Yc).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, C.c_double(S2), gps, 0, 3, 1,
                                     C.byref(out)), 1)
        handle_unchanged()
        hp = C.c_void_p()
        refused(lib.lmm_oilmm_posterior_create(L.Arr(x).ptr, 1, n, L.Arr(Yc).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, C.c_double(S2), gps, 0, 3,
                                               C.byref(hp)), 1)
        assert not hp.value
        handle_unchanged()
        # the gradients with respect to locations refuse a sum latent, whichever creator its tag came from
        gg = (L.GpGradT * 3)()
        gy, gx, val, gs2 = np.empty(n * P_OUT), np.empty(n), C.c_double(), C.c_double()
        for arr in (gps, L.statespace_gps_array([plain[0], dict(sho_sum, terms=[term_desc(("matern32", 0.8, 1.1)), term_desc(("matern12", 0.5, 1.9))]), plain[1]])):
            refused(lib.lmm_oilmm_logpdf_grad_statespace_x(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, arr, 0, 3, 1,
                                                           C.byref(val), L.Arr(gy, True).ptr, C.byref(gs2), None, None, gg,
                                                           L.Arr(gx, True).ptr), 1)
            handle_unchanged()
        xsd = torch.tensor(xq, device="cuda")
        cot = torch.ones(3 * P_OUT, dtype=torch.float64, device="cuda")
        gxs = torch.zeros(3, dtype=torch.float64, device="cuda")
        refused(lib.lmm_oilmm_statespace_post_mean_and_var_grad_xs(post._ptr, xsd.data_ptr(), 3, cot.data_ptr(), None, gxs.data_ptr()), 0)
        handle_unchanged()
        # D >= 5 and three terms: refused by the state-space entry points, naming the latent
        m32, m52 = term_desc(("matern32", 0.8, 1.1)), term_desc(("matern52", 0.5, 1.9))
        for bad in ({"kind": "sum", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0, "terms": [m32, m52]},
                    {"kind": "sum", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0, "terms": [m32, m32, m32]}):
            refused(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2,
                                                    L.statespace_gps_array([plain[0], plain[1], bad]), 0, 3, 1, C.byref(out)), 2)
            handle_unchanged()
        # and the next valid call is served
        close_value(lmm.statespace_logpdf(fx, y), dense(LATS, x, U, S, Y)["value"], tol)
