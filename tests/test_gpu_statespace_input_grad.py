"""-m gpu: gradients with respect to locations on the state-space path (include/lmm_hip.h, lmm_oilmm_logpdf_grad_statespace_x,
lmm_dev_statespace_grad_x and lmm_oilmm_statespace_post_mean_and_var_grad_xs; DESIGN.md 4.18 "Gradients with respect to locations"):
the one-latent building block against the NumPy restatement, statespace_logpdf_and_gradient(inputs=True) against the restatement and
the dense (Cholesky) path, StateSpacePosterior.mean_and_var_vjp against the restatement and the dense mean_and_var_vjp, and the C
ABI's refusals.

Tolerance (the rule of tests/test_gpu_statespace.py): max(1e-10, 100 DELTA) of max|reference| per array, DELTA =
test_statespace_input_grad_abi.delta_input_grad() (1.65e-13) for d lml / d x and delta_query_grad() (2.74e-13) for the query
derivatives: 1e-10 both.  The factor 100 covers the GPU's other summation order and its fused multiply-adds.  The reference is always
the NumPy restatement or another path of the library (the dense one), never the code under test."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_statespace as GS
import test_gpu_statespace_posterior as GP
import test_sho_abi as S
import test_statespace_abi as T
import test_statespace_input_grad_abi as IG
import test_statespace_posterior_abi as PA

pytestmark = pytest.mark.gpu

LATENTS = GP.LATENTS
S2 = GS.S2
close, dev, nan_dev = GP.close, GP.dev, GP.nan_dev


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * IG.delta_input_grad())


@pytest.fixture(scope="module")
def qtol():
    return max(1e-10, 100.0 * IG.delta_query_grad())


# ---------------------------------------------------------------------------------------------------
# the building block
# ---------------------------------------------------------------------------------------------------
_REF = {}


def block_reference(lat, n, unobserved):
    """test_gpu_statespace_posterior.block_case (runs of unobserved points longer than a chunk; an oscillator's inputs have ties) and
    the restated d lml / d x, computed once."""
    key = (lat, n, unobserved)
    if key not in _REF:
        model, x, w, r = GP.block_case(lat, n, unobserved)
        _REF[key] = (model, x, w, r, IG.input_grad(model, x, w, r))
    return _REF[key]


def gpu_grad_x(lmm, model, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    xd, wd, rd = dev(x), dev(w), dev(r)
    gx = nan_dev(n)
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])                       # the mean is not read
    L.check(lmm.load().lmm_dev_statespace_grad_x(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, gx.data_ptr()))
    return gx.cpu().numpy()


@pytest.mark.parametrize("n,unobserved", [(1, False), (1, True), (2, False), (2, True), (17, True), (63, False), (63, True), (333, True),
                                          (2100, True), (4097, True)])
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_building_block_against_the_restatement(lmm, tol, lat, n, unobserved):
    """One and two points, a ragged last chunk (17 = 16 + 1), two workgroups of the scan at chunk 16 (2100 points: 132 aggregates),
    the switch to chunk 64 (4097)."""
    model, x, w, r, ref = block_reference(lat, n, unobserved)
    got = gpu_grad_x(lmm, model, x, w, r, 0)
    assert (got[~np.isfinite(w)] == 0.0).all()                     # exactly 0 where nothing is observed
    if n == 1 or not np.isfinite(w).any():
        assert (got == 0.0).all()
        return
    close(got, ref, tol, "grad_x")
    assert (gpu_grad_x(lmm, model, x, w, r, 0) == got).all()       # bitwise on a repeated call


@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_building_block_explicit_chunks(lmm, tol, lat):
    model, x, w, r, ref = block_reference(lat, 63, True)
    for chunk in (1, 63):
        got = gpu_grad_x(lmm, model, x, w, r, chunk)
        close(got, ref, tol, f"chunk {chunk}")
        assert (got[~np.isfinite(w)] == 0.0).all()
        assert (gpu_grad_x(lmm, model, x, w, r, chunk) == got).all()


# ---------------------------------------------------------------------------------------------------
# the OILMM through the mirror
# ---------------------------------------------------------------------------------------------------
SHO = GP.SHO
MIXED = [GS.GPS[0], GS.GPS[2], SHO]                                 # Matern12, Matern52, SHO


def model_of(g):
    return S.sho(g["variance"], g["lengthscale"], g["quality"]) if g["kind"] == "sho" else PA.model_of(g["kind"], g["variance"], g["lengthscale"])


def latent_data(gps, U, Sv, x, s2, Y):
    """Per latent the front end's (w, r) over the SORTED points (include/lmm_hip.h "state space"): with H = U sqrt(S), o the observed
    outputs of point t and G = H_o' H_o, z = G^-1 H_o' y_o, r_l = z_l - mean_l and w_l = sigma2 (G^-1)_ll; w = +Inf where nothing is
    observed.  Returns (order, x sorted, [(model, w, r)])."""
    order = np.argsort(x, kind="stable")
    xs_, Ys = x[order], Y[:, order]
    n, m = len(x), len(gps)
    H = U * np.sqrt(Sv)[None, :]
    w, r = np.full((m, n), np.inf), np.zeros((m, n))
    for t in range(n):
        o = ~np.isnan(Ys[:, t])
        if not o.any():
            continue
        Gi = np.linalg.inv(H[o].T @ H[o])
        z = Gi @ (H[o].T @ Ys[o, t])
        w[:, t] = s2 * np.diag(Gi)
        r[:, t] = z - np.array([g["mean"] for g in gps])
    return order, xs_, [(model_of(g), w[l], r[l]) for l, g in enumerate(gps)]


def input_grad_reference(gps, U, Sv, x, s2, Y, fn=IG.input_grad):
    """d logpdf / d x in the callers' order: the latents' d lml_l / d x added (the regulariser and the projection do not depend on x).
    fn: IG.input_grad (the restatement) or IG.dense_input_grad (the dense analytic gradient)."""
    order, xs_, lat = latent_data(gps, U, Sv, x, s2, Y)
    g = np.zeros(len(x))
    g[order] = sum(fn(model, xs_, w, r) for model, w, r in lat)
    return g


def problem(n, nan):
    """p = 7, m = 3.  nan: the patterns of tests/test_gpu_missing.py, and four points whose outputs are all NaN."""
    if not nan:
        return GS.problem(n, p=7)
    x, U, Sv, Y = GS.nan_problem(n)
    Y = Y.copy()
    Y[:, [0, 5, 6, n - 1]] = np.nan
    return x, U, Sv, Y


def same_but_x(a, b):
    """Every entry of the gradient dicts but "x" is bitwise the same."""
    keys = [k for k in ("value", "y", "sigma2", "S", "U") if k in a or k in b]
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert len(a["gps"]) == len(b["gps"])
    for ga, gb in zip(a["gps"], b["gps"]):
        assert ga == gb


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("n", [63, 333])
def test_oilmm_through_the_mirror(lmm, tol, n, nan):
    import torch
    x, U, Sv, Y = problem(n, nan)
    p, y = Y.shape[0], Y.reshape(-1)
    f = GP.model(lmm, U, Sv, MIXED)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), S2)
    ref = input_grad_reference(MIXED, U, Sv, x, S2, Y)
    for with_reg in (True, False):
        base = lmm.statespace_logpdf_and_gradient(fx, y, with_reg)
        got = lmm.statespace_logpdf_and_gradient(fx, y, with_reg, inputs=True)
        assert "x" not in base and set(got) - set(base) == {"x"}
        assert isinstance(got["x"], np.ndarray) and got["x"].shape == x.shape and got["x"].dtype == np.float64
        close(got["x"], ref, tol, "x")
        same_but_x(got, base)
        if nan:
            allnan = np.isnan(Y).all(axis=0)
            assert allnan.sum() == 4 and (got["x"][allnan] == 0.0).all()
            with pytest.raises(NotImplementedError):
                got["S"]
    # unsorted inputs: "x" comes back in the callers' order (x has no ties: the stable sort hands the library the same sequence)
    tp = np.random.default_rng(n).permutation(n)
    un = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x[tp], p), S2), Y[:, tp].reshape(-1), inputs=True)
    assert (un["x"] == got0(lmm, fx, y)["x"][tp]).all()
    # a torch device x: a device tensor with the same numbers
    td = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(torch.tensor(x, device="cuda"), p), S2),
                                            torch.tensor(y, device="cuda"), inputs=True)
    assert td["x"].is_cuda and td["x"].dtype == torch.float64 and tuple(td["x"].shape) == x.shape
    assert (td["x"].cpu().numpy() == got0(lmm, fx, y)["x"]).all()


def got0(lmm, fx, y):
    return lmm.statespace_logpdf_and_gradient(fx, y, inputs=True)


@pytest.mark.parametrize("kinds", [("matern12",) * 3, ("matern32",) * 3, ("matern52",) * 3, ("matern12", "matern32", "matern52")], ids=str)
def test_dense_cross_check(lmm, tol, kinds):
    """Against logpdf_and_gradient(inputs=True) of the Cholesky path, n = 63 without ties."""
    x, U, Sv, Y = GS.problem(63)
    gps = [dict(g, kind=k) for g, k in zip(GS.GPS, kinds)]
    fx = GS.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, GS.P_OUT), S2)
    y = Y.reshape(-1)
    got = lmm.statespace_logpdf_and_gradient(fx, y, inputs=True)
    ref = lmm.logpdf_and_gradient(fx, y, inputs=True)
    close(got["x"], ref["x"], tol, "x vs dense")
    close(got["x"], input_grad_reference(gps, U, Sv, x, S2, Y), tol, "x vs restatement")


def test_sho_against_the_numpy_references(lmm, tol):
    """The dense path refuses inputs=True for SHO latents: the restatement and the dense analytic gradient in NumPy stand in."""
    x, U, Sv, Y = GS.problem(63)
    gps = [dict(SHO, quality=Q) for Q in S.QS]
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, GS.P_OUT), S2)
    with pytest.raises(NotImplementedError):
        lmm.logpdf_and_gradient(fx, Y.reshape(-1), inputs=True)
    got = lmm.statespace_logpdf_and_gradient(fx, Y.reshape(-1), inputs=True)["x"]
    close(got, input_grad_reference(gps, U, Sv, x, S2, Y), tol, "x vs restatement")
    close(got, input_grad_reference(gps, U, Sv, x, S2, Y, IG.dense_input_grad), tol, "x vs dense analytic")


def test_duplicated_inputs(lmm, tol):
    x, U, Sv, Y = GS.problem(63)
    x = x.copy()
    x[10:13] = x[10]
    x[40] = x[41]
    y = Y.reshape(-1)
    gps = [GS.GPS[1], GS.GPS[2], SHO]                               # Matern32, Matern52, SHO: differentiable at a tie
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, GS.P_OUT), S2)
    got = lmm.statespace_logpdf_and_gradient(fx, y, inputs=True)["x"]
    close(got, input_grad_reference(gps, U, Sv, x, S2, Y, IG.dense_input_grad), tol, "x vs dense analytic")
    # Matern12 has a kink at a tie: served and finite, not compared
    fx12 = GS.model(lmm, U, Sv)(lmm.MOInputIsotopicByOutputs(x, GS.P_OUT), S2)
    g12 = lmm.statespace_logpdf_and_gradient(fx12, y, inputs=True)["x"]
    assert g12.shape == x.shape and np.isfinite(g12).all()


@pytest.mark.parametrize("m", [20, 40])
def test_more_latents_than_a_launch(lmm, tol, m):
    """m Matern32 latents, p = m, n = 63 against the dense path (a launch takes at most 32 latents)."""
    rng = np.random.default_rng(m)
    n = 63
    x = np.sort(rng.uniform(0.0, 8.0, n))
    U = np.linalg.qr(rng.standard_normal((m, m)))[0]
    Sv = rng.uniform(0.5, 2.0, m)
    gps = [{"kind": "matern32", "variance": float(rng.uniform(0.5, 1.5)), "lengthscale": float(rng.uniform(0.5, 1.5)),
            "mean": float(rng.uniform(-0.5, 0.5))} for _ in range(m)]
    y = rng.standard_normal(m * n)
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, m), S2)
    got = lmm.statespace_logpdf_and_gradient(fx, y, inputs=True)
    same_but_x(got, lmm.statespace_logpdf_and_gradient(fx, y))
    close(got["x"], lmm.logpdf_and_gradient(fx, y, inputs=True)["x"], tol, "x vs dense")


# ---------------------------------------------------------------------------------------------------
# the posterior object's queries
# ---------------------------------------------------------------------------------------------------
def vjp_reference(gps, U, Sv, x, s2, Y, Q, dmean, dvar):
    """sum_l (sum_o dmean[o, q] H[o, l]) d mean_l / d s + (sum_o dvar[o, q] H[o, l]^2) d var_l / d s from the restated derivatives."""
    _, xs_, lat = latent_data(gps, U, Sv, x, s2, Y)
    H = U * np.sqrt(Sv)[None, :]
    p, ns = U.shape[0], len(Q)
    out = np.zeros(ns)
    for l, (model, w, r) in enumerate(lat):
        dmu, dv = IG.query_grad(model, xs_, PA.full_states(model, xs_, w, r), Q)
        if dmean is not None:
            out += (H[:, l] @ dmean.reshape(p, ns)) * dmu
        if dvar is not None:
            out += ((H[:, l] ** 2) @ dvar.reshape(p, ns)) * dv
    return out


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("n", [1, 63, 333])
def test_mean_and_var_vjp(lmm, qtol, n, nan):
    import torch
    gps = GS.GPS + [SHO]
    x, U, Sv, Y, _ = GP.nan_problem(n, True) if nan else GP.complete_problem(n, True)
    p, y = Y.shape[0], Y.reshape(-1)
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    Q = PA.queries(x)
    ns = len(Q)
    rng = np.random.default_rng([n, int(nan)])
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    with lmm.statespace_posterior(fx, y) as post:
        for dm, dv in ((dmean, dvar), (dmean, None), (None, dvar)):
            got = post.mean_and_var_vjp(Q, dm, dv)
            assert set(got) == {"x"} and isinstance(got["x"], np.ndarray) and got["x"].shape == Q.shape
            close(got["x"], vjp_reference(gps, U, Sv, x, S2, Y, Q, dm, dv), qtol, "vjp vs restatement")
        both = post.mean_and_var_vjp(Q, dmean, dvar)["x"]
        assert (post.mean_and_var_vjp(Q, dmean)["x"] == post.mean_and_var_vjp(Q, dmean, None)["x"]).all()
        # a query's entry does not depend on the other queries
        sub = np.array([0, 3, 17, ns - 1])
        cols = lambda d: d.reshape(p, ns)[:, sub].reshape(-1)
        assert (post.mean_and_var_vjp(Q[sub], cols(dmean), cols(dvar))["x"] == both[sub]).all()
        # a device xs: a device tensor with the same numbers
        td = post.mean_and_var_vjp(torch.tensor(Q, device="cuda"), torch.tensor(dmean, device="cuda"), torch.tensor(dvar, device="cuda"))["x"]
        assert td.is_cuda and (td.cpu().numpy() == both).all()
        with pytest.raises(ValueError, match="ns \\* p"):
            post.mean_and_var_vjp(Q, dmean[:-1])
        with pytest.raises(ValueError, match="both None"):
            post.mean_and_var_vjp(Q)
    with pytest.raises(ValueError, match="closed"):
        post.mean_and_var_vjp(Q, dmean)


def test_mean_and_var_vjp_against_the_dense_path(lmm, qtol):
    """Matern latents: mean_and_var_vjp of posterior(fx, y) on the Cholesky path.  Queries equal to a training input are left out: the
    Matern12 latent's mean has a kink there, and the two paths need not pick the same side."""
    x, U, Sv, Y, gps = GP.complete_problem(63, False)
    p, y = Y.shape[0], Y.reshape(-1)
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    Q = PA.queries(x)
    Q = Q[~np.isin(Q, x)]
    ns = len(Q)
    rng = np.random.default_rng(63)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    dense = lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(Q, p), S2)
    with lmm.statespace_posterior(fx, y) as post:
        for dm, dv in ((dmean, dvar), (dmean, None)):
            close(post.mean_and_var_vjp(Q, dm, dv)["x"], lmm.mean_and_var_vjp(dense, dm, dv)["x"], qtol, "vjp vs dense")


def test_mean_and_var_vjp_central_differences(lmm):
    """A sanity check only: central differences of post.mean_and_var itself, h = 1e-6, away from the training inputs (Matern12 kinks)
    by more than 10 h.  Values of order 1 leave eps / h = 2e-10 of rounding per entry, the 5 p = 25 entries a query sums about 1e-8, and
    the truncation (h / dt)^2 is below 1e-8 as well: the tolerance is 1e-5 of max|vjp|."""
    x, U, Sv, Y, gps = GP.complete_problem(63, True)
    p, y = Y.shape[0], Y.reshape(-1)
    fx = GP.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    h = 1e-6
    Q = PA.queries(x)
    Q = Q[np.abs(Q[:, None] - x[None, :]).min(axis=1) > 10 * h]
    ns = len(Q)
    rng = np.random.default_rng(1)
    dmean, dvar = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    with lmm.statespace_posterior(fx, y) as post:
        got = post.mean_and_var_vjp(Q, dmean, dvar)["x"]
        mp, vp = post.mean_and_var(Q + h)
        mm, vm = post.mean_and_var(Q - h)
    fd = ((dmean * (mp - mm)).reshape(p, ns).sum(axis=0) + (dvar * (vp - vm)).reshape(p, ns).sum(axis=0)) / (2 * h)
    close(got, fd, 1e-5, "vjp vs central differences")


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_c_abi(lmm, tol, qtol):
    from lmm_amd import _lib as L
    x, U, Sv, Y = GS.problem(63)
    y = Y.reshape(-1)
    p, n = GS.P_OUT, 63
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(Sv)
    gps = L.gps_array(GS.GPS)
    fx = GS.model(lmm, U, Sv)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    want = lmm.statespace_logpdf_and_gradient(fx, y, inputs=True)

    def grad_x(xa, gx, l0=0, l1=3, n_=n):
        val = C.c_double(float("nan"))
        rc = lib.lmm_oilmm_logpdf_grad_statespace_x(None if xa is None else L.Arr(xa).ptr, n_, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, 3, S2, gps,
                                                    l0, l1, 1, C.byref(val), None, None, None, None, None,
                                                    None if gx is None else L.Arr(gx, True).ptr)
        return rc, val.value

    gx = np.full(n, np.nan)
    # refusals: a NULL x, n < 1, unsorted inputs with the index
    assert grad_x(None, gx)[0] == L.LMM_ERR_ARG
    assert grad_x(x, gx, n_=0)[0] == L.LMM_ERR_ARG
    xb = x.copy()
    xb[20], xb[21] = x[21], x[20]
    assert grad_x(xb, gx)[0] == L.LMM_ERR_ARG
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert info.value == 21 and np.isnan(gx).all()
    # the next valid call is served; grad_x = NULL is the entry point without `_x`; shards are partial sums
    rc, val = grad_x(x, gx)
    assert rc == L.LMM_OK and val == want["value"] and (gx == want["x"]).all()
    rc, val = grad_x(x, None)
    assert rc == L.LMM_OK and val == want["value"]
    parts = np.zeros(n)
    for l0, l1 in ((0, 1), (1, 3)):
        gk = np.full(n, np.nan)
        assert grad_x(x, gk, l0, l1)[0] == L.LMM_OK
        parts += gk
    close(parts, want["x"], tol, "shards")
    # the building block: NULL and size refusals, then a valid call
    model, xb_, w, r, ref = block_reference("matern52", 63, True)
    xd, wd, rd, gd = dev(xb_), dev(w), dev(r), nan_dev(63)
    gp = L.gps_array([model.desc()])
    blk = lib.lmm_dev_statespace_grad_x
    assert blk(None, 63, gp, wd.data_ptr(), rd.data_ptr(), 0, gd.data_ptr()) == L.LMM_ERR_ARG
    assert blk(xd.data_ptr(), 63, gp, wd.data_ptr(), rd.data_ptr(), 0, None) == L.LMM_ERR_ARG
    assert blk(xd.data_ptr(), 0, gp, wd.data_ptr(), rd.data_ptr(), 0, gd.data_ptr()) == L.LMM_ERR_ARG
    assert blk(xd.data_ptr(), 63, gp, wd.data_ptr(), rd.data_ptr(), -1, gd.data_ptr()) == L.LMM_ERR_ARG
    L.check(blk(xd.data_ptr(), 63, gp, wd.data_ptr(), rd.data_ptr(), 0, gd.data_ptr()))
    close(gd.cpu().numpy(), ref, tol, "block")
    # the posterior's pullback
    h = C.c_void_p()
    L.check(lib.lmm_oilmm_statespace_posterior_create(L.Arr(x).ptr, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, 3, S2, gps, 0, 3, C.byref(h), None))
    Q = PA.queries(x)
    ns = len(Q)
    rng = np.random.default_rng(2)
    dm, dv = rng.standard_normal(ns * p), rng.standard_normal(ns * p)
    gq = np.full(ns, np.nan)
    vjp = lib.lmm_oilmm_statespace_post_mean_and_var_grad_xs
    assert vjp(None, L.Arr(Q).ptr, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr) == L.LMM_ERR_ARG
    assert vjp(h, None, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr) == L.LMM_ERR_ARG
    assert vjp(h, L.Arr(Q).ptr, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, None) == L.LMM_ERR_ARG
    assert vjp(h, L.Arr(Q).ptr, 0, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr) == L.LMM_ERR_ARG
    assert vjp(h, L.Arr(Q).ptr, ns, None, None, L.Arr(gq, True).ptr) == L.LMM_ERR_ARG
    assert b"both NULL" in lib.lmm_last_error_string()
    qb = Q.copy()
    qb[7] = np.inf
    assert vjp(h, L.Arr(qb).ptr, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr) == L.LMM_ERR_ARG
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert info.value == 7 and np.isnan(gq).all()
    lmm.set_compute_dtype("f32")
    try:
        assert vjp(h, L.Arr(Q).ptr, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr) == L.LMM_ERR_UNSUPPORTED
    finally:
        lmm.set_compute_dtype("f64")
    L.check(vjp(h, L.Arr(Q).ptr, ns, L.Arr(dm).ptr, L.Arr(dv).ptr, L.Arr(gq, True).ptr))
    close(gq, vjp_reference(GS.GPS, U, Sv, x, S2, Y, Q, dm, dv), qtol, "vjp")
    gm = np.full(ns, np.nan)
    L.check(vjp(h, L.Arr(Q).ptr, ns, L.Arr(dm).ptr, None, L.Arr(gm, True).ptr))
    close(gm, vjp_reference(GS.GPS, U, Sv, x, S2, Y, Q, dm, None), qtol, "vjp of the mean")
    assert lib.lmm_statespace_post_destroy(h) == L.LMM_OK
