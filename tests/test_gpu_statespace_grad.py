"""-m gpu: gradients of the state-space logpdf (include/lmm_hip.h "state space"): the building block
lmm_dev_statespace_grad against the NumPy restatement of tests/test_statespace_grad_abi.py, statespace_logpdf_and_gradient against the
library's Cholesky path (logpdf_and_gradient) and the oracle, NaN data against the missing-data gradient, and the refusals.

Tolerance (the rule of tests/test_gpu_statespace.py): max(1e-10, 100 DELTA) of max|reference| per array, and relative for a scalar,
with DELTA the largest disagreement between the restatement and the dense analytic gradient (test_statespace_grad_abi.delta_grad():
3.0e-14, so the tolerance is 1e-10)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_statespace as GS
import test_statespace_abi as T
import test_statespace_grad_abi as TG

pytestmark = pytest.mark.gpu

GPS, P_OUT, S2 = GS.GPS, GS.P_OUT, GS.S2


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * TG.delta_grad())


close, close_value = GS.close, GS.close_value


# ---------------------------------------------------------------------------------------------------
# the building block
# ---------------------------------------------------------------------------------------------------
_REF = {}


def grad_reference(kind, n, unobserved):
    key = (kind, n, unobserved)
    if key not in _REF:
        v, ell, x, w, r = GS.block_case(kind, n, unobserved)
        _REF[key] = ((v, ell, x, w, r), TG.statespace_grad_reference(kind, v, ell, x, w, r))
    return _REF[key]


def gpu_grad(lmm, kind, v, ell, x, w, r, chunk, with_filter=False):
    """(lml, grad_r, grad_w, d/d variance, d/d lengthscale) of lmm_dev_statespace_grad, and lmm_dev_statespace_filter's lml."""
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, wd, rd = dev(x), dev(w), dev(r)
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")
    gr, gw, lml, gth, fm, fv, flml = nan(n), nan(n), nan(1), nan(2), nan(n), nan(n), nan(1)
    torch.cuda.synchronize()
    gp = L.gps_array([dict(GS.kernel_of(lmm, kind, v, ell).desc(), mean=0.7)])      # the mean is not read
    lib = lmm.load()
    L.check(lib.lmm_dev_statespace_grad(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, lml.data_ptr(), gr.data_ptr(),
                                        gw.data_ptr(), gth.data_ptr()))
    got = (float(lml.cpu()[0]), gr.cpu().numpy(), gw.cpu().numpy(), float(gth.cpu()[0]), float(gth.cpu()[1]))
    if not with_filter:
        return got
    L.check(lib.lmm_dev_statespace_filter(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, fm.data_ptr(), fv.data_ptr(),
                                          flml.data_ptr()))
    return got, float(flml.cpu()[0])


def check_block(got, ref, case, tol):
    v, ell, x, w, r = case
    close_value(got[0], ref[0], tol)
    close(got[1], ref[1], tol); close(got[2], ref[2], tol)
    close_value(got[3], ref[3], tol); close_value(got[4], ref[4], tol)
    unobs = ~np.isfinite(w)
    assert (got[1][unobs] == 0).all() and (got[2][unobs] == 0).all()
    # the scaling identity v g_v + sum w g_w + sum r g_r / 2 = -n_obs / 2 on the GPU outputs, to the tolerance of the terms' size
    lhs, mag, rhs = TG.scaling_identity(v, w, r, got[1], got[2], got[3])
    assert abs(lhs - rhs) <= tol * max(mag, abs(rhs)), (lhs, rhs, mag)


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", GS.BLOCK_N)
@pytest.mark.parametrize("kind", T.KINDS)
def test_gradient_block(lmm, tol, kind, n, unobserved):
    case, ref = grad_reference(kind, n, unobserved)
    results = {}
    for chunk in (1, 7, 64, 0, n):
        got, flml = gpu_grad(lmm, kind, *case, chunk, with_filter=True)
        assert got[0] == flml                                                     # the value is the filter's, bitwise
        check_block(got, ref, case, tol)
        results[chunk] = got
    again = gpu_grad(lmm, kind, *case, 7)
    assert again[0] == results[7][0] and again[3:] == results[7][3:]             # bitwise
    assert (again[1] == results[7][1]).all() and (again[2] == results[7][2]).all()


@pytest.mark.parametrize("kind", T.KINDS)
def test_dual_scan_recurses(lmm, tol, kind):
    """n = 5000 with chunk = 1: 5000 (value, tangent) aggregates per seed, 40 or 79 workgroups of the scan, whose totals are scanned by
    a second level."""
    case, ref = grad_reference(kind, 5000, True)
    check_block(gpu_grad(lmm, kind, *case, 1), ref, case, tol)


# ---------------------------------------------------------------------------------------------------
# the OILMM entry point
# ---------------------------------------------------------------------------------------------------
def check_dict(got, ref, tol, mixing=True):
    close_value(got["value"], ref["value"], tol)
    close(got["y"], ref["y"], tol)
    close_value(got["sigma2"], ref["sigma2"], tol)
    if mixing:
        close(got["S"], ref["S"], tol); close(got["U"], ref["U"], tol)
    assert len(got["gps"]) == len(ref["gps"])
    for a, b in zip(got["gps"], ref["gps"]):
        for key in ("variance", "lengthscale", "mean"):
            close_value(a[key], b[key], tol)


@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n", [1, 63, 333])
def test_gradient_vs_cholesky_path_and_oracle(lmm, tol, n, with_reg):
    import torch
    x, U, S, Y = GS.problem(n)
    f = GS.model(lmm, U, S)
    y = Y.reshape(-1)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    got = lmm.statespace_logpdf_and_gradient(fx, y, with_reg)
    assert set(got) == {"value", "y", "sigma2", "S", "U", "gps"}
    assert isinstance(got["y"], np.ndarray) and got["y"].shape == y.shape and got["y"].dtype == y.dtype
    check_dict(got, lmm.logpdf_and_gradient(fx, y, with_reg), tol)
    assert got["value"] == lmm.statespace_logpdf(fx, y, with_reg)                        # bitwise
    if with_reg:                                  # the oracle has Matern32 and Matern52 (and always the regulariser)
        f2 = GS.model(lmm, U[:, 1:], S[1:], GPS[1:])
        got2 = lmm.statespace_logpdf_and_gradient(f2(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y)
        check_dict(got2, T.O.oilmm_logpdf_grad(GPS[1:], U[:, 1:], S[1:], x, S2, y), tol)
    # unsorted inputs give the sorted result, with "y" in the callers' order
    perm = np.random.default_rng(n).permutation(n)
    gp = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x[perm], P_OUT), S2), Y[:, perm].reshape(-1), with_reg)
    assert gp["value"] == got["value"] and gp["sigma2"] == got["sigma2"]
    assert (gp["y"].reshape(P_OUT, n) == got["y"].reshape(P_OUT, n)[:, perm]).all()
    assert (gp["S"] == got["S"]).all() and (gp["U"] == got["U"]).all() and gp["gps"] == got["gps"]
    # torch device inputs: a device "y", the same numbers
    gt = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(torch.tensor(x, device="cuda"), P_OUT), S2),
                                            torch.tensor(y, device="cuda"), with_reg)
    assert gt["y"].is_cuda and gt["y"].dtype == torch.float64 and (gt["y"].cpu().numpy() == got["y"]).all()
    assert gt["value"] == got["value"] and gt["sigma2"] == got["sigma2"] and (gt["S"] == got["S"]).all() and gt["gps"] == got["gps"]


def test_gradient_with_duplicated_inputs(lmm, tol):
    x, U, S, Y = GS.problem(63)
    x = x.copy()
    x[10:13] = x[10]
    fx = GS.model(lmm, U, S)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    got = lmm.statespace_logpdf_and_gradient(fx, Y.reshape(-1))
    check_dict(got, lmm.logpdf_and_gradient(fx, Y.reshape(-1)), tol)


@pytest.mark.parametrize("n", [64, 333])
def test_gradient_nan_vs_the_missing_data_path(lmm, tol, n):
    x, U, S, Y = GS.nan_problem(n)
    p = Y.shape[0]
    f = GS.model(lmm, U, S)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), S2)
    y = Y.reshape(-1)
    for with_reg in (True, False):
        got = lmm.statespace_logpdf_and_gradient(fx, y, with_reg)
        check_dict(got, lmm.logpdf_and_gradient(fx, y, with_reg), tol, mixing=False)
        assert (got["y"][np.isnan(y)] == 0).all()
        assert got["value"] == lmm.statespace_logpdf(fx, y, with_reg)
        for key in ("S", "U"):
            with pytest.raises(NotImplementedError, match="NaN"):
                got[key]
    got = lmm.statespace_logpdf_and_gradient(fx, y)
    # appended all-NaN points (in front, between, equal to a training input, behind) change no gradient and get zero rows in "y"
    xe = np.array([x[0] - 1.0, 0.5 * (x[3] + x[4]), x[20], x[-1] + 2.0])
    x2 = np.concatenate([x, xe])
    Y2 = np.concatenate([Y, np.full((p, len(xe)), np.nan)], axis=1)
    got2 = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x2, p), S2), Y2.reshape(-1))
    g2y = got2["y"].reshape(p, n + len(xe))
    assert (g2y[:, n:] == 0).all()
    check_dict(dict(got2, y=g2y[:, :n].reshape(-1)), got, tol, mixing=False)
    # complete data beside all-NaN points goes the same way
    x3, U3, S3, Y3 = GS.problem(63)
    f3 = GS.model(lmm, U3, S3)
    ref3 = lmm.statespace_logpdf_and_gradient(f3(lmm.MOInputIsotopicByOutputs(x3, P_OUT), S2), Y3.reshape(-1))
    Y4 = np.concatenate([Y3, np.full((P_OUT, 2), np.nan)], axis=1)
    got4 = lmm.statespace_logpdf_and_gradient(f3(lmm.MOInputIsotopicByOutputs(np.concatenate([x3, [1.0, 9.5]]), P_OUT), S2), Y4.reshape(-1))
    g4y = got4["y"].reshape(P_OUT, 65)
    assert (g4y[:, 63:] == 0).all()
    check_dict(dict(got4, y=g4y[:, :63].reshape(-1)), ref3, tol, mixing=False)


def abi_grad(lmm, gps, x, y, p, U, S, l0, l1, with_reg, want_mixing=True):
    from lmm_amd import _lib as L
    m, n = len(gps), len(x)
    val, gs2 = C.c_double(), C.c_double()
    gy, gS, gU = np.empty(n * p), np.empty(m), np.empty(p * m)
    gg = (L.GpGradT * m)()
    rc = lmm.load().lmm_oilmm_logpdf_grad_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, p, L.Arr(L.colmajor(U)).ptr, L.Arr(S).ptr, m, S2,
                                                     L.gps_array(gps), l0, l1, int(with_reg), C.byref(val), L.Arr(gy, True).ptr,
                                                     C.byref(gs2), L.Arr(gS, True).ptr if want_mixing else None,
                                                     L.Arr(gU, True).ptr if want_mixing else None, gg)
    flat = np.array([[g.variance, g.lengthscale, g.mean] for g in gg])
    return rc, (val.value, gy, gs2.value, gS, gU, flat)


def test_shards_sum_to_the_whole(lmm, tol):
    """Matern32, Matern32, Matern52 (the first two share a launch): the shards [0, 1) and [1, 3) of the C ABI give partial sums of the
    whole, with the regulariser counted once by the caller's flag."""
    gps = [dict(GPS[1], mean=-0.2, lengthscale=0.9), GPS[1], GPS[2]]
    x, U, S, Y = GS.problem(333)
    y = Y.reshape(-1)
    rc, whole = abi_grad(lmm, gps, x, y, P_OUT, U, S, 0, 3, True)
    assert rc == 0
    parts = []
    for l0, l1 in ((0, 1), (1, 3)):
        rc, part = abi_grad(lmm, gps, x, y, P_OUT, U, S, l0, l1, l0 == 0)
        assert rc == 0
        assert (part[5][:l0] == 0).all() and (part[5][l1:] == 0).all()
        parts.append(part)
    close_value(parts[0][0] + parts[1][0], whole[0], tol)
    close_value(parts[0][2] + parts[1][2], whole[2], tol)
    for k in (1, 3, 4, 5):
        close(parts[0][k] + parts[1][k], whole[k], tol)
    fx = GS.model(lmm, U, S, gps)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    ref = lmm.logpdf_and_gradient(fx, y)
    close(whole[1], ref["y"], tol); close(whole[3], ref["S"], tol); close(whole[4].reshape(3, P_OUT).T, ref["U"], tol)


def test_gradient_refusals(lmm):
    from lmm_amd import _lib as L
    x, U, S, Y = GS.problem(63)
    y = Y.reshape(-1)
    f = GS.model(lmm, U, S)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    # grad_S / grad_U with NaN in y
    ynan = y.copy()
    ynan[5] = np.nan
    rc, _ = abi_grad(lmm, GPS, x, ynan, P_OUT, U, S, 0, 3, True)
    assert rc == L.LMM_ERR_UNSUPPORTED and b"NaN" in lib.lmm_last_error_string()
    rc, _ = abi_grad(lmm, GPS, x, ynan, P_OUT, U, S, 0, 3, True, want_mixing=False)
    assert rc == 0
    # a non-Matern latent, naming the latent
    se = [GPS[0], {"kind": "se", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0}, GPS[2]]
    rc, _ = abi_grad(lmm, se, x, y, P_OUT, U, S, 0, 3, True)
    assert rc == L.LMM_ERR_UNSUPPORTED
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert lat.value == 1 and b"latent 1" in lib.lmm_last_error_string()
    fse = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.Matern12Kernel()), lmm.GP(lmm.SEKernel()), lmm.GP(lmm.Matern52Kernel())]),
                   lmm.Orthogonal(U, S))
    with pytest.raises(NotImplementedError, match="latent 1"):
        lmm.statespace_logpdf_and_gradient(fse(xin, S2), y)
    # the fp32 compute mode
    lmm.set_compute_dtype("f32")
    try:
        with pytest.raises(NotImplementedError, match="Float64 only"):
            lmm.statespace_logpdf_and_gradient(f(xin, S2), y)
    finally:
        lmm.set_compute_dtype("f64")
    # and the next valid call is served
    got = lmm.statespace_logpdf_and_gradient(f(xin, S2), y)
    assert np.isfinite(got["value"]) and np.isfinite(got["y"]).all()
