"""-m gpu: state-space inference for Matern latents (include/lmm_hip.h "state space"): the filter and smoother
building blocks against the NumPy restatement of tests/test_statespace_abi.py, statespace_logpdf against the oracle and the library's
Cholesky path, NaN data against the missing-data path, statespace_mean_and_var against the exact posterior, and the refusals.

Tolerance (the rule of tests/test_gpu_sparse.py): max(1e-10, 100 DELTA) of max|reference| per array, and relative for a value, with
DELTA the largest disagreement between the restatement and the dense Gaussian (test_statespace_abi.delta(): 7.6e-15, so the
tolerance is 1e-10)."""
import ctypes as C

import numpy as np
import pytest

import test_statespace_abi as T

pytestmark = pytest.mark.gpu

BLOCK_N = (1, 2, 3, 63, 64, 65, 257, 1000)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * T.delta())


def close(got, ref, tol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    assert err <= tol * scale, (err, scale)


def close_value(got, ref, tol):
    assert np.isfinite(got) and abs(got - ref) <= tol * abs(ref), (got, ref)


# ---------------------------------------------------------------------------------------------------
# the building blocks
# ---------------------------------------------------------------------------------------------------
def kernel_of(lmm, kind, v, ell):
    return {"matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}[kind](v, ell)


def block_case(kind, n, unobserved):
    """test_statespace_abi.case, with (unobserved) the first and the last point unobserved and runs of unobserved points longer than
    a chunk of 7 (n >= 63) and of 64 (n >= 257)."""
    v, ell, x, w, r = T.case(kind, n, unobserved=unobserved)
    if unobserved:
        w[-1] = np.inf
        if n >= 63:
            w[20:40] = np.inf
        if n >= 257:
            w[100:180] = np.inf
    return v, ell, x, w, r


_REF = {}


def block_reference(kind, n, unobserved):
    key = (kind, n, unobserved)
    if key not in _REF:
        v, ell, x, w, r = block_case(kind, n, unobserved)
        _REF[key] = ((v, ell, x, w, r), T.statespace_reference(kind, v, ell, x, w, r))
    return _REF[key]


def gpu_blocks(lmm, kind, v, ell, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, wd, rd = dev(x), dev(w), dev(r)
    out = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]
    lml = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gp = L.gps_array([dict(kernel_of(lmm, kind, v, ell).desc(), mean=0.7)])      # the mean is not read
    lib = lmm.load()
    L.check(lib.lmm_dev_statespace_filter(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[0].data_ptr(),
                                          out[1].data_ptr(), lml.data_ptr()))
    L.check(lib.lmm_dev_statespace_smooth(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[2].data_ptr(),
                                          out[3].data_ptr()))
    return (float(lml.cpu()[0]),) + tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("kind", T.KINDS)
def test_filter_and_smoother_blocks(lmm, tol, kind, n, unobserved):
    (v, ell, x, w, r), ref = block_reference(kind, n, unobserved)
    results = {}
    for chunk in (1, 7, 64, 0, n, n + 3):
        got = gpu_blocks(lmm, kind, v, ell, x, w, r, chunk)
        close_value(got[0], ref[0], tol)
        for a, b in zip(got[1:], ref[1:]):
            close(a, b, tol)
        results[chunk] = got
    again = gpu_blocks(lmm, kind, v, ell, x, w, r, 7)
    assert again[0] == results[7][0] and all((a == b).all() for a, b in zip(again[1:], results[7][1:]))      # bitwise
    for chunk, got in results.items():              # different chunks agree
        close_value(got[0], results[0][0], tol)
        for a, b in zip(got[1:], results[0][1:]):
            close(a, b, tol)
    assert (results[n][1] == results[n + 3][1]).all()      # chunk >= n: one sequential thread either way


@pytest.mark.parametrize("kind", T.KINDS)
def test_aggregate_scan_recurses(lmm, tol, kind):
    """n = 5000 with chunk = 1: 5000 aggregates, 40 workgroups of the scan, whose totals are scanned by a second level."""
    (v, ell, x, w, r), ref = block_reference(kind, 5000, True)
    got = gpu_blocks(lmm, kind, v, ell, x, w, r, 1)
    close_value(got[0], ref[0], tol)
    for a, b in zip(got[1:], ref[1:]):
        close(a, b, tol)


def test_unsorted_inputs_are_refused_with_the_index(lmm):
    import torch
    from lmm_amd import _lib as L
    x = np.arange(300.0)
    x[211], x[57] = 1.0, 60.0             # x[57] >= x[56] still holds; x[58] < x[57] is the first violation
    xd = torch.tensor(x, device="cuda")
    o = torch.zeros(300, dtype=torch.float64, device="cuda")
    gp = L.gps_array([dict(lmm.Matern32Kernel().desc(), mean=0.0)])
    lib = lmm.load()
    rc = lib.lmm_dev_statespace_filter(xd.data_ptr(), 300, gp, o.data_ptr(), o.data_ptr(), 0, o.data_ptr(), o.data_ptr(), o.data_ptr())
    assert rc == L.LMM_ERR_ARG
    lat, info = C.c_int(), C.c_int()
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert info.value == 58 and b"x[58]" in lib.lmm_last_error_string()


# ---------------------------------------------------------------------------------------------------
# the OILMM entry points
# ---------------------------------------------------------------------------------------------------
GPS = [{"kind": "matern12", "variance": 1.2, "lengthscale": 0.8, "mean": 0.0},
       {"kind": "matern32", "variance": 0.7, "lengthscale": 1.3, "mean": 0.4},
       {"kind": "matern52", "variance": 1.5, "lengthscale": 0.6, "mean": 0.0}]
P_OUT, S2 = 5, 0.1


def model(lmm, U, S, gps=GPS):
    fs = lmm.independent_mogp([lmm.GP(g["mean"], kernel_of(lmm, g["kind"], g["variance"], g["lengthscale"])) for g in gps])
    return lmm.ILMM(fs, lmm.Orthogonal(U, S))


_PROBLEM = {}


def problem(n, p=P_OUT, seed=0):
    key = (n, p, seed)
    if key not in _PROBLEM:
        rng = np.random.default_rng([seed, n, p])
        m = len(GPS)
        x = np.sort(rng.uniform(0.0, 8.0, n))
        U = np.linalg.qr(rng.standard_normal((p, m)))[0]
        S = rng.uniform(0.5, 2.0, m)
        _PROBLEM[key] = (x, U, S, rng.standard_normal((p, n)))
    return _PROBLEM[key]


def oracle_logpdf(gps, U, S, x, s2, Y, with_reg):
    """oracle.oilmm_logpdf (src/oilmm.jl:79-93) with this module's Matern12 next to the oracle's Matern32 / Matern52."""
    O = T.O
    Tm, ST = O.project_orthogonal(U, S, s2)
    Ty = Tm @ Y
    n = len(x)
    val = sum(O.gaussian_logpdf(np.full(n, g["mean"]), T.matern_K(g["kind"], g["variance"], g["lengthscale"], x) + ST[l] * np.eye(n),
                                Ty[l]) for l, g in enumerate(gps))
    return float(val + (O.regulariser_oilmm(U, S, s2, Y) if with_reg else 0.0))


def test_oracle_restatement_is_the_oracle():
    x, U, S, Y = problem(63)
    got = oracle_logpdf(GPS[1:], U[:, 1:], S[1:], x, S2, Y, True)
    ref = T.O.oilmm_logpdf(GPS[1:], U[:, 1:], S[1:], x, S2, Y.reshape(-1))
    assert abs(got - ref) <= 1e-13 * abs(ref)


@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n", [1, 63, 333])
def test_logpdf_vs_oracle_and_cholesky_path(lmm, tol, n, with_reg):
    x, U, S, Y = problem(n)
    f = model(lmm, U, S)
    y = Y.reshape(-1)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    got = lmm.statespace_logpdf(fx, y, with_reg)
    close_value(got, oracle_logpdf(GPS, U, S, x, S2, Y, with_reg), tol)
    close_value(got, lmm.logpdf(fx, y, with_reg), tol)
    assert lmm.statespace_logpdf(fx, y, with_reg) == got                                 # bitwise
    perm = np.random.default_rng(n).permutation(n)                                       # unsorted inputs give the sorted result
    fxp = f(lmm.MOInputIsotopicByOutputs(x[perm], P_OUT), S2)
    assert lmm.statespace_logpdf(fxp, Y[:, perm].reshape(-1), with_reg) == got


def test_duplicated_inputs_are_served(lmm, tol):
    x, U, S, Y = problem(63)
    x = x.copy()
    x[10:13] = x[10]
    x[40] = x[41]
    fx = model(lmm, U, S)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    got = lmm.statespace_logpdf(fx, Y.reshape(-1))
    close_value(got, oracle_logpdf(GPS, U, S, x, S2, Y, True), tol)
    close_value(got, lmm.logpdf(fx, Y.reshape(-1)), tol)


def test_latents_of_one_kind_share_a_launch_and_shards_sum_to_the_whole(lmm, tol):
    """Matern32, Matern32, Matern52: the first two run in one launch (blockIdx.z = 0, 1).  Through the C ABI the shards [0, 1) and
    [1, 3) give partial sums of the whole (the regulariser and the noise counted once)."""
    from lmm_amd import _lib as L
    gps = [dict(GPS[1], mean=-0.2, lengthscale=0.9), GPS[1], GPS[2]]
    x, U, S, Y = problem(333)
    y = Y.reshape(-1)
    f = model(lmm, U, S, gps)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    whole = lmm.statespace_logpdf(f(xin, S2), y)
    close_value(whole, lmm.logpdf(f(xin, S2), y), tol)
    post = lmm.posterior(f(xin, S2), y)
    rm, rv = lmm.mean_and_var(post(xin, S2), False)
    gm, gv = lmm.statespace_mean_and_var(f(xin, S2), y, False)
    close(gm, rm, tol); close(gv, rv, tol)
    lib, arr = lmm.load(), L.gps_array(gps)
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    val, ms, vs = 0.0, np.zeros(333 * P_OUT), np.zeros(333 * P_OUT)
    for l0, l1 in ((0, 1), (1, 3)):
        out, mo, vo = C.c_double(), np.empty(333 * P_OUT), np.empty(333 * P_OUT)
        L.check(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, 333, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, arr, l0, l1, int(l0 == 0),
                                                C.byref(out)))
        L.check(lib.lmm_oilmm_mean_and_var_statespace(L.Arr(x).ptr, 333, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, arr, l0, l1, 0,
                                                      L.Arr(mo, True).ptr, L.Arr(vo, True).ptr))
        val, ms, vs = val + out.value, ms + mo, vs + vo
    close_value(val, whole, tol)
    close(ms, gm, tol); close(vs, gv, tol)


def test_launch_grouping_is_invisible_in_the_bits(lmm):
    """33 Matern32 latents, then 2 SHO: more entries of one model than a launch takes (LMM_MAX_BATCH = 32), and a model change between
    two kinds that share D = 2 but not a launch.  A launch is independent per latent, so however the entries are grouped the whole
    logpdf is bitwise the left-to-right sum of the 35 one-latent shards, and 12 posterior samples of the 3-latent shard [31, 34)
    (36 (latent, sample) entries across the model change) are bitwise the 12 one-sample calls on their slices of z, xi and eps."""
    from lmm_amd import _lib as L
    n, m = 63, 35
    p, N, l0, l1 = m, 12, 31, 34
    rng = np.random.default_rng(35)
    gps = [{"kind": "matern32", "variance": rng.uniform(0.5, 2.0), "lengthscale": rng.uniform(0.4, 1.6), "mean": rng.normal()} for _ in range(33)]
    gps += [{"kind": "sho", "variance": 1.1, "lengthscale": 1.7, "mean": 0.3, "quality": 2.0},
            {"kind": "sho", "variance": 0.8, "lengthscale": 0.9, "mean": -0.1, "quality": 0.7}]
    x = np.sort(rng.uniform(0.0, 8.0, n))
    U, S = np.linalg.qr(rng.standard_normal((p, m)))[0], rng.uniform(0.5, 2.0, m)
    y = rng.standard_normal(p * n)
    lib, arr, Ua, Sa = lmm.load(), L.gps_array(gps), L.Arr(L.colmajor(U)), L.Arr(S)

    def logpdf(a, b):
        out = C.c_double()
        L.check(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, S2, arr, a, b, 0, C.byref(out)))
        return out.value

    whole, val = logpdf(0, m), 0.0
    for l in range(m):
        val += logpdf(l, l + 1)
    assert np.isfinite(whole) and val == whole, (val, whole)

    zl = 2 * n * m                                                                       # every latent has D = 2
    z, xi, eps = rng.standard_normal((N, zl)), rng.standard_normal((N, m * n)), rng.standard_normal((N, n * p))

    def rand(q0, nq):
        o = np.full((nq, n * p), np.nan)
        L.check(lib.lmm_oilmm_rand_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, S2, arr, l0, l1, 1, nq,
                                              L.Arr(np.ascontiguousarray(z[q0:q0 + nq])).ptr, L.Arr(np.ascontiguousarray(xi[q0:q0 + nq])).ptr,
                                              L.Arr(np.ascontiguousarray(eps[q0:q0 + nq])).ptr, L.Arr(o, True).ptr))
        return o

    together = rand(0, N)
    assert np.isfinite(together).all()
    for q in range(N):
        assert np.array_equal(rand(q, 1)[0], together[q]), q


def nan_problem(n, p=7):
    """The patterns of tests/test_gpu_missing.py: its well-conditioned U and, per point, up to (p - m) // 2 deleted outputs."""
    import test_gpu_missing as GM
    x, U, S, Y = GM.problem(n, 1, p=p, m=len(GPS), seed=n)
    Y[1, n // 2] = np.nan                     # at least one, whatever the draw (that point keeps >= p - 3 outputs)
    assert np.isnan(Y).any() and (~np.isnan(Y)).sum(axis=0).min() >= len(GPS)
    return x, U, S, Y


@pytest.mark.parametrize("n", [64, 333])
def test_nan_vs_the_missing_data_path(lmm, tol, n):
    x, U, S, Y = nan_problem(n)
    p = Y.shape[0]
    f = model(lmm, U, S)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), S2)
    for with_reg in (True, False):
        got = lmm.statespace_logpdf(fx, Y.reshape(-1), with_reg)
        close_value(got, lmm.logpdf(fx, Y.reshape(-1), with_reg), tol)
    got = lmm.statespace_logpdf(fx, Y.reshape(-1))
    # all-NaN points leave the value unchanged: in front, between, equal to a training input, behind
    xe = np.array([x[0] - 1.0, 0.5 * (x[3] + x[4]), x[20], x[-1] + 2.0])
    x2 = np.concatenate([x, xe])
    Y2 = np.concatenate([Y, np.full((p, len(xe)), np.nan)], axis=1)
    got2 = lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(x2, p), S2), Y2.reshape(-1))
    close_value(got2, got, tol)
    close_value(got2, lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x2, p), S2), Y2.reshape(-1)), tol)


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("n", [1, 63, 333])
def test_mean_and_var_vs_exact_posterior(lmm, tol, n, nan):
    import torch
    if nan:
        x, U, S, Y = nan_problem(max(n, 2))           # (a single point with a NaN: n = 2)
    else:
        x, U, S, Y = problem(n)
    n, p = len(x), Y.shape[0]
    f = model(lmm, U, S)
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    y = Y.reshape(-1)
    post = lmm.posterior(f(xin, S2), y)
    xs = np.concatenate([np.linspace(x[0] - 0.7, x[-1] + 0.9, 11), x[:1]]) + 0.0        # new inputs, one equal to a training input
    xsin = lmm.MOInputIsotopicByOutputs(xs, p)
    mg = lmm.marginals(post(xin, S2))
    for add_noise in (True, False):
        rm, rv = lmm.mean_and_var(post(xin, S2), add_noise)
        gm, gv = lmm.statespace_mean_and_var(f(xin, S2), y, add_noise)
        close(gm, rm, tol); close(gv, rv, tol)
        if add_noise:
            close(gm, mg.mu, tol); close(gv, mg.sigma ** 2, tol)
        rms, rvs = lmm.mean_and_var(post(xsin, S2), add_noise)
        gms, gvs = lmm.statespace_mean_and_var(f(xin, S2), y, add_noise, xs=xs)
        assert gms.shape == (len(xs) * p,)
        close(gms, rms, tol); close(gvs, rvs, tol)
        # torch device inputs: device outputs, the same numbers
        xt, yt = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        tm, tv = lmm.statespace_mean_and_var(f(lmm.MOInputIsotopicByOutputs(xt, p), S2), yt, add_noise, xs=torch.tensor(xs, device="cuda"))
        assert tm.is_cuda and tv.is_cuda
        assert (tm.cpu().numpy() == gms).all() and (tv.cpu().numpy() == gvs).all()
    # unsorted training inputs: results come back in the callers' order
    perm = np.random.default_rng(n).permutation(n)
    pm, pv = lmm.statespace_mean_and_var(f(lmm.MOInputIsotopicByOutputs(x[perm], p), S2), Y[:, perm].reshape(-1))
    gm, gv = lmm.statespace_mean_and_var(f(xin, S2), y)
    assert (pm.reshape(p, n) == gm.reshape(p, n)[:, perm]).all() and (pv.reshape(p, n) == gv.reshape(p, n)[:, perm]).all()
    lt = lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(torch.tensor(x, device="cuda"), p), S2), torch.tensor(y, device="cuda"))
    assert lt == lmm.statespace_logpdf(f(xin, S2), y)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals(lmm):
    from lmm_amd import _lib as L
    x, U, S, Y = problem(63)
    y = Y.reshape(-1)
    f = model(lmm, U, S)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()

    def abi(gps):
        out = C.c_double()
        Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
        return lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 3, S2, L.gps_array(gps), 0, 3, 1,
                                               C.byref(out))

    # d = 2
    with pytest.raises(NotImplementedError, match="d = 2"):
        lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(np.zeros((2, 63)), P_OUT), S2), y)
    # an SE latent and a sum latent: the mirror, and the C ABI naming the latent
    se = [GPS[0], {"kind": "se", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0}, GPS[2]]
    ksum = [GPS[0], GPS[1], {"kind": "sum", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0, "terms": [dict(GPS[1], mean=0.0), GPS[2]]}]
    ard = [dict(GPS[0], lengthscale=np.array([0.8])), GPS[1], GPS[2]]
    for gps, bad in ((se, 1), (ksum, 2), (ard, 0)):
        assert abi(gps) == L.LMM_ERR_UNSUPPORTED
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        assert lat.value == bad and b"latent %d" % bad in lib.lmm_last_error_string()
    fse = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.Matern12Kernel()), lmm.GP(lmm.SEKernel()), lmm.GP(lmm.Matern52Kernel())]),
                   lmm.Orthogonal(U, S))
    fsum = lmm.ILMM(lmm.independent_mogp([lmm.GP(lmm.Matern12Kernel()), lmm.GP(lmm.Matern32Kernel()),
                                          lmm.GP(lmm.Matern32Kernel() + lmm.Matern52Kernel())]), lmm.Orthogonal(U, S))
    for fn in (lmm.statespace_logpdf, lmm.statespace_mean_and_var):
        with pytest.raises(NotImplementedError, match="latent 1"):
            fn(fse(xin, S2), y)
        with pytest.raises(NotImplementedError, match="latent 2"):
            fn(fsum(xin, S2), y)
    # the fp32 compute mode
    lmm.set_compute_dtype("f32")
    try:
        for fn in (lmm.statespace_logpdf, lmm.statespace_mean_and_var):
            with pytest.raises(NotImplementedError, match="Float64 only"):
                fn(f(xin, S2), y)
    finally:
        lmm.set_compute_dtype("f64")
    # 0 < p_t < m names the point; p_t = 0 is served
    few = Y.copy()
    few[:3, 17] = np.nan                      # p_t = 2 < m = 3
    for fn in (lmm.statespace_logpdf, lmm.statespace_mean_and_var):
        with pytest.raises(NotImplementedError, match="point 17 observes 2 outputs"):
            fn(f(xin, S2), few.reshape(-1))
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert (lat.value, info.value) == (-1, 17)
    few[:, 17] = np.nan
    assert np.isfinite(lmm.statespace_logpdf(f(xin, S2), few.reshape(-1)))
    # and the next valid call is served
    assert np.isfinite(lmm.statespace_logpdf(f(xin, S2), y))
