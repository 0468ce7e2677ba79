"""-m gpu: SHO (damped-oscillator) latents on the state-space and dense paths (include/lmm_hip.h LMM_KERNEL_SHO and "state space";
DESIGN.md 4.18): the filter, smoother, gradient and sampling building blocks against the NumPy restatement of tests/test_sho_abi.py,
statespace_logpdf / statespace_mean_and_var / statespace_logpdf_and_gradient / statespace_rand of an OILMM whose latents interleave
Matern and SHO kinds ([Matern32, SHO(Q = 3), Matern12, SHO(Q = 0.6)]: the two D = 2 models must not share a launch) against dense
Gaussians in NumPy and against the library's own dense verbs, and the dense path itself (Gram, logpdf, posterior marginals, rand and
logpdf_and_gradient of an OILMM, an IndependentMOGP and a dense-H ILMM) against dense Gaussians in NumPy.

Tolerances (the rule of tests/test_gpu_statespace.py): max(1e-10, 100 DELTA) of max|reference| per array, and relative for a value,
with DELTA measured by the restatement against the dense Gaussian in tests/test_sho_abi.py, never taken from the code under test:
delta() = 2.4e-13 (values and marginals: 1e-10), delta_grad() = 1.4e-12 (gradients: 1.5e-10), delta_rand() = 3.9e-14 (sampling:
1e-10).  Paths for fixed normals are compared at spacings of 0.5 - 2 periods; elsewhere only their law is pinned."""
import ctypes as C

import numpy as np
import pytest

import test_sho_abi as S
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
    return max(1e-10, 100.0 * S.delta())


@pytest.fixture(scope="module")
def tolg():
    return max(1e-10, 100.0 * S.delta_grad())


@pytest.fixture(scope="module")
def tolr():
    return max(1e-10, 100.0 * S.delta_rand())


def close(got, ref, tol, scale=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max() if scale is None else scale
    print(f"err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, (err, scale)


def close_value(got, ref, tol):
    print(f"got {got!r} ref {ref!r}")
    assert np.isfinite(got) and abs(got - ref) <= tol * abs(ref), (got, ref)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def nan_dev(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def gp_of(model):
    from lmm_amd import _lib as L
    return L.gps_array([model.desc(mean=0.7)])      # the mean is not read


# ---------------------------------------------------------------------------------------------------
# the filter and smoother blocks
# ---------------------------------------------------------------------------------------------------
def block_case(Q, n, unobserved):
    """test_sho_abi.case (ties in x for n >= 63), with (unobserved) the first and the last point unobserved and runs of unobserved
    points longer than a chunk of 7 (n >= 63) and of 64 (n >= 257)."""
    v, P, x, w, r = S.case(Q, n, unobserved=unobserved)
    if unobserved:
        w[-1] = np.inf
        if n >= 63:
            w[20:40] = np.inf
        if n >= 257:
            w[100:180] = np.inf
    return v, P, x, w, r


_REF = {}


def block_reference(Q, n, unobserved):
    key = (Q, n, unobserved)
    if key not in _REF:
        v, P, x, w, r = block_case(Q, n, unobserved)
        _REF[key] = ((v, P, x, w, r), S.statespace_reference(S.sho(v, P, Q), x, w, r))
    return _REF[key]


def gpu_blocks(lmm, model, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    xd, wd, rd = dev(x), dev(w), dev(r)
    out = [nan_dev(n) for _ in range(4)]
    lml = nan_dev(1)
    torch.cuda.synchronize()
    gp, lib = gp_of(model), lmm.load()
    L.check(lib.lmm_dev_statespace_filter(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[0].data_ptr(),
                                          out[1].data_ptr(), lml.data_ptr()))
    L.check(lib.lmm_dev_statespace_smooth(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, out[2].data_ptr(),
                                          out[3].data_ptr()))
    return (float(lml.cpu()[0]),) + tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("Q", S.QS)
def test_filter_and_smoother_blocks(lmm, tol, Q, n, unobserved):
    (v, P, x, w, r), ref = block_reference(Q, n, unobserved)
    model = S.sho(v, P, Q)
    results = {}
    for chunk in (1, 7, 64, 0, n, n + 3):
        got = gpu_blocks(lmm, model, x, w, r, chunk)
        close_value(got[0], ref[0], tol) if ref[0] != 0.0 else None
        assert ref[0] != 0.0 or got[0] == 0.0
        for a, b in zip(got[1:], ref[1:]):
            close(a, b, tol)
        results[chunk] = got
    again = gpu_blocks(lmm, model, x, w, r, 7)
    assert again[0] == results[7][0] and all((a == b).all() for a, b in zip(again[1:], results[7][1:]))      # bitwise
    for chunk, got in results.items():              # different chunks agree
        assert abs(got[0] - results[0][0]) <= tol * abs(results[0][0])
        for a, b in zip(got[1:], results[0][1:]):
            close(a, b, tol)
    assert (results[n][1] == results[n + 3][1]).all()      # chunk >= n: one sequential thread either way


def test_untagged_latent_has_quality_one(lmm, tol):
    """A kind-12 descriptor without "quality" carries no tag and runs Q = 1."""
    from lmm_amd import _lib as L
    import torch
    (v, P, x, w, r), _ = block_reference(2.0, 63, True)
    ref = S.statespace_reference(S.sho(v, P, 1.0), x, w, r)
    xd, wd, rd = dev(x), dev(w), dev(r)
    fm, fv, lml = nan_dev(63), nan_dev(63), nan_dev(1)
    gp = L.gps_array([{"kind": "sho", "variance": v, "lengthscale": P}])
    assert gp.ard.tags[0] == 0
    torch.cuda.synchronize()
    L.check(lmm.load().lmm_dev_statespace_filter(xd.data_ptr(), 63, gp, wd.data_ptr(), rd.data_ptr(), 0, fm.data_ptr(), fv.data_ptr(),
                                                 lml.data_ptr()))
    close_value(float(lml.cpu()[0]), ref[0], tol)
    close(fm.cpu().numpy(), ref[1], tol); close(fv.cpu().numpy(), ref[2], tol)


def test_aggregate_scan_recurses(lmm, tol):
    """n = 5000 with chunk = 1: 5000 aggregates, 40 workgroups of the scan, whose totals are scanned by a second level."""
    (v, P, x, w, r), ref = block_reference(2.0, 5000, True)
    got = gpu_blocks(lmm, S.sho(v, P, 2.0), x, w, r, 1)
    close_value(got[0], ref[0], tol)
    for a, b in zip(got[1:], ref[1:]):
        close(a, b, tol)


# ---------------------------------------------------------------------------------------------------
# the gradient block
# ---------------------------------------------------------------------------------------------------
def gpu_grad(lmm, model, x, w, r, chunk):
    """((lml, grad_r, grad_w, d/dv, d/dP, d/dQ) of lmm_dev_statespace_grad_sho, the two values of lmm_dev_statespace_grad, the
    filter's lml)."""
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    xd, wd, rd = dev(x), dev(w), dev(r)
    gr, gw, lml, gth, gth2, fm, fv, flml = nan_dev(n), nan_dev(n), nan_dev(1), nan_dev(3), nan_dev(2), nan_dev(n), nan_dev(n), nan_dev(1)
    gr2, gw2, lml2 = nan_dev(n), nan_dev(n), nan_dev(1)
    torch.cuda.synchronize()
    gp, lib = gp_of(model), lmm.load()
    L.check(lib.lmm_dev_statespace_grad_sho(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, lml.data_ptr(), gr.data_ptr(),
                                            gw.data_ptr(), gth.data_ptr()))
    L.check(lib.lmm_dev_statespace_grad(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, lml2.data_ptr(), gr2.data_ptr(),
                                        gw2.data_ptr(), gth2.data_ptr()))
    L.check(lib.lmm_dev_statespace_filter(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, fm.data_ptr(), fv.data_ptr(),
                                          flml.data_ptr()))
    th = gth.cpu().numpy()
    return ((float(lml.cpu()[0]), gr.cpu().numpy(), gw.cpu().numpy(), float(th[0]), float(th[1]), float(th[2])),
            gth2.cpu().numpy(), float(flml.cpu()[0]))


_GREF = {}


def grad_reference(Q, n, unobserved):
    key = (Q, n, unobserved)
    if key not in _GREF:
        v, P, x, w, r = block_case(Q, n, unobserved)
        _GREF[key] = ((v, P, x, w, r), S.statespace_grad_reference(v, P, Q, x, w, r))
    return _GREF[key]


def check_grad_block(got, ref, w, tolg):
    if ref[0] != 0.0:
        close_value(got[0], ref[0], tolg)
    close(got[1], ref[1], tolg, scale=max(np.abs(ref[1]).max(), 1e-300)); close(got[2], ref[2], tolg, scale=max(np.abs(ref[2]).max(), 1e-300))
    for k in (3, 4, 5):
        if ref[k] != 0.0:
            close_value(got[k], ref[k], tolg)
        else:
            assert got[k] == 0.0
    unobs = ~np.isfinite(w)
    assert (got[1][unobs] == 0).all() and (got[2][unobs] == 0).all()


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("Q", S.QS)
def test_gradient_block(lmm, tolg, Q, n, unobserved):
    (v, P, x, w, r), ref = grad_reference(Q, n, unobserved)
    model = S.sho(v, P, Q)
    results = {}
    for chunk in (1, 7, 64, 0, n):
        got, two, flml = gpu_grad(lmm, model, x, w, r, chunk)
        assert got[0] == flml                                                     # the value is the filter's, bitwise
        assert two[0] == got[3] and two[1] == got[4]                              # the two-value block: the same numbers
        check_grad_block(got, ref, w, tolg)
        results[chunk] = got
    again = gpu_grad(lmm, model, x, w, r, 7)[0]
    assert again[0] == results[7][0] and again[3:] == results[7][3:]             # bitwise
    assert (again[1] == results[7][1]).all() and (again[2] == results[7][2]).all()


def test_dual_scan_recurses(lmm, tolg):
    """n = 5000 with chunk = 1: 5000 (value, tangent) aggregates for each of the three seeds."""
    (v, P, x, w, r), ref = grad_reference(2.0, 5000, True)
    check_grad_block(gpu_grad(lmm, S.sho(v, P, 2.0), x, w, r, 1)[0], ref, w, tolg)


# ---------------------------------------------------------------------------------------------------
# the sampling blocks
# ---------------------------------------------------------------------------------------------------
def gpu_sample(lmm, model, x, Z, chunk, w=None, r=None, Xi=None):
    """lmm_dev_statespace_sample (w None) or _sample_posterior: Z (N, 2 n), Xi (N, n) -> (N, n)."""
    import torch
    from lmm_amd import _lib as L
    n, N = len(x), Z.shape[0]
    xd, zd = dev(x), dev(Z)
    f = nan_dev(N, n)
    torch.cuda.synchronize()
    if w is None:
        L.check(lmm.load().lmm_dev_statespace_sample(xd.data_ptr(), n, gp_of(model), zd.data_ptr(), N, chunk, f.data_ptr()))
    else:
        wd, rd, xid = dev(w), dev(r), dev(Xi)
        L.check(lmm.load().lmm_dev_statespace_sample_posterior(xd.data_ptr(), n, gp_of(model), wd.data_ptr(), rd.data_ptr(),
                                                               zd.data_ptr(), xid.data_ptr(), N, chunk, f.data_ptr()))
    return f.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 129, 1000])
@pytest.mark.parametrize("Q", S.QS)
def test_prior_block_vs_restatement(lmm, tolr, Q, n):
    v, P, x, zeta = S.rand_case(Q, n)
    model = S.sho(v, P, Q)
    ref = S.prior_path(model, x, zeta)
    Z = zeta.reshape(1, -1)
    got = {chunk: gpu_sample(lmm, model, x, Z, chunk)[0] for chunk in (1, 7, 64, 0, n)}
    for f in got.values():
        close(f, ref, tolr, scale=max(np.abs(ref).max(), np.sqrt(v)))
    assert (gpu_sample(lmm, model, x, Z, 7)[0] == got[7]).all()                  # bitwise
    dup = np.flatnonzero(np.diff(x) == 0.0) + 1          # an equal input repeats the state: bitwise within one thread's run
    assert (got[n][dup] == got[n][dup - 1]).all()
    # column q of an N-sample call is the single-sample call
    Z3 = np.vstack([Z, np.random.default_rng(n).standard_normal((2, 2 * n))])
    many = gpu_sample(lmm, model, x, Z3, 7)
    assert (many[0] == got[7]).all() and (many[2] == gpu_sample(lmm, model, x, Z3[2:], 7)[0]).all()


@pytest.mark.parametrize("Q", S.QS)
def test_law_of_the_prior_block(lmm, tolr, Q):
    """2 n unit vectors of normals as the samples of ONE call: M M' is the kernel matrix, small spacings included."""
    model = S.sho(S.RAND_V, S.RAND_P, Q)
    cases = [S.law_case(sp) for sp in S.LAW_SPACINGS] + [S.case(Q, 150, ties=True)[2]]
    for x in cases:
        n = len(x)
        for chunk in (7, 1):
            M = gpu_sample(lmm, model, x, np.eye(2 * n), chunk).T
            close(M @ M.T, model.K(x), tolr, scale=S.RAND_V)


def unobserved_runs(w, n):
    if n >= 2:
        w[0] = w[-1] = np.inf
    if n >= 17:
        w[3:12] = np.inf
    if n >= 257:
        w[100:180] = np.inf
    return w


@pytest.mark.parametrize("Q", S.QS)
def test_posterior_block(lmm, tol, tolr, Q):
    """Zero normals give the smoothed mean bitwise; the law of the posterior block (mean and covariance through the unit vectors of
    (zeta, xi)) is the dense posterior's at spacings 0.01 - 1 periods; for fixed normals at separated inputs it is the pathwise
    conditioning of the restatement."""
    for n in (17, 1000):
        v, P, x, w, r = S.case(Q, n)
        w = unobserved_runs(w, n)
        model = S.sho(v, P, Q)
        for chunk in (7, 0):
            f = gpu_sample(lmm, model, x, np.zeros((2, 2 * n)), chunk, w, r, np.zeros((2, n)))
            sm = gpu_blocks(lmm, model, x, w, r, chunk)[3]
            assert (f[0] == sm).all() and (f[1] == sm).all()                     # bitwise
    n = 40
    v, P, x, w, r = S.case(Q, n)
    w = unobserved_runs(w, n)
    w[20:30] = np.inf
    model = S.sho(v, P, Q)
    E = np.vstack([np.zeros((1, 3 * n)), np.eye(3 * n)])
    mu, Sg = S.dense_posterior(model, x, w, r)
    for chunk in (7, 1):
        f = gpu_sample(lmm, model, x, E[:, :2 * n], chunk, w, r, E[:, 2 * n:])
        close(f[0], mu, tolr)
        B = (f[1:] - f[:1]).T
        close(B @ B.T, Sg, tolr)
    for n in (1, 17, 1000):
        v, P, x, zeta = S.rand_case(Q, n)
        rng = np.random.default_rng([n, 5])
        w = unobserved_runs(rng.uniform(0.05, 0.5, n), n)
        r, xi = rng.standard_normal(n), rng.standard_normal(n)
        model = S.sho(v, P, Q)
        ref = S.pathwise_posterior(model, x, w, r, zeta, xi)
        for chunk in (7, 64, 0):
            close(gpu_sample(lmm, model, x, zeta.reshape(1, -1), chunk, w, r, xi.reshape(1, -1))[0], ref, tolr,
                  scale=max(np.abs(ref).max(), np.sqrt(v)))


# ---------------------------------------------------------------------------------------------------
# the OILMM entry points: Matern and SHO latents interleaved
# ---------------------------------------------------------------------------------------------------
MODELS = [S.Model("matern32", 0.7, 1.3), S.sho(1.2, 1.1, 3.0), S.Model("matern12", 1.5, 0.8), S.sho(0.9, 0.6, 0.6)]
MEANS = [0.4, 0.0, -0.3, 0.2]
P_OUT, S2 = 4, 0.1


def kernel_of(lmm, mdl):
    if mdl.kind == "sho":
        return lmm.SHOKernel(mdl.v, mdl.ell, mdl.quality)
    return {"matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}[mdl.kind](mdl.v, mdl.ell)


def oilmm(lmm, U, Sv, models=MODELS, means=MEANS):
    fs = lmm.independent_mogp([lmm.GP(mu, kernel_of(lmm, mdl)) for mdl, mu in zip(models, means)])
    return lmm.ILMM(fs, lmm.Orthogonal(U, Sv))


_PROBLEM = {}


def problem(n, seed=0):
    """Sorted inputs with a tie, an orthonormal U (p = m = 4), S and data."""
    if (n, seed) not in _PROBLEM:
        rng = np.random.default_rng([seed, n, 12])
        x = np.sort(rng.uniform(0.0, 8.0, n))
        if n > 10:
            x[7] = x[6]
        U = np.linalg.qr(rng.standard_normal((P_OUT, len(MODELS))))[0]
        _PROBLEM[(n, seed)] = (x, U, rng.uniform(0.5, 2.0, len(MODELS)), rng.standard_normal((P_OUT, n)))
    return _PROBLEM[(n, seed)]


def shuffled(n):
    """A permutation of the points that keeps the two tied inputs (6 and 7) in their order: the stable sort then hands the library
    the very same sequence of points, so results are bitwise those of the sorted call."""
    perm = np.random.default_rng(n).permutation(n)
    i, j = int(np.flatnonzero(perm == 6)[0]), int(np.flatnonzero(perm == 7)[0])
    if i > j:
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def projected(U, Sv, Y):
    """Per latent (w, r + mean): the OILMM projection of complete data, T = S^-1/2 U', noise sigma2 / S_l."""
    Tm, ST = T.O.project_orthogonal(U, Sv, S2)
    return Tm, ST, Tm @ Y


def dense_logpdf(x, U, Sv, Y, with_reg, models=MODELS, means=MEANS):
    _, ST, Ty = projected(U, Sv, Y)
    n = len(x)
    val = sum(T.O.gaussian_logpdf(np.full(n, mu), mdl.K(x) + ST[l] * np.eye(n), Ty[l]) for l, (mdl, mu) in enumerate(zip(models, means)))
    return float(val + (T.O.regulariser_oilmm(U, Sv, S2, Y) if with_reg else 0.0))


def restated_logpdf(x, U, Sv, Y, with_reg):
    _, ST, Ty = projected(U, Sv, Y)
    val = sum(S.kalman_filter(mdl, x, np.full(len(x), ST[l]), Ty[l] - mu)[0] for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)))
    return float(val + (T.O.regulariser_oilmm(U, Sv, S2, Y) if with_reg else 0.0))


def dense_marginals(x, U, Sv, Y, xs, add_noise):
    """mean_and_var(posterior(fx, y)(xs, sigma2)) by outputs, from a dense Gaussian per latent (reference src/oilmm.jl:56-76)."""
    _, ST, Ty = projected(U, Sv, Y)
    H = U * np.sqrt(Sv)[None, :]
    mean, var = np.zeros((P_OUT, len(xs))), np.zeros((P_OUT, len(xs)))
    for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)):
        G = np.linalg.solve(mdl.K(x) + ST[l] * np.eye(len(x)), mdl.K(x, xs))
        ml = mu + G.T @ (Ty[l] - mu)
        vl = mdl.v - np.einsum("ij,ij->j", mdl.K(x, xs), G)
        mean += np.outer(H[:, l], ml)
        var += np.outer(H[:, l] ** 2, vl)
    return mean.reshape(-1), (var + (S2 if add_noise else 0.0)).reshape(-1)


@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n", [63, 257])
def test_logpdf_vs_restatement_and_dense_gaussian(lmm, tol, n, with_reg):
    x, U, Sv, Y = problem(n)
    f = oilmm(lmm, U, Sv)
    y = Y.reshape(-1)
    got = lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y, with_reg)
    close_value(got, restated_logpdf(x, U, Sv, Y, with_reg), tol)
    close_value(got, dense_logpdf(x, U, Sv, Y, with_reg), tol)
    close_value(got, lmm.logpdf(f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y, with_reg), tol)      # the library's dense path
    assert lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y, with_reg) == got      # bitwise
    perm = shuffled(n)                              # unsorted inputs (with the tie) give the sorted result
    assert lmm.statespace_logpdf(f(lmm.MOInputIsotopicByOutputs(x[perm], P_OUT), S2), Y[:, perm].reshape(-1), with_reg) == got
    # every order of the latents gives the sum of the same per-latent terms
    order = [3, 1, 0, 2]
    f2 = oilmm(lmm, U[:, order], Sv[order], [MODELS[k] for k in order], [MEANS[k] for k in order])
    close_value(lmm.statespace_logpdf(f2(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y, with_reg), got, tol)


def test_sho_alone_and_matern_regression(lmm, tol):
    """Only SHO latents; and the Matern latents of the mixed model alone give what they gave before."""
    x, U, Sv, Y = problem(63)
    y = Y.reshape(-1)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    for keep in ([1, 3], [0, 2]):
        models, means = [MODELS[k] for k in keep], [MEANS[k] for k in keep]
        fx = oilmm(lmm, U[:, keep], Sv[keep], models, means)(xin, S2)
        got = lmm.statespace_logpdf(fx, y)
        close_value(got, dense_logpdf(x, U[:, keep], Sv[keep], Y, True, models, means), tol)
        close_value(got, lmm.logpdf(fx, y), tol)


@pytest.mark.parametrize("n", [63, 257])
def test_mean_and_var_vs_dense_posterior(lmm, tol, n):
    import torch
    x, U, Sv, Y = problem(n)
    f = oilmm(lmm, U, Sv)
    y = Y.reshape(-1)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    xs = np.concatenate([np.linspace(x[0] - 0.7, x[-1] + 0.9, 11), x[:1]]) + 0.0        # new inputs, one equal to a training input
    for add_noise in (True, False):
        gm, gv = lmm.statespace_mean_and_var(f(xin, S2), y, add_noise)
        rm, rv = dense_marginals(x, U, Sv, Y, x, add_noise)
        close(gm, rm, tol); close(gv, rv, tol)
        gms, gvs = lmm.statespace_mean_and_var(f(xin, S2), y, add_noise, xs=xs)
        rms, rvs = dense_marginals(x, U, Sv, Y, xs, add_noise)
        assert gms.shape == (len(xs) * P_OUT,)
        close(gms, rms, tol); close(gvs, rvs, tol)
        post = lmm.posterior(f(xin, S2), y)                                          # the library's dense path
        lm, lv = lmm.mean_and_var(post(xin, S2), add_noise)
        close(gm, lm, tol); close(gv, lv, tol)
        lms, lvs = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2), add_noise)
        close(gms, lms, tol); close(gvs, lvs, tol)
    tm, tv = lmm.statespace_mean_and_var(f(lmm.MOInputIsotopicByOutputs(torch.tensor(x, device="cuda"), P_OUT), S2),
                                         torch.tensor(y, device="cuda"), False, xs=torch.tensor(xs, device="cuda"))
    assert tm.is_cuda and (tm.cpu().numpy() == gms).all() and (tv.cpu().numpy() == gvs).all()
    perm = shuffled(n)                              # unsorted inputs: results in the callers' order
    pm, pv = lmm.statespace_mean_and_var(f(lmm.MOInputIsotopicByOutputs(x[perm], P_OUT), S2), Y[:, perm].reshape(-1))
    gm, gv = lmm.statespace_mean_and_var(f(xin, S2), y)
    assert (pm.reshape(P_OUT, n) == gm.reshape(P_OUT, n)[:, perm]).all() and (pv.reshape(P_OUT, n) == gv.reshape(P_OUT, n)[:, perm]).all()


def nan_front(U, Sv, Y):
    """The missing-data front end restated for p = m (every G_t over all outputs; a point is complete or has no output at all is not
    what it is for): per point with observed outputs O, z_t = G_t^-1 H_O' y_O and noise sigma2 diag(G_t^-1), G_t = H_O' H_O."""
    H = U * np.sqrt(Sv)[None, :]
    m, n = H.shape[1], Y.shape[1]
    w, z = np.full((m, n), np.inf), np.zeros((m, n))
    for t in range(n):
        O = ~np.isnan(Y[:, t])
        if O.any():
            Gi = np.linalg.inv(H[O].T @ H[O])
            z[:, t], w[:, t] = Gi @ H[O].T @ Y[O, t], S2 * np.diag(Gi)
    return w, z


def test_nan_data(lmm, tol):
    """p = 6 outputs over m = 4 latents with scattered NaN (every point keeps >= m outputs) and points without any output: the value
    without the regulariser and the marginals against the restatement on the front end's pseudo-observations; the regulariser's
    share does not depend on the kernels, so it equals that of the all-Matern model, which the dense missing-data path serves."""
    n, p = 63, 6
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 8.0, n))
    U = np.linalg.qr(rng.standard_normal((p, 4)))[0]
    Sv = rng.uniform(0.5, 2.0, 4)
    Y = rng.standard_normal((p, n))
    for t in range(0, n, 3):
        Y[rng.choice(p, rng.integers(1, 3), replace=False), t] = np.nan
    Y[:, [0, 30, 31, n - 1]] = np.nan                      # predict-only points, the first and the last among them
    assert min(c for c in (~np.isnan(Y)).sum(axis=0) if c) >= 4
    fs = lmm.independent_mogp([lmm.GP(mu, kernel_of(lmm, mdl)) for mdl, mu in zip(MODELS, MEANS)])
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    fx = lmm.ILMM(fs, lmm.Orthogonal(U, Sv))(xin, S2)
    w, z = nan_front(U, Sv, Y)
    got = lmm.statespace_logpdf(fx, Y.reshape(-1), False)
    ref = sum(S.kalman_filter(mdl, x, w[l], z[l] - mu)[0] for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)))
    close_value(got, ref, tol)
    mat = [S.Model("matern32", 1.0, 1.0)] * 4
    fm = lmm.ILMM(lmm.independent_mogp([lmm.GP(mu, kernel_of(lmm, k)) for k, mu in zip(mat, MEANS)]), lmm.Orthogonal(U, Sv))(xin, S2)
    reg_matern = lmm.statespace_logpdf(fm, Y.reshape(-1), True) - lmm.statespace_logpdf(fm, Y.reshape(-1), False)
    reg_dense = lmm.logpdf(fm, Y.reshape(-1), True) - lmm.logpdf(fm, Y.reshape(-1), False)
    reg = lmm.statespace_logpdf(fx, Y.reshape(-1), True) - got
    assert abs(reg - reg_matern) <= tol * abs(reg) and abs(reg - reg_dense) <= 1e-9 * abs(reg)
    gm, gv = lmm.statespace_mean_and_var(fx, Y.reshape(-1), True)
    H = U * np.sqrt(Sv)[None, :]
    rm, rv = np.zeros((p, n)), np.zeros((p, n))
    for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)):
        _, _, _, sm, sv = S.statespace_reference(mdl, x, w[l], z[l] - mu)
        rm += np.outer(H[:, l], sm + mu); rv += np.outer(H[:, l] ** 2, sv)
    close(gm, rm.reshape(-1), tol); close(gv, (rv + S2).reshape(-1), tol)
    # the dense missing-data path: value with and without the regulariser, marginals, gradient
    for with_reg in (True, False):
        close_value(lmm.statespace_logpdf(fx, Y.reshape(-1), with_reg), lmm.logpdf(fx, Y.reshape(-1), with_reg), tol)
    dm, dv = lmm.mean_and_var(lmm.posterior(fx, Y.reshape(-1))(xin, S2))
    close(gm, dm, tol); close(gv, dv, tol)
    gs, gd = lmm.statespace_logpdf_and_gradient(fx, Y.reshape(-1)), lmm.logpdf_and_gradient(fx, Y.reshape(-1))
    tg = max(1e-10, 100.0 * S.delta_grad())
    close_value(gs["value"], gd["value"], tg); close(gs["y"], gd["y"], tg); close_value(gs["sigma2"], gd["sigma2"], tg)
    for a, b in zip(gs["gps"], gd["gps"]):
        assert set(a) == set(b)
        for key in b:
            close_value(a[key], b[key], tg)


def dense_gradient(x, U, Sv, Y):
    """Value and gradient of the OILMM logpdf WITHOUT the regulariser, analytically from dense Gaussians: per latent the dense
    gradient with respect to (r, w, kernel parameters) of tests/test_sho_abi.py and tests/test_statespace_grad_abi.py, then the chain
    rule of r_l = (S^-1/2 U' y)_l - mean_l and w_l = sigma2 / S_l."""
    import test_statespace_grad_abi as TG
    Tm, ST, Ty = projected(U, Sv, Y)
    n = len(x)
    out = {"value": 0.0, "y": np.zeros_like(Y), "sigma2": 0.0, "S": np.zeros(len(MODELS)), "U": np.zeros_like(U), "gps": []}
    for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)):
        w, r = np.full(n, ST[l]), Ty[l] - mu
        if mdl.kind == "sho":
            val, gr, gw, gv, gl, gq = S.dense_grad_reference(mdl.v, mdl.ell, mdl.quality, x, w, r)
        else:
            val, gr, gw, gv, gl = TG.dense_grad_reference(mdl.kind, mdl.v, mdl.ell, x, w, r)
        out["value"] += val
        out["y"] += np.outer(Tm[l], gr)
        out["sigma2"] += gw.sum() / Sv[l]
        out["S"][l] = -gw.sum() * S2 / Sv[l] ** 2 - 0.5 * (gr @ Ty[l]) / Sv[l]
        out["U"][:, l] = Y @ gr / np.sqrt(Sv[l])
        g = {"variance": gv, "lengthscale": gl, "mean": -gr.sum()}
        if mdl.kind == "sho":
            g["quality"] = gq
        out["gps"].append(g)
    out["y"] = out["y"].reshape(-1)
    return out


def check_dict(got, ref, tolg):
    close_value(got["value"], ref["value"], tolg)
    close(got["y"], ref["y"], tolg)
    close_value(got["sigma2"], ref["sigma2"], tolg)
    close(got["S"], ref["S"], tolg); close(got["U"], ref["U"], tolg)
    assert len(got["gps"]) == len(ref["gps"])
    for a, b in zip(got["gps"], ref["gps"]):
        assert set(a) == set(b)                                                  # "quality" exactly for the SHO latents
        for key in b:
            close_value(a[key], b[key], tolg)


@pytest.mark.parametrize("n", [63, 257])
def test_gradient_vs_dense_analytic_gradient(lmm, tolg, n):
    x, U, Sv, Y = problem(n)
    f = oilmm(lmm, U, Sv)
    y = Y.reshape(-1)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    got = lmm.statespace_logpdf_and_gradient(f(xin, S2), y, False)
    assert set(got) == {"value", "y", "sigma2", "S", "U", "gps"}
    assert [sorted(g) for g in got["gps"]] == [["lengthscale", "mean", "variance"], ["lengthscale", "mean", "quality", "variance"]] * 2
    check_dict(got, dense_gradient(x, U, Sv, Y), tolg)
    assert got["value"] == lmm.statespace_logpdf(f(xin, S2), y, False)                   # bitwise
    check_dict(got, lmm.logpdf_and_gradient(f(xin, S2), y, False), tolg)                 # the library's dense path
    full = lmm.statespace_logpdf_and_gradient(f(xin, S2), y, True)
    assert full["value"] == lmm.statespace_logpdf(f(xin, S2), y, True)
    assert full["gps"] == got["gps"]
    check_dict(full, lmm.logpdf_and_gradient(f(xin, S2), y, True), tolg)
    # unsorted inputs give the sorted result, with "y" in the callers' order
    perm = shuffled(n)
    gp = lmm.statespace_logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x[perm], P_OUT), S2), Y[:, perm].reshape(-1), False)
    assert gp["value"] == got["value"] and gp["gps"] == got["gps"]
    assert (gp["y"].reshape(P_OUT, n) == got["y"].reshape(P_OUT, n)[:, perm]).all()


def test_quality_gradient_reaches_the_tag_and_shards_sum(lmm, tolg):
    """Through the C ABI: lmm_kernel_tag_quality_grad after a gradient call, zero after a call without grad_gps, and the shards [0, 2)
    and [2, 4) give partial sums of the whole."""
    from lmm_amd import _lib as L
    x, U, Sv, Y = problem(63)
    y = Y.reshape(-1)
    ref = dense_gradient(x, U, Sv, Y)
    lib = lmm.load()
    arr = L.gps_array([mdl.desc(mu) for mdl, mu in zip(MODELS, MEANS)])
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(Sv)

    def call(l0, l1, want_gps=True):
        val, gg = C.c_double(), (L.GpGradT * 4)()
        L.check(lib.lmm_oilmm_logpdf_grad_statespace(L.Arr(x).ptr, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, S2, arr, l0, l1, 0,
                                                     C.byref(val), None, None, None, None, gg if want_gps else None))
        return val.value, gg, [arr.ard.quality_grad(l) if arr.ard.has_quality[l] else None for l in range(4)]

    val, gg, gq = call(0, 4)
    close_value(val, ref["value"], tolg)
    for l in (1, 3):
        close_value(gq[l], ref["gps"][l]["quality"], tolg)
        close_value(gg[l].lengthscale, ref["gps"][l]["lengthscale"], tolg)
    assert gq[0] is None and gq[2] is None
    va, _, qa = call(0, 2)
    vb, _, qb = call(2, 4)
    close_value(va + vb, val, tolg)
    assert qa[1] == gq[1] and qa[3] == 0.0 and qb[3] == gq[3] and qb[1] == 0.0
    assert call(0, 4, want_gps=False)[2] == [None, 0.0, None, 0.0]


class Recorder:
    """A NumPy Generator that keeps what it drew."""

    def __init__(self, seed):
        self.rng, self.draws = np.random.default_rng(seed), []

    def standard_normal(self, count):
        self.draws.append(self.rng.standard_normal(count))
        return self.draws[-1]


def test_statespace_rand(lmm, tolr):
    """The prior for fixed normals against the restated paths at well-separated inputs; the posterior at new inputs against pathwise
    conditioning in NumPy; column q of an N-sample call is the single-sample call; bitwise repeatability."""
    n, m, p = 50, len(MODELS), P_OUT
    x = S.rand_case(2.0, n)[2]
    _, U, Sv, _ = problem(63)
    H = U * np.sqrt(Sv)[None, :]
    fx = oilmm(lmm, U, Sv)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    for add_noise in (True, False):
        rec = Recorder(11)
        out = lmm.statespace_rand(rec, fx, add_noise=add_noise)
        assert out.shape == (n * p,) and len(rec.draws) == m + int(add_noise)
        assert [d.size for d in rec.draws[:m]] == [mdl.D * n for mdl in MODELS]
        F = np.stack([mu + S.prior_path(mdl, x, rec.draws[l].reshape(mdl.D, n)) for l, (mdl, mu) in enumerate(zip(MODELS, MEANS))])
        ref = H @ F + (np.sqrt(S2) * rec.draws[m].reshape(p, n) if add_noise else 0.0)
        close(out, ref.reshape(-1), tolr)
        assert (lmm.statespace_rand(Recorder(11), fx, add_noise=add_noise) == out).all()                 # bitwise
    # posterior at the training inputs and at new ones, N = 3
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((p, n))
    xs = np.array([x[0] - 0.4, 0.5 * (x[3] + x[4]), x[10], x[-1] + 1.0])
    rec = Recorder(12)
    out = lmm.statespace_rand(rec, fx, Y.reshape(-1), N=3, add_noise=False, xs=xs)
    assert out.shape == (len(xs) * p, 3) and len(rec.draws) == 3 * (m + 1)
    xa = np.concatenate([x, xs])
    perm = np.argsort(xa, kind="stable")
    xsort, na = xa[perm], n + len(xs)
    _, ST, Ty = projected(U, Sv, Y)
    new = np.flatnonzero(perm >= n)
    for q in range(3):
        draws = rec.draws[q * (m + 1):(q + 1) * (m + 1)]
        F = np.zeros((m, na))
        for l, (mdl, mu) in enumerate(zip(MODELS, MEANS)):
            w, r = np.full(na, np.inf), np.zeros(na)
            w[perm < n], r[perm < n] = ST[l], (Ty[l] - mu)[perm[perm < n]]
            F[l] = mu + S.pathwise_posterior(mdl, xsort, w, r, draws[l].reshape(mdl.D, na), draws[m].reshape(m, na)[l])
        ref = (H @ F)[:, new][:, np.argsort(perm[new])]
        close(out[:, q], ref.reshape(-1), tolr)

    class Replay:
        def __init__(self, draws):
            self.draws = list(draws)

        def standard_normal(self, count):
            return self.draws.pop(0)

    one = lmm.statespace_rand(Replay(rec.draws[m + 1:2 * (m + 1)]), fx, Y.reshape(-1), add_noise=False, xs=xs)
    assert (one == out[:, 1]).all()


# ---------------------------------------------------------------------------------------------------
# the dense path
# ---------------------------------------------------------------------------------------------------
def gram(lmm, gp, x, diag=0.25):
    """lmm_dev_gram of one latent descriptor over the (n,) inputs x: the lower triangle of K + diag I."""
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    NR = (n + 63) // 64 * 64
    ld = NR + 16
    A = nan_dev(NR, ld)
    xd = dev(x)
    torch.cuda.synchronize()
    rc = lmm.load().lmm_dev_gram(C.c_void_p(A.data_ptr()), ld, NR, NR, C.c_void_p(xd.data_ptr()), 1, n, L.gps_array([gp]), C.c_double(diag))
    assert rc == 0, lmm.load().lmm_last_error_string()
    return A.T.cpu().numpy()[:n, :n]


def gram_inputs(n):
    """Unsorted inputs over 40 periods with a tie (n >= 2)."""
    x = np.random.default_rng([n, 4]).uniform(0.0, 30.0, n)
    if n >= 2:
        x[n // 2] = x[0]
    return x


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("Q", S.QS)
def test_dense_gram(lmm, tol, Q, n):
    """Element-wise against k_sho: the generic tiles (n = 1, 63) and interior tiles next to border ones (n = 130)."""
    x = gram_inputs(n)
    mdl = S.sho(1.7, 0.75, Q)
    il = np.tril_indices(n)
    close(gram(lmm, mdl.desc(), x)[il], (mdl.K(x) + 0.25 * np.eye(n))[il], tol)


def test_dense_gram_untagged_latent_has_quality_one(lmm, tol):
    """A kind-12 descriptor without a tag is the Q = 1 oscillator, not another kernel."""
    x = gram_inputs(130)
    il = np.tril_indices(130)
    got = gram(lmm, {"kind": "sho", "variance": 1.7, "lengthscale": 0.75}, x)[il]
    close(got, (S.sho(1.7, 0.75, 1.0).K(x) + 0.25 * np.eye(130))[il], tol)
    m52 = 1.7 * (lambda s: (1 + s + s * s / 3) * np.exp(-s))(np.sqrt(5.0) * np.abs(x[:, None] - x[None, :]) / 0.75)
    assert np.abs(got - (m52 + 0.25 * np.eye(130))[il]).max() > 0.1


# The dense-H path projects with (H' H / sigma2 + 1e-9 I)^-1, as the reference does (src/ilmm.jl:63): against the naive Gaussian that is
# a relative change of 1e-9 sigma2 / lambda_min(H' H) in the projected noise.  This H (lambda_min(H' H) = 3.4) and DENSE_S2 make it
# 3e-12, below the tolerance; at sigma2 = 0.1 and half this H it would be 1e-10 and the naive Gaussian no reference.
DENSE_H = 2.0 * np.array([[1.0, 0.3], [-0.4, 0.8], [0.6, 0.5]])
DENSE_S2 = 0.01
DENSE_MODELS, DENSE_MEANS = [MODELS[1], MODELS[3]], [0.0, 0.2]


def dense_models(lmm, which, n):
    """(model, H as the naive Gaussian sees it, latent models, means, inputs with a tie, data by outputs, sigma2) of the three model
    kinds."""
    x, U, Sv, Y = problem(n)
    if which == "oilmm":
        return oilmm(lmm, U, Sv), U * np.sqrt(Sv)[None, :], MODELS, MEANS, x, Y.reshape(-1), S2
    if which == "mogp":
        fs = lmm.independent_mogp([lmm.GP(mu, kernel_of(lmm, mdl)) for mdl, mu in zip(MODELS, MEANS)])
        return fs, np.eye(4), MODELS, MEANS, x, Y.reshape(-1), S2
    fs = lmm.independent_mogp([lmm.GP(mu, kernel_of(lmm, mdl)) for mdl, mu in zip(DENSE_MODELS, DENSE_MEANS)])
    return lmm.ILMM(fs, DENSE_H), DENSE_H, DENSE_MODELS, DENSE_MEANS, x, Y[:3].reshape(-1), DENSE_S2


def naive_cov(models, H, x, x2=None):
    """sum_l h_l h_l' (x) K_l, by outputs."""
    return sum(np.kron(np.outer(H[:, l], H[:, l]), mdl.K(x, x2)) for l, mdl in enumerate(models))


def naive_mean(means, H, n):
    return np.repeat(H @ np.asarray(means), n)


@pytest.mark.parametrize("n", [63, 130])
@pytest.mark.parametrize("which", ["oilmm", "mogp", "dense"])
def test_dense_logpdf_and_posterior_marginals(lmm, tol, which, n):
    """logpdf and mean_and_var(posterior(fx, y)(xs, sigma2)) against the naive Gaussian over all outputs."""
    f, H, models, means, x, y, s2 = dense_models(lmm, which, n)
    p = H.shape[0]
    xin = lmm.MOInputIsotopicByOutputs(x, p)
    Cn = naive_cov(models, H, x) + s2 * np.eye(n * p)
    close_value(lmm.logpdf(f(xin, s2), y), float(T.O.gaussian_logpdf(naive_mean(means, H, n), Cn, y)), tol)
    xs = np.concatenate([np.linspace(x[0] - 0.7, x[-1] + 0.9, 11), x[:1]]) + 0.0
    Cs = naive_cov(models, H, x, xs)
    G = np.linalg.solve(Cn, Cs)
    rm = naive_mean(means, H, len(xs)) + G.T @ (y - naive_mean(means, H, n))
    rv = np.diag(naive_cov(models, H, xs)) - np.einsum("ij,ij->j", Cs, G) + s2
    post = lmm.posterior(f(xin, s2), y)
    gm, gv = lmm.mean_and_var(post(lmm.MOInputIsotopicByOutputs(xs, p), s2))
    close(gm, rm, tol); close(gv, rv, tol)
    assert lmm.marginals(post(lmm.MOInputIsotopicByOutputs(xs, p), s2)) is not None
    close(lmm.mean(post(lmm.MOInputIsotopicByOutputs(xs, p), s2)), rm, tol)
    close(lmm.var(post(lmm.MOInputIsotopicByOutputs(xs, p), s2)), rv, tol)


@pytest.mark.parametrize("n", [63, 130])
@pytest.mark.parametrize("which", ["oilmm", "mogp", "dense"])
def test_dense_rand_fixed_normals(lmm, tolr, which, n):
    """rand for recorded normals against m + chol(K + jitter I) z per latent, mixed and with noise added as the reference does (jitter:
    1e-18 for an OILMM, 1e-12 for a dense-H ILMM, sigma2 for an IndependentMOGP, which adds no further noise).  Inputs 0.5 - 2 apart
    (periods are 0.6 and 1.1): the Cholesky factor of a Gram matrix of close inputs amplifies the rounding of its elements, and only the
    law, not the path, is then defined to the tolerance."""
    f, H, models, means, _, _, s2 = dense_models(lmm, which, n)
    x = np.cumsum(np.random.default_rng([n, 8]).uniform(0.5, 2.0, n))
    p, m = H.shape
    rec = Recorder(21)
    out = lmm.rand(rec, f(lmm.MOInputIsotopicByOutputs(x, p), s2))
    z = rec.draws[0] if len(rec.draws) <= 2 else np.concatenate(rec.draws[:m])
    jit = {"oilmm": T.O.JITTER_DEFAULT, "dense": T.O.JITTER_ILMM_RAND, "mogp": s2}[which]
    F = np.stack([mu + np.linalg.cholesky(mdl.K(x) + jit * np.eye(n)) @ z.reshape(-1)[l * n:(l + 1) * n]
                  for l, (mdl, mu) in enumerate(zip(models, means))])
    ref = (H @ F).reshape(-1)
    if which != "mogp":
        ref = ref + np.sqrt(s2) * np.concatenate(rec.draws).reshape(-1)[m * n:]
    close(out, ref, tolr)


def naive_gradient(models, means, H, x, y, s2):
    """Value and gradient of the naive Gaussian with respect to y, sigma2, H and every SHO latent's (variance, period, quality, mean):
    with A = alpha alpha' - C^-1, d/d theta = tr(A dC / d theta) / 2 and dC / d H_ol = (e_o h_l' + h_l e_o') (x) K_l."""
    n, (p, m) = len(x), H.shape
    Cn = naive_cov(models, H, x) + s2 * np.eye(n * p)
    Ci = np.linalg.inv(Cn)
    Ci = 0.5 * (Ci + Ci.T)
    mean = naive_mean(means, H, n)
    alpha = Ci @ (y - mean)
    A = np.outer(alpha, alpha) - Ci
    out = {"value": float(T.O.gaussian_logpdf(mean, Cn, y)), "y": -alpha, "sigma2": 0.5 * np.trace(A), "H": np.zeros((p, m)), "gps": []}
    tau = np.abs(x[:, None] - x[None, :])
    Ab = A.reshape(p, n, p, n)
    for l, (mdl, mu) in enumerate(zip(models, means)):
        hh = np.outer(H[:, l], H[:, l])
        dv, dP, dQ = (0.5 * np.sum(A * np.kron(hh, dK)) for dK in S.dk_sho(mdl.v, mdl.ell, mdl.quality, tau))
        out["gps"].append({"variance": dv, "lengthscale": dP, "quality": dQ, "mean": float(alpha @ np.repeat(H[:, l], n))})
        K = mdl.K(x)
        for o in range(p):
            out["H"][o, l] = sum(H[o2, l] * np.sum(Ab[o, :, o2, :] * K) for o2 in range(p)) + mu * alpha[o * n:(o + 1) * n].sum()
    return out


@pytest.mark.parametrize("n", [63, 130])
def test_dense_gradient_oilmm_and_tag(lmm, tolg, n):
    """logpdf_and_gradient of the OILMM against the dense analytic gradient; then through the C ABI, lmm_kernel_tag_quality_grad after
    the gradient call."""
    from lmm_amd import _lib as L
    x, U, Sv, Y = problem(n)
    y = Y.reshape(-1)
    ref = dense_gradient(x, U, Sv, Y)
    got = lmm.logpdf_and_gradient(oilmm(lmm, U, Sv)(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), y, False)
    check_dict(got, ref, tolg)
    lib = lmm.load()
    arr = L.gps_array([mdl.desc(mu) for mdl, mu in zip(MODELS, MEANS)])
    val, gg = C.c_double(), (L.GpGradT * 4)()
    L.check(lib.lmm_oilmm_logpdf_grad(L.Arr(x).ptr, 1, n, L.Arr(y).ptr, P_OUT, L.Arr(L.colmajor(U)).ptr, L.Arr(Sv).ptr, 4, C.c_double(S2),
                                      arr, 0, 4, 0, C.byref(val), None, None, None, None, gg))
    close_value(val.value, ref["value"], tolg)
    for l in (1, 3):
        close_value(arr.ard.quality_grad(l), ref["gps"][l]["quality"], tolg)
        close_value(gg[l].lengthscale, ref["gps"][l]["lengthscale"], tolg)
        close_value(gg[l].variance, ref["gps"][l]["variance"], tolg)


@pytest.mark.parametrize("n", [63, 130])
def test_dense_gradient_mogp(lmm, tolg, n):
    """An IndependentMOGP is a sum over its latents: each against the dense analytic gradient at noise sigma2."""
    import test_statespace_grad_abi as TG
    f, _, models, means, x, y, _ = dense_models(lmm, "mogp", n)
    got = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, 4), S2), y)
    val, gy, gs2 = 0.0, [], 0.0
    for l, (mdl, mu) in enumerate(zip(models, means)):
        w, r = np.full(n, S2), y[l * n:(l + 1) * n] - mu
        if mdl.kind == "sho":
            v, gr, gw, gv, gl, gq = S.dense_grad_reference(mdl.v, mdl.ell, mdl.quality, x, w, r)
        else:
            v, gr, gw, gv, gl = TG.dense_grad_reference(mdl.kind, mdl.v, mdl.ell, x, w, r)
        val += v; gy.append(gr); gs2 += gw.sum()
        ref = {"variance": gv, "lengthscale": gl, "mean": -gr.sum()}
        if mdl.kind == "sho":
            ref["quality"] = gq
        assert set(got["gps"][l]) == set(ref)
        for key in ref:
            close_value(got["gps"][l][key], ref[key], tolg)
    close_value(got["value"], val, tolg); close(got["y"], np.concatenate(gy), tolg); close_value(got["sigma2"], gs2, tolg)


@pytest.mark.parametrize("n", [63, 130])
def test_dense_gradient_dense_h(lmm, tolg, n):
    f, H, models, means, x, y, s2 = dense_models(lmm, "dense", n)
    got = lmm.logpdf_and_gradient(f(lmm.MOInputIsotopicByOutputs(x, 3), s2), y)
    ref = naive_gradient(models, means, H, x, y, s2)
    assert set(got) == set(ref)
    close_value(got["value"], ref["value"], tolg); close(got["y"], ref["y"], tolg); close_value(got["sigma2"], ref["sigma2"], tolg)
    close(got["H"], ref["H"], tolg)
    for a, b in zip(got["gps"], ref["gps"]):
        assert set(a) == set(b)
        for key in b:
            close_value(a[key], b[key], tolg)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi_name_the_latent(lmm):
    """d > 1, input gradients and the inducing-point bound refuse a kind-12 latent with LMM_ERR_UNSUPPORTED, naming it, and the next
    valid call is served; so do tag misuse (LMM_ERR_ARG) and the fp32 mode on the state-space path."""
    from lmm_amd import _lib as L
    x, U, Sv, Y = problem(63)
    y = Y.reshape(-1)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    descs = [mdl.desc(mu) for mdl, mu in zip(MODELS, MEANS)]
    arr = L.gps_array(descs)
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(Sv)
    out = C.c_double()
    x2 = np.ascontiguousarray(np.stack([x, x], axis=1))                     # d = 2, column-major d x n
    rc = lib.lmm_oilmm_logpdf(L.Arr(x2).ptr, 2, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, C.c_double(S2), arr, 0, 4, 1, C.byref(out))
    assert rc == L.LMM_ERR_UNSUPPORTED
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert lat.value == 1 and b"latent 1" in lib.lmm_last_error_string() and b"SHO" in lib.lmm_last_error_string()
    gg, gx = (L.GpGradT * 4)(), np.zeros(63)
    rc = lib.lmm_oilmm_logpdf_grad_x(L.Arr(x).ptr, 1, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, C.c_double(S2), arr, 0, 4, 1,
                                     C.byref(out), None, None, None, None, gg, L.Arr(gx, True).ptr)
    assert rc == L.LMM_ERR_UNSUPPORTED and b"latent 1" in lib.lmm_last_error_string() and b"SHO" in lib.lmm_last_error_string()
    rc = lib.lmm_oilmm_logpdf(L.Arr(x).ptr, 1, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, C.c_double(S2), arr, 0, 4, 1, C.byref(out))
    assert rc == L.LMM_OK and np.isfinite(out.value)                        # the next valid call is served
    # an untagged kind-12 latent over d = 2 through the Gram building block
    import torch
    A, xd = nan_dev(64, 64), dev(x2)
    torch.cuda.synchronize()
    rc = lib.lmm_dev_gram(C.c_void_p(A.data_ptr()), 64, 64, 64, C.c_void_p(xd.data_ptr()), 2, 63,
                          L.gps_array([{"kind": "sho", "variance": 1.0, "lengthscale": 1.0}]), C.c_double(0.0))
    assert rc == L.LMM_ERR_UNSUPPORTED and b"latent 0" in lib.lmm_last_error_string()
    # a quality tag on a Matern latent, an RQ tag on an SHO latent
    tq, ta = C.c_int(), C.c_int()
    assert lib.lmm_kernel_tag_create_sho(C.c_double(2.0), C.byref(tq)) == L.LMM_OK
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK
    try:
        for kind in (L.KERNEL_KINDS["matern32"] | tq.value << 8, L.KERNEL_SHO | ta.value << 8):
            bad = (L.GpT * 4)(*[L.GpT(a.kind, a.variance, a.lengthscale, a.mean) for a in arr])
            bad[2].kind = kind
            rc = lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, S2, bad, 0, 4, 1, C.byref(out))
            assert rc == L.LMM_ERR_ARG and b"latent 2" in lib.lmm_last_error_string()
            rc = lib.lmm_oilmm_logpdf(L.Arr(x).ptr, 1, 63, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, 4, C.c_double(S2), bad, 0, 4, 1, C.byref(out))
            assert rc == L.LMM_ERR_ARG and b"latent 2" in lib.lmm_last_error_string()
    finally:
        lib.lmm_ard_destroy(tq.value); lib.lmm_ard_destroy(ta.value)
    f = oilmm(lmm, U, Sv)
    xin = lmm.MOInputIsotopicByOutputs(x, P_OUT)
    lmm.set_compute_dtype("f32")
    try:
        with pytest.raises(NotImplementedError, match="Float64 only"):
            lmm.statespace_logpdf(f(xin, S2), y)
    finally:
        lmm.set_compute_dtype("f64")
    vfe = lmm.VFE(np.linspace(0.0, 8.0, 5))
    for verb in (lambda: lmm.logpdf_and_gradient(f(xin, S2), y, inputs=True), lambda: lmm.elbo(vfe, f(xin, S2), y),
                 lambda: lmm.mean_and_var_vjp(f(xin, S2), np.ones(63 * P_OUT))):
        with pytest.raises(NotImplementedError, match="latent 1"):
            verb()
    # and the next valid calls are served
    assert np.isfinite(lmm.statespace_logpdf(f(xin, S2), y)) and np.isfinite(lmm.logpdf(f(xin, S2), y))
