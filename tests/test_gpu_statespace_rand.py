"""-m gpu: state-space sampling (include/lmm_hip.h "state space", lmm_oilmm_rand_statespace; DESIGN.md 4.18 "Sampling"): the prior and
posterior building blocks against the NumPy restatement of tests/test_statespace_rand_abi.py at well-separated inputs, their LAW (the
covariance of the linear map from normals to path) at every spacing, the entry point and its Python mirror against the dense Gaussian,
bitwise reproducibility, and the refusals.

Tolerance: 1e-10 of max|reference| per array: the rule max(1e-10, 100 DELTA) of tests/test_gpu_statespace.py with DELTA the largest of
test_statespace_rand_abi's delta_rand / delta_law / delta_post (4.2e-15, each asserted <= 1e-12 there).  Paths for fixed normals are
compared only where the spacings are 0.5 - 2 lengthscales: elsewhere the path is ill-conditioned in its normals and only its law is
pinned."""
import ctypes as C

import numpy as np
import pytest

import test_statespace_abi as T
import test_statespace_rand_abi as R

pytestmark = pytest.mark.gpu

DIM = R.DIM


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * R.delta())


def close(got, ref, tol, scale=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max() if scale is None else scale
    print(f"err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, (err, scale)


def kernel_of(lmm, kind, v, ell):
    return {"matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}[kind](v, ell)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def gp_of(lmm, kind, v, ell):
    from lmm_amd import _lib as L
    return L.gps_array([dict(kernel_of(lmm, kind, v, ell).desc(), mean=0.7)])      # the mean is not read


def gpu_sample(lmm, kind, v, ell, x, Z, chunk):
    """lmm_dev_statespace_sample: Z (N, D n) -> (N, n)."""
    import torch
    from lmm_amd import _lib as L
    n, N = len(x), Z.shape[0]
    xd, zd = dev(x), dev(Z)
    f = torch.full((N, n), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L.check(lmm.load().lmm_dev_statespace_sample(xd.data_ptr(), n, gp_of(lmm, kind, v, ell), zd.data_ptr(), N, chunk, f.data_ptr()))
    return f.cpu().numpy()


def gpu_sample_post(lmm, kind, v, ell, x, w, r, Z, Xi, chunk):
    """lmm_dev_statespace_sample_posterior: Z (N, D n), Xi (N, n) -> (N, n)."""
    import torch
    from lmm_amd import _lib as L
    n, N = len(x), Z.shape[0]
    xd, wd, rd, zd, xid = dev(x), dev(w), dev(r), dev(Z), dev(Xi)
    f = torch.full((N, n), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L.check(lmm.load().lmm_dev_statespace_sample_posterior(xd.data_ptr(), n, gp_of(lmm, kind, v, ell), wd.data_ptr(), rd.data_ptr(),
                                                           zd.data_ptr(), xid.data_ptr(), N, chunk, f.data_ptr()))
    return f.cpu().numpy()


def gpu_smooth(lmm, kind, v, ell, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n = len(x)
    xd, wd, rd = dev(x), dev(w), dev(r)
    sm, sv = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    L.check(lmm.load().lmm_dev_statespace_smooth(xd.data_ptr(), n, gp_of(lmm, kind, v, ell), wd.data_ptr(), rd.data_ptr(), chunk,
                                                 sm.data_ptr(), sv.data_ptr()))
    return sm.cpu().numpy(), sv.cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# the prior block
# ---------------------------------------------------------------------------------------------------
_PRIOR = {}


def prior_reference(kind, n):
    if (kind, n) not in _PRIOR:
        v, ell, x, zeta = R.rand_case(kind, n)
        _PRIOR[(kind, n)] = ((v, ell, x, zeta), R.prior_path(kind, v, ell, x, zeta))
    return _PRIOR[(kind, n)]


@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 129, 1000, 5000])
@pytest.mark.parametrize("kind", T.KINDS)
def test_prior_block_vs_restatement(lmm, tol, kind, n):
    (v, ell, x, zeta), ref = prior_reference(kind, n)
    Z = zeta.reshape(1, -1)
    got = {chunk: gpu_sample(lmm, kind, v, ell, x, Z, chunk)[0] for chunk in (1, 7, 64, 0, n)}
    for chunk, f in got.items():
        close(f, ref, tol)
    assert (gpu_sample(lmm, kind, v, ell, x, Z, 7)[0] == got[7]).all()          # bitwise
    dup = np.flatnonzero(np.diff(x) == 0.0) + 1          # an equal input repeats the state: bitwise within a thread's run (chunk n is
    assert (got[n][dup] == got[n][dup - 1]).all()        # one thread), to rounding across a restart from the scanned prefix
    for f in got.values():
        assert np.abs(f[dup] - f[dup - 1]).max(initial=0.0) <= tol * np.abs(ref).max()


def test_prior_block_three_scan_levels(lmm, tol):
    """n = 16500 at chunk 1: 16500 aggregates, 129 workgroups, whose totals take two workgroups, whose totals take one."""
    (v, ell, x, zeta), ref = prior_reference("matern52", 16500)
    close(gpu_sample(lmm, "matern52", v, ell, x, zeta.reshape(1, -1), 1)[0], ref, tol)


def law_inputs():
    cases = [("spacing %g" % sp, R.law_case(sp)) for sp in R.LAW_SPACINGS]
    cases.append(("n = 300", T.case("matern52", 300)[2]))                         # spacings 0.01 - 1 lengthscales
    return cases


@pytest.mark.parametrize("kind", T.KINDS)
def test_law_of_the_prior_block(lmm, tol, kind):
    """D n unit vectors of normals as the samples of ONE call: M M' is the Matern covariance, small spacings included."""
    D = DIM[kind]
    for name, x in law_inputs():
        n = len(x)
        K = T.matern_K(kind, R.VAR, R.ELL, x)
        for chunk in (7, 1):
            M = gpu_sample(lmm, kind, R.VAR, R.ELL, x, np.eye(D * n), chunk).T
            print(name, "chunk", chunk)
            close(M @ M.T, K, tol, scale=R.VAR)


# ---------------------------------------------------------------------------------------------------
# the posterior block
# ---------------------------------------------------------------------------------------------------
def unobserved_runs(w, n):
    """First and last point unobserved, and runs of unobserved points longer than a chunk of 7 (n >= 17) and of 64 (n >= 257)."""
    if n >= 2:
        w[0] = w[-1] = np.inf
    if n >= 17:
        w[3:12] = np.inf
    if n >= 257:
        w[100:180] = np.inf
    return w


@pytest.mark.parametrize("kind", T.KINDS)
def test_posterior_block_with_zero_normals_is_the_smoothed_mean(lmm, kind):
    for n in (17, 1000):
        v, ell, x, w, r = T.case(kind, n)
        w = unobserved_runs(w, n)
        D = DIM[kind]
        for chunk in (7, 0):
            f = gpu_sample_post(lmm, kind, v, ell, x, w, r, np.zeros((2, D * n)), np.zeros((2, n)), chunk)
            sm, _ = gpu_smooth(lmm, kind, v, ell, x, w, r, chunk)
            assert (f[0] == sm).all() and (f[1] == sm).all()                     # bitwise


@pytest.mark.parametrize("kind", T.KINDS)
def test_law_of_the_posterior_block(lmm, tol, kind):
    """n = 40, spacings 0.01 - 1 lengthscales: sample 0 has zero normals, the others the unit vectors of (zeta, xi)."""
    n, D = 40, DIM[kind]
    v, ell, x, w, r = T.case(kind, n)
    w = unobserved_runs(w, n)
    w[20:30] = np.inf
    E = np.vstack([np.zeros((1, D * n + n)), np.eye(D * n + n)])
    mu, Sg = R.dense_posterior(kind, v, ell, x, w, r)
    for chunk in (7, 1):
        f = gpu_sample_post(lmm, kind, v, ell, x, w, r, E[:, :D * n], E[:, D * n:], chunk)
        close(f[0], mu, tol)
        B = (f[1:] - f[:1]).T
        close(B @ B.T, Sg, tol)
        _, sv = gpu_smooth(lmm, kind, v, ell, x, w, r, chunk)
        close(np.diag(B @ B.T), sv, tol)


@pytest.mark.parametrize("n", [1, 17, 1000])
@pytest.mark.parametrize("kind", T.KINDS)
def test_posterior_block_vs_restatement(lmm, tol, kind, n):
    v, ell, x, zeta = R.rand_case(kind, n)
    rng = np.random.default_rng([n, 5])
    w = unobserved_runs(rng.uniform(0.05, 0.5, n), n)
    r, xi = rng.standard_normal(n), rng.standard_normal(n)
    ref = R.pathwise_posterior(kind, v, ell, x, w, r, zeta, xi)
    for chunk in (7, 64, 0):
        close(gpu_sample_post(lmm, kind, v, ell, x, w, r, zeta.reshape(1, -1), xi.reshape(1, -1), chunk)[0], ref, tol)


# ---------------------------------------------------------------------------------------------------
# the entry point and its mirror
# ---------------------------------------------------------------------------------------------------
GPS = [{"kind": "matern12", "variance": 1.2, "lengthscale": 0.8, "mean": 0.3},
       {"kind": "matern32", "variance": 0.7, "lengthscale": 1.3, "mean": -0.4},
       {"kind": "matern52", "variance": 1.5, "lengthscale": 0.6, "mean": 0.9}]
P_OUT, S2 = 4, 0.1


def mixing(seed=0):
    rng = np.random.default_rng([seed, P_OUT])
    return np.linalg.qr(rng.standard_normal((P_OUT, len(GPS))))[0], rng.uniform(0.5, 2.0, len(GPS))


def model(lmm, U, S):
    fs = lmm.independent_mogp([lmm.GP(g["mean"], kernel_of(lmm, g["kind"], g["variance"], g["lengthscale"])) for g in GPS])
    return lmm.ILMM(fs, lmm.Orthogonal(U, S))


class Recorder:
    """A NumPy Generator that keeps what it drew."""

    def __init__(self, seed):
        self.rng, self.draws = np.random.default_rng(seed), []

    def standard_normal(self, count):
        self.draws.append(self.rng.standard_normal(count))
        return self.draws[-1]


class Replay:
    """Hands out recorded draws."""

    def __init__(self, draws):
        self.draws = list(draws)

    def standard_normal(self, count):
        d = self.draws.pop(0)
        assert d.shape == (count,)
        return d


class UnitVectors:
    """Sample 0 draws zeros; sample q >= 1 draws the (q - 1)-th unit vector of the `total` normals one sample takes."""

    def __init__(self, total):
        self.total, self.q, self.off = total, 0, 0

    def standard_normal(self, count):
        out = np.zeros(count)
        i = self.q - 1 - self.off
        if self.q >= 1 and 0 <= i < count:
            out[i] = 1.0
        self.off += count
        assert self.off <= self.total
        if self.off == self.total:
            self.q, self.off = self.q + 1, 0
        return out


def test_entry_point_prior(lmm, tol):
    from lmm_amd import _lib as L
    n, m, p = 50, len(GPS), P_OUT
    x = R.rand_case("matern52", n)[2]                                             # sorted, well separated, with duplicates
    U, S = mixing()
    H = U * np.sqrt(S)[None, :]
    fx = model(lmm, U, S)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    for add_noise in (True, False):
        rec = Recorder(11)
        out = lmm.statespace_rand(rec, fx, add_noise=add_noise)
        assert isinstance(out, np.ndarray) and out.shape == (n * p,) and len(rec.draws) == m + int(add_noise)
        F = np.stack([g["mean"] + R.prior_path(g["kind"], g["variance"], g["lengthscale"], x, rec.draws[l].reshape(DIM[g["kind"]], n))
                      for l, g in enumerate(GPS)])
        ref = H @ F + (np.sqrt(S2) * rec.draws[m].reshape(p, n) if add_noise else 0.0)
        close(out, ref.reshape(-1), tol)
    # through the C ABI the shards [0, 1) and [1, 3) are partial sums of the whole (the noise added once)
    z, eps = np.concatenate(rec.draws[:m]), Recorder(12).standard_normal(n * p)
    lib, arr, Ua, Sa = lmm.load(), L.gps_array(GPS), L.Arr(L.colmajor(U)), L.Arr(S)

    def shard(l0, l1, noise):
        o = np.full(n * p, np.nan)
        L.check(lib.lmm_oilmm_rand_statespace(L.Arr(x).ptr, n, None, p, Ua.ptr, Sa.ptr, m, S2, arr, l0, l1, noise, 1, L.Arr(z).ptr, None,
                                              L.Arr(eps).ptr if noise else None, L.Arr(o, True).ptr))
        return o

    whole = shard(0, m, 1)
    close(whole, (H @ F + np.sqrt(S2) * eps.reshape(p, n)).reshape(-1), tol)
    close(shard(0, 1, 1) + shard(1, m, 0), whole, tol)


def posterior_problem():
    """30 training inputs and 7 new ones, unsorted, with duplicates among and across them."""
    rng = np.random.default_rng(21)
    x = rng.uniform(0.0, 8.0, 30)
    x[7], x[19] = x[3], x[3]
    xs = rng.uniform(-0.5, 8.5, 7)
    xs[2], xs[5] = x[11], xs[0]
    return x, xs, rng.standard_normal((P_OUT, 30))


def dense_oilmm_posterior(U, S, x, Y, xs):
    """Mean and covariance (by outputs, without the observation noise) of the OILMM's posterior at xs over the complete data Y (p, n),
    from dense Gaussians per latent (the oracle's mathematics with this module's Matern12: reference src/oilmm.jl:56-76)."""
    Tm, ST = T.O.project_orthogonal(U, S, S2)
    Ty = Tm @ Y
    H = U * np.sqrt(S)[None, :]
    ns, p = len(xs), U.shape[0]
    mean, cov = np.zeros((p, ns)), np.zeros((p * ns, p * ns))
    for l, g in enumerate(GPS):
        k = (g["kind"], g["variance"], g["lengthscale"])
        G = np.linalg.solve(T.matern_K(*k, x) + ST[l] * np.eye(len(x)), T.matern_K(*k, x, xs))
        ml = g["mean"] + G.T @ (Ty[l] - g["mean"])
        Cl = T.matern_K(*k, xs) - T.matern_K(*k, xs, x) @ G
        mean += np.outer(H[:, l], ml)
        cov += np.kron(np.outer(H[:, l], H[:, l]), Cl)
    return mean.reshape(-1), cov


def test_entry_point_posterior(lmm, tol):
    x, xs, Y = posterior_problem()
    n, ns, m, p = len(x), len(xs), len(GPS), P_OUT
    na, y = n + ns, Y.reshape(-1)
    U, S = mixing()
    f = model(lmm, U, S)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), S2)
    total = sum(DIM[g["kind"]] for g in GPS) * na + m * na
    out = lmm.statespace_rand(UnitVectors(total), fx, y, N=total + 1, add_noise=False, xs=xs)
    assert out.shape == (ns * p, total + 1)
    mu, Sg = dense_oilmm_posterior(U, S, x, Y, xs)
    close(out[:, 0], mu, tol)                                                     # zero normals: the posterior mean
    sm, sv = lmm.statespace_mean_and_var(fx, y, True, xs=xs)
    close(out[:, 0], sm, tol)
    B = out[:, 1:] - out[:, :1]
    cov = B @ B.T + S2 * np.eye(ns * p)
    close(cov, Sg + S2 * np.eye(ns * p), tol)
    close(np.diag(cov), sv, tol)
    post = lmm.posterior(fx, y)
    cm, cc = lmm.mean_and_cov(post(lmm.MOInputIsotopicByOutputs(xs, p), S2))      # the library's Cholesky path
    close(out[:, 0], cm, tol)
    close(cov, cc, tol)
    # NaN in y (one output of a point, and every output of another): the sample variances are the smoother's
    Yn = Y.copy()
    Yn[1, 4] = np.nan
    Yn[:, 9] = np.nan
    out = lmm.statespace_rand(UnitVectors(total), fx, Yn.reshape(-1), N=total + 1, add_noise=False, xs=xs)
    sm, sv = lmm.statespace_mean_and_var(fx, Yn.reshape(-1), True, xs=xs)
    close(out[:, 0], sm, tol)
    B = out[:, 1:] - out[:, :1]
    close((B * B).sum(axis=1) + S2, sv, tol)
    # at the training inputs, the point without observations included
    out = lmm.statespace_rand(UnitVectors(total - 6 * ns - m * ns), fx, Yn.reshape(-1), N=total - 6 * ns - m * ns + 1, add_noise=False)
    sm, sv = lmm.statespace_mean_and_var(fx, Yn.reshape(-1), True)
    assert out.shape[0] == n * p
    close(out[:, 0], sm, tol)
    B = out[:, 1:] - out[:, :1]
    close((B * B).sum(axis=1) + S2, sv, tol)


def test_reproducibility_and_device_normals(lmm):
    import torch
    x, xs, Y = posterior_problem()
    p, y = P_OUT, Y.reshape(-1)
    U, S = mixing()
    fx = model(lmm, U, S)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    for kw in (dict(), dict(y=y), dict(y=y, xs=xs)):
        rec = Recorder(3)
        five = lmm.statespace_rand(rec, fx, N=5, **kw)
        again = lmm.statespace_rand(Replay(rec.draws), fx, N=5, **kw)
        assert five.shape[1] == 5 and (five == again).all()                       # two calls: bitwise
        per = len(rec.draws) // 5
        for q in range(5):                                                        # column q is the single-sample call on its normals
            one = lmm.statespace_rand(Replay(rec.draws[q * per:(q + 1) * per]), fx, **kw)
            assert one.shape == (five.shape[0],) and (one == five[:, q]).all()
        dn = lmm.statespace_rand(lmm.DeviceNormals(5), fx, N=2, **kw)
        assert torch.is_tensor(dn) and dn.is_cuda and dn.shape == five[:, :2].shape and bool(torch.isfinite(dn).all())
        d1 = lmm.statespace_rand(lmm.DeviceNormals(5), fx, **kw)
        assert d1.is_cuda and (d1 == dn[:, 0]).all()
    # torch device inputs with host normals: the same numbers
    xt, yt = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    rec = Recorder(4)
    a = lmm.statespace_rand(rec, fx, y, xs=xs)
    b = lmm.statespace_rand(Replay(rec.draws), fx.f(lmm.MOInputIsotopicByOutputs(xt, p), S2), yt, xs=torch.tensor(xs, device="cuda"))
    assert (np.asarray(b) == a).all()
    # device inputs AND device normals: the sort of the inputs is still in flight on torch's stream when the normals are generated on
    # the library's; every repeat must see the sorted inputs and give the same sample
    fxt = fx.f(lmm.MOInputIsotopicByOutputs(torch.tensor(np.sort(x), device="cuda"), p), S2)
    first = lmm.statespace_rand(lmm.DeviceNormals(9), fxt)
    for _ in range(5):
        assert (lmm.statespace_rand(lmm.DeviceNormals(9), fxt) == first).all()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals(lmm):
    import torch
    from lmm_amd import _lib as L
    n, m, p = 30, len(GPS), P_OUT
    x = np.sort(posterior_problem()[0])
    Y = posterior_problem()[2]
    U, S = mixing()
    lib, Ua = lmm.load(), L.Arr(L.colmajor(U))
    lat, info = C.c_int(), C.c_int()
    zl = 6 * n
    z, xi, eps, out = np.zeros(zl), np.zeros(m * n), np.zeros(n * p), np.zeros(n * p)

    def call(x=x, y=Y.reshape(-1), S=S, s2=S2, gps=GPS, l0=0, l1=m, noise=1, N=1, z=z, xi=xi, eps=eps):
        ptr = lambda a: None if a is None else L.Arr(a).ptr
        rc = lib.lmm_oilmm_rand_statespace(ptr(x), n, ptr(y), p, Ua.ptr, L.Arr(np.asarray(S)).ptr, m, s2, L.gps_array(gps), l0, l1, noise,
                                           N, ptr(z), ptr(xi), ptr(eps), L.Arr(out, True).ptr)
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        return rc, lib.lmm_last_error_string()

    assert call()[0] == L.LMM_OK and call(y=None, xi=None)[0] == L.LMM_OK and call(noise=0, eps=None)[0] == L.LMM_OK
    for kw, code, text in ((dict(N=0), L.LMM_ERR_ARG, b"nsamples"), (dict(N=-3), L.LMM_ERR_ARG, b"nsamples"),
                           (dict(z=None), L.LMM_ERR_ARG, b"z is NULL"), (dict(xi=None), L.LMM_ERR_ARG, b"xi is NULL"),
                           (dict(eps=None), L.LMM_ERR_ARG, b"eps is NULL"), (dict(x=None), L.LMM_ERR_ARG, b"bad arguments"),
                           (dict(s2=0.0), L.LMM_ERR_ARG, b"sigma2"), (dict(S=[1.0, -1.0, 1.0]), L.LMM_ERR_ARG, b"S[1]"),
                           (dict(l0=2, l1=1), L.LMM_ERR_ARG, b"shard"), (dict(l1=m + 1), L.LMM_ERR_ARG, b"shard")):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    # a latent that is not a plain Matern: named, for the prior sample as well
    se = [GPS[0], {"kind": "se", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0}, GPS[2]]
    for kw in (dict(), dict(y=None, xi=None)):
        rc, msg = call(gps=se, **kw)
        assert rc == L.LMM_ERR_UNSUPPORTED and lat.value == 1 and b"latent 1" in msg
    # unsorted inputs: the first offending index
    xu = x.copy()
    xu[12] = xu[10] - 1e-3
    rc, msg = call(x=xu)
    assert rc == L.LMM_ERR_ARG and info.value == 12 and b"x[12]" in msg
    # 0 < p_t < m names the point; p_t = 0 is served
    few = Y.copy()
    few[:2, 17] = np.nan
    rc, msg = call(y=few.reshape(-1))
    assert rc == L.LMM_ERR_UNSUPPORTED and (lat.value, info.value) == (-1, 17) and b"point 17 observes 2 outputs" in msg
    few[:, 17] = np.nan
    assert call(y=few.reshape(-1))[0] == L.LMM_OK and np.isfinite(out).all()
    # the fp32 compute mode
    lmm.set_compute_dtype("f32")
    try:
        rc, msg = call()
        assert rc == L.LMM_ERR_UNSUPPORTED and b"Float64 only" in msg
    finally:
        lmm.set_compute_dtype("f64")
    # the building blocks
    xd, o = torch.tensor(x, device="cuda"), torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    gp = L.gps_array([GPS[2]])
    assert lib.lmm_dev_statespace_sample(xd.data_ptr(), n, gp, o.data_ptr(), 0, 0, o.data_ptr()) == L.LMM_ERR_ARG
    assert b"nsamples" in lib.lmm_last_error_string()
    assert lib.lmm_dev_statespace_sample(xd.data_ptr(), n, gp, None, 1, 0, o.data_ptr()) == L.LMM_ERR_ARG
    assert lib.lmm_dev_statespace_sample(xd.data_ptr(), n, gp, o.data_ptr(), 1, -1, o.data_ptr()) == L.LMM_ERR_ARG
    assert lib.lmm_dev_statespace_sample_posterior(xd.data_ptr(), n, gp, o.data_ptr(), o.data_ptr(), o.data_ptr(), None, 1, 0,
                                                   o.data_ptr()) == L.LMM_ERR_ARG
    assert lib.lmm_dev_statespace_sample(xd.data_ptr(), n, L.gps_array([se[1]]), o.data_ptr(), 1, 0, o.data_ptr()) == L.LMM_ERR_UNSUPPORTED
    # and the next valid call is served
    assert call()[0] == L.LMM_OK
