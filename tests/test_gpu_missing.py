"""-m gpu: missing observations (NaN in y) for the OILMM logpdf, posterior and gradients (include/lmm_hip.h "missing observations";
DESIGN.md 4.15).  The reference for everything but the exactness test is `restatement` below: the diagonal approximation of Bruinsma et
al. 2020 written as a per-point NumPy loop, followed by one Float64 LAPACK GP per latent."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

RTOL32 = 2e-4           # tests/test_gpu_f32.py:14


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


# ---------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------
def restatement(Y, H, s2):
    """Y: (p, n) with NaN at the missing entries.  z (n, m), noise (n, m) = s2 diag(G_t^-1), reg = sum_t r_t, max_t cond(G_t)."""
    (p, n), m = Y.shape, H.shape[1]
    z, noise, reg, cond = np.zeros((n, m)), np.zeros((n, m)), 0.0, 0.0
    for t in range(n):
        ob = ~np.isnan(Y[:, t])
        Ht, yt = H[ob], Y[ob, t]
        G = Ht.T @ Ht
        Gi = np.linalg.inv(G)
        z[t] = np.linalg.solve(G, Ht.T @ yt)
        noise[t] = s2 * np.diag(Gi)
        r = yt - Ht @ z[t]
        reg += -0.5 * ((ob.sum() - m) * math.log(2.0 * math.pi * s2) + np.linalg.slogdet(G)[1] + r @ r / s2)
        cond = max(cond, np.linalg.cond(G))
    return z, noise, reg, cond


def kmat(g, x, x2=None):
    """Latent kernel matrix of a descriptor: a base kind of the oracle, or {"kind": "sum", "variance", "lengthscale", "terms"}."""
    if g["kind"] != "sum":
        return O.kernelmatrix(g, x, x2)
    return sum(O.kernelmatrix({"kind": t["kind"], "variance": g["variance"] * t["variance"],
                               "lengthscale": g["lengthscale"] * t["lengthscale"]}, x, x2) for t in g["terms"])


def restated_logpdf(gps, H, x, s2, Y, with_reg=True, latents=None):
    z, noise, reg, _ = restatement(Y, H, s2)
    n = Y.shape[1]
    tot = reg if with_reg else 0.0
    for l in (range(len(gps)) if latents is None else latents):
        tot += O.gaussian_logpdf(np.full(n, gps[l]["mean"]), kmat(gps[l], x) + np.diag(noise[:, l]), z[:, l])
    return tot


def restated_marginals(gps, H, x, s2, Y, xs):
    """Predictive mean and variance (by outputs, observation noise s2 included) of the restated model at xs."""
    z, noise, _, _ = restatement(Y, H, s2)
    ml, vl = [], []
    for l, g in enumerate(gps):
        Cl = kmat(g, x) + np.diag(noise[:, l])
        Ks = kmat(g, x, xs)
        ml.append(g["mean"] + Ks.T @ np.linalg.solve(Cl, z[:, l] - g["mean"]))
        vl.append(np.diag(kmat(g, xs)) - np.sum(Ks * np.linalg.solve(Cl, Ks), axis=0))
    return (H @ np.array(ml)).reshape(-1), ((H * H) @ np.array(vl) + s2).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def flat_orthogonal(rng, p, m):
    """p x m orthonormal U whose complement is spanned by perturbed sign vectors: every row of the complement has about the same
    norm (and no two rows are parallel), so deleting a few outputs leaves H_t' H_t well conditioned (the tests assert cond <= 1e3)."""
    W = np.linalg.qr(rng.choice([-1.0, 1.0], size=(p, p - m)) + 0.3 * rng.standard_normal((p, p - m)))[0]
    Q = np.linalg.qr(np.hstack([W, rng.standard_normal((p, m))]))[0]
    return np.ascontiguousarray(Q[:, p - m:])


def distinct_masks(rng, p, m, count):
    """Up to `count` different sets of deleted outputs, each of at most max(1, (p - m) // 2) outputs (never more than p - m)."""
    kmax = min(p - m, max(1, (p - m) // 2))
    seen, out = set(), []
    singles = [(o,) for o in range(p)]
    for dele in [()] + singles:
        if len(out) < count:
            seen.add(dele); out.append(dele)
    tries = 0
    while len(out) < count and kmax >= 2 and tries < 100 * count:
        tries += 1
        dele = tuple(sorted(rng.choice(p, size=int(rng.integers(2, kmax + 1)), replace=False).tolist()))
        if dele not in seen:
            seen.add(dele); out.append(dele)
    return out


def with_deleted(Y, masks):
    Y = Y.copy()
    for t in range(Y.shape[1]):
        Y[list(masks[t % len(masks)]), t] = np.nan
    return Y


def project_missing(lmm, Y, U, S, s2, means=None):
    lib = lmm.load()
    p, n = Y.shape
    m = U.shape[1]
    y = np.ascontiguousarray(Y.reshape(-1))
    Uc, Sc = np.ascontiguousarray(U.T.reshape(-1)), np.ascontiguousarray(S, dtype=np.float64)      # column-major U
    z, nz, reg, npat = np.empty(n * m), np.empty(n * m), C.c_double(), C.c_int()
    mp = None if means is None else np.ascontiguousarray(means, dtype=np.float64).ctypes.data_as(C.c_void_p)
    rc = lib.lmm_oilmm_project_missing(y.ctypes.data_as(C.c_void_p), n, p, Uc.ctypes.data_as(C.c_void_p),
                                       Sc.ctypes.data_as(C.c_void_p), m, C.c_double(s2), mp, z.ctypes.data_as(C.c_void_p),
                                       nz.ctypes.data_as(C.c_void_p), C.byref(reg), C.byref(npat))
    return rc, z.reshape(m, n).T, nz.reshape(m, n).T, reg.value, npat.value


def model(lmm, gps):
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}

    def kern(g):
        if g["kind"] == "sum":
            return lmm.KernelSum(*[kern(t) for t in g["terms"]], variance=g["variance"], lengthscale=g["lengthscale"])
        if g["kind"] == "periodic":
            return lmm.PeriodicKernel(g["variance"], g["lengthscale"], g["r"])
        return K[g["kind"]](g["variance"], g["lengthscale"])
    return lmm.independent_mogp([lmm.GP(g.get("mean", 0.0), kern(g)) for g in gps])


GPS3 = [{"kind": "se", "variance": 1.3, "lengthscale": 0.9, "mean": 0.2},
        {"kind": "matern52", "variance": 0.8, "lengthscale": 1.4, "mean": -0.3},
        {"kind": "sum", "variance": 1.1, "lengthscale": 1.2, "mean": 0.1,
         "terms": [{"kind": "se", "variance": 0.7, "lengthscale": 0.6}, {"kind": "matern32", "variance": 0.5, "lengthscale": 2.0}]}]


def problem(n, d, p=7, m=3, seed=0, frac=0.2):
    """x, U, S, Y (p, n) with NaN: each point loses at most (p - m) // 2 outputs."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 6, size=n)) if d == 1 else rng.uniform(0, 3, size=(d, n))
    U, S = flat_orthogonal(rng, p, m), rng.uniform(0.5, 2.0, size=m)
    Y = rng.standard_normal((p, n))
    for t in range(n):
        k = int(rng.integers(0, (p - m) // 2 + 1)) if rng.uniform() < 3 * frac else 0
        Y[rng.choice(p, size=k, replace=False), t] = np.nan
    return x, U, S, Y


# ---------------------------------------------------------------------------------------------------
# 1. the front end, element-wise
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,m", [(2, 1), (5, 4), (33, 32), (70, 33), (70, 65), (130, 128)])
def test_front_end_elementwise(lmm, p, m):
    """z, noise and reg of lmm_oilmm_project_missing against the restatement, to 1e-10 of each array's largest magnitude (about
    m eps cond(G_t) with cond(G_t) <= 1e3, asserted).  Masks: n = 1; n = 65 with one pattern; n = 130 with as many different
    patterns as the shape has (every point its own where p allows 130 of them); a NaN only in the last output; only in output 0."""
    rng = np.random.default_rng(1000 * p + m)
    U, S, s2 = flat_orthogonal(rng, p, m), rng.uniform(0.5, 2.0, size=m), 0.3
    H = U * np.sqrt(S)
    means = rng.standard_normal(m)
    many = distinct_masks(rng, p, m, 130)
    cases = [(1, [many[1]]), (65, [many[-1]]), (130, many), (65, [(p - 1,)]), (65, [(0,)])]
    for n, masks in cases:
        Y = with_deleted(rng.standard_normal((p, n)), masks)
        zr, nr, rr, cond = restatement(Y, H, s2)
        assert cond <= 1e3, (n, masks[0], cond)
        rc, z, noise, reg, npat = project_missing(lmm, Y, U, S, s2, means)
        assert rc == 0, lmm.load().lmm_last_error_string()
        assert npat == min(len(masks), n)
        zr = zr - means
        print(f"p={p} m={m} n={n} npat={npat} cond={cond:.1f} dz={np.abs(z - zr).max() / np.abs(zr).max():.2e} "
              f"dnoise={np.abs(noise - nr).max() / nr.max():.2e} dreg={abs(reg - rr) / abs(rr):.2e}")
        assert np.abs(z - zr).max() <= 1e-10 * np.abs(zr).max()
        assert np.abs(noise - nr).max() <= 1e-10 * nr.max()
        assert abs(reg - rr) <= 1e-10 * abs(rr)


@pytest.mark.parametrize("p,m", [(70, 33), (130, 65)])
def test_more_patterns_than_workgroups(lmm, p, m):
    """n = 300 points, each its own pattern: more patterns than the 256 workgroups of the pattern kernel's grid, so workgroups walk
    several patterns and reuse their m x m storage (LDS at m = 33, the global scratch block at m = 65).  Same bound as above."""
    rng = np.random.default_rng(77 * p + m)
    U, S, s2, n = flat_orthogonal(rng, p, m), rng.uniform(0.5, 2.0, size=m), 0.3, 300
    masks = distinct_masks(rng, p, m, n)
    assert len(masks) == n
    Y = with_deleted(rng.standard_normal((p, n)), masks)
    zr, nr, rr, cond = restatement(Y, U * np.sqrt(S), s2)
    assert cond <= 1e3, cond
    rc, z, noise, reg, npat = project_missing(lmm, Y, U, S, s2)
    assert rc == 0 and npat == n
    print(f"p={p} m={m} npat={npat} cond={cond:.1f} dz={np.abs(z - zr).max() / np.abs(zr).max():.2e} "
          f"dnoise={np.abs(noise - nr).max() / nr.max():.2e} dreg={abs(reg - rr) / abs(rr):.2e}")
    assert np.abs(z - zr).max() <= 1e-10 * np.abs(zr).max()
    assert np.abs(noise - nr).max() <= 1e-10 * nr.max()
    assert abs(reg - rr) <= 1e-10 * abs(rr)


# ---------------------------------------------------------------------------------------------------
# 2. no NaN: the _missing entry points equal the complete-data ones
# ---------------------------------------------------------------------------------------------------
def test_without_nan_equals_the_complete_data_paths(lmm):
    n, p, m = 130, 7, 3
    x, U, S, Y = problem(n, 1, p, m, seed=3)
    y = np.ascontiguousarray(np.nan_to_num(Y, nan=0.37).reshape(-1))
    lib = lmm.load()
    from lmm_amd import _lib as L
    gps = L.gps_array([{k: v for k, v in g.items()} for g in GPS3])
    xa, ya, Ua, Sa = L.Arr(x), L.Arr(y), L.Arr(np.ascontiguousarray(U.T.reshape(-1))), L.Arr(S)
    a, b = C.c_double(), C.c_double()
    args = (xa.ptr, 1, n, ya.ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(0.2), gps, 0, m)
    L.check(lib.lmm_oilmm_logpdf(*args, 1, C.byref(a)))
    L.check(lib.lmm_oilmm_logpdf_missing(*args, 1, C.byref(b)))
    assert b.value == pytest.approx(a.value, rel=1e-12)
    xs = np.linspace(0.1, 5.9, 40)
    out = []
    for fn in (lib.lmm_oilmm_posterior_create, lib.lmm_oilmm_posterior_create_missing):
        h = C.c_void_p()
        L.check(fn(*args, C.byref(h)))
        mu, var = np.empty(40 * p), np.empty(40 * p)
        L.check(lib.lmm_oilmm_mean_and_var(h, gps, Ua.ptr, Sa.ptr, p, m, 0, m, C.c_double(0.2), 1, L.Arr(xs).ptr, 1, 40, None,
                                           L.Arr(mu, True).ptr, L.Arr(var, True).ptr))
        L.check(lib.lmm_post_destroy(h))
        out.append((mu, var))
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-10, atol=1e-10 * np.abs(out[0][0]).max())
    np.testing.assert_allclose(out[1][1], out[0][1], rtol=1e-10)


# ---------------------------------------------------------------------------------------------------
# 3. logpdf and posterior marginals against the restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(63, 1), (63, 3), (130, 1), (130, 3)])
def test_logpdf_and_marginals_vs_restatement(lmm, n, d):
    """Tolerances of tests/test_gpu_parity.py for an OILMM of this size (test_c0_oilmm_logpdf_posterior: m = 3, n = 200): rel 1e-10 on
    the logpdf (line 275); rtol 1e-7 + atol 1e-9 on the posterior means and rtol 1e-7 on the variances (line 280)."""
    p, m, s2 = 7, 3, 0.15
    x, U, S, Y = problem(n, d, p, m, seed=10 * n + d)
    assert np.isnan(Y).any()
    H = U * np.sqrt(S)
    fx = lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2)
    y = Y.reshape(-1)
    got, ref = lmm.logpdf(fx, y), restated_logpdf(GPS3, H, x, s2, Y)
    print(f"n={n} d={d} logpdf rel diff {abs(got - ref) / abs(ref):.2e}")
    assert got == pytest.approx(ref, rel=1e-10)
    assert lmm.logpdf(fx, y, with_regulariser=False) == pytest.approx(restated_logpdf(GPS3, H, x, s2, Y, False), rel=1e-10)
    xs = np.linspace(0.2, 5.5, 21) if d == 1 else np.random.default_rng(5).uniform(0, 3, size=(d, 21))
    mg = lmm.marginals(lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(xs, p), s2))
    mo, vo = restated_marginals(GPS3, H, x, s2, Y, xs)
    np.testing.assert_allclose(mg.mu, mo, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(mg.sigma ** 2, vo, rtol=1e-7)


# ---------------------------------------------------------------------------------------------------
# 4. exactness: diagonal G_t
# ---------------------------------------------------------------------------------------------------
def test_exact_when_every_G_is_diagonal(lmm):
    """U = [I; I] / sqrt2 with one copy of an output deleted at random: G_t stays diagonal, so the value is the dense Gaussian
    log-density of the observed entries (rel 1e-9)."""
    n, m, s2 = 40, 3, 0.2
    p = 2 * m
    rng = np.random.default_rng(11)
    x = np.sort(rng.uniform(0, 5, size=n))
    U, S = np.vstack([np.eye(m), np.eye(m)]) / math.sqrt(2.0), np.array([1.7, 0.9, 0.6])
    H = U * np.sqrt(S)
    gps = GPS3[:2] + [{"kind": "matern32", "variance": 0.9, "lengthscale": 0.7, "mean": 0.4}]
    Y = rng.standard_normal((p, n))
    for t in range(n):
        if rng.uniform() < 0.7:
            Y[int(rng.integers(0, p)), t] = np.nan
    Cf = s2 * np.eye(p * n)
    for l, g in enumerate(gps):
        Cf += np.kron(np.outer(H[:, l], H[:, l]), O.kernelmatrix(g, x))
    mean = np.kron(H @ np.array([g["mean"] for g in gps]), np.ones(n))
    ob = ~np.isnan(Y.reshape(-1))
    dense = O.gaussian_logpdf(mean[ob], Cf[np.ix_(ob, ob)], Y.reshape(-1)[ob])
    fx = lmm.ILMM(model(lmm, gps), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2)
    assert lmm.logpdf(fx, Y.reshape(-1)) == pytest.approx(dense, rel=1e-9)


# ---------------------------------------------------------------------------------------------------
# 5. shards, 6. fp32 compute mode
# ---------------------------------------------------------------------------------------------------
def test_shards_sum_to_the_whole(lmm):
    n, p, m, s2 = 63, 7, 3, 0.15
    x, U, S, Y = problem(n, 1, p, m, seed=21)
    xin, y = lmm.MOInputIsotopicByOutputs(x, p), Y.reshape(-1)
    whole = lmm.logpdf(lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S))(xin, s2), y)
    a = lmm.logpdf(lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S), shard=(0, 2))(xin, s2), y, with_regulariser=True)
    b = lmm.logpdf(lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S), shard=(2, 3))(xin, s2), y, with_regulariser=False)
    assert a + b == pytest.approx(whole, rel=1e-12)


def test_fp32_compute_mode(lmm):
    n, p, m, s2 = 130, 7, 3, 0.15
    x, U, S, Y = problem(n, 1, p, m, seed=22)
    fx = lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(x, p), s2)
    ref = lmm.logpdf(fx, Y.reshape(-1))
    lmm.set_compute_dtype("f32")
    try:
        got = lmm.logpdf(fx, Y.reshape(-1))
    finally:
        lmm.set_compute_dtype("f64")
    assert got == pytest.approx(ref, rel=RTOL32)


# ---------------------------------------------------------------------------------------------------
# 7. gradients against central differences of the logpdf itself
# ---------------------------------------------------------------------------------------------------
H_FD, FD_REL, FD_ABS = 1e-6, 2e-5, 1e-6          # tests/test_gpu_kernel_families.py:247, 263


def check_gradients(lmm, gps, n, p, m, seed, term_keys=()):
    s2 = 0.2
    x, U, S, Y = problem(n, 1, p, m, seed=seed, frac=0.3)
    assert np.isnan(Y).any()
    xin, y = lmm.MOInputIsotopicByOutputs(x, p), Y.reshape(-1)

    def value(g2=gps, s=s2, yy=y):
        return lmm.logpdf(lmm.ILMM(model(lmm, g2), lmm.Orthogonal(U, S))(xin, s), yy)

    def fd(f):
        return (f(H_FD) - f(-H_FD)) / (2 * H_FD)

    G = lmm.logpdf_and_gradient(lmm.ILMM(model(lmm, gps), lmm.Orthogonal(U, S))(xin, s2), y)
    assert G["value"] == pytest.approx(value(), rel=1e-12)
    assert G["sigma2"] == pytest.approx(fd(lambda h: value(s=s2 + h)), rel=FD_REL, abs=FD_ABS)
    gy = np.asarray(G["y"])
    assert gy.shape == (n * p,) and np.all(gy[np.isnan(y)] == 0.0) and np.all(gy[~np.isnan(y)] != 0.0)
    rng = np.random.default_rng(seed)
    for k in rng.choice(np.flatnonzero(~np.isnan(y)), size=5, replace=False):
        def at(h, k=k):
            y2 = y.copy(); y2[k] += h
            return value(yy=y2)
        assert gy[k] == pytest.approx(fd(at), rel=FD_REL, abs=FD_ABS), k

    def bumped(l, key, h, c=None):
        g2 = [dict(g) for g in gps]
        if c is None:
            g2[l][key] = g2[l][key] + h
        else:
            g2[l]["terms"] = [dict(t) for t in g2[l]["terms"]]
            g2[l]["terms"][c][key] = g2[l]["terms"][c][key] + h
        return g2
    for l, g in enumerate(gps):
        for key in ("variance", "lengthscale", "mean"):
            assert G["gps"][l][key] == pytest.approx(fd(lambda h: value(g2=bumped(l, key, h))), rel=FD_REL, abs=FD_ABS), (l, key)
        for c, keys in term_keys if g["kind"] == "sum" else ():
            for key in keys:
                assert G["gps"][l]["terms"][c][key] == pytest.approx(fd(lambda h: value(g2=bumped(l, key, h, c))), rel=FD_REL,
                                                                      abs=FD_ABS), (l, c, key)
    for key in ("S", "U"):
        with pytest.raises(NotImplementedError):
            G[key]


def test_gradients_vs_central_differences(lmm):
    check_gradients(lmm, GPS3[:2], n=65, p=5, m=2, seed=31)


def test_gradients_of_a_periodic_plus_matern52_sum(lmm):
    gps = [{"kind": "sum", "variance": 1.2, "lengthscale": 0.9, "mean": 0.1,
            "terms": [{"kind": "periodic", "variance": 0.8, "lengthscale": 1.7, "r": 0.9},
                      {"kind": "matern52", "variance": 0.6, "lengthscale": 1.1}]},
           GPS3[0]]
    check_gradients(lmm, gps, n=130, p=5, m=2, seed=32, term_keys=((0, ("variance", "lengthscale", "r")), (1, ("variance", "lengthscale"))))


# ---------------------------------------------------------------------------------------------------
# 8. refusals are status codes of valid launches
# ---------------------------------------------------------------------------------------------------
def test_refusals_and_the_next_valid_call(lmm):
    from lmm_amd import _lib as L
    rng = np.random.default_rng(41)
    n, p, m, s2 = 20, 6, 3, 0.2
    # column 0 lives on outputs {0, 1} only: a point that misses both has p_t = 4 >= m and a singular G_t
    U = np.zeros((p, m))
    U[0, 0] = U[1, 0] = 1.0 / math.sqrt(2.0)
    U[2:, 1:] = np.linalg.qr(rng.standard_normal((4, 2)))[0]
    S = np.array([1.5, 1.0, 0.7])
    Y = rng.standard_normal((p, n))
    Y[3, 2] = np.nan
    good = project_missing(lmm, Y, U, S, s2)
    assert good[0] == L.LMM_OK and good[4] == 2
    bad = Y.copy()
    bad[:2, 13] = np.nan
    rc = project_missing(lmm, bad, U, S, s2)[0]
    assert rc == L.LMM_ERR_NOT_PD
    with pytest.raises(L.PosDefException) as e:
        L.check(rc)
    assert e.value.info == 13
    few = Y.copy()
    few[:4, 7] = np.nan                       # p_t = 2 < m
    rc = project_missing(lmm, few, U, S, s2)[0]
    assert rc == L.LMM_ERR_UNSUPPORTED
    info = C.c_int()
    lmm.load().lmm_last_error_detail(None, C.byref(info))
    assert info.value == 7
    again = project_missing(lmm, Y, U, S, s2)
    assert again[0] == L.LMM_OK
    np.testing.assert_array_equal(again[1], good[1])
    np.testing.assert_array_equal(again[2], good[2])
    assert again[3] == good[3]
    # the mirror raises the same errors
    fx = lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S))(lmm.MOInputIsotopicByOutputs(np.arange(n) * 0.3, p), s2)
    with pytest.raises(L.PosDefException):
        lmm.logpdf(fx, bad.reshape(-1))
    with pytest.raises(NotImplementedError, match="point 7"):
        lmm.logpdf(fx, few.reshape(-1))
    assert math.isfinite(lmm.logpdf(fx, Y.reshape(-1)))


# ---------------------------------------------------------------------------------------------------
# 9. the Python mirror, end to end
# ---------------------------------------------------------------------------------------------------
def test_python_mirror_end_to_end(lmm):
    import torch
    n, p, m, s2 = 63, 7, 3, 0.15
    x, U, S, Y = problem(n, 1, p, m, seed=51)
    Y[:, 17] = np.nan                         # a point without any observation: dropped by the mirror
    keep = np.arange(n) != 17
    H = U * np.sqrt(S)
    f = lmm.ILMM(model(lmm, GPS3), lmm.Orthogonal(U, S))
    xin, y = lmm.MOInputIsotopicByOutputs(x, p), Y.reshape(-1)
    ref = restated_logpdf(GPS3, H, x[keep], s2, Y[:, keep])
    val = lmm.logpdf(f(xin, s2), y)
    assert val == pytest.approx(ref, rel=1e-10)          # tests/test_gpu_parity.py:275
    xs = np.linspace(0.2, 5.5, 15)
    xsin = lmm.MOInputIsotopicByOutputs(xs, p)
    mg = lmm.marginals(lmm.posterior(f(xin, s2), y)(xsin, s2))
    mo, vo = restated_marginals(GPS3, H, x[keep], s2, Y[:, keep], xs)
    np.testing.assert_allclose(mg.mu, mo, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(mg.sigma ** 2, vo, rtol=1e-7)
    G = lmm.logpdf_and_gradient(f(xin, s2), y)
    assert G["value"] == pytest.approx(val, rel=1e-12)
    gy = G["y"].reshape(p, n)
    assert np.all(gy[np.isnan(Y)] == 0.0) and np.all(gy[:, 17] == 0.0) and np.all(gy[~np.isnan(Y)] != 0.0)
    # a torch device tensor
    yt = torch.tensor(y, device="cuda:0")
    assert lmm.logpdf(f(xin, s2), yt) == pytest.approx(val, rel=1e-12)
    mt = lmm.marginals(lmm.posterior(f(xin, s2), yt)(xsin, s2))
    np.testing.assert_allclose(mt.mu, mg.mu, rtol=1e-12, atol=1e-12)
    Gt = lmm.logpdf_and_gradient(f(xin, s2), yt)
    assert Gt["y"].is_cuda and Gt["value"] == pytest.approx(val, rel=1e-12)
    np.testing.assert_allclose(Gt["y"].cpu().numpy(), G["y"], rtol=1e-12, atol=1e-12)
    assert Gt["sigma2"] == pytest.approx(G["sigma2"], rel=1e-10)
    # where missing data is not taken
    post = lmm.posterior(f(xin, s2), np.nan_to_num(y))
    y2 = np.random.default_rng(1).standard_normal(15 * p)
    y2[4] = np.nan
    with pytest.raises(NotImplementedError, match="do not take missing data"):
        lmm.posterior(post(xsin, s2), y2)                 # lmm_post_condition
    with pytest.raises(NotImplementedError, match="do not take missing data"):
        lmm.logpdf(post(xsin, s2), y2)                    # predictive logpdf with NaN ys
    with pytest.raises(NotImplementedError, match="do not take missing data"):
        lmm.logpdf(f(xin, s2), np.stack([y, y], axis=1))  # matrix Y
    with pytest.raises(NotImplementedError, match="do not take missing data"):
        lmm.logpdf(lmm.ILMM(model(lmm, GPS3), H)(xin, s2), y)      # dense H
    # the posterior built from data with NaN conditions on complete further data
    y2 = np.nan_to_num(y2)
    po2 = lmm.posterior(lmm.posterior(f(xin, s2), y)(xsin, s2), y2)
    assert np.all(np.isfinite(lmm.marginals(po2(xsin, s2)).mu))
