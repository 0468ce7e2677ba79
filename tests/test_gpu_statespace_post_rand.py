"""-m gpu: sampling from the state-space posterior object (include/lmm_hip.h "state space: sampling from the posterior object";
DESIGN.md 4.18 "Sampling from the posterior object"): the block lmm_dev_statespace_post_sample against the sequential restatement on
fixed normals, its law against the dense Gaussian joint posterior, every shape of window, a window long enough for three levels of the
scan, StateSpacePosterior.rand end to end against the dense OILMM posterior, reproducibility, and the C ABI's refusals.  The states
the block reads come from lmm_dev_statespace_states.

Tolerance (the rule of tests/test_gpu_statespace.py): max(1e-10, 100 DELTA) of max|reference| per array, DELTA the largest of
test_statespace_abi.delta() (7.6e-15), test_statespace_posterior_abi.delta_posterior() (1.7e-13) and
test_statespace_post_rand_abi.delta_post_rand() (5.2e-13): 1e-10.  Covariances are measured against the latent's variance (the
outputs': max|reference|).  For fixed normals a path is ill-conditioned in the spacings where they are small against the lengthscale
(its law is not), so the fixed-normal comparisons keep every query at least 0.05 lengthscales from every other window point; the law
tests put queries on training inputs and 1e-9 beside them.  The reference is always the NumPy restatement, the dense Gaussian or
another path of the library, never the code under test.  On an MI355X the largest error any comparison saw was 6.9e-13 of
max|reference| (the three-level window) and 1.5e-15 of the variance on a law."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_statespace as GS
import test_gpu_statespace_posterior as PG
import test_gpu_statespace_rand as GR
import test_sho_abi as S
import test_statespace_abi as T
import test_statespace_posterior_abi as PA
import test_statespace_post_rand_abi as PR

pytestmark = pytest.mark.gpu

LATENTS = tuple(T.KINDS) + (("sho", 2.0),)
VAR, ELL = 1.3, 0.7


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * max(T.delta(), PA.delta_posterior(), PR.delta_post_rand()))


def close(got, ref, tol, what="", scale=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, scale = np.abs(got - ref).max(), np.abs(ref).max() if scale is None else scale
    print(f"{what} err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def model_of(lat):
    return PA.model_of(lat, VAR, ELL) if lat in T.KINDS else S.sho(VAR, ELL, lat[1])


def separated_case(lat, n, seed=0):
    """(model, x, w, r): spacings of 0.1 - 1 lengthscales; the first and the last point unobserved (n >= 2), and runs of unobserved
    points longer than a chunk of 7 (n >= 17) and of 64 (n >= 1000)."""
    rng = np.random.default_rng([seed, n, LATENTS.index(lat)])
    x = np.cumsum(ELL * rng.uniform(0.1, 1.0, n)) - 1.0
    w, r = rng.uniform(0.05, 0.5, n), rng.standard_normal(n)
    if n >= 2:
        w[0] = w[-1] = np.inf
    if n >= 17:
        w[3:12] = np.inf
    if n >= 1000:
        w[100:180] = np.inf
    return model_of(lat), x, w, r


def separated_queries(x, lo, hi, count, seed=0):
    """`count` sorted queries, each at least 0.05 lengthscales from every training input and every other query: one half a
    lengthscale outside [lo, hi] at either end, the others uniform on [lo, hi]."""
    rng = np.random.default_rng([seed, len(x), count])
    out = [lo - 0.5 * ELL, hi + 0.5 * ELL]
    taken = list(x) + out
    for c in rng.uniform(lo, hi, 20 * count):
        if len(out) < count and np.abs(np.asarray(taken) - c).min() >= 0.05 * ELL:
            out.append(c)
            taken.append(c)
    assert len(out) == count
    return np.sort(np.array(out))


def gpu_post_sample(lmm, model, x, fpk, spk, q, Z, chunk):
    """lmm_dev_statespace_post_sample: Z (N, D W) -> f (N, ns)."""
    import torch
    from lmm_amd import _lib as L
    Z = np.atleast_2d(Z)
    xd, fd, sd, qd, zd = PG.dev(x), PG.dev(fpk), PG.dev(spk), PG.dev(q), PG.dev(Z)
    f = PG.nan_dev(Z.shape[0], len(q))
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])                       # the mean is not read
    L.check(lmm.load().lmm_dev_statespace_post_sample(xd.data_ptr(), len(x), gp, fd.data_ptr(), sd.data_ptr(), qd.data_ptr(), len(q),
                                                      zd.data_ptr(), Z.shape[0], chunk, f.data_ptr()))
    return f.cpu().numpy()


_STATES = {}


def states_of(lmm, key, model, x, w, r):
    """(restated states, the packed states of lmm_dev_statespace_states), computed once per case."""
    if key not in _STATES:
        _STATES[key] = (PA.full_states(model, x, w, r), PG.gpu_states(lmm, model, x, w, r, 0))
    return _STATES[key]


# ---------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 1000])
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_block_vs_restatement_on_fixed_normals(lmm, tol, lat, n):
    """Queries over the whole range and two lengthscales beyond either end; n = 17 and 1000 have runs of unobserved training points
    longer than a chunk inside the window.  chunk = 7 at n = 1000 has more aggregates than one workgroup of the scan takes."""
    model, x, w, r = separated_case(lat, n)
    q = separated_queries(x, x[0] - 2.0 * ELL, x[-1] + 2.0 * ELL, 12 if n < 1000 else 60)
    st, (gf, gs) = states_of(lmm, ("sep", lat, n), model, x, w, r)
    W = len(PR.window(x, q)[2])
    assert W == len(q) + n                                                           # every training point lies inside the window
    zeta = np.random.default_rng([n, 3]).standard_normal((2, model.D * W))
    ref = PR.sample_paths(model, x, st, q, zeta)
    got = {}
    for chunk in (7, 1, 0):
        got[chunk] = gpu_post_sample(lmm, model, x, gf, gs, q, zeta, chunk)
        close(got[chunk], ref, tol, f"chunk {chunk}")
    again = gpu_post_sample(lmm, model, x, gf, gs, q, zeta, 7)
    assert (again == got[7]).all()                                                   # bitwise
    one = gpu_post_sample(lmm, model, x, gf, gs, q, zeta[1:], 7)
    assert (one[0] == got[7][1]).all()                                               # a sample does not depend on its neighbours


def law_case(lat):
    """n = 40 at spacings of 0.01 - 1 lengthscales with unobserved runs, and 30 queries: 19 uniform, 5 training inputs, both ends,
    1e-9 beyond either end, two duplicates."""
    if lat in T.KINDS:
        v, ell, x, w, r = T.case(lat, 40)
        model = PA.model_of(lat, v, ell)
    else:
        v, P, x, w, r = S.case(lat[1], 40)
        model = S.sho(v, P, lat[1])
    w = GR.unobserved_runs(w.copy(), 40)
    w[20:30] = np.inf
    rng = np.random.default_rng([40, LATENTS.index(lat)])
    u = rng.uniform(x[0] - 2.0, x[-1] + 2.0, 19)
    q = np.concatenate([u, rng.choice(x, 5, replace=False), [x[0], x[-1], x[0] - 1e-9, x[-1] + 1e-9], u[:2]])
    assert len(q) == 30
    return model, x, w, r, np.sort(q, kind="stable")


@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_law_of_the_block(lmm, tol, lat):
    """Sample 0 has zero normals, the others the D W unit vectors: sample 0 is the posterior mean, and the differences B span the
    covariance, B B' = the dense joint posterior covariance at the queries."""
    model, x, w, r, q = law_case(lat)
    gf, gs = PG.gpu_states(lmm, model, x, w, r, 0)
    W = len(PR.window(x, q)[2])
    E = np.vstack([np.zeros((1, model.D * W)), np.eye(model.D * W)])
    dm, dS = PR.dense_joint(model, x, w, r, q)
    im, iv = PG.gpu_interp(lmm, model, x, gf, gs, q)
    for chunk in (7, 1):
        f = gpu_post_sample(lmm, model, x, gf, gs, q, E, chunk)
        close(f[0], im, tol, f"chunk {chunk}: mean vs interp")
        close(f[0], dm, tol, f"chunk {chunk}: mean vs dense")
        B = (f[1:] - f[:1]).T
        close(B @ B.T, dS, tol, f"chunk {chunk}: law", scale=model.v)
        close(np.diag(B @ B.T), iv, tol, f"chunk {chunk}: variances vs interp", scale=model.v)


WINDOWS = ("behind", "front", "one", "gap", "span")


@pytest.mark.parametrize("shape", WINDOWS)
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_window_shapes(lmm, tol, lat, shape):
    """n = 17.  behind: every query behind the data (W = ns, no training point is touched); front: every query in front of it; one: a
    single query; gap: every query inside one gap between two training points (count = 0); span: queries around all of the data."""
    model, x, w, r = separated_case(lat, 17)
    gap = int(np.argmax(np.diff(x)))
    q = {"behind": x[-1] + ELL * np.array([0.06, 0.3, 0.9, 2.5, 6.0]),
         "front": x[0] - ELL * np.array([5.0, 1.1, 0.4, 0.07]),
         "one": np.array([0.5 * (x[8] + x[9])]),
         "gap": x[gap] + (x[gap + 1] - x[gap]) * np.array([0.2, 0.5, 0.8]),
         "span": np.concatenate([[x[0] - 0.3], 0.5 * (x[4:9] + x[5:10]), [x[-1] + 0.3]])}[shape]
    st, (gf, gs) = states_of(lmm, ("sep", lat, 17), model, x, w, r)
    a, b, src = PR.window(x, q)
    W = len(src)
    assert W - len(q) == {"behind": 0, "front": 0, "one": 0, "gap": 0, "span": 17}[shape]
    mean, M = PR.sample_map(model, x, st, q)
    E = np.vstack([np.zeros((1, model.D * W)), np.eye(model.D * W), np.random.default_rng(1).standard_normal((1, model.D * W))])
    for chunk in (0, 2):
        f = gpu_post_sample(lmm, model, x, gf, gs, q, E, chunk)
        close(f[0], mean, tol, f"chunk {chunk}: mean")
        close((f[1:-1] - f[:1]).T, M, tol, f"chunk {chunk}: map")
        close(f[-1], mean + M @ E[-1], tol, f"chunk {chunk}: path")
    dm, dS = PR.dense_joint(model, x, w, r, q)
    close(M @ M.T, dS, 1e-12, "restated law", scale=model.v)


def test_three_scan_levels(lmm, tol):
    """W = 16500 at chunk = 1 (16000 training points inside the window and 500 queries, Matern52): 16500 aggregates, 129 workgroups of
    the scan, whose totals take two workgroups, whose totals take a third level."""
    n, lat = 16000, "matern52"
    model, x, w, r = separated_case(lat, n)
    gaps = np.random.default_rng(2).choice(n - 1, 498, replace=False)
    q = np.sort(np.concatenate([[x[0] - 0.5 * ELL], 0.5 * (x[gaps] + x[gaps + 1]), [x[-1] + 0.5 * ELL]]))
    st, (gf, gs) = states_of(lmm, ("sep", lat, n), model, x, w, r)
    W = len(PR.window(x, q)[2])
    assert W == 16500 and W > 128 * 128
    zeta = np.random.default_rng(4).standard_normal((1, model.D * W))
    ref = PR.sample_paths(model, x, st, q, zeta)
    close(gpu_post_sample(lmm, model, x, gf, gs, q, zeta, 1), ref, tol, "chunk 1")
    close(gpu_post_sample(lmm, model, x, gf, gs, q, zeta, 0), ref, tol, "chunk 0")


# ---------------------------------------------------------------------------------------------------
# the entry point and its mirror
# ---------------------------------------------------------------------------------------------------
DIMS = (1, 2, 3, 2)          # GS.GPS (Matern12, 32, 52) and PG.SHO


def entry_problem():
    """m = 4 latents, one of each kind, p = 5, n = 60 with NaN entries (every point keeps >= 4 of its 5 outputs); 21 queries in
    shuffled order: inside, behind and in front of the data, one on a training input, one duplicate."""
    x, U, Sv, Y, gps = PG.complete_problem(60, True)
    Y = Y.copy()
    Y[1, 7] = Y[3, 20] = Y[0, 41] = np.nan
    rng = np.random.default_rng(60)
    xs = np.concatenate([rng.uniform(x[10], x[30], 12), x[-1] + np.array([0.2, 0.9, 2.0, 4.0]), x[0] - np.array([0.1, 0.8, 2.5]), [x[17]]])
    xs = rng.permutation(np.append(xs, xs[3]))
    return x, U, Sv, Y, gps, xs


def test_entry_point(lmm, tol):
    x, U, Sv, Y, gps, xs = entry_problem()
    n, ns, p, y = len(x), len(xs), Y.shape[0], Y.reshape(-1)
    fx = PG.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), PG.S2)
    dense = lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(xs, p), PG.S2)
    cm, cc = lmm.mean_and_cov(dense)                                                  # the library's Cholesky path, noise included
    with lmm.statespace_posterior(fx, y) as post:
        first, count = post.window(xs)
        assert first == (x <= xs.min()).sum() and count == (x <= xs.max()).sum() - first
        W = ns + count
        for add_noise in (True, False):
            total = sum(DIMS) * W + (ns * p if add_noise else 0)
            out = post.rand(GR.UnitVectors(total), xs, N=total + 1, add_noise=add_noise)
            assert isinstance(out, np.ndarray) and out.shape == (ns * p, total + 1)
            close(out[:, 0], post.mean(xs), tol, "zero normals: post.mean")
            close(out[:, 0], cm, tol, "zero normals: dense mean")
            B = out[:, 1:] - out[:, :1]
            cov = B @ B.T + (0.0 if add_noise else PG.S2) * np.eye(ns * p)
            close(cov, cc, tol, f"law, add_noise={add_noise}")
            close(np.diag(B @ B.T), post.var(xs, add_noise), tol, f"variances, add_noise={add_noise}")
        # the callers' order: a permutation of the queries permutes the rows (the normals belong to sorted positions)
        perm = np.random.default_rng(1).permutation(ns)
        rec = GR.Recorder(8)
        a = post.rand(rec, xs).reshape(p, ns)
        b = post.rand(GR.Replay(rec.draws), xs[perm]).reshape(p, ns)
        distinct = np.array([np.sum(xs == v) == 1 for v in xs])                       # equal queries keep their order, not their rows
        assert (b[:, distinct[perm]] == a[:, perm][:, distinct[perm]]).all()
        assert post.rand(np.random.default_rng(0), np.zeros(0)).shape == (0,)
    with pytest.raises(ValueError, match="closed"):
        post.rand(np.random.default_rng(0), xs)


def recording_device_normals(lmm, seed):
    """A DeviceNormals that keeps (on the host) what it drew."""
    class Rec(lmm.DeviceNormals):
        def __init__(self, seed):
            super().__init__(seed)
            self.draws = []

        def standard_normal(self, count):
            out = super().standard_normal(count)
            self.draws.append(out.cpu().numpy())
            return out
    return Rec(seed)


def test_reproducibility_and_device_normals(lmm):
    import torch
    x, U, Sv, Y, gps, xs = entry_problem()
    p, y = Y.shape[0], Y.reshape(-1)
    fx = PG.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), PG.S2)
    with lmm.statespace_posterior(fx, y) as post:
        for kw in (dict(), dict(add_noise=False)):
            rec = GR.Recorder(3)
            five = post.rand(rec, xs, N=5, **kw)
            again = post.rand(GR.Replay(rec.draws), xs, N=5, **kw)
            assert five.shape == (len(xs) * p, 5) and (five == again).all()           # two calls: bitwise
            per = len(rec.draws) // 5
            assert per == len(DIMS) + int(kw.get("add_noise", True))
            for k in range(5):                                                        # column k is the single-sample call on its normals
                one = post.rand(GR.Replay(rec.draws[k * per:(k + 1) * per]), xs, **kw)
                assert one.shape == (len(xs) * p,) and (one == five[:, k]).all()
            dn = recording_device_normals(lmm, 5)
            dev2 = post.rand(dn, xs, N=2, **kw)
            assert torch.is_tensor(dev2) and dev2.is_cuda and dev2.shape == (len(xs) * p, 2)
            host2 = post.rand(GR.Replay(dn.draws), xs, N=2, **kw)                     # the same values from the host
            assert isinstance(host2, np.ndarray) and (host2 == dev2.cpu().numpy()).all()
            d1 = post.rand(lmm.DeviceNormals(5), xs, **kw)
            assert d1.is_cuda and (d1 == dev2[:, 0]).all()
        # torch device queries with host normals: host result, the same numbers
        rec = GR.Recorder(4)
        a = post.rand(rec, xs)
        b = post.rand(GR.Replay(rec.draws), torch.tensor(xs, device="cuda"))
        assert isinstance(b, np.ndarray) and (a == b).all()
        assert post.window(torch.tensor(xs, device="cuda")) == post.window(xs)


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals(lmm, tol):
    from lmm_amd import _lib as L
    x, U, Sv, Y, gps, xs = entry_problem()
    p, y = Y.shape[0], Y.reshape(-1)
    fx = PG.model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), PG.S2)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    q = np.sort(xs)
    ns = len(q)
    with lmm.statespace_posterior(fx, y) as post:
        h = post._ptr
        first, count = C.c_int(-1), C.c_int(-1)

        def window(lo, hi, post=h, a=C.byref(first), b=C.byref(count)):
            return lib.lmm_statespace_post_window(post, lo, hi, a, b)

        assert window(q[0], q[-1]) == L.LMM_OK
        assert (first.value, count.value) == ((x <= q[0]).sum(), (x <= q[-1]).sum() - (x <= q[0]).sum())
        assert window(x[-1] + 1.0, x[-1] + 2.0) == L.LMM_OK and (first.value, count.value) == (len(x), 0)
        assert window(x[0] - 2.0, x[0] - 1.0) == L.LMM_OK and (first.value, count.value) == (0, 0)
        assert window(x[5], x[5]) == L.LMM_OK and (first.value, count.value) == (6, 0)
        for lo, hi in ((1.0, 0.5), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf)):
            assert window(lo, hi) == L.LMM_ERR_ARG
        assert window(0.0, 1.0, post=None) == L.LMM_ERR_ARG and window(0.0, 1.0, a=None) == L.LMM_ERR_ARG
        assert window(0.0, 1.0, b=None) == L.LMM_ERR_ARG
        W = ns + (x <= q[-1]).sum() - (x <= q[0]).sum()
        z, eps, out = np.zeros(sum(DIMS) * W), np.zeros(ns * p), np.full(ns * p, np.nan)
        ptr = lambda a: None if a is None else L.Arr(a).ptr

        def call(post=h, xs=q, ns=ns, z=z, eps=eps, N=1, noise=1, o=out):
            rc = lib.lmm_oilmm_statespace_post_rand(post, ptr(xs), ns, ptr(z), ptr(eps), N, noise, None if o is None else L.Arr(o, True).ptr)
            lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
            return rc, lib.lmm_last_error_string()

        assert call()[0] == L.LMM_OK
        close(out, post.mean(q), tol, "zero normals through the C ABI")
        assert call(noise=0, eps=None)[0] == L.LMM_OK
        # an unsorted or non-finite xs: LMM_ERR_ARG with the first offending index
        bad = q.copy()
        bad[9], bad[10] = q[10] + 1e-3, q[9]
        assert bad[10] < bad[9]
        rc, msg = call(xs=bad)
        assert rc == L.LMM_ERR_ARG and info.value == 10 and b"[10]" in msg
        for value, at in ((np.nan, 7), (np.inf, ns - 1), (-np.inf, 0)):
            bad = q.copy()
            bad[at] = value
            rc, msg = call(xs=bad)
            assert rc == L.LMM_ERR_ARG and info.value == at and b"xs[%d]" % at in msg
        for kw, code, text in ((dict(eps=None), L.LMM_ERR_ARG, b"eps is NULL"), (dict(z=None), L.LMM_ERR_ARG, b"z is NULL"),
                               (dict(post=None), L.LMM_ERR_ARG, b"bad arguments"), (dict(xs=None), L.LMM_ERR_ARG, b"bad arguments"),
                               (dict(o=None), L.LMM_ERR_ARG, b"bad arguments"), (dict(ns=0), L.LMM_ERR_ARG, b"bad arguments"),
                               (dict(ns=-2), L.LMM_ERR_ARG, b"bad arguments"), (dict(N=0), L.LMM_ERR_ARG, b"nsamples"),
                               (dict(N=-1), L.LMM_ERR_ARG, b"nsamples")):
            rc, msg = call(**kw)
            assert rc == code and text in msg, (kw, rc, msg)
        lmm.set_compute_dtype("f32")
        try:
            rc, msg = call()
            assert rc == L.LMM_ERR_UNSUPPORTED and b"Float64 only" in msg
        finally:
            lmm.set_compute_dtype("f64")
        # the next valid call is served
        out[:] = np.nan
        assert call()[0] == L.LMM_OK
        close(out, post.mean(q), tol, "after the refusals")
    # the block: NULL, sizes, the fp32 mode
    model, xb, w, r = separated_case("matern32", 17)
    gf, gs = PG.gpu_states(lmm, model, xb, w, r, 0)
    qb = np.array([xb[3] + 0.05, xb[9] + 0.05])
    Wb = 2 + 6
    xd, fd, sd, qd, zd, f = PG.dev(xb), PG.dev(gf), PG.dev(gs), PG.dev(qb), PG.dev(np.zeros(2 * Wb)), PG.nan_dev(2)
    gp = L.gps_array([model.desc()])
    P = lambda t: None if t is None else t.data_ptr()

    def block(x=xd, n=17, gp=gp, fs=fd, ss=sd, xs=qd, ns=2, z=zd, N=1, chunk=0, f=f):
        return lib.lmm_dev_statespace_post_sample(P(x), n, gp, P(fs), P(ss), P(xs), ns, P(z), N, chunk, P(f))

    assert block() == L.LMM_OK
    im, _ = PG.gpu_interp(lmm, model, xb, gf, gs, qb)
    close(f.cpu().numpy(), im, tol, "block with zero normals")
    for kw in (dict(x=None), dict(gp=None), dict(fs=None), dict(ss=None), dict(xs=None), dict(z=None), dict(f=None), dict(n=0), dict(ns=0),
               dict(N=0), dict(chunk=-1)):
        assert block(**kw) == L.LMM_ERR_ARG, kw
    assert block(xs=PG.dev(qb[::-1])) == L.LMM_ERR_ARG
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert info.value == 1
    lmm.set_compute_dtype("f32")
    try:
        assert block() == L.LMM_ERR_UNSUPPORTED and b"Float64 only" in lib.lmm_last_error_string()
    finally:
        lmm.set_compute_dtype("f64")
