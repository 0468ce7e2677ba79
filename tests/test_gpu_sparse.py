"""-m gpu: inducing-point (VFE) inference for the OILMM (include/lmm_hip.h "inducing points"): the moments kernel,
elbo / dtc, the exact limit, the bound, approx_posterior and the two refusals that need the library.

The reference for every value is the NumPy restatement in this module: per latent the DENSE formula
    dtc = log N(r; 0, Q_ff + diag w),   elbo = dtc - 1/2 sum_t (k_tt - Q_tt) / w_t,   Q_ff = K_fu (K_uu + eps I)^-1 K_uf,
and for predictions the dense Q-form posterior  mean = mu + Q_*f (Q_ff + W)^-1 r,  var = k_** - Q_*f (Q_ff + W)^-1 Q_f*.
`lowrank_*` restates the library's own algebra (Phi, b, L_u, B, L_B, c) on the CPU; tests/test_sparse_abi.py checks that the two
agree on every case below, and their relative disagreement delta fixes the tolerance: the GPU value must agree with the dense
restatement to max(1e-10, 100 delta) (the factor 100: another summation order over n and the MFMA accumulation order).

delta per case (this module's NumPy, Float64; `python tests/test_gpu_sparse.py` prints the table):

    case                              delta(elbo)   delta(dtc)
    elbo (n, M) = (63, 16)              < 1e-16       4.3e-16
    elbo (n, M) = (333, 70)             4.2e-13       4.2e-13
    elbo (n, M) = (1000, 130)           6.0e-13       3.5e-12
    exact limit n = M = 96              < 1e-16       2.9e-16     (Q_ff against K_ff: 1.4e-10, 1.2e-11)
    posterior (333, 70), n* = 9         mean 1.3e-11  var 9.8e-12
    posterior (333, 70), n* = 70        mean 2.9e-11  var 1.1e-11
    posterior (333, 70), n* = 130       mean 2.9e-11  var 1.1e-11
All are <= 1e-9, as the cases were chosen to be (Matern latents, d = 1, x in [0, 10], z equispaced, eps = 1e-6)."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

LOG2PI = math.log(2.0 * math.pi)
EPS = 1e-6
ELBO_SHAPES = [(63, 16), (333, 70), (1000, 130)]
MOMENT_SHAPES = [(1, 1), (63, 16), (200, 70), (1000, 130)]
NSTAR = [9, 70, 130]


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


# ---------------------------------------------------------------------------------------------------
# the NumPy restatement (kernels are described by (kind, variance, lengthscale[, r]) tuples or ("sum", v0, s0, terms))
# ---------------------------------------------------------------------------------------------------
def cols(x):
    x = np.asarray(x, dtype=np.float64)
    return x[None, :] if x.ndim == 1 else x


def _kbase(k, A, B, v0=1.0, s0=1.0):
    kind, v, ls = k[0], k[1], np.broadcast_to(np.asarray(k[2], dtype=np.float64), (A.shape[0],)) * s0
    D = (A[:, :, None] - B[:, None, :]) / ls[:, None, None]
    if kind == "periodic":
        return v0 * v * np.exp(-0.5 * (np.sin(np.pi * D) ** 2).sum(0) / k[3] ** 2)
    r = np.sqrt((D ** 2).sum(0))
    if kind == "se":
        g = np.exp(-0.5 * r * r)
    elif kind == "matern12":
        g = np.exp(-r)
    elif kind == "matern32":
        g = (1.0 + math.sqrt(3.0) * r) * np.exp(-math.sqrt(3.0) * r)
    else:
        assert kind == "matern52", kind
        g = (1.0 + math.sqrt(5.0) * r + 5.0 * r * r / 3.0) * np.exp(-math.sqrt(5.0) * r)
    return v0 * v * g


def kmat(k, a, b):
    A, B = cols(a), cols(b)
    if k[0] == "sum":
        return sum(_kbase(t, A, B, k[1], k[2]) for t in k[3])
    return _kbase(k, A, B)


def kdiag(k):
    return k[1] * sum(t[1] for t in k[3]) if k[0] == "sum" else k[1]


def to_kernel(lmm, k):
    cls = {"se": lmm.SEKernel, "matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    if k[0] == "sum":
        return lmm.KernelSum(*[to_kernel(lmm, t) for t in k[3]], variance=k[1], lengthscale=k[2])
    if k[0] == "periodic":
        return lmm.PeriodicKernel(k[1], k[2], r=k[3])
    return cls[k[0]](k[1], k[2])


def moments_ref(k, x, z, w, r):
    A = kmat(k, z, x) / np.sqrt(w)[None, :]
    return A @ A.T, A @ (r / np.sqrt(w)), float(np.sum(r * r / w)), float(kdiag(k) * np.sum(1.0 / w)), float(np.sum(np.log(w)))


def dense_latent(k, x, z, w, r, eps, exact=False):
    """(elbo, dtc) of one latent by the dense formula; exact: K_ff in place of Q_ff (the exact log marginal likelihood, twice)."""
    n = len(w)
    Kuf = kmat(k, z, x)
    Lu = np.linalg.cholesky(kmat(k, z, z) + eps * np.eye(Kuf.shape[0]))
    A = sla.solve_triangular(Lu, Kuf, lower=True)
    Q = kmat(k, x, x) if exact else A.T @ A
    Lc = np.linalg.cholesky(Q + np.diag(w))
    v = sla.solve_triangular(Lc, r, lower=True)
    dtc = -0.5 * (n * LOG2PI + 2.0 * np.sum(np.log(np.diag(Lc))) + v @ v)
    return dtc - 0.5 * np.sum((kdiag(k) - np.diag(Q)) / w), dtc


def lowrank_state(k, x, z, w, r, eps):
    Phi, b, s, kap, lam = moments_ref(k, x, z, w, r)
    M = len(b)
    Lu = np.linalg.cholesky(kmat(k, z, z) + eps * np.eye(M))
    Cq = sla.solve_triangular(Lu, sla.solve_triangular(Lu, Phi, lower=True).T, lower=True)
    LB = np.linalg.cholesky(np.eye(M) + 0.5 * (Cq + Cq.T))
    c = sla.solve_triangular(LB, sla.solve_triangular(Lu, b, lower=True), lower=True)
    return Lu, LB, c, Cq, s, kap, lam


def lowrank_latent(k, x, z, w, r, eps):
    """(elbo, dtc) of one latent by the library's algebra."""
    Lu, LB, c, Cq, s, kap, lam = lowrank_state(k, x, z, w, r, eps)
    dtc = -0.5 * (len(w) * LOG2PI + lam + 2.0 * np.sum(np.log(np.diag(LB))) + s - c @ c)
    return dtc - 0.5 * (kap - np.trace(Cq)), dtc


def project(P):
    """(T y)_l (m, n), w_l = sigma2 / S_l and the OILMM regulariser (reference src/oilmm.jl:20-30, 101-113)."""
    U, S, s2, Y = P["U"], P["S"], P["s2"], P["Y"]
    (p, n), m = Y.shape, len(S)
    Ty = (U / np.sqrt(S)[None, :]).T @ Y
    R = Y - U @ (U.T @ Y)
    reg = -0.5 * (n * (np.sum(np.log(S)) + (p - m) * math.log(2.0 * math.pi * s2)) + np.sum(R * R) / s2)
    return Ty, s2 / S, reg


def model_values(P, latent_fn, with_reg=True, **kw):
    Ty, wl, reg = project(P)
    n = P["Y"].shape[1]
    e = t = reg if with_reg else 0.0
    for l, (k, mu) in enumerate(P["gps"]):
        el, tl = latent_fn(k, P["x"], P["z"], np.full(n, wl[l]), Ty[l] - mu, P["eps"], **kw)
        e, t = e + el, t + tl
    return e, t


def predict(P, xs, add_noise, lowrank):
    """(mean, var), each (p, n*) by outputs, of the sparse posterior OILMM at xs."""
    Ty, wl, _ = project(P)
    n, H = P["Y"].shape[1], P["U"] * np.sqrt(P["S"])[None, :]
    ml, vl = [], []
    for l, (k, mu) in enumerate(P["gps"]):
        w, r = np.full(n, wl[l]), Ty[l] - mu
        Ksu = kmat(k, xs, P["z"])
        if lowrank:
            Lu, LB, c, _, _, _, _ = lowrank_state(k, P["x"], P["z"], w, r, P["eps"])
            a = sla.solve_triangular(Lu, Ksu.T, lower=True)
            a2 = sla.solve_triangular(LB, a, lower=True)
            ml.append(mu + a2.T @ c)
            vl.append(kdiag(k) - np.sum(a * a, 0) + np.sum(a2 * a2, 0))
        else:
            Lu = np.linalg.cholesky(kmat(k, P["z"], P["z"]) + P["eps"] * np.eye(Ksu.shape[1]))
            A = sla.solve_triangular(Lu, kmat(k, P["z"], P["x"]), lower=True)
            Qsf = sla.solve_triangular(Lu, Ksu.T, lower=True).T @ A
            Lc = np.linalg.cholesky(A.T @ A + np.diag(w))
            ml.append(mu + Qsf @ sla.cho_solve((Lc, True), r))
            V = sla.solve_triangular(Lc, Qsf.T, lower=True)
            vl.append(kdiag(k) - np.sum(V * V, 0))
    ml, vl = np.array(ml), np.array(vl)
    return H @ ml, (H * H) @ (vl + 1e-18) + (P["s2"] if add_noise else 0.0)


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
MIXED = [(("matern52", 1.2, 0.5), 0.0), (("matern32", 0.8, 0.7), 0.3), (("matern12", 1.0, 1.0), 0.0)]
MOMENT_KERNELS = {
    1: ("matern52", 1.3, 0.5),
    2: ("matern32", 1.1, [0.7, 1.3]),                  # a plain ARD kernel at d > 1: the scaled distance and its square root
    3: ("sum", 1.3, 1.1, [("matern52", 0.8, [0.6, 0.9, 1.4]), ("periodic", 0.5, [2.0, 3.0, 2.5], 0.9)]),
}


def problem(n, M, gps=MIXED, eps=EPS, seed=0, x=None, z=None):
    rng = np.random.default_rng(1000 * n + M + seed)
    p, m = 5, len(gps)
    U = np.linalg.qr(rng.normal(size=(p, m)))[0]
    S = np.array([2.0, 0.7, 1.3])[:m]
    x = np.sort(rng.uniform(0.0, 10.0, n)) if x is None else x
    z = np.linspace(0.0, 10.0, M) if z is None else z
    Y = rng.normal(size=(p, n)) + np.sin(x)[None, :] * rng.normal(size=(p, 1))
    return {"U": U, "S": S, "s2": 0.1, "x": x, "z": z, "Y": Y, "gps": gps, "eps": eps}


def exact_problem():
    gps = [(("matern12", 1.2, 1.0), 0.0), (("matern12", 0.8, 0.7), 0.3), (("matern12", 1.0, 1.0), 0.0)]
    x = 1.5 * np.arange(96.0)
    return problem(96, 96, gps=gps, eps=1e-10, x=x, z=x.copy())


def moment_problem(n, M, d):
    rng = np.random.default_rng(7 * n + M + d)
    x = rng.uniform(0.0, 10.0, (d, n))
    z = np.linspace(0.0, 10.0, M)[None, :] * np.ones((d, 1)) + (0.3 * rng.normal(size=(d, M)) if d > 1 else 0.0)
    return MOMENT_KERNELS[d], x, z, rng.uniform(0.05, 0.5, n), rng.normal(size=n)


def rel(a, b):
    return abs(a - b) / abs(b)


def tol(delta):
    return max(1e-10, 100.0 * delta)


_CACHE = {}


def reference(n, M):
    """The CPU values of one elbo case, computed once per session: problem, dense and low-rank (elbo, dtc) with and without the regulariser."""
    key = (n, M)
    if key not in _CACHE:
        P = exact_problem() if key == (96, 96) else problem(n, M)
        _CACHE[key] = (P, {wr: (model_values(P, dense_latent, wr), model_values(P, lowrank_latent, wr)) for wr in (True, False)})
    return _CACHE[key]


def model(lmm, P):
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(mu, to_kernel(lmm, k)) for k, mu in P["gps"]]), lmm.Orthogonal(P["U"], P["S"]))
    return f, f(lmm.MOInputIsotopicByOutputs(P["x"], 5), P["s2"]), P["Y"].reshape(-1)


# ---------------------------------------------------------------------------------------------------
# lmm_dev_sparse_moments
# ---------------------------------------------------------------------------------------------------
def gpu_moments(lmm, k, x, z, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    d, n, M = x.shape[0], x.shape[1], z.shape[1]
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, zd, wd, rd = dev(x.T), dev(z.T), dev(w), dev(r)
    Phi = torch.full((M, M), float("nan"), dtype=torch.float64, device="cuda")
    b, sc = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gp = L.gps_array([dict(to_kernel(lmm, k).desc(), mean=0.0)])
    L.check(lmm.load().lmm_dev_sparse_moments(xd.data_ptr(), d, n, zd.data_ptr(), M, gp, wd.data_ptr(), rd.data_ptr(), chunk,
                                              Phi.data_ptr(), M, b.data_ptr(), sc.data_ptr()))
    return Phi.cpu().numpy().T, b.cpu().numpy(), sc.cpu().numpy()       # column-major (M, M) -> (row, col)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n,M", MOMENT_SHAPES)
def test_moments(lmm, n, M, d):
    k, x, z, w, r = moment_problem(n, M, d)
    Phi, b, s, kap, lam = moments_ref(k, x, z, w, r)
    chunk = n // 3 + 4 if n >= 3 else 1                # three chunks, the last ragged: 63 -> 25, 25, 13;  1000 -> 337, 337, 326
    assert n < 3 or (2 * chunk < n < 3 * chunk)
    got = {c: gpu_moments(lmm, k, x, z, w, r, c) for c in (0, chunk)}
    low = np.tril_indices(M)
    for c, (gP, gb, gs) in got.items():
        print(f"n={n} M={M} d={d} chunk={c}: Phi {np.abs(gP[low] - Phi[low]).max() / np.abs(Phi).max():.2e}  b {np.abs(gb - b).max() / np.abs(b).max():.2e}  "
              f"s {rel(gs[0], s):.2e} kappa {rel(gs[1], kap):.2e} lambda {rel(gs[2], lam):.2e}")
        assert np.abs(gP[low] - Phi[low]).max() <= 1e-10 * np.abs(Phi).max()
        assert np.isnan(gP[np.triu_indices(M, 1)]).all()           # only the lower triangle is written
        assert np.abs(gb - b).max() <= 1e-10 * np.abs(b).max()
        assert rel(gs[0], s) <= 1e-10 and rel(gs[1], kap) <= 1e-10 and rel(gs[2], lam) <= 1e-10
    (P0, b0, s0), (P1, b1, s1) = got[0], got[chunk]
    assert np.abs(P0[low] - P1[low]).max() <= 1e-10 * np.abs(Phi).max() and np.abs(b0 - b1).max() <= 1e-10 * np.abs(b).max()
    assert np.allclose(s0, s1, rtol=1e-10, atol=0.0)
    again = gpu_moments(lmm, k, x, z, w, r, chunk)                   # the same chunking twice: bitwise
    for u, v in zip(got[chunk], again):
        assert np.array_equal(u[low] if u.ndim == 2 else u, v[low] if v.ndim == 2 else v)


# a sum latent without a periodic term (sparse_moments_kernel's own instantiation; the d = 3 kernel above has one): the same checks
def test_moments_sum_latent(lmm, monkeypatch):
    monkeypatch.setitem(MOMENT_KERNELS, 2, ("sum", 1.3, 1.1, [("matern52", 0.8, [0.6, 0.9]), ("se", 0.5, 1.4)]))
    test_moments(lmm, 63, 16, 2)


# ---------------------------------------------------------------------------------------------------
# elbo, dtc, the bound, the exact limit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n,M", ELBO_SHAPES)
def test_elbo_and_dtc(lmm, n, M, with_reg):
    import torch
    P, ref = reference(n, M)
    (de, dt), (le, lt) = ref[with_reg]
    f, fx, y = model(lmm, P)
    vfe = lmm.VFE(P["z"], EPS)
    e, t = lmm.elbo(vfe, fx, y, with_reg), lmm.dtc(vfe, fx, y, with_reg)
    print(f"n={n} M={M} reg={with_reg}: elbo {e:.12f} ref {de:.12f} rel {rel(e, de):.2e} (delta {rel(le, de):.2e});  "
          f"dtc {t:.12f} ref {dt:.12f} rel {rel(t, dt):.2e} (delta {rel(lt, dt):.2e})")
    assert rel(le, de) <= 1e-9 and rel(lt, dt) <= 1e-9
    assert rel(e, de) <= tol(rel(le, de))
    assert rel(t, dt) <= tol(rel(lt, dt))
    assert e <= t                                                   # the bound
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    assert lmm.elbo(vfe, fx, yd, with_reg) == e and lmm.dtc(vfe, fx, yd, with_reg) == t
    if n <= 333:
        assert e <= lmm.logpdf(fx, y, with_reg)


def test_exact_limit(lmm):
    """z = x, Matern12 with the points 1.5 lengthscales (or more) apart, eps = 1e-10: Q_ff = K_ff up to eps, so elbo = dtc = logpdf."""
    P, ref = reference(96, 96)
    (de, dt), (le, lt) = ref[True]
    ex = model_values(P, dense_latent, True, exact=True)[1]
    d_exact = max(rel(de, ex), rel(dt, ex), rel(le, de), rel(lt, dt))
    f, fx, y = model(lmm, P)
    vfe = lmm.VFE(P["z"], 1e-10)
    e, t, lp = lmm.elbo(vfe, fx, y), lmm.dtc(vfe, fx, y), lmm.logpdf(fx, y)
    print(f"exact limit: elbo {e:.12f} dtc {t:.12f} logpdf {lp:.12f} restated {ex:.12f}; Q_ff against K_ff {d_exact:.2e}")
    assert d_exact <= 1e-9
    assert rel(e, ex) <= tol(d_exact) and rel(t, ex) <= tol(d_exact) and rel(lp, ex) <= tol(d_exact)
    assert rel(e, lp) <= tol(d_exact) and rel(t, lp) <= tol(d_exact)
    assert e <= t and e <= lp + tol(d_exact) * abs(lp)


# ---------------------------------------------------------------------------------------------------
# approx_posterior
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def posterior_case(lmm):
    P, _ = reference(333, 70)
    f, fx, y = model(lmm, P)
    return P, lmm.approx_posterior(lmm.VFE(P["z"], EPS), fx, y)


@pytest.mark.parametrize("ns", NSTAR)
def test_approx_posterior(lmm, posterior_case, ns):
    P, po = posterior_case
    xs = np.linspace(-0.5, 10.5, ns) + 0.013
    fxs = po(lmm.MOInputIsotopicByOutputs(xs, 5), P["s2"])
    for add_noise in (True, False):
        rm, rv = predict(P, xs, add_noise, lowrank=False)
        lm, lv = predict(P, xs, add_noise, lowrank=True)
        dm, dv = np.abs(lm - rm).max() / np.abs(rm).max(), np.abs(lv - rv).max() / np.abs(rv).max()
        gm, gv = lmm.mean_and_var(fxs, add_noise)
        gm, gv = gm.reshape(5, ns), gv.reshape(5, ns)
        em, ev = np.abs(gm - rm).max() / np.abs(rm).max(), np.abs(gv - rv).max() / np.abs(rv).max()
        print(f"n*={ns} add_noise={add_noise}: mean {em:.2e} (delta {dm:.2e})  var {ev:.2e} (delta {dv:.2e})")
        assert dm <= 1e-9 and dv <= 1e-9
        assert em <= tol(dm) and ev <= tol(dv)
        assert (gv > 0.0).all()
    rm, rv = predict(P, xs, True, lowrank=False)
    lm, lv = predict(P, xs, True, lowrank=True)
    dm, dv = np.abs(lm - rm).max() / np.abs(rm).max(), np.abs(lv - rv).max() / np.abs(rv).max()
    N = lmm.marginals(fxs)
    assert np.abs(N.mu.reshape(5, ns) - rm).max() <= tol(dm) * np.abs(rm).max()
    assert np.abs(N.sigma.reshape(5, ns) ** 2 - rv).max() <= tol(dv) * np.abs(rv).max()
    assert np.abs(lmm.mean(fxs).reshape(5, ns) - rm).max() <= tol(dm) * np.abs(rm).max()
    assert np.abs(lmm.var(fxs).reshape(5, ns) - rv).max() <= tol(dv) * np.abs(rv).max()


# ---------------------------------------------------------------------------------------------------
# refusals that come from the library
# ---------------------------------------------------------------------------------------------------
def test_failing_pivot_names_the_latent(lmm):
    """Two coincident inducing points and a jitter below the rounding of K_uu's diagonal: the pivot of the second one is not > 0.  A
    status code of a completed launch."""
    P, _ = reference(63, 16)
    f, fx, y = model(lmm, P)
    z = P["z"].copy()
    z[1] = z[0]
    with pytest.raises(lmm.PosDefException, match="latent") as ei:
        lmm.elbo(lmm.VFE(z, 1e-300), fx, y)
    assert 0 <= ei.value.latent < 3 and ei.value.info > 0
    with pytest.raises(lmm.PosDefException, match="latent"):
        lmm.approx_posterior(lmm.VFE(z, 1e-300), fx, y)
    e = lmm.elbo(lmm.VFE(P["z"], EPS), fx, y)                       # the library is usable afterwards
    assert rel(e, reference(63, 16)[1][True][0][0]) <= 1e-9


def test_more_than_1024_inducing_points_are_refused(lmm):
    P, _ = reference(63, 16)
    f, fx, y = model(lmm, P)
    vfe = lmm.VFE(np.linspace(0.0, 10.0, 1025), EPS)
    with pytest.raises(NotImplementedError, match="1024"):
        lmm.elbo(vfe, fx, y)
    with pytest.raises(NotImplementedError, match="1024"):
        lmm.approx_posterior(vfe, fx, y)


def delta_table():
    rows = []
    for n, M in ELBO_SHAPES + [(96, 96)]:
        P, ref = reference(n, M)
        (de, dt), (le, lt) = ref[True]
        rows.append((f"elbo (n, M) = ({n}, {M})", rel(le, de), rel(lt, dt)))
    P, _ = reference(96, 96)
    ex = model_values(P, dense_latent, True, exact=True)[1]
    rows.append(("exact limit: Q_ff against K_ff", rel(reference(96, 96)[1][True][0][0], ex), rel(reference(96, 96)[1][True][0][1], ex)))
    P, _ = reference(333, 70)
    for ns in NSTAR:
        xs = np.linspace(-0.5, 10.5, ns) + 0.013
        (rm, rv), (lm, lv) = predict(P, xs, True, False), predict(P, xs, True, True)
        rows.append((f"posterior (333, 70), n* = {ns} (mean, var)", np.abs(lm - rm).max() / np.abs(rm).max(), np.abs(lv - rv).max() / np.abs(rv).max()))
    return rows


if __name__ == "__main__":
    for name, a, b in delta_table():
        print(f"{name:48s} {a:.1e}  {b:.1e}")
