"""Sampling on the Toeplitz path on the GPU (DESIGN.md 4.22 "Sampling").  With J steps per launch, R rows per workgroup and NS samples
per pass the sizes sit on toep_schur_sample_kernel's boundaries, as test_gpu_toeplitz_blocked.py's do.  References are dense NumPy for
the same normals; every matrix they factor has condition number <= 1e5 (the model level runs at h = 0.7 with jitter 0.05, which the
periodic latents need: test_toeplitz_rand_abi).  Tolerance, relative to max |reference|: 1e-10, the CPU restatement's deltas
(delta_toeplitz_rand 1.6e-13, delta_toeplitz_post_rand 1.7e-12) being <= 1e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_toeplitz import CTOR, MIXES, P_OUT, S2
from test_gpu_toeplitz_blocked import J, R
from test_toeplitz_abi import LATENTS, row, toeplitz

pytestmark = pytest.mark.gpu
NS, TOL, HG, JIT = 4, 1e-10, 0.7, 0.05


def sample(t, Z):
    """lmm_dev_toeplitz_sample: the columns of L Z, L L' = Toeplitz(t)"""
    import torch
    lmm.init(0)
    td, zd = torch.tensor(t, device="cuda"), torch.tensor(np.ascontiguousarray(Z.T), device="cuda")
    fd = torch.empty_like(zd)
    L.check(lmm.load().lmm_dev_toeplitz_sample(td.data_ptr(), zd.data_ptr(), len(t), Z.shape[1], fd.data_ptr()))
    return fd.cpu().numpy().T


@functools.lru_cache(maxsize=None)
def dense_factor(n):
    t = row(LATENTS["lp"] + LATENTS["matern52"], 0.013 * np.arange(n)); t[0] += 0.1
    return t, np.linalg.cholesky(toeplitz(t))


@pytest.mark.parametrize("N", (1, NS, NS + 1))
@pytest.mark.parametrize("n", (1, 2, 3, J, J + 1, 2 * J + 1, R, R + 1, R + J + 1, 2 * R + J + 3))
def test_building_block_against_dense_cholesky(n, N):
    t, Lc = dense_factor(n)
    Z = np.random.default_rng(7 * n + N).standard_normal((n, N))
    ref, got = Lc @ Z, sample(t, Z)
    print(f"n={n} N={N}: {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
    assert np.abs(got - ref).max() <= TOL * np.abs(ref).max()
    assert np.array_equal(got, sample(t, Z))                          # two calls are bitwise equal
    assert np.array_equal(got[:, -1], sample(t, Z[:, -1:])[:, 0])     # a column is the one-sample call on its normals


@pytest.mark.parametrize("kind", ("se", "periodic"))
def test_the_law_with_the_default_jitter(kind):
    n = R + J + 1
    t = row(LATENTS[kind], 0.01 * np.arange(n)); t[0] += 1e-9
    Lg = sample(t, np.eye(n))
    err = np.abs(Lg @ Lg.T - toeplitz(t)).max()
    print(f"{kind}: max |L L' - K| = {err:.2e}")
    assert err <= TOL * t[0] and np.array_equal(Lg, np.tril(Lg))


def model(names, n):
    rng = np.random.default_rng(n)
    x, S = 0.5 + HG * np.arange(n), np.array([1.0, 1.6, 0.7])
    U = np.linalg.qr(rng.standard_normal((P_OUT, len(names))))[0]
    ks = [CTOR[LATENTS[k][0][0]](*LATENTS[k][0][1:]) if len(LATENTS[k]) == 1 else lmm.KernelSum(*[CTOR[t[0]](*t[1:]) for t in LATENTS[k]])
          for k in names]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, S))
    return f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2), rng.standard_normal(n * P_OUT), U, S


@functools.lru_cache(maxsize=None)
def dense_latents(names, n, nt):
    """per latent: K over the nt points, cholesky(K + JIT I), (K_xx + w I)^-1 K_x,all -- each factored matrix with cond <= 1e5"""
    out = []
    for l, k in enumerate(names):
        K = toeplitz(row(LATENTS[k], HG * np.arange(nt)))
        Kw = K[:n, :n] + (S2 / np.array([1.0, 1.6, 0.7])[l]) * np.eye(n)
        for A in (K + JIT * np.eye(nt), Kw):
            ev = np.linalg.eigvalsh(A)
            assert ev[-1] <= 1e5 * ev[0], (k, nt)
        out.append((np.linalg.cholesky(K + JIT * np.eye(nt)), np.linalg.solve(Kw, K[:n]).T))
    return out


def dense_sample(names, n, hz, U, S, y, rng, Ns, add_noise):
    """the draw order of toeplitz_rand against dense Gaussians: y None for the prior"""
    nt, m, cols = n + hz, len(names), []
    for _ in range(Ns):
        z = [rng.standard_normal(nt) for _ in range(m)]
        xi = rng.standard_normal(m * n).reshape(m, n) if y is not None else None
        F = np.zeros((m, nt))
        for l, (Lc, G) in enumerate(dense_latents(names, n, nt)):
            F[l] = Lc @ z[l]
            if y is not None:
                F[l] += G @ (U[:, l] @ y.reshape(P_OUT, n) / np.sqrt(S[l]) - F[l, :n] - np.sqrt(S2 / S[l]) * xi[l])
        out = (U * np.sqrt(S)) @ F
        cols.append((out + np.sqrt(S2) * rng.standard_normal(nt * P_OUT).reshape(P_OUT, nt) if add_noise else out).reshape(-1))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("N, add_noise", ((None, True), (NS + 1, False)))
@pytest.mark.parametrize("hz", (0, 7))
@pytest.mark.parametrize("n", (2 * J + 1, R + J + 1))
@pytest.mark.parametrize("names", MIXES)
def test_model_level_against_dense_gaussians(names, n, hz, N, add_noise):
    fx, y, U, S = model(names, n)
    Ns, kw = N or 1, dict(N=N, add_noise=add_noise, horizon=hz, jitter=JIT)
    prior = dense_sample(names, n, hz, U, S, None, np.random.default_rng(1), Ns, add_noise)
    post = dense_sample(names, n, hz, U, S, y, np.random.default_rng(2), Ns, add_noise)
    got = [lmm.toeplitz_rand(np.random.default_rng(1), fx, **kw), lmm.toeplitz_rand(np.random.default_rng(2), fx, y, **kw)]
    with lmm.toeplitz_posterior(fx, y, blocked=False) as h:      # the handle of the other schedule serves rand too
        before = (h.logpdf, h.mean_and_var(fx.x.x[:5] + 0.1))
        got.append(h.rand(np.random.default_rng(2), **kw))
        after = (h.logpdf, h.mean_and_var(fx.x.x[:5] + 0.1))
        assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
        assert np.array_equal(got[2], h.rand(np.random.default_rng(2), **kw))      # two calls are bitwise equal
        if N is not None:                                                          # column 0 is the one-sample call
            assert np.array_equal(got[2][:, 0], h.rand(np.random.default_rng(2), **dict(kw, N=None)))
    for g, ref, what in zip(got, (prior, post, post), ("prior", "posterior", "post.rand")):
        assert g.shape == ((n + hz) * P_OUT,) + (() if N is None else (N,))
        err = np.abs(g.reshape(ref.shape) - ref).max() / np.abs(ref).max()
        print(f"{names} n={n} hz={hz} {what}: {err:.2e}")
        assert err <= TOL, what


def test_implied_posterior_mean_and_covariance():
    """The path is affine in its normals: zero normals give its mean, unit normals its covariance, which are the dense Gaussian
    posterior's over grid + horizon (a prior K + JIT I conditioned through cov(f, f_x) = K, as the path is defined)."""
    names, n, hz = MIXES[1], J + 1, 3
    fx, y, U, S = model(names, n)
    nt, m = n + hz, len(names)

    class Unit:
        """standard_normal that returns e_j of the concatenated draws of one sample (j = -1: zeros)"""
        def __init__(self, j):
            self.j, self.off = j, 0

        def standard_normal(self, c):
            v = np.zeros(c)
            if self.off <= self.j < self.off + c:
                v[self.j - self.off] = 1.0
            self.off += c
            return v

    Hm = U * np.sqrt(S)
    mean = sum(np.outer(Hm[:, l], G @ (U[:, l] @ y.reshape(P_OUT, n) / np.sqrt(S[l]))) for l, (_, G) in enumerate(dense_latents(names, n, nt)))
    cov = np.zeros((nt * P_OUT, nt * P_OUT))
    for l, (Lc, G) in enumerate(dense_latents(names, n, nt)):
        M = np.eye(nt); M[:, :n] -= G
        cov += np.kron(np.outer(Hm[:, l], Hm[:, l]), M @ Lc @ Lc.T @ M.T + (S2 / S[l]) * G @ G.T)
    with lmm.toeplitz_posterior(fx, y, blocked=True) as h:
        m0 = h.rand(Unit(-1), add_noise=False, horizon=hz, jitter=JIT)
        A = np.stack([h.rand(Unit(j), add_noise=False, horizon=hz, jitter=JIT) - m0 for j in range(m * nt + m * n)], axis=1)
    print(f"mean {np.abs(m0 - mean.reshape(-1)).max() / np.abs(mean).max():.2e}, cov {np.abs(A @ A.T - cov).max() / np.abs(cov).max():.2e}")
    assert np.abs(m0 - mean.reshape(-1)).max() <= TOL * np.abs(mean).max()
    assert np.abs(A @ A.T - cov).max() <= TOL * np.abs(cov).max()


def test_device_normals_and_refusals():
    import torch
    names, n = MIXES[0], 2 * J + 1
    fx, y, U, S = model(names, n)
    a, b = (lmm.toeplitz_rand(lmm.DeviceNormals(5), fx, y, N=2, horizon=3, jitter=JIT) for _ in range(2))
    assert a.is_cuda and a.shape == ((n + 3) * P_OUT, 2) and torch.equal(a, b)
    with pytest.raises(lmm.PosDefException, match=r"latent 2, step \d+\): raise jitter") as e:      # the periodic latent
        lmm.toeplitz_rand(np.random.default_rng(0), fx, jitter=0.0)
    assert e.value.latent == 2 and e.value.info >= 1
    with lmm.toeplitz_posterior(fx, y) as h:
        want = h.mean_and_var(fx.x.x[:3])
        with pytest.raises(lmm.PosDefException, match="latent 2"):
            h.rand(np.random.default_rng(0), jitter=0.0)
        assert all(np.array_equal(u, v) for u, v in zip(want, h.mean_and_var(fx.x.x[:3])))      # unchanged after a refusal
        lmm.set_compute_dtype("f32")
        try:
            for call in (lambda: h.rand(np.random.default_rng(0)), lambda: lmm.toeplitz_rand(np.random.default_rng(0), fx)):
                with pytest.raises(NotImplementedError, match="Float64 only"):
                    call()
        finally:
            lmm.set_compute_dtype("f64")
    lib, o = lmm.load(), torch.zeros(8, device="cuda", dtype=torch.float64)
    bad = torch.tensor([1.0, 1.2, 0.3, 0.1, 0.0], device="cuda", dtype=torch.float64)
    with pytest.raises(lmm.PosDefException, match="latent 0") as e:
        L.check(lib.lmm_dev_toeplitz_sample(bad.data_ptr(), o.data_ptr(), 5, 1, o.data_ptr()))
    assert e.value.info == 1      # 1 + the step whose rho left (-1, 1): step 0
    rc = lib.lmm_oilmm_rand_toeplitz(L.Arr(fx.x.x).ptr, n, P_OUT, L.Arr(L.colmajor(U)).ptr, L.Arr(S).ptr, 3, S2, L.gps_array([g.desc() for g in fx.f.f.fs]),
                                     0, 3, lib.lmm_toeplitz_blocked_max_n(), -1.0, 0, 1, o.data_ptr(), None, o.data_ptr())
    with pytest.raises(NotImplementedError, match=r"n \+ horizon"):
        L.check(rc)
