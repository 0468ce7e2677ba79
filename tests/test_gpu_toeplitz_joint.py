"""The joint predictive of the Toeplitz posterior handle (DESIGN.md 4.22 "Joint predictive") on the GPU: the one-latent covariance
against a dense Cholesky solve, predictive_logpdf and rand(xs=) against per-latent dense Gaussians built in NumPy and mixed through H,
reproducibility, independence of the other queries and of the chunking, refusals.  n = 1, 3 (the degenerate recursions), R - 1 (one
row block), R + 1 (a pair of blocks), 2 R + 1 (an odd count: three chunks at R rows per chunk); ns = 1, Q - 1, Q + 1 and T - 1, T + 1
around the Gram kernel's tile.  Tolerance: 100 x the committed CPU delta where that exceeds 1e-11, else 1e-10; of C relative to
kappa(0), of the log density relative to |reference|, of the paths relative to max |reference|."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_toeplitz import CTOR, H, MIXES, P_OUT, S2, problem
from test_gpu_toeplitz_rand import HG, model
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_joint_abi import JITTER, delta_toeplitz_joint_cov, delta_toeplitz_joint_rand, delta_toeplitz_predictive, rand_queries
from test_toeplitz_posterior_abi import Q, R, queries

pytestmark = pytest.mark.gpu
CAP, T = C.c_int(), C.c_int()
lmm.load().lmm_toeplitz_joint_shape(C.byref(CAP), C.byref(T), None)
CAP, T = CAP.value, T.value


def tol(delta):
    return 100.0 * delta if delta > 1e-11 else 1e-10


def reference(kinds, x, xs, w, r):
    """per latent (mu*, C) at xs from the dense Gaussian: kernel kinds[l] over x with noise w[l] and data r[l]"""
    out = []
    for k, wl, rl in zip(kinds, w, r):
        K = toeplitz(row(k, x - x[0])) + wl * np.eye(len(x))
        Ks = row(k, np.abs(x[:, None] - xs[None, :]))
        sol = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), np.column_stack([Ks, rl]))
        out.append((Ks.T @ sol[:, -1], row(k, np.abs(xs[:, None] - xs[None, :])) - Ks.T @ sol[:, :-1]))
    return out


@pytest.mark.parametrize("chunk", (0, R))
@pytest.mark.parametrize("ns", (1, Q - 1, Q + 1, T - 1, T + 1))
@pytest.mark.parametrize("n", (1, 3, R - 1, R + 1, 2 * R + 1))
def test_building_block_against_dense_solve(n, ns, chunk):
    import torch
    lmm.init(0)
    lib = lmm.load()
    terms, h, d = LATENTS["lp"] + LATENTS["matern52"], 0.013, 0.05
    x, xs = h * np.arange(n), queries(0.0, h, n, ns)
    ref = reference([terms], x, xs, [0.05], [np.zeros(n)])[0][1] + d * np.eye(ns)
    gp = L.gps_array([lmm.GP(lmm.KernelSum(*[CTOR[c[0]](*c[1:]) for c in terms])).desc()])
    t = row(terms, x); t[0] += 0.05
    td, xd = torch.tensor(t, device="cuda"), torch.tensor(xs, device="cuda")
    pd, qd = torch.empty_like(td), torch.empty_like(td)
    L.check(lib.lmm_dev_toeplitz_factor(td.data_ptr(), torch.zeros_like(td).data_ptr(), n, None, None, pd.data_ptr(), qd.data_ptr()))

    def cov(xq, rows):
        """(i, j) of the result at [i, j]; NaN where the call wrote nothing"""
        out = torch.full((len(xq), len(xq) + 3), np.nan, device="cuda", dtype=torch.float64)
        L.check(lib.lmm_dev_toeplitz_predict_cov(0.0, h, n, gp, pd.data_ptr(), qd.data_ptr(), xq.data_ptr(), len(xq), d, rows, out.data_ptr(),
                                                 len(xq) + 3))
        return out.cpu().numpy().T

    got = cov(xd, chunk)
    lo = np.tril_indices(ns)
    err = np.abs(got[lo] - ref[lo]).max() / row(terms, 0.0)
    print(f"n={n} ns={ns} chunk={chunk}: {err:.2e}")
    assert err <= tol(delta_toeplitz_joint_cov())
    assert np.isnan(got[:ns][np.triu_indices(ns, 1)]).all() and np.isnan(got[ns:]).all()      # the triangle and nothing else
    assert np.array_equal(got, cov(xd, chunk), equal_nan=True)                                # two calls are bitwise equal
    assert np.array_equal(got, cov(xd, R - chunk), equal_nan=True)                            # and so is the other chunking
    i, j = ns - 1, ns // 2
    if i > j:                                                                                 # a pair alone: bitwise its entries
        pair = cov(xd[[j, i]].contiguous(), chunk)
        assert pair[1, 0] == got[i, j] and pair[0, 0] == got[j, j] and pair[1, 1] == got[i, i]
        assert cov(xd[[i, j]].contiguous(), chunk)[1, 0] == got[i, j]


@pytest.mark.parametrize("names, n, ns, blocked, s2", [(m, n, ns, False, None) for m in MIXES for n in (3, R + 1) for ns in (1, Q + 1)]
                         + [(MIXES[1], R + 1, Q + 1, True, None), (MIXES[0], R + 1, Q + 1, False, 0.35)])
def test_predictive_logpdf_against_dense_gaussians(names, n, ns, blocked, s2):
    fx, x, y, U, S = problem(names, n)
    xs, ys = queries(0.5, H, n, ns), np.random.default_rng(n + ns).standard_normal(ns * P_OUT)
    Y, Ys, sq = y.reshape(P_OUT, n), ys.reshape(P_OUT, ns), s2 or S2
    PY = Ys - U @ (U.T @ Ys)
    ref = -0.5 * ns * (np.log(S).sum() + (P_OUT - len(names)) * np.log(2 * np.pi * sq)) - 0.5 * np.sum(PY * PY) / sq
    lat = reference([LATENTS[k] for k in names], x, xs, S2 / S, [U[:, l] @ Y / np.sqrt(S[l]) for l in range(len(names))])
    for l, (mu, Cl) in enumerate(lat):
        A, v = Cl + (sq / S[l]) * np.eye(ns), U[:, l] @ Ys / np.sqrt(S[l]) - mu
        ref += -0.5 * (v @ np.linalg.solve(A, v) + np.linalg.slogdet(A)[1] + ns * np.log(2 * np.pi))
    with lmm.toeplitz_posterior(fx, y, blocked=blocked) as post:
        before = (post.logpdf, post.mean_and_var(xs))
        got = post.predictive_logpdf(xs, ys, s2)
        err = abs(got - ref) / abs(ref)
        print(f"{names} n={n} ns={ns} blocked={blocked} sigma2={s2}: {err:.2e}")
        assert err <= tol(delta_toeplitz_predictive())
        assert got == post.predictive_logpdf(xs, ys, s2)                                      # two calls are bitwise equal
        after = (post.logpdf, post.mean_and_var(xs))
        assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))


@pytest.mark.parametrize("add_noise", (True, False))
@pytest.mark.parametrize("N", (None, 3))
@pytest.mark.parametrize("names", MIXES)
def test_rand_at_new_inputs_against_numpy_paths(names, N, add_noise):
    n, m = R + 1, len(names)
    fx, y, U, S = model(names, n)
    x = 0.5 + HG * np.arange(n)
    xs = rand_queries(0.5, HG, n)[::-1].copy()                                                # in the caller's order: descending
    ns, jit = len(xs), JITTER * max(row(LATENTS[k], 0.0) for k in names)
    lat = reference([LATENTS[k] for k in names], x, xs, S2 / S, [U[:, l] @ y.reshape(P_OUT, n) / np.sqrt(S[l]) for l in range(m)])
    rng, cols = np.random.default_rng(2), []
    for _ in range(N or 1):
        F = np.array([mu + np.linalg.cholesky(Cl + jit * np.eye(ns)) @ rng.standard_normal(ns) for mu, Cl in lat])
        out = (U * np.sqrt(S)) @ F
        cols.append((out + np.sqrt(S2) * rng.standard_normal(ns * P_OUT).reshape(P_OUT, ns) if add_noise else out).reshape(-1))
    ref, kw = np.stack(cols, axis=1), dict(add_noise=add_noise, jitter=jit, xs=xs)
    with lmm.toeplitz_posterior(fx, y) as post:
        plain = post.rand(np.random.default_rng(5), jitter=0.05)
        got = post.rand(np.random.default_rng(2), N=N, **kw)
        assert got.shape == (ns * P_OUT,) + (() if N is None else (N,))
        err = np.abs(got.reshape(ref.shape) - ref).max() / np.abs(ref).max()
        print(f"{names} N={N} add_noise={add_noise}: {err:.2e}")
        assert err <= tol(delta_toeplitz_joint_rand())
        assert np.array_equal(got, post.rand(np.random.default_rng(2), N=N, **kw))            # two calls are bitwise equal
        rng = np.random.default_rng(2)                                                        # column q is the one-sample call on its normals
        assert all(np.array_equal(got[:, q], post.rand(rng, **kw)) for q in range(N or 0))
        assert np.array_equal(plain, post.rand(np.random.default_rng(5), jitter=0.05))        # rand() without xs is what it was


def test_refusals_leave_the_handle_unchanged():
    fx, x, y, U, S = problem(MIXES[0], 65)
    xs, lib, rng = queries(0.5, H, 65, Q + 1), lmm.load(), np.random.default_rng(0)
    ys, out, post = rng.standard_normal(len(xs) * P_OUT), C.c_double(), lmm.toeplitz_posterior(fx, y)
    before = (*post.mean_and_var(xs), post.predictive_logpdf(xs, ys))

    def unchanged():
        return all(np.array_equal(a, b) for a, b in zip((*post.mean_and_var(xs), post.predictive_logpdf(xs, ys)), before))

    def logpdf(ptr, xq, nq):
        L.check(lib.lmm_oilmm_toeplitz_post_logpdf(ptr, L.Arr(xq).ptr, nq, L.Arr(np.zeros(max(nq, 1) * P_OUT)).ptr, -1.0, C.byref(out)))

    def rand_at(ptr, xq, nq):
        z, o = np.zeros(3 * max(nq, 1)), np.empty(max(nq, 1) * P_OUT)
        L.check(lib.lmm_oilmm_toeplitz_post_rand_at(ptr, L.Arr(xq).ptr, nq, -1.0, 0, 1, L.Arr(z).ptr, None, L.Arr(o, True).ptr))

    bad, big, ynan = xs.copy(), np.linspace(0.0, 1.0, CAP + 1), ys.copy()
    bad[3], ynan[len(xs) + 2] = np.inf, np.nan
    for call in (logpdf, rand_at):                                                            # the library's own refusals
        with pytest.raises(ValueError, match="bad arguments"):
            call(None, xs, len(xs))
        with pytest.raises(ValueError, match=r"ns must be >= 1 \(ns = 0\)"):
            call(post._ptr, xs, 0)
        with pytest.raises(ValueError, match=r"Toeplitz posterior: xs\[3\] is not finite"):
            call(post._ptr, bad, len(bad))
        with pytest.raises(NotImplementedError, match=f"lmm_toeplitz_joint_max_ns; ns = {CAP + 1}"):
            call(post._ptr, big, CAP + 1)
        assert unchanged()
    with pytest.raises(NotImplementedError, match="lmm_toeplitz_joint_max_ns"):                  # the mirror's, before any call
        post.rand(rng, xs=big)
    with pytest.raises(NotImplementedError, match="point 2 has a NaN in ys"):
        post.predictive_logpdf(xs, ynan)
    with pytest.raises(lmm.PosDefException, match=r"latent \d"):                              # coincident queries without jitter
        post.rand(rng, jitter=0.0, add_noise=False, xs=np.repeat(xs[:8], 4))
    assert unchanged()
    calls = (lambda: post.predictive_logpdf(xs, ys), lambda: post.rand(rng, xs=xs), lambda: logpdf(post._ptr, xs, len(xs)),
             lambda: rand_at(post._ptr, xs, len(xs)))
    lmm.set_compute_dtype("f32")
    try:
        for call in calls:
            with pytest.raises(NotImplementedError, match="Float64 only"):
                call()
    finally:
        lmm.set_compute_dtype("f64")
    assert unchanged()
    post.close()
    for call in calls[:2]:
        with pytest.raises(ValueError, match="closed"):
            call()
