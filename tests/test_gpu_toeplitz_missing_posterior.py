"""The posterior handle for gappy grids (DESIGN.md 4.22 "Posterior handle for gappy grids") on the GPU: the rows of T^-1 K* against
(np.linalg.inv(T) @ K*)[S] with k and ns around the 128-wide tile, mean_and_var against the dense Gaussian of the observed points built
from the front end's definition, the handle's contracts.  Tolerance: 100 x the CPU delta where that exceeds 1e-11, else 1e-10; V
relative to max |T^-1 K*|, the mean to max |reference|, the variance to the largest prior output variance."""
import functools

import numpy as np
import pytest

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_missing import flat_orthogonal, restatement
from test_gpu_toeplitz import CTOR
from test_gpu_toeplitz_missing import factored, indices
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_missing_posterior_abi import delta_toeplitz_missing_posterior

pytestmark = pytest.mark.gpu
TOL = 100.0 * delta_toeplitz_missing_posterior() if delta_toeplitz_missing_posterior() > 1e-11 else 1e-10
P_OUT, S2, SV, H, X0 = 5, 0.1, np.array([1.0, 1.6, 0.7]), 0.01, 0.5
MIX = (LATENTS["se"], LATENTS["matern52"] + LATENTS["lp"], LATENTS["lp"])       # SE, Matern52 + SE x Periodic, locally periodic


@pytest.mark.parametrize("shape", ("run", "scattered", "run+ends"))
@pytest.mark.parametrize("ns", (1, 33, 130))
@pytest.mark.parametrize("k", (1, 127, 129, 300))
def test_inverse_rows_against_dense_inverse(k, ns, shape):
    import torch
    n, h = 1025, 0.05
    Ti, pd, qd = factored("se", n)
    S = indices(shape, n, k)
    k, idx = len(S), torch.tensor(S, device="cuda", dtype=torch.int32)
    xs = np.random.default_rng(ns).uniform(-3 * h, (n + 2) * h, ns)
    xs[0] = h * S[0]
    ref = Ti @ row(LATENTS["se"], np.abs(h * np.arange(n)[:, None] - xs[None, :]))
    xd, gp = torch.tensor(xs, device="cuda"), L.gps_array([lmm.GP(CTOR["se"](*LATENTS["se"][0][1:])).desc()])

    def rows(forced):
        out = torch.full((k + 2, ns + 3), np.nan, device="cuda", dtype=torch.float64)
        L.check(lmm.load().lmm_dev_toeplitz_inverse_rows(0.0, h, n, gp, pd.data_ptr(), qd.data_ptr(), idx.data_ptr(), k, xd.data_ptr(), ns, forced,
                                                         out.data_ptr(), ns + 3))
        return out.cpu().numpy()

    got = rows(0)
    err = np.abs(got[:k, :ns] - ref[S]).max() / np.abs(ref).max()
    print(f"k={k} ns={ns} {shape}: {err:.2e}")
    assert err <= TOL
    assert np.isnan(got[k:]).all() and np.isnan(got[:, ns:]).all()                          # (k, ns) and nothing else
    for forced in (0, 256, 768):                                                            # reproducible, whatever the chunks of rows
        assert np.array_equal(got, rows(forced), equal_nan=True)


def problem(n, gaps):
    """fx, Y (P_OUT x n), U with the pattern of test_gpu_toeplitz_missing: 40 scattered points miss one or two outputs, an outage of 130
    points and both ends have no data"""
    rng = np.random.default_rng(n)
    U, Y = flat_orthogonal(rng, P_OUT, len(MIX)), rng.standard_normal((P_OUT, n))
    if gaps:
        for t in rng.choice(np.arange(1, n - 1), 40, replace=False):
            Y[rng.choice(P_OUT, int(rng.integers(1, 3)), replace=False), t] = np.nan
        Y[:, [0, n - 1]] = np.nan
        Y[:, n // 2:n // 2 + 130] = np.nan
    ks = [CTOR[t[0][0]](*t[0][1:]) if len(t) == 1 else lmm.KernelSum(*[CTOR[c[0]](*c[1:]) for c in t]) for t in MIX]
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(k) for k in ks]), lmm.Orthogonal(U, SV))
    return f(lmm.MOInputIsotopicByOutputs(X0 + H * np.arange(n), P_OUT), S2), Y, U


def queries(n, Y):
    """in the outage, on partially observed points, between grid points, outside the grid; shuffled"""
    part = np.flatnonzero(np.isnan(Y).any(axis=0) & ~np.isnan(Y).all(axis=0))[:3]
    at = np.concatenate([n // 2 + np.array([0.0, 64.5, 129.0]), part, [3.5, n - 2.25, -2.0, -0.4, n - 0.6, n + 3.0]])
    return X0 + H * np.random.default_rng(3).permutation(at)


@functools.lru_cache(maxsize=None)
def reference(n):
    """mean, var without the added noise (by outputs) and the largest prior output variance: per latent the dense Gaussian of z over the
    points with data with noise S2 (G_t^-1)_ll, mixed as mix_marginals does: H M, H^2 (V + 1e-18)"""
    _, Y, U = problem(n, True)
    xs, ob = queries(n, Y), ~np.isnan(Y).all(axis=0)
    z, noise, _, cond = restatement(Y[:, ob], U * np.sqrt(SV), S2)
    assert cond <= 1e3
    x, ml, vl, k0 = X0 + H * np.arange(n), [], [], []
    for l, terms in enumerate(MIX):
        A = toeplitz(row(terms, H * np.arange(n)))[np.ix_(ob, ob)] + np.diag(noise[:, l])
        Ks = row(terms, np.abs(x[ob, None] - xs[None, :]))
        sol = np.linalg.solve(A, np.column_stack([Ks, z[:, l]]))
        k0.append(row(terms, 0.0))
        ml.append(Ks.T @ sol[:, -1]); vl.append(k0[-1] - np.sum(Ks * sol[:, :-1], axis=0))
    Hm = U * np.sqrt(SV)
    return xs, (Hm @ np.array(ml)).reshape(-1), (Hm ** 2 @ (np.array(vl) + 1e-18)).reshape(-1), (Hm ** 2 @ np.array(k0)).max() + S2


@pytest.mark.parametrize("device_xs", (False, True))
@pytest.mark.parametrize("n, blocked", ((1025, False), (1793, True)))
def test_mean_and_var_against_dense_gaussian_of_observed_points(n, blocked, device_xs):
    fx, Y, _ = problem(n, True)
    xs, rm, rv, prior = reference(n)
    if device_xs:
        import torch
        xq = torch.tensor(xs, device="cuda")
    with lmm.toeplitz_posterior_missing(fx, Y.reshape(-1), blocked) as post:
        assert post.k == int(np.isnan(Y).any(axis=0).sum()) and post.logpdf == lmm.toeplitz_logpdf_missing(fx, Y.reshape(-1), blocked)
        for add_noise in (True, False):
            gm, gv = post.mean_and_var(xq if device_xs else xs, add_noise)
            gm, gv = (a.cpu().numpy() if device_xs else a for a in (gm, gv))
            em, ev = np.abs(gm - rm).max() / np.abs(rm).max(), np.abs(gv - rv - (S2 if add_noise else 0.0)).max() / prior
            print(f"n={n} blocked={blocked}: mean {em:.2e}, var {ev:.2e}")
            assert em <= TOL and ev <= TOL
        ns, sub = len(xs), np.array([7, 2, 9])                                              # a query's result depends on no other query
        ms, vs = post.mean_and_var(xs[sub], False)
        pick = (np.arange(P_OUT)[:, None] * ns + sub[None, :]).reshape(-1)
        assert np.array_equal(ms, gm[pick]) and np.array_equal(vs, gv[pick]) and np.array_equal(post.mean(xs), gm)
        for verb in (lambda: post.rand(np.random.default_rng(0)), lambda: post.rand(np.random.default_rng(0), xs=xs),
                     lambda: post.predictive_logpdf(xs, np.zeros(ns * P_OUT)), lambda: post.mean_and_var_vjp(xs, dmean=np.ones(ns * P_OUT))):
            with pytest.raises(NotImplementedError, match="gap state"):
                verb()


def test_complete_data_gives_the_complete_data_handle():
    fx, Y, _ = problem(1025, False)
    xs = queries(1025, Y)
    with lmm.toeplitz_posterior_missing(fx, Y.reshape(-1)) as post, lmm.toeplitz_posterior(fx, Y.reshape(-1)) as full:
        assert post.k == 0 and post.logpdf == full.logpdf
        for a, b in zip(post.mean_and_var(xs), full.mean_and_var(xs)):
            assert np.array_equal(a, b)
        assert np.array_equal(post.mean_and_var_vjp(xs, dmean=np.ones(len(xs) * P_OUT))["x"], full.mean_and_var_vjp(xs, dmean=np.ones(len(xs) * P_OUT))["x"])


def test_refusals():
    cap = lmm.load().lmm_toeplitz_missing_max_k()
    fx, Y, _ = problem(cap + 9, False)
    Y[0, :cap + 1] = np.nan
    with pytest.raises(NotImplementedError, match=f"lmm_toeplitz_missing_max_k; k = {cap + 1}"):
        lmm.toeplitz_posterior_missing(fx, Y.reshape(-1))
    fx, Y, _ = problem(65, False)
    Y[:3, 17] = np.nan
    with pytest.raises(NotImplementedError, match="point 17 observes 2 outputs"):
        lmm.toeplitz_posterior_missing(fx, Y.reshape(-1))
    with pytest.raises(NotImplementedError, match="needs complete data"):                   # toeplitz_posterior still refuses NaN
        lmm.toeplitz_posterior(fx, Y.reshape(-1))
    Y[:] = np.nan
    with pytest.raises(ValueError, match="no point has an observed output"):
        lmm.toeplitz_posterior_missing(fx, Y.reshape(-1))
