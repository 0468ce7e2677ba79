"""ToeplitzPosterior.mean_and_var_vjp (DESIGN.md 4.22 "Gradients with respect to the queries") on the GPU: the public method against
per-latent dense Gaussians built in NumPy (d kappa / d xs by the complex step of test_toeplitz_vjp_abi.drow) and mixed with random
cotangents, the one-latent building block against a dense Cholesky solve, reproducibility, independence of the queries, refusals.
n = 1, 2, 3 (the degenerate recursions), 255 (one row block), 257 (the first paired blocks), 1025 (several s-tiles); ns = 15, 17: either
side of the query block of 16.  Tolerance: 100 x the committed CPU delta where that exceeds 1e-11, else 1e-10; of "x" relative to
max |reference "x"|, of the building block's d var / d xs relative to max |d K* / d xs| and of its d mean / d xs to max |reference|."""
import numpy as np
import pytest
import scipy.linalg

import lmm_amd as lmm
from lmm_amd import _lib as L
from test_gpu_toeplitz import CTOR, H, MIXES, P_OUT, S2, problem
from test_toeplitz_abi import LATENTS, row, toeplitz
from test_toeplitz_posterior_abi import SIZES, queries
from test_toeplitz_vjp_abi import delta_toeplitz_vjp_mean, delta_toeplitz_vjp_var, drow

pytestmark = pytest.mark.gpu


def tol(*deltas):
    return max(100.0 * d if d > 1e-11 else 1e-10 for d in deltas)


def reference(names, n, y, U, S, xs, dmean, dvar):
    """ "x" from per-latent dense Gaussians (r_l = S_l^-1/2 U_l' Y, noise S2 / S_l), mixed as the library mixes: mbar = H' dmean,
    vbar = (H o H)' dvar; a missing cotangent is zero"""
    Y, x, Hm = y.reshape(P_OUT, n), 0.5 + H * np.arange(n), U * np.sqrt(S)
    out = np.zeros(len(xs))
    for l, k in enumerate(names):
        dl = xs[None, :] - x[:, None]
        t = row(LATENTS[k], x - x[0]); t[0] += S2 / S[l]
        Ks, dKs = row(LATENTS[k], np.abs(dl)), drow(LATENTS[k], dl)
        sol = np.linalg.solve(toeplitz(t), np.column_stack([Ks, U[:, l] @ Y / np.sqrt(S[l])]))
        if dmean is not None:
            out += (Hm[:, l] @ dmean.reshape(P_OUT, -1)) * (dKs.T @ sol[:, -1])
        if dvar is not None:
            out += (Hm[:, l] ** 2 @ dvar.reshape(P_OUT, -1)) * (-2.0 * np.sum(dKs * sol[:, :-1], axis=0))
    return out


@pytest.mark.parametrize("names, n, ns, blocked", [(m, n, ns, False) for m in MIXES for n in SIZES for ns in (15, 17)] + [(MIXES[1], 257, 17, True)])
def test_vjp_against_dense_gaussians(names, n, ns, blocked):
    fx, x, y, U, S = problem(names, n)
    xs, rng = queries(0.5, H, n, ns), np.random.default_rng(n + ns)
    dm, dv = rng.standard_normal(ns * P_OUT), rng.standard_normal(ns * P_OUT)
    with lmm.toeplitz_posterior(fx, y, blocked=blocked) as post:
        for cm, cv, delta in ((dm, dv, (delta_toeplitz_vjp_mean(), delta_toeplitz_vjp_var())), (dm, None, (delta_toeplitz_vjp_mean(),)),
                              (None, dv, (delta_toeplitz_vjp_var(),))):
            got, ref = post.mean_and_var_vjp(xs, cm, cv)["x"], reference(names, n, y, U, S, xs, cm, cv)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"{names} n={n} ns={ns} dmean={cm is not None} dvar={cv is not None}: {err:.2e}")
            assert got.shape == xs.shape and err <= tol(*delta)
            assert np.array_equal(post.mean_and_var_vjp(xs, cm, cv)["x"], got)              # two calls are bitwise equal
            j = ns // 2                                                                      # a query alone: bitwise its entry in the batch
            one = post.mean_and_var_vjp(xs[j:j + 1], None if cm is None else cm[j::ns], None if cv is None else cv[j::ns])["x"]
            assert np.array_equal(one, got[j:j + 1])


def test_building_block_against_dense_solve(n=2049):
    import torch
    lmm.init(0)
    lib = lmm.load()
    terms, lags, ns = LATENTS["lp"] + LATENTS["matern52"], 0.013 * np.arange(n), 33
    t = row(terms, lags); t[0] += 0.05
    r, xs = np.random.default_rng(7 * n).standard_normal(n), queries(0.0, 0.013, n, ns)
    dl = xs[None, :] - lags[:, None]
    Ks, dKs = row(terms, np.abs(dl)), drow(terms, dl)
    sol = scipy.linalg.cho_solve(scipy.linalg.cho_factor(toeplitz(t), lower=True), np.column_stack([Ks, r]))
    rm, rv = dKs.T @ sol[:, -1], -2.0 * np.sum(dKs * sol[:, :-1], axis=0)
    gp = lmm.GP(lmm.KernelSum(*[CTOR[c[0]](*c[1:]) for c in terms]))
    td, rd, xd = (torch.tensor(v, device="cuda") for v in (t, r, xs))
    pd, qd, ad, md, vd = torch.empty_like(td), torch.empty_like(td), torch.empty_like(td), torch.empty_like(xd), torch.empty_like(xd)
    L.check(lib.lmm_dev_toeplitz_factor(td.data_ptr(), rd.data_ptr(), n, None, None, pd.data_ptr(), qd.data_ptr()))
    L.check(lib.lmm_dev_toeplitz_solve(pd.data_ptr(), qd.data_ptr(), rd.data_ptr(), n, ad.data_ptr()))
    L.check(lib.lmm_dev_toeplitz_predict_grad(0.0, 0.013, n, L.gps_array([gp.desc()]), pd.data_ptr(), qd.data_ptr(), ad.data_ptr(),
                                              xd.data_ptr(), ns, md.data_ptr(), vd.data_ptr()))
    em, ev = np.abs(md.cpu().numpy() - rm).max() / np.abs(rm).max(), np.abs(vd.cpu().numpy() - rv).max() / np.abs(dKs).max()
    print(f"building block n={n}: d mean {em:.2e}, d var {ev:.2e}")
    assert em <= tol(delta_toeplitz_vjp_mean()) and ev <= tol(delta_toeplitz_vjp_var())
    only = torch.empty_like(xd)                                                              # dvar_dx = NULL: the means alone, bitwise
    L.check(lib.lmm_dev_toeplitz_predict_grad(0.0, 0.013, n, L.gps_array([gp.desc()]), pd.data_ptr(), qd.data_ptr(), ad.data_ptr(),
                                              xd.data_ptr(), ns, only.data_ptr(), None))
    assert torch.equal(only, md)


def test_refusals_leave_the_handle_unchanged():
    fx, x, y, U, S = problem(MIXES[0], 65)
    xs, cot = queries(0.5, H, 65, 17), np.random.default_rng(0).standard_normal(17 * P_OUT)
    post, lib = lmm.toeplitz_posterior(fx, y), lmm.load()
    before = post.mean_and_var(xs) + (post.mean_and_var_vjp(xs, cot, cot)["x"],)

    def unchanged():
        now = post.mean_and_var(xs) + (post.mean_and_var_vjp(xs, cot, cot)["x"],)
        return all(np.array_equal(a, b) for a, b in zip(now, before))

    bad, out = xs.copy(), np.empty(len(xs))
    bad[3] = np.nan
    with pytest.raises(ValueError, match=r"Toeplitz posterior: xs\[3\] is not finite"):      # the library's own refusal
        L.check(lib.lmm_oilmm_toeplitz_post_mean_and_var_grad_xs(post._ptr, L.Arr(bad).ptr, len(bad), L.Arr(cot).ptr, None, L.Arr(out, True).ptr))
    with pytest.raises(ValueError, match="both NULL"):
        L.check(lib.lmm_oilmm_toeplitz_post_mean_and_var_grad_xs(post._ptr, L.Arr(xs).ptr, len(xs), None, None, L.Arr(out, True).ptr))
    assert unchanged()
    with pytest.raises(ValueError, match=r"\(ns,\)"):
        post.mean_and_var_vjp(xs.reshape(-1, 1), cot)
    with pytest.raises(ValueError, match="both None"):
        post.mean_and_var_vjp(xs)
    assert unchanged()
    post.close()
    with pytest.raises(ValueError, match="closed"):
        post.mean_and_var_vjp(xs, cot)
