"""-m gpu: the gradient of the inducing-point (VFE) bound (include/lmm_hip.h "inducing points"): the second pass over
the points (lmm_dev_sparse_grad) against NumPy, elbo_and_gradient against autograd of the dense model value, one central difference
through elbo itself, and the refusals that need the library.

The references, the cases and their CPU disagreement delta are those of tests/test_sparse_grad_abi.py, which checks delta <= 1e-9 and
cond(K_uu + eps I) <= 1e4 per case without a GPU.  Tolerances: the building block 1e-10 max|reference| per output array (the tolerance
test_gpu_sparse.py::test_moments uses for the same kind of sum over n); elbo_and_gradient the project's rule max(1e-10, 100 delta) per
entry, delta that entry's CPU disagreement (the factor 100: another summation order over n and the MFMA accumulation order)."""
import numpy as np
import pytest

import test_sparse_grad_abi as R

pytestmark = pytest.mark.gpu

NGRAD, MAX_TERMS = 10, 4


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


# ---------------------------------------------------------------------------------------------------
# lmm_dev_sparse_grad
# ---------------------------------------------------------------------------------------------------
def block_problem(case):
    """Per-point w, a random symmetric PhiBar and beta for a case of the CPU file."""
    k, x, z, r = R.case_problem(*case)
    n, M = x.shape[1], z.shape[1]
    rng = np.random.default_rng(11 * n + M)
    A = rng.normal(size=(M, M))
    return k, x, z, r, rng.uniform(0.05, 0.5, n), 0.5 * (A + A.T), rng.normal(size=M)


def block_reference(k, x, z, r, w, PhiBar, beta):
    """(term records, grad_z, grad_r) of the K_uf pass: sum g dk with dk from autograd of the kernel matrix."""
    import torch
    d = x.shape[0]
    with torch.no_grad():
        Kuf = R.kmat_t(k, R.tparams(k), R.tens(z), R.tens(x)).numpy()
    G = (2.0 * PhiBar @ Kuf + np.outer(beta, r)) / w[None, :]
    theta, gz = R.contract(k, x, z, G)
    terms = k[3] if k[0] == "sum" else [k]
    assert k[0] != "sum" or k[2] == 1.0                # the records are derivatives with respect to s0 l_c: the cases keep s0 = 1
    rec = np.zeros((MAX_TERMS, NGRAD + d))
    for c, t in enumerate(terms):
        pre = f"terms.{c}." if k[0] == "sum" else ""
        gl = theta[pre + "lengthscale"]
        if gl.ndim == 1:                               # per-dimension lengthscales: the multiplier is 1
            rec[c, 0], rec[c, NGRAD:] = float(gl @ np.asarray(t[2])), gl
        else:
            assert d == 1
            rec[c, 0] = rec[c, NGRAD] = float(gl)
        rec[c, 7] = float(theta[pre + "variance"]) * t[1]         # sum g k_c: k_c is linear in its variance
        rec[c, 8] = float(theta.get(pre + "alpha", theta.get(pre + "r", 0.0)))
        rec[c, 9] = float(theta.get(pre + "decay", 0.0))
    return rec, gz, (beta @ Kuf - r) / w


def gpu_block(lmm, k, x, z, r, w, PhiBar, beta, chunk):
    import torch
    from lmm_amd import _lib as L
    d, n, M = x.shape[0], x.shape[1], z.shape[1]
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xd, zd, wd, rd, Pd, bd = dev(x.T), dev(z.T), dev(w), dev(r), dev(PhiBar), dev(beta)
    rec = torch.full((MAX_TERMS, NGRAD + d), float("nan"), dtype=torch.float64, device="cuda")
    gz = torch.full((M, d), float("nan"), dtype=torch.float64, device="cuda")
    gr = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gp = L.gps_array([dict(R.to_kernel(lmm, k).desc(), mean=0.0)])
    L.check(lmm.load().lmm_dev_sparse_grad(xd.data_ptr(), d, n, zd.data_ptr(), M, gp, wd.data_ptr(), rd.data_ptr(), Pd.data_ptr(), M,
                                           bd.data_ptr(), chunk, rec.data_ptr(), gz.data_ptr(), gr.data_ptr()))
    return rec.cpu().numpy(), gz.cpu().numpy().T, gr.cpu().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(map(str, c)))
def test_second_pass(lmm, case):
    k, x, z, r, w, PhiBar, beta = block_problem(case)
    n = x.shape[1]
    ref = block_reference(k, x, z, r, w, PhiBar, beta)
    chunk = n // 3 + 4 if n >= 3 else 1                # three chunks, the last ragged: 63 -> 25, 25, 13;  1000 -> 337, 337, 326
    assert n < 3 or (2 * chunk < n < 3 * chunk)
    got = {c: gpu_block(lmm, k, x, z, r, w, PhiBar, beta, c) for c in (0, chunk)}
    for c, g in got.items():
        errs = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(g, ref)]
        print(f"{case} chunk={c}: records {errs[0]:.2e}  grad_z {errs[1]:.2e}  grad_r {errs[2]:.2e}")
        for a, b in zip(g, ref):
            assert np.isfinite(a).all()
            assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max()
    for a, b, f in zip(got[0], got[chunk], ref):
        assert np.abs(a - b).max() <= 1e-10 * np.abs(f).max()
    again = gpu_block(lmm, k, x, z, r, w, PhiBar, beta, chunk)       # the same chunking twice: bitwise
    for a, b in zip(got[chunk], again):
        assert np.array_equal(a, b)


# the 4 < d <= 8 (a sum latent) and d > 8 (a plain latent) instantiations of sparse_grad_kernel: the same checks, same tolerance
@pytest.mark.parametrize("case", [(130, 70, 6, "m12+se+m32", 4.0, True), (130, 70, 12, "m52", 4.0, True)], ids=lambda c: "-".join(map(str, c)))
def test_second_pass_wide_inputs(lmm, case, monkeypatch):
    monkeypatch.setattr(R, "ARD", np.concatenate([R.ARD, 1.0 + 0.1 * np.arange(9)]))      # per-dimension factors for d up to 12
    test_second_pass(lmm, case)


# ---------------------------------------------------------------------------------------------------
# elbo_and_gradient
# ---------------------------------------------------------------------------------------------------
def model(lmm, P):
    f = lmm.ILMM(lmm.independent_mogp([lmm.GP(mu, R.to_kernel(lmm, k)) for k, mu in P["gps"]]), lmm.Orthogonal(P["U"], P["S"]))
    return f(lmm.MOInputIsotopicByOutputs(P["x"], 5), P["s2"]), P["Y"].reshape(-1)


def tol(delta):
    return max(1e-10, 100.0 * delta)


@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n,M,l", R.MODEL_SHAPES)
def test_elbo_and_gradient(lmm, n, M, l, with_reg):
    import torch
    P, ref, delta = R.model_reference(n, M, l, with_reg)
    fx, y = model(lmm, P)
    vfe = lmm.VFE(P["z"], R.EPS)
    g = lmm.elbo_and_gradient(vfe, fx, y, with_reg)
    assert set(g) == {"value", "y", "sigma2", "S", "U", "gps", "z"}
    assert g["value"] == lmm.elbo(vfe, fx, y, with_reg)
    assert abs(g["value"] - ref["value"]) <= 1e-9 * abs(ref["value"])
    assert isinstance(g["z"], np.ndarray) and g["z"].shape == P["z"].shape and g["y"].shape == y.shape and g["U"].shape == P["U"].shape
    got, want = R.library_entries(g), R.model_entries(ref)
    assert set(got) == set(want)
    bad = []
    for a in sorted(want):
        scale = np.abs(np.atleast_1d(want[a])).max()
        err = np.abs(np.atleast_1d(got[a]) - np.atleast_1d(want[a])).max() / scale
        print(f"({n}, {M}) reg={with_reg} {a}: error {err:.2e}  (delta {delta[a]:.1e}, rule {tol(delta[a]):.1e})")
        if not err <= tol(delta[a]):
            bad.append((a, err))
    assert not bad, bad
    assert isinstance(g["gps"][0]["lengthscale"], np.ndarray) and isinstance(g["gps"][1]["lengthscale"], float)
    # y on the device: the same numbers, torch outputs on its side
    gd = lmm.elbo_and_gradient(vfe, fx, torch.tensor(y, dtype=torch.float64, device="cuda"), with_reg)
    assert torch.is_tensor(gd["y"]) and gd["y"].is_cuda and gd["value"] == g["value"]
    gotd = R.library_entries(gd)
    for a in got:
        assert np.array_equal(np.atleast_1d(gotd[a]), np.atleast_1d(got[a])), a
    if n == 63:                                        # z as a device tensor: "z" comes back as one
        gz = lmm.elbo_and_gradient(lmm.VFE(torch.tensor(P["z"], dtype=torch.float64, device="cuda"), R.EPS), fx, y, with_reg)
        assert torch.is_tensor(gz["z"]) and gz["z"].is_cuda and np.array_equal(gz["z"].cpu().numpy(), g["z"])


def test_central_difference_through_elbo(lmm):
    """Value and gradient belong together: one lengthscale, sigma2 and one z_i at (63, 16), h = 1e-5 (the CPU experiment gave 6e-10)."""
    n, M, l = R.MODEL_SHAPES[0]
    P, _, _ = R.model_reference(n, M, l, True)
    h = 1e-5

    def value(gps=None, s2=None, z=None):
        Q = dict(P, gps=gps or P["gps"], s2=P["s2"] if s2 is None else s2)
        fx, y = model(lmm, Q)
        return lmm.elbo(lmm.VFE(P["z"] if z is None else z, R.EPS), fx, y)

    fx, y = model(lmm, P)
    g = lmm.elbo_and_gradient(lmm.VFE(P["z"], R.EPS), fx, y)

    def with_ls(v):                                    # the Matern52 term of the sum latent
        (name, v0, s0, terms), mu = P["gps"][2]
        return P["gps"][:2] + [((name, v0, s0, [(terms[0][0], terms[0][1], v)] + terms[1:]), mu)]

    l0 = P["gps"][2][0][3][0][2]
    zp, zm = P["z"].copy(), P["z"].copy()
    zp[5] += h
    zm[5] -= h
    for name, fd, an in (("lengthscale", (value(gps=with_ls(l0 + h)) - value(gps=with_ls(l0 - h))) / (2 * h), g["gps"][2]["terms"][0]["lengthscale"]),
                         ("sigma2", (value(s2=P["s2"] + h) - value(s2=P["s2"] - h)) / (2 * h), g["sigma2"]),
                         ("z[5]", (value(z=zp) - value(z=zm)) / (2 * h), g["z"][5])):
        print(f"{name}: central difference {fd:.10e}  gradient {an:.10e}  rel {abs(fd - an) / abs(an):.2e}")
        assert abs(fd - an) <= 1e-6 * abs(an)


# ---------------------------------------------------------------------------------------------------
# refusals that come from the library
# ---------------------------------------------------------------------------------------------------
def test_refusals(lmm):
    """On the Matern latents of tests/test_gpu_sparse.py (one of unit variance): two coincident inducing points and a jitter below the
    rounding of K_uu's diagonal leave a pivot that is not > 0, a status code of a completed launch."""
    import test_gpu_sparse as G
    P, _ = G.reference(63, 16)
    _, fx, y = G.model(lmm, P)
    with pytest.raises(NotImplementedError, match="1024"):
        lmm.elbo_and_gradient(lmm.VFE(np.linspace(0.0, 10.0, 1025), R.EPS), fx, y)
    z = P["z"].copy()
    z[1] = z[0]
    with pytest.raises(lmm.PosDefException, match="latent") as ei:
        lmm.elbo_and_gradient(lmm.VFE(z, 1e-300), fx, y)
    assert 0 <= ei.value.latent < 3 and ei.value.info > 0
    vfe = lmm.VFE(P["z"], R.EPS)
    good = lmm.elbo_and_gradient(vfe, fx, y)            # the library is usable afterwards
    assert good["value"] == lmm.elbo(vfe, fx, y)
    lmm.set_compute_dtype("f32")
    try:
        with pytest.raises(NotImplementedError, match="Float64"):
            lmm.elbo_and_gradient(vfe, fx, y)
    finally:
        lmm.set_compute_dtype("f64")
    assert lmm.elbo_and_gradient(vfe, fx, y)["value"] == good["value"]
