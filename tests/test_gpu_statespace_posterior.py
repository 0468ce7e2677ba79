"""-m gpu: the state-space posterior object (include/lmm_hip.h "state space: the posterior object"; DESIGN.md 4.18 "Posterior object"):
the interpolation kernel alone on the restatement's states, the full-state block against the restatement, statespace_posterior end to
end against the dense posterior and the `xs=` route of statespace_mean_and_var, independence of the queries, duplicates, torch device
inputs, more latents than a launch holds, and the C ABI's refusals.

Tolerance (the rule of tests/test_gpu_statespace.py): max(1e-10, 100 DELTA) of max|reference| per array, DELTA the larger of
test_statespace_abi.delta() (7.6e-15) and test_statespace_posterior_abi.delta_posterior() (1.7e-13): 1e-10.  A stored state is compared
component by component (f, f', f'' and their covariances have different units).  The reference is always the NumPy restatement or
another path of the library (the dense posterior, the `xs=` route), never the code under test."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_statespace as GS
import test_sho_abi as S
import test_statespace_abi as T
import test_statespace_posterior_abi as PA

pytestmark = pytest.mark.gpu

BLOCK_N = GS.BLOCK_N
LATENTS = tuple(T.KINDS) + tuple(("sho", Q) for Q in S.QS)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * max(T.delta(), PA.delta_posterior()))


def close(got, ref, tol, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what} err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def nan_dev(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ---------------------------------------------------------------------------------------------------
# the building blocks
# ---------------------------------------------------------------------------------------------------
def block_case(lat, n, unobserved):
    """(model, x, w, r): test_gpu_statespace.block_case for a Matern kind; for the oscillator test_sho_abi.case (ties in x for
    n >= 63) with the same unobserved runs."""
    if lat in T.KINDS:
        v, ell, x, w, r = GS.block_case(lat, n, unobserved)
        return PA.model_of(lat, v, ell), x, w, r
    v, P, x, w, r = S.case(lat[1], n, unobserved=unobserved)
    if unobserved:
        w[-1] = np.inf
        if n >= 63:
            w[20:40] = np.inf
        if n >= 257:
            w[100:180] = np.inf
    return S.sho(v, P, lat[1]), x, w, r


_REF = {}


def block_reference(lat, n, unobserved):
    """The case and the restatement's full filtered and smoothed states, computed once."""
    key = (lat, n, unobserved)
    if key not in _REF:
        model, x, w, r = block_case(lat, n, unobserved)
        _REF[key] = (model, x, w, r, PA.full_states(model, x, w, r))
    return _REF[key]


def pack(m, P):
    """(n, D), (n, D, D) -> the library's point-major layout (n, D + D (D + 1) / 2): per point the means, then the upper triangle
    by rows."""
    D = m.shape[1]
    rows = [m[:, i] for i in range(D)] + [P[:, i, j] for i in range(D) for j in range(i, D)]
    return np.ascontiguousarray(np.stack(rows, axis=1))


def gpu_interp(lmm, model, x, fpk, spk, xs):
    import torch
    from lmm_amd import _lib as L
    xd, fd, sd, xsd = dev(x), dev(fpk), dev(spk), dev(xs)
    mean, var = nan_dev(len(xs)), nan_dev(len(xs))
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])                       # the mean is not read
    L.check(lmm.load().lmm_dev_statespace_interp(xd.data_ptr(), len(x), gp, fd.data_ptr(), sd.data_ptr(), xsd.data_ptr(), len(xs),
                                                 mean.data_ptr(), var.data_ptr()))
    return mean.cpu().numpy(), var.cpu().numpy()


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_interpolation_kernel_alone(lmm, tol, lat, n, unobserved):
    """lmm_dev_statespace_interp on the states of the RESTATEMENT: only the new kernel is under test."""
    model, x, w, r, st = block_reference(lat, n, unobserved)
    xs = PA.queries(x)
    rm, rv = PA.interp_reference(model, x, st, xs)
    gm, gv = gpu_interp(lmm, model, x, pack(st[0], st[1]), pack(st[2], st[3]), xs)
    if np.abs(rm).max() > 0:
        close(gm, rm, tol, "mean")
    else:
        assert np.abs(gm).max() == 0.0
    close(gv, rv, tol, "var")


@pytest.mark.parametrize("ns", [1, 63, 257, 70000])
def test_interpolation_grid_edges(lmm, tol, ns):
    """n = 1000 with ns queries (one workgroup takes 256).  The 70000 queries repeat 700 distinct values in a random order, so the
    reference is 700 restated interpolations and every thread is still checked."""
    model, x, w, r, st = block_reference("matern52", 1000, True)
    rng = np.random.default_rng(ns)
    if ns <= 700:
        distinct = np.concatenate([PA.queries(x), rng.uniform(x[0] - 2.0, x[-1] + 2.0, 700)])[:ns]
        idx = np.arange(ns)
    else:
        distinct = np.concatenate([PA.queries(x), rng.uniform(x[0] - 2.0, x[-1] + 2.0, 700 - 49)])
        idx = np.concatenate([np.arange(700), rng.integers(0, 700, ns - 700)])
        idx = rng.permutation(idx)
    rm, rv = PA.interp_reference(model, x, st, distinct)
    gm, gv = gpu_interp(lmm, model, x, pack(st[0], st[1]), pack(st[2], st[3]), distinct[idx])
    close(gm, rm[idx], tol, "mean"); close(gv, rv[idx], tol, "var")


@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_component_major_states_give_the_same_bits(lmm, lat):
    """lmm_dev_statespace_interp_layout with the states transposed (comps x n, point_major = 0) returns bitwise what the library's
    point-major layout does."""
    import torch
    from lmm_amd import _lib as L
    model, x, w, r, st = block_reference(lat, 257, True)
    xs = PA.queries(x)
    fpk, spk = pack(st[0], st[1]), pack(st[2], st[3])
    gm, gv = gpu_interp(lmm, model, x, fpk, spk, xs)
    xd, fd, sd, xsd = dev(x), dev(fpk.T), dev(spk.T), dev(xs)
    mean, var = nan_dev(len(xs)), nan_dev(len(xs))
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])
    L.check(lmm.load().lmm_dev_statespace_interp_layout(xd.data_ptr(), len(x), gp, fd.data_ptr(), sd.data_ptr(), 0, xsd.data_ptr(),
                                                        len(xs), mean.data_ptr(), var.data_ptr()))
    assert (mean.cpu().numpy() == gm).all() and (var.cpu().numpy() == gv).all()


def close_state(got, ref, tol, D, what):
    """A state as (comps, n) (the transpose of the packed layout) against its reference, row by row: the components have different
    units (f, f', f''), so each row has its own scale.  A variance row P_ii: max|reference|.  A covariance row P_ij: sqrt(max|P_ii| max|P_jj|), the bound that
    Cauchy-Schwarz puts on it (several covariances are zero analytically, e.g. cov(f, f') of a stationary state, and their reference
    is rounding noise).  A mean row m_i: max|reference|, and sqrt(max|P_ii|) where nothing is observed and the mean is zero."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    row = {}
    for i in range(D):
        for j in range(i, D):
            row[(i, j)] = D + i * D - i * (i - 1) // 2 + (j - i)
    sd = [np.sqrt(np.abs(ref[row[(i, i)]]).max()) for i in range(D)]
    for i in range(D):
        scale = np.abs(ref[i]).max() or sd[i]
        err = np.abs(got[i] - ref[i]).max()
        print(f"{what} mean {i} err {err:.3e} scale {scale:.3e}")
        assert err <= tol * scale, (what, "mean", i, err, scale)
    for (i, j), c in row.items():
        scale = sd[i] * sd[j]
        err = np.abs(got[c] - ref[c]).max()
        print(f"{what} cov {i}{j} err {err:.3e} scale {scale:.3e}")
        assert err <= tol * scale, (what, "cov", i, j, err, scale)


def gpu_states(lmm, model, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    n, comps = len(x), model.D + model.D * (model.D + 1) // 2
    xd, wd, rd = dev(x), dev(w), dev(r)
    fs, ss = nan_dev(n, comps), nan_dev(n, comps)
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])
    L.check(lmm.load().lmm_dev_statespace_states(xd.data_ptr(), n, gp, wd.data_ptr(), rd.data_ptr(), chunk, fs.data_ptr(), ss.data_ptr()))
    return fs.cpu().numpy(), ss.cpu().numpy()


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("n", BLOCK_N)
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_states_block(lmm, tol, lat, n, unobserved):
    """lmm_dev_statespace_states against the restatement's full states, component by component; chunk = 7 at n = 1000 has more
    aggregates than one workgroup of the scan takes, so the scan recurses."""
    model, x, w, r, st = block_reference(lat, n, unobserved)
    rf, rs = pack(st[0], st[1]), pack(st[2], st[3])
    got = {}
    for chunk in (0, 7, 64):
        gf, gs = gpu_states(lmm, model, x, w, r, chunk)
        assert gf.shape == rf.shape and gs.shape == rs.shape
        close_state(gf.T, rf.T, tol, model.D, f"filtered chunk {chunk}")
        close_state(gs.T, rs.T, tol, model.D, f"smoothed chunk {chunk}")
        got[chunk] = (gf, gs)
    again = gpu_states(lmm, model, x, w, r, 7)
    assert (again[0] == got[7][0]).all() and (again[1] == got[7][1]).all()          # bitwise


def test_states_block_agrees_with_the_filter_and_smoother_blocks(lmm, tol):
    """The first components of the full states are what lmm_dev_statespace_filter / _smooth return: the filtered ones bitwise (one
    kernel writes both), the smoothed ones within the tolerance (the full-state smoother is a second instantiation of the kernel)."""
    model, x, w, r, _ = block_reference("matern52", 257, True)
    _, fm, fv, sm, sv = GS.gpu_blocks(lmm, "matern52", model.v, model.ell, x, w, r, 7)
    gf, gs = gpu_states(lmm, model, x, w, r, 7)
    assert (gf[:, 0] == fm).all() and (gf[:, 3] == fv).all()
    close(gs[:, 0], sm, tol, "smoothed mean"); close(gs[:, 3], sv, tol, "smoothed variance")


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
SHO = {"kind": "sho", "variance": 0.9, "lengthscale": 1.1, "quality": 3.0, "mean": -0.2}
S2 = GS.S2


def kernel_of(lmm, g):
    if g["kind"] == "sho":
        return lmm.SHOKernel(g["variance"], g["lengthscale"], g["quality"])
    return GS.kernel_of(lmm, g["kind"], g["variance"], g["lengthscale"])


def model(lmm, U, Sv, gps):
    fs = lmm.independent_mogp([lmm.GP(g["mean"], kernel_of(lmm, g)) for g in gps])
    return lmm.ILMM(fs, lmm.Orthogonal(U, Sv))


def complete_problem(n, with_sho):
    """test_gpu_statespace.problem(n) (p = 5, three mixed Matern latents); with_sho: a fourth orthonormal column of U and a fourth S
    for the SHO latent."""
    x, U, Sv, Y = GS.problem(n)
    if not with_sho:
        return x, U, Sv, Y, GS.GPS
    rng = np.random.default_rng([n, 4])
    U4 = np.linalg.qr(np.hstack([U, rng.standard_normal((U.shape[0], 1))]))[0]
    return x, U4, np.append(Sv, 1.1), Y, GS.GPS + [SHO]


def nan_problem(n, with_sho):
    """test_gpu_statespace.nan_problem(n) (p = 7); with_sho: the same patterns for m = 4 (a point keeps >= 5 of its 7 outputs)."""
    if not with_sho:
        return GS.nan_problem(n) + (GS.GPS,)
    import test_gpu_missing as GM
    x, U, Sv, Y = GM.problem(n, 1, p=7, m=4, seed=n)
    Y[1, n // 2] = np.nan
    assert np.isnan(Y).any() and (~np.isnan(Y)).sum(axis=0).min() >= 4
    return x, U, Sv, Y, GS.GPS + [SHO]


@pytest.mark.parametrize("with_sho", [False, True])
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("n", [1, 63, 333])
def test_end_to_end(lmm, tol, n, nan, with_sho):
    x, U, Sv, Y, gps = nan_problem(n, with_sho) if nan else complete_problem(n, with_sho)
    p = Y.shape[0]
    f = model(lmm, U, Sv, gps)
    y = Y.reshape(-1)
    fx = f(lmm.MOInputIsotopicByOutputs(x, p), S2)
    Q = PA.queries(x)
    with lmm.statespace_posterior(fx, y) as post:
        assert isinstance(post, lmm.StateSpacePosterior) and post.n == n and post.p == p
        assert post.logpdf == lmm.statespace_logpdf(fx, y)                                  # bitwise
        dense = None if nan else lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(Q, p), S2)
        for add_noise in (True, False):
            gm, gv = post.mean_and_var(Q, add_noise)
            assert gm.shape == (len(Q) * p,) and gv.shape == (len(Q) * p,)
            sm, sv = lmm.statespace_mean_and_var(fx, y, add_noise, xs=Q)
            close(gm, sm, tol, "mean vs xs= route"); close(gv, sv, tol, "var vs xs= route")
            if dense is not None:
                dm, dv = lmm.mean_and_var(dense, add_noise)
                close(gm, dm, tol, "mean vs dense"); close(gv, dv, tol, "var vs dense")
            assert (post.var(Q, add_noise) == gv).all()
        assert (post.mean(Q) == gm).all()
        mg = post.marginals(Q)
        nm, nv = post.mean_and_var(Q, True)
        assert (mg.mu == nm).all() and (mg.sigma == nv ** 0.5).all()
        em, ev = post.mean_and_var(np.zeros(0))
        assert em.shape == (0,) and ev.shape == (0,)
    with pytest.raises(ValueError, match="closed"):
        post.mean_and_var(Q)


def test_independence_and_order(lmm):
    x, U, Sv, Y, gps = complete_problem(333, True)
    p, y = Y.shape[0], Y.reshape(-1)
    f = model(lmm, U, Sv, gps)
    Q = PA.queries(x)
    ns = len(Q)
    post = lmm.statespace_posterior(f(lmm.MOInputIsotopicByOutputs(x, p), S2), y)
    gm, gv = post.mean_and_var(Q)
    perm = np.random.default_rng(5).permutation(ns)
    pm, pv = post.mean_and_var(Q[perm])
    assert (pm.reshape(p, ns) == gm.reshape(p, ns)[:, perm]).all() and (pv.reshape(p, ns) == gv.reshape(p, ns)[:, perm]).all()
    for k in (0, 17, ns - 1):                       # a one-point call is that point's entry of the batched call
        m1, v1 = post.mean_and_var(Q[k:k + 1])
        assert (m1 == gm.reshape(p, ns)[:, k]).all() and (v1 == gv.reshape(p, ns)[:, k]).all()
    am, av = post.mean_and_var(Q)                  # two calls on one handle
    assert (am == gm).all() and (av == gv).all()
    # unsorted training inputs (x has no ties: the stable sort hands the library the same sequence)
    tp = np.random.default_rng(6).permutation(len(x))
    post2 = lmm.statespace_posterior(f(lmm.MOInputIsotopicByOutputs(x[tp], p), S2), Y[:, tp].reshape(-1))
    um, uv = post2.mean_and_var(Q)
    assert post2.logpdf == post.logpdf and (um == gm).all() and (uv == gv).all()
    post.close(); post2.close()
    post.close()                                     # closing twice is fine


def test_duplicated_training_inputs(lmm, tol):
    x, U, Sv, Y, gps = complete_problem(63, True)
    x = x.copy()
    x[10:13] = x[10]
    x[40] = x[41]
    p, y = Y.shape[0], Y.reshape(-1)
    fx = model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    Q = np.concatenate([PA.queries(x), x[[10, 11, 12, 40, 41]]])
    with lmm.statespace_posterior(fx, y) as post:
        for add_noise in (True, False):
            gm, gv = post.mean_and_var(Q, add_noise)
            sm, sv = lmm.statespace_mean_and_var(fx, y, add_noise, xs=Q)
            close(gm, sm, tol, "mean vs xs= route"); close(gv, sv, tol, "var vs xs= route")
            dm, dv = lmm.mean_and_var(lmm.posterior(fx, y)(lmm.MOInputIsotopicByOutputs(Q, p), S2), add_noise)
            close(gm, dm, tol, "mean vs dense"); close(gv, dv, tol, "var vs dense")
            # a query on a duplicated input returns that input's smoothed marginal
            tm, tv = lmm.statespace_mean_and_var(fx, y, add_noise)
            qm, qv = post.mean_and_var(x, add_noise)
            close(qm, tm, tol, "mean at the training inputs"); close(qv, tv, tol, "var at the training inputs")


def test_torch_device_inputs(lmm):
    import torch
    x, U, Sv, Y, gps = complete_problem(63, True)
    p, y = Y.shape[0], Y.reshape(-1)
    f = model(lmm, U, Sv, gps)
    Q = PA.queries(x)
    with lmm.statespace_posterior(f(lmm.MOInputIsotopicByOutputs(x, p), S2), y) as post:
        gm, gv = post.mean_and_var(Q)
        with lmm.statespace_posterior(f(lmm.MOInputIsotopicByOutputs(torch.tensor(x, device="cuda"), p), S2),
                                      torch.tensor(y, device="cuda")) as tpost:
            assert tpost.logpdf == post.logpdf
            tm, tv = tpost.mean_and_var(torch.tensor(Q, device="cuda"))
            assert tm.is_cuda and tv.is_cuda
            assert (tm.cpu().numpy() == gm).all() and (tv.cpu().numpy() == gv).all()
            assert tpost.mean(torch.tensor(Q, device="cuda")).is_cuda
            hm, hv = tpost.mean_and_var(Q)                      # host queries on the same handle: host outputs
            assert isinstance(hm, np.ndarray) and (hm == gm).all() and (hv == gv).all()
            with pytest.raises(ValueError, match="finite"):
                tpost.mean_and_var(torch.tensor([0.0, float("nan")], device="cuda"))


@pytest.mark.parametrize("m", [20, 40])
def test_more_latents_than_a_launch(lmm, tol, m):
    """m Matern32 latents, p = m, n = 63 against the `xs=` route (a launch takes at most 32 latents)."""
    rng = np.random.default_rng(m)
    n = 63
    x = np.sort(rng.uniform(0.0, 8.0, n))
    U = np.linalg.qr(rng.standard_normal((m, m)))[0]
    Sv = rng.uniform(0.5, 2.0, m)
    gps = [{"kind": "matern32", "variance": float(rng.uniform(0.5, 1.5)), "lengthscale": float(rng.uniform(0.5, 1.5)),
            "mean": float(rng.uniform(-0.5, 0.5))} for _ in range(m)]
    y = rng.standard_normal(m * n)
    fx = model(lmm, U, Sv, gps)(lmm.MOInputIsotopicByOutputs(x, m), S2)
    Q = PA.queries(x)
    with lmm.statespace_posterior(fx, y) as post:
        assert post.logpdf == lmm.statespace_logpdf(fx, y)
        gm, gv = post.mean_and_var(Q)
        sm, sv = lmm.statespace_mean_and_var(fx, y, xs=Q)
        close(gm, sm, tol, "mean"); close(gv, sv, tol, "var")


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_c_abi(lmm, tol):
    from lmm_amd import _lib as L
    x, U, Sv, Y = GS.problem(63)
    y = Y.reshape(-1)
    p, n = GS.P_OUT, 63
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(Sv)

    def create(gps, l0=0, l1=3):
        h, out = C.c_void_p(), C.c_double(float("nan"))
        rc = lib.lmm_oilmm_statespace_posterior_create(L.Arr(x).ptr, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, 3, S2, L.gps_array(gps), l0, l1,
                                                       C.byref(h), C.byref(out))
        return rc, h, out.value

    assert lib.lmm_statespace_post_destroy(None) == L.LMM_OK                          # NULL is accepted
    rc, h, val = create(GS.GPS)
    assert rc == L.LMM_OK and h.value
    fx = GS.model(lmm, U, Sv)(lmm.MOInputIsotopicByOutputs(x, p), S2)
    assert val == lmm.statespace_logpdf(fx, y)
    Q = PA.queries(x)
    ns = len(Q)
    mean, var = np.empty(ns * p), np.empty(ns * p)
    # a non-finite xs: LMM_ERR_ARG with its index, whichever comes first
    for bad, at in ((np.nan, 7), (np.inf, 30), (-np.inf, 0)):
        q = Q.copy()
        q[at] = bad
        q[45] = np.nan
        assert lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(q).ptr, ns, 1, L.Arr(mean, True).ptr, L.Arr(var, True).ptr) == L.LMM_ERR_ARG
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        assert info.value == at and b"xs[%d]" % at in lib.lmm_last_error_string()
    # NULL arguments and ns < 1
    assert lib.lmm_oilmm_statespace_post_mean_and_var(None, L.Arr(Q).ptr, ns, 1, L.Arr(mean, True).ptr, None) == L.LMM_ERR_ARG
    assert lib.lmm_oilmm_statespace_post_mean_and_var(h, None, ns, 1, L.Arr(mean, True).ptr, None) == L.LMM_ERR_ARG
    assert lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(Q).ptr, ns, 1, None, None) == L.LMM_ERR_ARG
    assert lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(Q).ptr, 0, 1, L.Arr(mean, True).ptr, None) == L.LMM_ERR_ARG
    # the fp32 mode is refused, at creation and at a query
    lmm.set_compute_dtype("f32")
    try:
        rc32, h32, _ = create(GS.GPS)
        assert rc32 == L.LMM_ERR_UNSUPPORTED and not h32.value and b"Float64 only" in lib.lmm_last_error_string()
        assert lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(Q).ptr, ns, 1, L.Arr(mean, True).ptr, None) == L.LMM_ERR_UNSUPPORTED
    finally:
        lmm.set_compute_dtype("f64")
    # an SE latent: LMM_ERR_UNSUPPORTED naming the latent, and no handle
    se = [GS.GPS[0], {"kind": "se", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0}, GS.GPS[2]]
    rcs, hs, _ = create(se)
    assert rcs == L.LMM_ERR_UNSUPPORTED and not hs.value
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert lat.value == 1 and b"latent 1" in lib.lmm_last_error_string()
    # unsorted inputs name the index, as lmm_oilmm_logpdf_statespace does
    xb = x.copy()
    xb[20], xb[21] = x[21], x[20]
    hb = C.c_void_p()
    assert lib.lmm_oilmm_statespace_posterior_create(L.Arr(xb).ptr, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, 3, S2, L.gps_array(GS.GPS), 0, 3,
                                                     C.byref(hb), None) == L.LMM_ERR_ARG
    lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
    assert info.value == 21 and not hb.value
    # the next valid call is served: var = NULL, and shards are partial sums of the whole
    L.check(lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(Q).ptr, ns, 1, L.Arr(mean, True).ptr, L.Arr(var, True).ptr))
    m2 = np.empty(ns * p)
    L.check(lib.lmm_oilmm_statespace_post_mean_and_var(h, L.Arr(Q).ptr, ns, 1, L.Arr(m2, True).ptr, None))
    assert (m2 == mean).all()
    sm, sv = lmm.statespace_mean_and_var(fx, y, True, xs=Q)
    close(mean, sm, tol, "mean"); close(var, sv, tol, "var")
    ms, vs = np.zeros(ns * p), np.zeros(ns * p)
    for l0, l1 in ((0, 1), (1, 3)):
        rck, hk, vk = create(GS.GPS, l0, l1)
        assert rck == L.LMM_OK
        mo, vo = np.empty(ns * p), np.empty(ns * p)
        L.check(lib.lmm_oilmm_statespace_post_mean_and_var(hk, L.Arr(Q).ptr, ns, 0, L.Arr(mo, True).ptr, L.Arr(vo, True).ptr))
        assert lib.lmm_statespace_post_destroy(hk) == L.LMM_OK
        ms, vs = ms + mo, vs + vo
    nm, nv = lmm.statespace_mean_and_var(fx, y, False, xs=Q)
    close(ms, nm, tol, "shard means"); close(vs, nv, tol, "shard vars")
    assert lib.lmm_statespace_post_destroy(h) == L.LMM_OK
