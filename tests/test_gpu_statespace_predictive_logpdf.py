"""-m gpu: the predictive log density of the state-space posterior object (include/lmm_hip.h "state space: predictive log density";
DESIGN.md 4.18 "Predictive log density from the posterior object"): the building block lmm_dev_statespace_post_logpdf on the
restatement's states at every schedule (a multi-level scan, a ragged last chunk, the single launch), StateSpacePosterior.
predictive_logpdf end to end against the one-shot difference, the dense mirror and the dense Gaussian in NumPy, forecasts against
append, laziness after an append, the C ABI's refusals, and the handle left as it was.

Tolerance (the rule of tests/test_gpu_statespace_posterior.py): max(1e-10, 100 DELTA) of max(1, |reference|), DELTA the largest of
test_statespace_abi.delta(), delta_posterior(), delta_post_rand(), delta_append() and delta_predictive() (2.0e-13): 1e-10.  The
reference is always the NumPy restatement, a dense Gaussian in NumPy or another path of the library (the one-shot filter, the dense
mirror, append), never the handle's own result."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_statespace as GS
import test_gpu_statespace_append as AE
import test_gpu_statespace_posterior as PP
import test_statespace_abi as T
import test_statespace_append_abi as AP
import test_statespace_post_rand_abi as PR
import test_statespace_posterior_abi as PA
import test_statespace_predictive_logpdf_abi as PL

pytestmark = pytest.mark.gpu

MODELS = tuple(T.KINDS) + (("sho", 2.0),)          # the four models of ss_dispatch
S2, P_OUT, GPS = AE.S2, AE.P_OUT, AE.GPS
N, NS = 300, 40


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * max(T.delta(), PA.delta_posterior(), PR.delta_post_rand(), AP.delta_append(), PL.delta_predictive()))


dev, nan_dev, pack = PP.dev, PP.nan_dev, PP.pack


def close1(got, ref, tol, what=""):
    print(f"{what} got {got!r} ref {ref!r} err {abs(got - ref):.3e}")
    assert np.isfinite(got) and abs(got - ref) <= tol * max(1.0, abs(ref)), (what, got, ref)


# ---------------------------------------------------------------------------------------------------
# the building block
# ---------------------------------------------------------------------------------------------------
def gpu_window_logpdf(lmm, model, x, fpk, spk, xs, ws, rs, chunk):
    import torch
    from lmm_amd import _lib as L
    xd, fd, sd, xsd, wd, rd = dev(x), dev(fpk), dev(spk), dev(xs), dev(ws), dev(rs)
    out = nan_dev(1)
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])                       # the mean is not read
    L.check(lmm.load().lmm_dev_statespace_post_logpdf(xd.data_ptr(), len(x), gp, fd.data_ptr(), sd.data_ptr(), xsd.data_ptr(), len(xs),
                                                      wd.data_ptr(), rd.data_ptr(), chunk, out.data_ptr()))
    return float(out.cpu()[0])


def block_queries(x):
    """{label: (sorted xs, ws, rs)}: test_statespace_posterior_abi.queries(x) (the whole range, ties with training inputs, both ends
    and 2 beyond either) with one unobserved query; a set entirely behind the data (a tie with the last input and a repeated query
    among them); one entirely in front of it (first = 0 and the prior branch)."""
    sets = PL.query_sets(x)
    out = {}
    for name in ("whole", "forecasts", "front"):
        xs, ws, rs = sets[name]
        order = np.argsort(xs, kind="stable")
        out[name] = (np.ascontiguousarray(xs[order]), np.ascontiguousarray(ws[order]), np.ascontiguousarray(rs[order]))
    return out


@pytest.mark.parametrize("lat", MODELS, ids=str)
def test_window_filter_block(lmm, tol, lat):
    """lmm_dev_statespace_post_logpdf on the states of the RESTATEMENT at n = 300.  The whole-range window has W = 49 + count > 256
    points: chunk = 1 gives more items than one workgroup of the scan takes (128), so the scan recurses and ss_addprefix_kernel runs
    on SSFwd; chunk = 16 leaves a ragged last chunk; chunk = W is the single launch.  The value does not depend on the chunk beyond
    the tolerance, and two calls at one chunk are bitwise equal."""
    model, x, w, r, st = PP.block_reference(lat, N, True)
    fpk, spk = pack(st[0], st[1]), pack(st[2], st[3])
    for name, (xs, ws, rs) in block_queries(x).items():
        ref = PL.window_logpdf(model, x, st, xs, ws, rs)
        W = len(PL.window_points(x, xs))
        if name == "whole":
            assert W > 256 and W % 16 != 0
        else:
            assert W == len(xs)                                    # no training point inside
        for chunk in (1, 16, W, 0):
            got = gpu_window_logpdf(lmm, model, x, fpk, spk, xs, ws, rs, chunk)
            close1(got, ref, tol, f"{name} chunk {chunk}")
            assert gpu_window_logpdf(lmm, model, x, fpk, spk, xs, ws, rs, chunk) == got          # bitwise
    xs, ws, rs = block_queries(x)["whole"]
    assert gpu_window_logpdf(lmm, model, x, fpk, spk, xs, np.full(len(xs), np.inf), rs, 16) == 0.0       # nothing observed


def test_window_filter_block_refusals(lmm):
    from lmm_amd import _lib as L
    model, x, w, r, st = PP.block_reference("matern32", N, True)
    xs, ws, rs = block_queries(x)["whole"]
    xd, fd, sd, xsd, wd, rd = dev(x), dev(pack(st[0], st[1])), dev(pack(st[2], st[3])), dev(xs), dev(ws), dev(rs)
    out = nan_dev(1)
    gp = L.gps_array([model.desc()])
    lib = lmm.load()

    def call(xq=xsd, ns=len(xs), wq=wd, chunk=0, o=out):
        return lib.lmm_dev_statespace_post_logpdf(xd.data_ptr(), len(x), gp, fd.data_ptr(), sd.data_ptr(), None if xq is None else xq.data_ptr(),
                                                  ns, None if wq is None else wq.data_ptr(), rd.data_ptr(), chunk, o.data_ptr())

    assert call(xq=None) == L.LMM_ERR_ARG and call(wq=None) == L.LMM_ERR_ARG and call(ns=0) == L.LMM_ERR_ARG and call(chunk=-1) == L.LMM_ERR_ARG
    xb = xs.copy()
    xb[3], xb[4] = xs[4] + 1.0, xs[3]
    assert call(xq=dev(xb)) == L.LMM_ERR_ARG                       # the block takes sorted queries
    xb = xs.copy()
    xb[5] = np.nan
    assert call(xq=dev(xb)) == L.LMM_ERR_ARG
    assert np.isnan(out.cpu().numpy()).all()                       # nothing was written
    assert call() == L.LMM_OK


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
_SPLIT = {}


def split_problem(nan):
    """AE.e2e_problem(N + NS) (p = 5, the three Matern latents and the SHO latent, ties in x) split into N training points and NS
    held-out ones: 30 drawn from the whole range (ties with training inputs among them) and the last 10, which are forecasts.
    nan: NaN entries in both parts, and held-out rows without any observation."""
    if nan not in _SPLIT:
        x, U, Sv, Y = AE.e2e_problem(N + NS, nan=nan)
        rng = np.random.default_rng([N, NS, 3])
        held = np.sort(np.concatenate([rng.choice(N + NS - 10, NS - 10, replace=False), np.arange(N + NS - 10, N + NS)]))
        train = np.setdiff1d(np.arange(N + NS), held)
        Yh = Y[:, held].copy()
        if nan:
            Yh[:, 4] = np.nan                                      # one all-NaN row for certain
            Yh[2, 9] = np.nan
        assert not nan or (np.isnan(Yh).all(axis=0).any() and np.isnan(Yh).any(axis=0).sum() > 3)
        _SPLIT[nan] = (x[train], Y[:, train], x[held], Yh, U, Sv)
    return _SPLIT[nan]


def handle(lmm, f, xt, Yt):
    return lmm.statespace_posterior(AE.fx_of(lmm, f, xt), np.ascontiguousarray(Yt).reshape(-1))


def one_shot_difference(lmm, f, xt, Yt, xs, Ys):
    """statespace_logpdf on all the points minus statespace_logpdf on the training points: the library's one-shot filter."""
    xa, Ya = np.concatenate([xt, xs]), np.concatenate([Yt, Ys], axis=1)
    return (lmm.statespace_logpdf(AE.fx_of(lmm, f, xa), np.ascontiguousarray(Ya).reshape(-1))
            - lmm.statespace_logpdf(AE.fx_of(lmm, f, xt), np.ascontiguousarray(Yt).reshape(-1)))


def dense_difference(xt, Yt, xs, Ys, U, Sv):
    """The same from dense Gaussians in NumPy (AE.dense_gaussian: the front end and every latent restated)."""
    xa, Ya = np.concatenate([xt, xs]), np.concatenate([Yt, Ys], axis=1)
    order = np.argsort(xa, kind="stable")
    return AE.dense_gaussian(xa[order], U, Sv, Ya[:, order], xa[:1])[0] - AE.dense_gaussian(xt, U, Sv, Yt, xt[:1])[0]


def _answers(post, Q):
    return post.mean_and_var(Q) + (post.n, post.logpdf)


def _same(a, b):
    return all((np.asarray(u) == np.asarray(v)).all() for u, v in zip(a, b))


def test_end_to_end_complete(lmm, tol):
    """A complete ys: against the one-shot difference, the dense mirror's predictive logpdf and the dense Gaussian in NumPy; with
    another sigma2 against the dense mirror; permuted and torch device inputs bitwise; no queries; the handle unchanged."""
    import torch
    xt, Yt, xs, Ys, U, Sv = split_problem(False)
    f = PP.model(lmm, U, Sv, GPS)
    ys = np.ascontiguousarray(Ys).reshape(-1)
    Q = AE.e2e_queries(xt)
    with handle(lmm, f, xt, Yt) as post:
        base = _answers(post, Q)
        got = post.predictive_logpdf(xs, ys)
        assert isinstance(got, float)
        close1(got, one_shot_difference(lmm, f, xt, Yt, xs, Ys), tol, "vs one-shot difference")
        close1(got, dense_difference(xt, Yt, xs, Ys, U, Sv), tol, "vs dense Gaussian")
        dense = lmm.posterior(AE.fx_of(lmm, f, xt), np.ascontiguousarray(Yt).reshape(-1))
        close1(got, lmm.logpdf(dense(lmm.MOInputIsotopicByOutputs(xs, P_OUT), S2), ys), tol, "vs dense mirror")
        assert post.predictive_logpdf(xs, ys, sigma2=S2) == got                            # the handle's own, given explicitly
        other = post.predictive_logpdf(xs, ys, sigma2=0.37)
        close1(other, lmm.logpdf(dense(lmm.MOInputIsotopicByOutputs(xs, P_OUT), 0.37), ys), tol, "sigma2 = 0.37 vs dense mirror")
        assert abs(other - got) > 1.0                                                      # and it is another number
        # distinct queries in any order, ys carried along: bitwise the sorted call
        keep = np.concatenate([[True], np.diff(xs) > 0])
        xd_, Yd = xs[keep], Ys[:, keep]
        perm = np.random.default_rng(5).permutation(len(xd_))
        assert post.predictive_logpdf(xd_[perm], np.ascontiguousarray(Yd[:, perm]).reshape(-1)) == \
            post.predictive_logpdf(xd_, np.ascontiguousarray(Yd).reshape(-1))
        # torch device tensors: bitwise the NumPy call
        assert post.predictive_logpdf(torch.tensor(xs, device="cuda"), torch.tensor(ys, device="cuda")) == got
        assert post.predictive_logpdf(np.zeros(0), np.zeros(0)) == 0.0
        assert _same(_answers(post, Q), base)                                              # the handle is what it was


def test_end_to_end_missing(lmm, tol):
    """NaN entries in ys and rows without any observation: against the one-shot difference and the dense Gaussian in NumPy; an
    all-NaN ys is 0."""
    xt, Yt, xs, Ys, U, Sv = split_problem(True)
    f = PP.model(lmm, U, Sv, GPS)
    Q = AE.e2e_queries(xt)
    with handle(lmm, f, xt, Yt) as post:
        base = _answers(post, Q)
        got = post.predictive_logpdf(xs, np.ascontiguousarray(Ys).reshape(-1))
        close1(got, one_shot_difference(lmm, f, xt, Yt, xs, Ys), tol, "vs one-shot difference")
        close1(got, dense_difference(xt, Yt, xs, Ys, U, Sv), tol, "vs dense Gaussian")
        rows = ~np.isnan(Ys).all(axis=0)                           # dropping the unobserved queries changes nothing
        close1(post.predictive_logpdf(xs[rows], np.ascontiguousarray(Ys[:, rows]).reshape(-1)), got, tol, "without the all-NaN rows")
        assert post.predictive_logpdf(xs, np.full(NS * P_OUT, np.nan)) == 0.0
        assert _same(_answers(post, Q), base)


def test_forecasts_agree_with_append(lmm, tol):
    """Held-out points at or behind the last input (a tie with it among them): what append returns on a second handle."""
    xt, Yt, _, _, U, Sv = split_problem(True)
    f = PP.model(lmm, U, Sv, GPS)
    rng = np.random.default_rng(8)
    xf = np.concatenate([[xt[-1]], xt[-1] + np.sort(rng.uniform(0.0, 3.0, 16))])
    xf[5] = xf[4]
    Yf = rng.standard_normal((P_OUT, 17))
    Yf[:, 3] = np.nan
    Yf[1, 7] = np.nan
    yf = np.ascontiguousarray(Yf).reshape(-1)
    with handle(lmm, f, xt, Yt) as post, handle(lmm, f, xt, Yt) as second:
        assert post.window(xf) == (N, 0)                           # no training point is touched
        got = post.predictive_logpdf(xf, yf)
        close1(got, second.append(xf, yf), tol, "vs append")
        close1(got, one_shot_difference(lmm, f, xt, Yt, xf, Yf), tol, "vs one-shot difference")
        assert post.n == N and second.n == N + 17


def test_laziness(lmm, tol):
    """After an append a forecast-only call leaves the smoothed states behind and returns bitwise what it returns after smooth(); a
    call with one query in the past brings them up to date and agrees with the one-shot difference on all the data."""
    xt, Yt, xs, Ys, U, Sv = split_problem(True)
    f = PP.model(lmm, U, Sv, GPS)
    n0 = N - 40
    fore = xt[-1] + np.array([0.0, 1e-9, 0.3, 5.0])                # the last input itself is a forecast
    Yfore = np.random.default_rng(4).standard_normal((P_OUT, 4))
    yfore = np.ascontiguousarray(Yfore).reshape(-1)
    with handle(lmm, f, xt[:n0], Yt[:, :n0]) as post:
        post.append(xt[n0:], np.ascontiguousarray(Yt[:, n0:]).reshape(-1))
        assert not post.smoothed
        a = post.predictive_logpdf(fore, yfore)
        assert not post.smoothed
        close1(a, one_shot_difference(lmm, f, xt, Yt, fore, Yfore), tol, "forecasts after an append")
        post.smooth()
        assert post.smoothed and post.predictive_logpdf(fore, yfore) == a
    with handle(lmm, f, xt[:n0], Yt[:, :n0]) as post:
        post.append(xt[n0:], np.ascontiguousarray(Yt[:, n0:]).reshape(-1))
        q = np.concatenate([fore, [xt[3] + 0.01]])                 # one query in the past among forecasts
        Yq = np.concatenate([Yfore, np.random.default_rng(6).standard_normal((P_OUT, 1))], axis=1)
        got = post.predictive_logpdf(q, np.ascontiguousarray(Yq).reshape(-1))
        assert post.smoothed
        close1(got, one_shot_difference(lmm, f, xt, Yt, q, Yq), tol, "one query in the past")
        got = post.predictive_logpdf(xs, np.ascontiguousarray(Ys).reshape(-1))
        close1(got, one_shot_difference(lmm, f, xt, Yt, xs, Ys), tol, "the held-out set after an append")


def test_more_latents_than_a_launch(lmm, tol):
    """m = 40 latents: 34 Matern52 in a row (a launch holds 32 latents of one model, so two launches), then the other models
    alternating (one latent per launch): against the one-shot difference."""
    n, ns, m = 120, 15, 40
    rng = np.random.default_rng(40)
    x = np.sort(rng.uniform(0.0, 10.0, n + ns))
    U = np.linalg.qr(rng.standard_normal((m + 2, m)))[0]
    Sv = rng.uniform(0.5, 2.0, m)
    Y = rng.standard_normal((m + 2, n + ns))
    kinds = [GPS[2]] * 34 + [GPS[0], GPS[1], GPS[3]] * 2
    assert len(kinds) == m
    f = PP.model(lmm, U, Sv, kinds)
    held = np.sort(rng.choice(n + ns, ns, replace=False))
    train = np.setdiff1d(np.arange(n + ns), held)

    def fx(xv):
        return f(lmm.MOInputIsotopicByOutputs(xv, m + 2), S2)

    y = lambda Yv: np.ascontiguousarray(Yv).reshape(-1)
    with lmm.statespace_posterior(fx(x[train]), y(Y[:, train])) as post:
        got = post.predictive_logpdf(x[held], y(Y[:, held]))
    ref = lmm.statespace_logpdf(fx(x), y(Y)) - lmm.statespace_logpdf(fx(x[train]), y(Y[:, train]))
    close1(got, ref, tol, "40 latents")


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals(lmm, tol):
    """Every refusal of lmm_oilmm_statespace_post_logpdf with its code and detail; after each the handle answers bitwise as before."""
    from lmm_amd import _lib as L
    xt, Yt, xs, Ys, U, Sv = split_problem(False)
    f = PP.model(lmm, U, Sv, GPS)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    Q = AE.e2e_queries(xt)
    ys = np.ascontiguousarray(Ys).reshape(-1)
    with handle(lmm, f, xt, Yt) as post:
        h = post._ptr
        base = _answers(post, Q)

        def untouched():
            assert post.smoothed and _same(_answers(post, Q), base)

        def call(xv, ns, yv, s2=0.0, handle_=h, want_out=True):
            out = C.c_double(float("nan"))
            rc = lib.lmm_oilmm_statespace_post_logpdf(handle_, None if xv is None else L.Arr(xv).ptr, ns, None if yv is None else L.Arr(yv).ptr,
                                                      s2, C.byref(out) if want_out else None)
            lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
            return rc, out.value

        rc, ref = call(xs, NS, ys)
        assert rc == L.LMM_OK and ref == post.predictive_logpdf(xs, ys)
        assert call(xs, NS, ys, handle_=None)[0] == L.LMM_ERR_ARG and call(xs, NS, ys, want_out=False)[0] == L.LMM_ERR_ARG
        assert call(xs, -1, ys)[0] == L.LMM_ERR_ARG
        assert call(None, NS, ys)[0] == L.LMM_ERR_ARG and call(xs, NS, None)[0] == L.LMM_ERR_ARG
        assert call(xs, 0, ys) == (L.LMM_OK, 0.0) and call(None, 0, None) == (L.LMM_OK, 0.0)      # no queries
        for s2 in (-0.1, float("nan"), float("inf")):
            assert call(xs, NS, ys, s2)[0] == L.LMM_ERR_ARG and b"sigma2" in lib.lmm_last_error_string()
        untouched()
        lmm.set_compute_dtype("f32")
        try:
            assert call(xs, NS, ys)[0] == L.LMM_ERR_UNSUPPORTED and b"Float64 only" in lib.lmm_last_error_string()
        finally:
            lmm.set_compute_dtype("f64")
        untouched()
        for bad, at in ((np.nan, 5), (np.inf, 0), (-np.inf, NS - 1)):
            xb = xs.copy()
            xb[at] = bad
            assert call(xb, NS, ys)[0] == L.LMM_ERR_ARG and info.value == at
            untouched()
        xb = xs.copy()
        xb[8], xb[9] = xs[9] + 0.5, xs[8]
        assert call(xb, NS, ys)[0] == L.LMM_ERR_ARG and info.value == 9                     # the C ABI takes sorted queries
        untouched()
        Yb = Ys.copy()
        Yb[:3, 6] = np.nan                                                  # 2 of 5 outputs, fewer than m = 4
        assert call(xs, NS, np.ascontiguousarray(Yb).reshape(-1))[0] == L.LMM_ERR_UNSUPPORTED
        assert info.value == 6 and b"point 6 " in lib.lmm_last_error_string()
        untouched()
        with pytest.raises(Exception, match="point 6 "):                    # the mirror hands the refusal on
            post.predictive_logpdf(xs, np.ascontiguousarray(Yb).reshape(-1))
        untouched()
        assert call(xs, NS, ys) == (L.LMM_OK, ref)                          # the next valid call is served, bitwise as before
