"""-m gpu: appending observations to the state-space posterior object (include/lmm_hip.h "state space: appending observations";
DESIGN.md 4.18 "Appending observations"): the filter from a stored state alone against the restatement, StateSpacePosterior.append end
to end against the one-shot handle and the dense Gaussian, the laziness rule, the capacity policy, determinism, the C ABI's refusals
and torch device inputs.

Tolerance (the rule of tests/test_gpu_statespace_posterior.py): max(1e-10, 100 DELTA) of max|reference| per array, DELTA the largest of
test_statespace_abi.delta() (7.6e-15), test_statespace_posterior_abi.delta_posterior() (1.7e-13),
test_statespace_post_rand_abi.delta_post_rand() and test_statespace_append_abi.delta_append() (1.4e-13): 1e-10.  A stored state is
compared component by component.  The reference is the NumPy restatement, a dense Gaussian built in NumPy or the library's one-shot
path (statespace_posterior on all the data), never the appended handle itself.  Where two results of the library must agree bitwise
(laziness, capacity, determinism, a refused call) they are compared with ==."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_missing as GM
import test_gpu_statespace as GS
import test_gpu_statespace_posterior as PP
import test_sho_abi as S
import test_statespace_abi as T
import test_statespace_append_abi as AP
import test_statespace_post_rand_abi as PR
import test_statespace_posterior_abi as PA

pytestmark = pytest.mark.gpu

LATENTS = PP.LATENTS
S2 = GS.S2
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return max(1e-10, 100.0 * max(T.delta(), PA.delta_posterior(), PR.delta_post_rand(), AP.delta_append()))


close, dev, nan_dev, pack = PP.close, PP.dev, PP.nan_dev, PP.pack


# ---------------------------------------------------------------------------------------------------
# the building block
# ---------------------------------------------------------------------------------------------------
N0 = 30          # points in front of the stored state


def from_case(lat, k, unobserved):
    """(model, x, w, r) of N0 + k points (test_gpu_statespace_posterior.block_case: unobserved runs longer than a chunk, ties for the
    oscillator); unobserved: the first new point is unobserved as well and lies at spacing 0 from the stored state's input."""
    model, x, w, r = PP.block_case(lat, N0 + k, unobserved)
    x, w = x.copy(), w.copy()
    w[N0 - 1] = 0.2
    if unobserved:
        x[N0] = x[N0 - 1]
        w[N0] = np.inf
    else:
        w[N0] = 0.3
    return model, x, w, r


_FROM = {}


def from_reference(lat, k, unobserved):
    """The case, the restated state of point N0 - 1 and the restated continuation, computed once."""
    key = (lat, k, unobserved)
    if key not in _FROM:
        model, x, w, r = from_case(lat, k, unobserved)
        _, _, _, fm0, fP0 = S.kalman_filter(model, x[:N0], w[:N0], r[:N0])
        _FROM[key] = (model, x, w, r, fm0[-1], fP0[-1], AP.filter_from(model, fm0[-1], fP0[-1], x[N0 - 1], x[N0:], w[N0:], r[N0:]))
    return _FROM[key]


def gpu_filter_from(lmm, model, m0, P0, x0, x, w, r, chunk):
    import torch
    from lmm_amd import _lib as L
    k, comps = len(x), model.D + model.D * (model.D + 1) // 2
    sd, xd, wd, rd = dev(pack(m0[None], P0[None])[0]), dev(x), dev(w), dev(r)
    fm, fv, fs, lml = nan_dev(k), nan_dev(k), nan_dev(k, comps), nan_dev(1)
    torch.cuda.synchronize()
    gp = L.gps_array([model.desc(mean=0.7)])                       # the mean is not read
    L.check(lmm.load().lmm_dev_statespace_filter_from(sd.data_ptr(), float(x0), xd.data_ptr(), k, gp, wd.data_ptr(), rd.data_ptr(), chunk,
                                                      fm.data_ptr(), fv.data_ptr(), fs.data_ptr(), lml.data_ptr()))
    return float(lml.cpu()[0]), fm.cpu().numpy(), fv.cpu().numpy(), fs.cpu().numpy()


@pytest.mark.parametrize("unobserved", [False, True])
@pytest.mark.parametrize("k", [1, 17, 40, 2100])
@pytest.mark.parametrize("lat", LATENTS, ids=str)
def test_filter_from_block(lmm, tol, lat, k, unobserved):
    """lmm_dev_statespace_filter_from on the RESTATEMENT's state against the restated continuation: k = 1 is one chunk (the restart
    kernel alone), 17 and 40 are two and three chunks of the default 16, 2100 is 132 aggregates (the scan recurses); chunk = k is the
    sequential filter, chunk = 7 another schedule."""
    model, x, w, r, m0, P0, (val, rm, rP) = from_reference(lat, k, unobserved)
    rs = pack(rm, rP)
    for chunk in (0, k, 7):
        lml, fm, fv, fs = gpu_filter_from(lmm, model, m0, P0, x[N0 - 1], x[N0:], w[N0:], r[N0:], chunk)
        print(f"chunk {chunk}: lml {lml!r} ref {val!r}")
        if val == 0.0:
            assert lml == 0.0                                      # nothing observed: no term at all
        else:
            assert np.isfinite(lml) and abs(lml - val) <= tol * abs(val), (chunk, lml, val)
        PP.close_state(fs.T, rs.T, tol, model.D, f"filtered chunk {chunk}")
        assert (fm == fs[:, 0]).all() and (fv == fs[:, model.D]).all()              # one kernel writes both
    if unobserved:                                                 # spacing 0, unobserved: the stored state, bit for bit
        assert (fs[0] == pack(m0[None], P0[None])[0]).all()
    again = gpu_filter_from(lmm, model, m0, P0, x[N0 - 1], x[N0:], w[N0:], r[N0:], 7)
    assert again[0] == lml and (again[3] == fs).all()


def test_filter_from_refuses_a_state_behind_the_points(lmm):
    from lmm_amd import _lib as L
    model, x, w, r, m0, P0, _ = from_reference("matern32", 17, False)
    comps = 5
    sd, xd, wd, rd = dev(pack(m0[None], P0[None])[0]), dev(x[N0:]), dev(w[N0:]), dev(r[N0:])
    fm, fv, fs, lml = nan_dev(17), nan_dev(17), nan_dev(17, comps), nan_dev(1)
    gp = L.gps_array([model.desc()])
    lib = lmm.load()
    args = (xd.data_ptr(), 17, gp, wd.data_ptr(), rd.data_ptr(), 0, fm.data_ptr(), fv.data_ptr(), fs.data_ptr(), lml.data_ptr())
    assert lib.lmm_dev_statespace_filter_from(sd.data_ptr(), float(x[N0] + 1e-9), *args) == L.LMM_ERR_ARG
    assert lib.lmm_dev_statespace_filter_from(None, float(x[N0 - 1]), *args) == L.LMM_ERR_ARG
    assert lib.lmm_dev_statespace_filter_from(sd.data_ptr(), float("nan"), *args) == L.LMM_ERR_ARG
    assert np.isnan(fs.cpu().numpy()).all()                        # nothing was written


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
GPS = GS.GPS + [PP.SHO]
P_OUT, M = 5, 4
_E2E = {}


def e2e_problem(n, ties=True, nan=True):
    """x (n,), U (5, 4), S (4,), Y (5, n): a jittered grid of spacing 0.1 (with runs of equal inputs when `ties`), and, when `nan`,
    one point in seven without any observation and one in five observing four of its five outputs (p_t >= m)."""
    key = (n, ties, nan)
    if key not in _E2E:
        rng = np.random.default_rng([n, 77])
        x = 0.1 * (np.arange(n) + rng.uniform(-0.3, 0.3, n))
        if ties:
            for t in range(3, n - 1, 23):
                x[t + 1] = x[t]
        U, Sv = GM.flat_orthogonal(rng, P_OUT, M), rng.uniform(0.5, 2.0, M)
        Y = rng.standard_normal((P_OUT, n))
        if nan:
            for t in range(n):
                if t % 7 == 2:
                    Y[:, t] = np.nan
                elif t % 5 == 1:
                    Y[int(rng.integers(0, P_OUT)), t] = np.nan
        _E2E[key] = (x, U, Sv, Y)
    return _E2E[key]


def models():
    return [S.Model(g["kind"], g["variance"], g["lengthscale"], g.get("quality")) for g in GPS]


def front(Y, U, Sv, s2):
    """The front end restated (test_gpu_missing.restatement, with points without any observation as w = +Inf, r = 0 and no
    regulariser term): w, r (m, n) per latent with the latent's mean taken off, reg (n,) per point."""
    H = U * np.sqrt(Sv)
    (p, n), m = Y.shape, H.shape[1]
    w, r, reg = np.full((m, n), np.inf), np.zeros((m, n)), np.zeros(n)
    means = np.array([g["mean"] for g in GPS])
    for t in range(n):
        ob = ~np.isnan(Y[:, t])
        if not ob.any():
            continue
        Ht, yt = H[ob], Y[ob, t]
        G = Ht.T @ Ht
        z = np.linalg.solve(G, Ht.T @ yt)
        w[:, t], r[:, t] = s2 * np.diag(np.linalg.inv(G)), z - means
        res = yt - Ht @ z
        reg[t] = -0.5 * ((ob.sum() - m) * np.log(2.0 * np.pi * s2) + np.linalg.slogdet(G)[1] + res @ res / s2)
    return H, w, r, reg


def dense_latent(mod, x, w, r, xs):
    """(log density of r, mean, var at xs) of one zero-mean latent from one Cholesky factor of K + diag(w) over the observed points."""
    import scipy.linalg as sla
    obs = np.flatnonzero(np.isfinite(w))
    if len(obs) == 0:
        return 0.0, np.zeros(len(xs)), np.full(len(xs), mod.v)
    Lc = np.linalg.cholesky(mod.K(x[obs]) + np.diag(w[obs]))
    V = sla.solve_triangular(Lc, mod.K(x[obs], xs), lower=True)
    u = sla.solve_triangular(Lc, r[obs], lower=True)
    val = -0.5 * (u @ u + 2.0 * np.log(np.diag(Lc)).sum() + len(obs) * np.log(2.0 * np.pi))
    return val, V.T @ u, mod.v - (V * V).sum(axis=0)


def dense_gaussian(x, U, Sv, Y, xs):
    """(logpdf, mean, var) of the restated model from dense Gaussians per latent."""
    H, w, r, reg = front(Y, U, Sv, S2)
    val, ml, vl = reg.sum(), [], []
    for l, mod in enumerate(models()):
        lv, mu, v = dense_latent(mod, x, w[l], r[l], np.asarray(xs))
        val += lv
        ml.append(mu + GPS[l]["mean"]); vl.append(v)
    return val, (H @ np.array(ml)).reshape(-1), ((H * H) @ np.array(vl) + S2).reshape(-1)


def restated_increment(x, U, Sv, Y, n0):
    """log p(y[n0:] | y[:n0]) of the restated model: per latent the filter continued from the restated state of point n0 - 1, and
    the regulariser terms of the new points."""
    _, w, r, reg = front(Y, U, Sv, S2)
    inc = reg[n0:].sum()
    for l, mod in enumerate(models()):
        _, _, _, fm, fP = S.kalman_filter(mod, x[:n0], w[l, :n0], r[l, :n0])
        inc += AP.filter_from(mod, fm[-1], fP[-1], x[n0 - 1], x[n0:], w[l, n0:], r[l, n0:])[0]
    return inc


def fx_of(lmm, f, x):
    return f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)


def e2e_queries(x):
    """Interior queries, training inputs (ties among them), the last input and forecasts behind it, shuffled."""
    rng = np.random.default_rng([len(x), 5])
    q = np.concatenate([rng.uniform(x[0] - 0.5, x[-1], 12), rng.choice(x, 4), x[[0, -1]], x[-1] + np.array([1e-9, 0.05, 0.7, 30.0])])
    return rng.permutation(q)


@pytest.mark.parametrize("seq", [(1,), (17, 1, 40), (2100,)], ids=str)
@pytest.mark.parametrize("n0", [1, 40, 300])
def test_append_end_to_end(lmm, tol, n0, seq):
    """Build on n0 points, append in the sequence; after every append the value, the increment and mean_and_var at interior, tied and
    forecast queries against the one-shot handle on all the data so far and against the dense Gaussian."""
    x, U, Sv, Y = e2e_problem(n0 + sum(seq))
    f = PP.model(lmm, U, Sv, GPS)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:n0]), Y[:, :n0].reshape(-1)) as post:
        n = n0
        for k in seq:
            perm = np.random.default_rng([n, k]).permutation(k)            # the caller's order is any order
            before = post.logpdf
            inc = post.append(x[n:n + k][perm], Y[:, n:n + k][:, perm].reshape(-1))
            ref_inc = restated_increment(x[:n + k], U, Sv, Y[:, :n + k], n)
            n += k
            assert post.n == n and post.logpdf == before + inc and not post.smoothed
            print(f"n {n}: increment {inc!r} ref {ref_inc!r}")
            assert abs(inc - ref_inc) <= tol * abs(ref_inc), (inc, ref_inc)
            Q = e2e_queries(x[:n])
            dval, dm, dv = dense_gaussian(x[:n], U, Sv, Y[:, :n], Q)
            with lmm.statespace_posterior(fx_of(lmm, f, x[:n]), Y[:, :n].reshape(-1)) as one:
                assert abs(post.logpdf - one.logpdf) <= tol * abs(one.logpdf), (post.logpdf, one.logpdf)
                assert abs(post.logpdf - dval) <= tol * abs(dval), (post.logpdf, dval)
                gm, gv = post.mean_and_var(Q)
                assert post.smoothed                                       # interior queries among them
                om, ov = one.mean_and_var(Q)
                close(gm, om, tol, "mean vs one-shot"); close(gv, ov, tol, "var vs one-shot")
                close(gm, dm, tol, "mean vs dense"); close(gv, dv, tol, "var vs dense")


def test_append_across_the_plan_threshold(lmm, tol):
    """The library's plan changes at 4096 points (16 -> 64 points per thread): k = 4200 new points take the 64-point plan in the
    filter from the stored state, and the 4500 kept states take it in the smoother, where every other test runs the 16-point plan.
    Against the one-shot handle and the restated increment."""
    n0, k = 300, 4200
    x, U, Sv, Y = e2e_problem(n0 + k)
    f = PP.model(lmm, U, Sv, GPS)
    Q = e2e_queries(x)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:n0]), Y[:, :n0].reshape(-1)) as post, \
            lmm.statespace_posterior(fx_of(lmm, f, x), Y.reshape(-1)) as one:
        inc = post.append(x[n0:], Y[:, n0:].reshape(-1))
        ref_inc = restated_increment(x, U, Sv, Y, n0)
        assert abs(inc - ref_inc) <= tol * abs(ref_inc), (inc, ref_inc)
        assert abs(post.logpdf - one.logpdf) <= tol * abs(one.logpdf), (post.logpdf, one.logpdf)
        gm, gv = post.mean_and_var(Q)
        om, ov = one.mean_and_var(Q)
        close(gm, om, tol, "mean vs one-shot"); close(gv, ov, tol, "var vs one-shot")


def test_vjp_and_rand_against_the_one_shot_handle(lmm, tol):
    """mean_and_var_vjp and rand (same normals; inputs and queries at least 0.02 apart, no ties) of a handle built on 40 points and
    appended to three times, against the one-shot handle on all 98."""
    x, U, Sv, Y = e2e_problem(98, ties=False)
    f = PP.model(lmm, U, Sv, GPS)
    rng = np.random.default_rng(3)
    Q = rng.permutation(np.concatenate([x[[5, 30, 41, 60, 90]] + 0.03, x[-1] + np.array([0.04, 0.5])]))
    dmean, dvar = rng.standard_normal(len(Q) * P_OUT), rng.standard_normal(len(Q) * P_OUT)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as post, \
            lmm.statespace_posterior(fx_of(lmm, f, x), Y.reshape(-1)) as one:
        n = 40
        for k in (17, 1, 40):
            post.append(x[n:n + k], Y[:, n:n + k].reshape(-1))
            n += k
        assert post.window(Q) == one.window(Q)
        for kw in ({"dmean": dmean, "dvar": dvar}, {"dmean": dmean}, {"dvar": dvar}):
            close(post.mean_and_var_vjp(Q, **kw)["x"], one.mean_and_var_vjp(Q, **kw)["x"], tol, f"vjp {sorted(kw)}")
        for add_noise in (True, False):
            a = post.rand(np.random.default_rng(11), Q, 3, add_noise)
            b = one.rand(np.random.default_rng(11), Q, 3, add_noise)
            close(a, b, tol, f"rand add_noise={add_noise}")


def test_laziness(lmm):
    """After an append the smoothed states are behind; a forecast-only query leaves them there and returns bitwise what it returns
    after smooth(); an interior query brings them up to date."""
    x, U, Sv, Y = e2e_problem(57)
    f = PP.model(lmm, U, Sv, GPS)
    fore = x[-1] + np.array([0.0, 1e-9, 0.3, 5.0])                        # the last input itself is a forecast
    dm = np.random.default_rng(1).standard_normal(len(fore) * P_OUT)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as post:
        assert post.smoothed
        post.append(x[40:], Y[:, 40:].reshape(-1))
        assert not post.smoothed
        gm, gv = post.mean_and_var(fore)
        gx = post.mean_and_var_vjp(fore, dm, dm)["x"]
        gr = post.rand(np.random.default_rng(2), fore, 2)
        assert post.window(fore) == (57, 0)
        assert not post.smoothed
        post.smooth()
        assert post.smoothed
        sm, sv = post.mean_and_var(fore)
        assert (sm == gm).all() and (sv == gv).all()
        assert (post.mean_and_var_vjp(fore, dm, dm)["x"] == gx).all()
        assert (post.rand(np.random.default_rng(2), fore, 2) == gr).all()
        post.smooth()                                                       # nothing to do
        im, iv = post.mean_and_var(x[:5] + 0.01)
    for trigger in ("mean_and_var", "vjp", "rand"):
        with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as post:
            post.append(x[40:], Y[:, 40:].reshape(-1))
            q = np.array([x[-1] + 1.0, x[3] + 0.01])                       # one interior query among forecasts
            if trigger == "mean_and_var":
                post.mean_and_var(q)
            elif trigger == "vjp":
                post.mean_and_var_vjp(q, np.ones(2 * P_OUT))
            else:
                post.rand(np.random.default_rng(0), q)
            assert post.smoothed, trigger
            am, av = post.mean_and_var(x[:5] + 0.01)
            assert (am == im).all() and (av == iv).all()                   # on demand or explicit: the same smoothed states


def _answers(post, Q):
    return post.mean_and_var(Q) + (post.rand(np.random.default_rng(4), Q, 2), post.logpdf)


def _same(a, b):
    return all((np.asarray(u) == np.asarray(v)).all() for u, v in zip(a, b))


def test_capacity(lmm):
    """Three appends that cross two growths (40 -> 80 -> 160) give bitwise what the same appends give after reserve; a handle never
    appended to has cap = n and answers bitwise like a second one built the same way."""
    x, U, Sv, Y = e2e_problem(140, ties=False)
    f = PP.model(lmm, U, Sv, GPS)
    Q = np.concatenate([x[[2, 50, 100, 139]] + 0.03, [x[-1] + 0.4]])
    pieces = ((40, 57), (57, 97), (97, 140))
    with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as grown, \
            lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as roomy, \
            lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as fresh:
        assert grown.capacity == 40 and _same(_answers(grown, Q), _answers(fresh, Q))
        roomy.reserve(1000)
        roomy.reserve(10)                                                   # smaller: nothing
        assert roomy.capacity == 1000 and roomy.smoothed and _same(_answers(roomy, Q), _answers(fresh, Q))
        caps = []
        for a, b in pieces:
            ia, ib = grown.append(x[a:b], Y[:, a:b].reshape(-1)), roomy.append(x[a:b], Y[:, a:b].reshape(-1))
            assert ia == ib
            caps.append(grown.capacity)
            fq = x[b - 1] + np.array([0.0, 0.2])
            assert _same(grown.mean_and_var(fq), roomy.mean_and_var(fq))    # forecasts from the filtered states alone
        assert caps == [80, 160, 160] and roomy.capacity == 1000
        assert _same(_answers(grown, Q), _answers(roomy, Q))
        assert fresh.capacity == 40 and fresh.n == 40 and fresh.smoothed


def test_determinism(lmm):
    x, U, Sv, Y = e2e_problem(120)
    f = PP.model(lmm, U, Sv, GPS)
    Q = e2e_queries(x)
    runs = []
    for _ in range(2):
        with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as post:
            incs = [post.append(x[40:41], Y[:, 40:41].reshape(-1))]
            fm = post.mean_and_var(x[40:41] + 0.5)
            incs.append(post.append(x[41:120], Y[:, 41:120].reshape(-1)))
            runs.append((np.array(incs),) + fm + post.mean_and_var(Q) + (post.mean_and_var_vjp(Q, np.ones(len(Q) * P_OUT))["x"],))
    assert _same(runs[0], runs[1])


def test_torch_device_inputs(lmm, tol):
    import torch
    x, U, Sv, Y = e2e_problem(57)
    f = PP.model(lmm, U, Sv, GPS)
    Q = e2e_queries(x)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:40]), Y[:, :40].reshape(-1)) as post, \
            lmm.statespace_posterior(fx_of(lmm, f, torch.tensor(x[:40], device="cuda")), torch.tensor(Y[:, :40].reshape(-1), device="cuda")) as tpost:
        perm = np.random.default_rng(9).permutation(17)
        xn, yn = x[40:][perm], Y[:, 40:][:, perm].reshape(-1)
        inc = post.append(xn, yn)
        tinc = tpost.append(torch.tensor(xn, device="cuda"), torch.tensor(yn, device="cuda"))
        assert tinc == inc and tpost.n == 57 and tpost.logpdf == post.logpdf
        tm, tv = tpost.mean_and_var(torch.tensor(Q, device="cuda"))
        gm, gv = post.mean_and_var(Q)
        assert tm.is_cuda and (tm.cpu().numpy() == gm).all() and (tv.cpu().numpy() == gv).all()
        with pytest.raises(ValueError, match="finite"):
            tpost.append(torch.tensor([x[-1] + 1.0, float("nan")], device="cuda"), torch.zeros(2 * P_OUT, device="cuda", dtype=torch.float64))
        with pytest.raises(ValueError, match="at or behind the last input"):
            tpost.append(torch.tensor([x[-1] - 1e-6], device="cuda"), torch.zeros(P_OUT, device="cuda", dtype=torch.float64))
        assert tpost.n == 57


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals(lmm, tol):
    """Every refusal of lmm_oilmm_statespace_post_append with its code and detail; after each the handle has its size and answers
    bitwise as before; k = 0 is a no-op."""
    from lmm_amd import _lib as L
    x, U, Sv, Y = e2e_problem(57, ties=False, nan=False)
    f = PP.model(lmm, U, Sv, GPS)
    lib = lmm.load()
    lat, info = C.c_int(), C.c_int()
    n, k = 40, 17
    Q = e2e_queries(x[:n])
    xn, yn = np.ascontiguousarray(x[n:]), np.ascontiguousarray(Y[:, n:]).reshape(-1)
    with lmm.statespace_posterior(fx_of(lmm, f, x[:n]), Y[:, :n].reshape(-1)) as post:
        h = post._ptr
        base = post.mean_and_var(Q)

        def size():
            a, b, c = C.c_int(), C.c_int(), C.c_int()
            assert lib.lmm_statespace_post_size(h, C.byref(a), C.byref(b), C.byref(c)) == L.LMM_OK
            return a.value, b.value, c.value

        def untouched():
            assert size() == (n, n, n) and _same(post.mean_and_var(Q), base)

        def append(xv, kk, yv, handle=h):
            out = C.c_double(float("nan"))
            rc = lib.lmm_oilmm_statespace_post_append(handle, None if xv is None else L.Arr(xv).ptr, kk, None if yv is None else L.Arr(yv).ptr,
                                                      C.byref(out))
            lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
            return rc, out.value

        assert size() == (n, n, n)
        assert lib.lmm_statespace_post_size(None, None, None, None) == L.LMM_ERR_ARG
        assert append(xn, k, yn, None)[0] == L.LMM_ERR_ARG
        assert append(xn, -1, yn)[0] == L.LMM_ERR_ARG
        assert append(None, k, yn)[0] == L.LMM_ERR_ARG and append(xn, k, None)[0] == L.LMM_ERR_ARG
        untouched()
        assert append(xn, 0, yn) == (L.LMM_OK, 0.0) and append(None, 0, None)[0] == L.LMM_OK      # k = 0: a no-op
        untouched()
        lmm.set_compute_dtype("f32")
        try:
            assert append(xn, k, yn)[0] == L.LMM_ERR_UNSUPPORTED and b"Float64 only" in lib.lmm_last_error_string()
            assert lib.lmm_statespace_post_smooth(h) == L.LMM_ERR_UNSUPPORTED
        finally:
            lmm.set_compute_dtype("f64")
        untouched()
        for bad, at in ((np.nan, 5), (np.inf, 0), (-np.inf, 16)):
            xb = xn.copy()
            xb[at] = bad
            assert append(xb, k, yn)[0] == L.LMM_ERR_ARG
            assert info.value == at and b"x_new[%d]" % at in lib.lmm_last_error_string()
            untouched()
        xb = xn.copy()
        xb[8], xb[9] = xn[9], xn[8]
        assert append(xb, k, yn)[0] == L.LMM_ERR_ARG and info.value == 9
        untouched()
        xb = xn.copy()
        xb[0] = x[n - 1] - 1e-9
        assert append(xb, k, yn)[0] == L.LMM_ERR_ARG and info.value == 0
        assert b"at or behind the last input" in lib.lmm_last_error_string()
        untouched()
        yb = Y[:, n:].copy()
        yb[:3, 6] = np.nan                                                  # 2 of 5 outputs, fewer than m = 4
        assert append(xn, k, np.ascontiguousarray(yb).reshape(-1))[0] == L.LMM_ERR_UNSUPPORTED
        assert info.value == n + 6 and b"point %d " % (n + 6) in lib.lmm_last_error_string()
        untouched()
        assert append(xn, INT_MAX, yn)[0] == L.LMM_ERR_ARG                  # n + k > INT_MAX: refused before anything is read
        untouched()
        assert lib.lmm_statespace_post_smooth(None) == L.LMM_ERR_ARG and lib.lmm_statespace_post_reserve(None, 10) == L.LMM_ERR_ARG
        assert lib.lmm_statespace_post_smooth(h) == L.LMM_OK                # nothing to do
        untouched()
        # the next valid call is served, and a tie with the last input is one
        xt = xn.copy()
        xt[0] = x[n - 1]
        rc, inc = append(xt, k, yn)
        assert rc == L.LMM_OK and np.isfinite(inc) and size() == (n + k, n, 2 * n)
        assert lib.lmm_statespace_post_reserve(h, 100) == L.LMM_OK and size() == (n + k, n, 100)
        assert lib.lmm_statespace_post_smooth(h) == L.LMM_OK and size() == (n + k, n + k, 100)
        post.n, post._x_last = n + k, float(xt[-1])                          # the mirror's own copies, for the calls below
        xall = np.concatenate([x[:n], xt])
        with lmm.statespace_posterior(fx_of(lmm, f, xall), Y.reshape(-1)) as one:
            qm, qv = post.mean_and_var(Q)
            om, ov = one.mean_and_var(Q)
            close(qm, om, tol, "mean after the tie"); close(qv, ov, tol, "var after the tie")
