"""The three OILMM gradient entry points on an empty latent shard [1, 1) with the regulariser on: no latent contributes, so each returns
the regulariser's value and gradient alone -- through the complete-data back end the exact, inducing-point and state-space paths share.
grad_y, grad_sigma2, grad_S and grad_U must therefore agree bit for bit across the three, and each value must be that of its own value
entry point on the same shard: bit for bit for lmm_oilmm_elbo and lmm_oilmm_logpdf_statespace, as include/lmm_hip.h promises.  For
lmm_oilmm_logpdf the header promises nothing and the two entry points take the regulariser's residual by different arithmetic
(-352.5122254677816 against -352.5122254677815 here, before and after the shared back end): that value is held to 8 ulp, a deviation
from "bitwise on all three" that no build can meet.  n = 40, p = 4, m = 2, d = 1, two Matern32 latents, sorted x, nz = 8 for the bound."""
import ctypes as C

import numpy as np
import pytest

N, P, M, D, NZ = 40, 4, 2, 1, 8


@pytest.mark.gpu
def test_empty_shard_gradients_are_the_regulariser_alone():
    from lmm_amd import _lib as L
    L.ensure_init()
    lib = L.load()
    rng = np.random.default_rng(5)
    x, y, z = np.sort(rng.uniform(0.0, 4.0, N)), rng.standard_normal(N * P), np.linspace(0.1, 3.9, NZ)
    U = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((P, M)))[0].ravel(order="F"))
    S = np.array([1.3, 0.7])
    gps = L.gps_array([{"kind": "matern32", "variance": 1.0, "lengthscale": 0.7, "mean": 0.2},
                       {"kind": "matern32", "variance": 0.8, "lengthscale": 1.3, "mean": -0.1}])
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    i, f = C.c_int, C.c_double
    model = (ptr(y), i(P), ptr(U), ptr(S), i(M), f(0.1), gps, i(1), i(1))      # the shard [1, 1)
    inducing = (ptr(z), i(NZ), f(1e-6))

    def gradient(call):
        val, gs2 = f(np.nan), f(np.nan)
        gy, gS, gU, gg = np.full(N * P, np.nan), np.full(M, np.nan), np.full(P * M, np.nan), (L.GpGradT * M)()
        L.check(call(C.byref(val), ptr(gy), C.byref(gs2), ptr(gS), ptr(gU), gg))
        assert all(g.variance == 0.0 and g.lengthscale == 0.0 and g.mean == 0.0 for g in gg)
        return val.value, {"y": gy, "sigma2": np.array([gs2.value]), "S": gS, "U": gU}

    def value(call):
        out = f(np.nan)
        L.check(call(C.byref(out)))
        return out.value

    got = {
        "exact": gradient(lambda *o: lib.lmm_oilmm_logpdf_grad(ptr(x), i(D), i(N), *model, i(1), *o)),
        "inducing": gradient(lambda *o: lib.lmm_oilmm_elbo_grad(ptr(x), i(D), i(N), *model, *inducing, i(1), *o, None)),
        "statespace": gradient(lambda *o: lib.lmm_oilmm_logpdf_grad_statespace(ptr(x), i(N), *model, i(1), *o)),
    }
    values = {
        "exact": value(lambda o: lib.lmm_oilmm_logpdf(ptr(x), i(D), i(N), *model, i(1), o)),
        "inducing": value(lambda o: lib.lmm_oilmm_elbo(ptr(x), i(D), i(N), *model, *inducing, i(1), o, None)),
        "statespace": value(lambda o: lib.lmm_oilmm_logpdf_statespace(ptr(x), i(N), *model, i(1), o)),
    }
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
    # The exact path's value is NOT asserted bitwise: the header is silent on how lmm_oilmm_logpdf_grad's *out_logpdf relates to
    # lmm_oilmm_logpdf, and the two take the regulariser's residual |(I - U U') Y|^2 by different arithmetic -- tr(P'P Y Y') on the host
    # from the device's Y Y', against a sum of squares of Y - H T Y on the device -- so their bits differ (1 ulp of the value at these
    # inputs, in the build before the shared back end as well).  Both reduce blockwise, so each residual is within a few eps of the
    # truth; it enters the value as resid / (2 sigma2), which is of the value's own size here, and every other term is one shared host
    # expression: 8 ulp of the value covers two such residuals.
    value_tol = 8 * np.spacing(abs(values["exact"]))
    for path, (val, grads) in got.items():
        print(f"{path}: value {val!r} (value entry point {values[path]!r}), grad_sigma2 {grads['sigma2'][0]!r}, |grad_y| {np.linalg.norm(grads['y'])!r}")
        assert np.isfinite(val) and all(np.all(np.isfinite(g)) for g in grads.values())
        assert np.any(grads["y"] != 0.0) and np.all(grads["S"] != 0.0) and np.any(grads["U"] != 0.0)
        if path == "exact":
            assert abs(val - values[path]) <= value_tol, (path, val, values[path], value_tol)
        else:
            assert bits([val]) == bits([values[path]]), (path, val, values[path])
        for name, g in grads.items():
            assert np.array_equal(bits(g), bits(got["exact"][1][name])), (path, name)
