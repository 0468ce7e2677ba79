"""Host-only checks of periodic latent kernels (KernelFunctions' PeriodicKernel; include/lmm_hip.h LMM_KERNEL_PERIODIC): the tag
registry entry points lmm_kernel_tag_create_periodic / lmm_kernel_tag_rho_grad, periodic terms of lmm_kernel_sum_create, the Python
mirror's PeriodicKernel and descriptors, and the Julia shim's methods.  No GPU and no lmm_init needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lmm_amd
from lmm_amd import _lib as L

DP = C.POINTER(C.c_double)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "linearmixingmodels.jl_amd", "julia", "LinearMixingModelsHIP.jl")
HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
PER = 7


def _rho_tag(lib, rho, ard=None):
    t = C.c_int(0)
    if ard is None:
        rc = lib.lmm_kernel_tag_create_periodic(0, None, C.c_double(rho), C.byref(t))
    else:
        a = np.ascontiguousarray(ard, dtype=np.float64)
        rc = lib.lmm_kernel_tag_create_periodic(int(a.size), a.ctypes.data_as(DP), C.c_double(rho), C.byref(t))
    return rc, t.value


def _sum(lib, *ts):
    arr = (L.GpT * len(ts))()
    for i, (kind, v, l) in enumerate(ts):
        arr[i].kind, arr[i].variance, arr[i].lengthscale, arr[i].mean = kind, v, l, 0.0
    t = C.c_int(0)
    return lib.lmm_kernel_sum_create(len(ts), arr, C.byref(t)), t.value


def test_periodic_symbols_declared_and_exported():
    lib = lmm_amd.load()
    for s in ("lmm_kernel_tag_create_periodic", "lmm_kernel_tag_rho_grad"):
        assert hasattr(lib, s) and s in L.SYMBOLS
    src = open(HEADER).read()
    assert re.search(r"#define\s+LMM_KERNEL_PERIODIC\s+7\b", src)
    assert "int lmm_kernel_tag_create_periodic(int d, const double* ard, double rho, int* tag);" in src
    assert "int lmm_kernel_tag_rho_grad(int tag, double* out);" in src
    # outside the enum and outside the mirror's table of base kinds
    enum = re.search(r"typedef enum \{([^}]*)\} lmm_kernel_kind;", src).group(1)
    assert "PERIODIC" not in enum
    assert L.KERNEL_PERIODIC == PER and PER not in L.KERNEL_KINDS.values() and "periodic" not in L.KERNEL_KINDS


def test_tag_create_periodic_validation():
    lib = lmm_amd.load()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _rho_tag(lib, bad)[0] == L.LMM_ERR_ARG, bad
    assert lib.lmm_kernel_tag_create_periodic(0, None, C.c_double(1.0), None) == L.LMM_ERR_ARG          # NULL tag pointer
    assert lib.lmm_kernel_tag_create_periodic(2, None, C.c_double(1.0), C.byref(C.c_int())) == L.LMM_ERR_ARG     # d > 0, NULL ard
    assert _rho_tag(lib, 1.0, [1.0, -2.0])[0] == L.LMM_ERR_ARG
    rc, t = _rho_tag(lib, 0.7, [1.0, 2.0, 0.5])
    assert rc == L.LMM_OK and t > 0
    out = C.c_double(-1.0)
    assert lib.lmm_kernel_tag_rho_grad(t, C.byref(out)) == L.LMM_OK and out.value == 0.0       # no gradient call yet
    assert lib.lmm_kernel_tag_rho_grad(t, None) == L.LMM_ERR_ARG
    g = np.full(3, -1.0)
    assert lib.lmm_ard_grad(t, g.ctypes.data_as(DP)) == L.LMM_OK and np.all(g == 0.0)
    assert lib.lmm_ard_destroy(t) == L.LMM_OK
    assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG                                             # destroyed twice
    assert lib.lmm_kernel_tag_rho_grad(t, C.byref(out)) == L.LMM_ERR_ARG


def test_alpha_and_rho_gradients_do_not_cross():
    lib = lmm_amd.load()
    ta = C.c_int(0)
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK        # alpha only
    rc, tr = _rho_tag(lib, 1.3)
    assert rc == L.LMM_OK
    tf = C.c_int(0)
    f = np.array([1.0, 2.0])
    assert lib.lmm_ard_create(2, f.ctypes.data_as(DP), C.byref(tf)) == L.LMM_OK                # factors only
    out = C.c_double(0.0)
    assert lib.lmm_kernel_tag_rho_grad(ta.value, C.byref(out)) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_rho_grad(tf.value, C.byref(out)) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_alpha_grad(tr, C.byref(out)) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_alpha_grad(ta.value, C.byref(out)) == L.LMM_OK
    for t in (ta.value, tr, tf.value):
        assert lib.lmm_ard_destroy(t) == L.LMM_OK


def test_sum_create_with_periodic_terms():
    lib = lmm_amd.load()
    rc, tr = _rho_tag(lib, 0.8)
    assert rc == L.LMM_OK
    ta = C.c_int(0)
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK
    made = []
    rc, t = _sum(lib, (PER, 1.0, 2.0), (0, 0.5, 1.0))                       # without a rho tag
    assert rc == L.LMM_OK; made.append(t)
    rc, t = _sum(lib, (PER | (tr << 8), 1.0, 2.0), (2, 0.5, 1.0))           # with one
    assert rc == L.LMM_OK; made.append(t)
    g = (L.GpGradT * 2)()
    assert lib.lmm_kernel_sum_grad(t, g) == L.LMM_OK and g[0].variance == 0.0 and g[0].mean == 0.0
    assert _sum(lib, (PER | (ta.value << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG          # a periodic term whose tag carries an alpha
    assert _sum(lib, (0 | (tr << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG                  # a non-periodic term whose tag carries a rho
    assert _sum(lib, (4 | (tr << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG
    for bad in (5, 6, 8, 9):
        assert _sum(lib, (bad, 1.0, 1.0))[0] == L.LMM_ERR_UNSUPPORTED, bad
    for t in made + [tr, ta.value]:
        assert lib.lmm_ard_destroy(t) == L.LMM_OK


def test_mirror_periodic_kernel():
    k = lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7)
    assert k.desc() == {"kind": "periodic", "variance": 0.9, "lengthscale": 2.5, "r": 0.7}
    assert k.period == 2.5 and k.kind == "periodic"
    assert k.key() != lmm_amd.PeriodicKernel(0.9, 2.5, r=0.8).key() and k.key() == lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7).key()
    assert k == lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7) and k != lmm_amd.PeriodicKernel(0.9, 2.5, r=0.71)
    assert k != lmm_amd.PeriodicKernel(0.9, 2.6, r=0.7) and k != lmm_amd.SEKernel(0.9, 2.5)
    assert "r=0.7" in repr(k) and repr(k).startswith("PeriodicKernel(")
    assert lmm_amd.PeriodicKernel().r == 1.0 and lmm_amd.PeriodicKernel().period == 1.0
    assert lmm_amd.PeriodicKernel(1.0, [2.0, 3.0], r=[0.5, 0.5]).r == 0.5            # a vector r with equal entries
    kv = lmm_amd.PeriodicKernel(1.0, [2.0, 3.0])
    assert np.array_equal(kv.period, [2.0, 3.0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), [0.5, 0.6], []):
        with pytest.raises(ValueError):
            lmm_amd.PeriodicKernel(1.0, 1.0, r=bad)
    assert lmm_amd.GP(0.3, k).desc()["mean"] == 0.3 and lmm_amd.GP(0.3, k).desc()["r"] == 0.7
    s = k + lmm_amd.SEKernel(0.4, 1.1)
    assert isinstance(s, lmm_amd.KernelSum) and s.desc()["terms"][0] == k.desc()
    assert s.key() != (lmm_amd.PeriodicKernel(0.9, 2.5, r=0.8) + lmm_amd.SEKernel(0.4, 1.1)).key()
    assert lmm_amd.KernelSum(k, lmm_amd.Matern32Kernel()) == lmm_amd.KernelSum(k, lmm_amd.Matern32Kernel())


def test_mirror_gps_array_tags():
    # a descriptor without "r" and with a scalar period: the bare kind, no tag
    arr = L.gps_array([{"kind": "periodic", "variance": 1.0, "lengthscale": 2.0}])
    assert arr[0].kind == PER and arr.ard.tags[0] == 0 and arr[0].lengthscale == 2.0
    # a kernel object always carries its r, so that its gradient is reported
    arr = L.gps_array([lmm_amd.PeriodicKernel(1.0, 2.0, r=0.6).desc(), lmm_amd.SEKernel().desc()])
    assert arr[0].kind & 0xFF == PER and arr[0].kind >> 8 == arr.ard.tags[0] > 0
    assert arr.ard.has_rho[0] and not arr.ard.has_ard[0] and not arr.ard.has_alpha[0] and not arr.ard.has_rho[1]
    assert arr.ard.rho_grad(0) == 0.0
    # a length-1 vector period: one factor in the tag, lengthscale 1 (the library folds it into the isotropic descriptor at d == 1)
    arr = L.gps_array([lmm_amd.PeriodicKernel(1.0, [2.5], r=0.6).desc()])
    assert arr.ard.has_ard[0] and arr.ard.has_rho[0] and arr[0].lengthscale == 1.0
    assert np.array_equal(arr.ard.grad(0, 1), [0.0])
    with pytest.raises(ValueError):
        L.gps_array([{"kind": "periodic", "lengthscale": 1.0, "r": [0.5, 0.7]}])
    with pytest.raises(ValueError):
        L.gps_array([{"kind": "periodic", "lengthscale": 1.0, "r": -1.0}])
    # as a sum term
    arr = L.gps_array([(lmm_amd.PeriodicKernel(1.0, 2.0, r=0.6) + lmm_amd.RationalQuadraticKernel(1.0, 1.0, alpha=3.0)).desc()])
    ta = arr.ard.terms[0]
    assert arr[0].kind & 0xFF == L.KERNEL_SUM and ta.has_rho == [True, False] and ta.has_alpha == [False, True]
    g = arr.ard.sum_grad(0, 1)
    assert g[0]["r"] == 0.0 and "alpha" not in g[0] and g[1]["alpha"] == 0.0 and "r" not in g[1]


def test_shim_periodic_methods():
    src = open(SHIM).read()
    assert re.search(r"_kind\(k::PeriodicKernel\)\s*=\s*Cint\(7\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_create_periodic,\s*liblmm\),\s*Cint,\s*\(Cint,\s*Ptr\{Cdouble\},\s*Cdouble,\s*Ref\{Cint\}\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_rho_grad,\s*liblmm\),\s*Cint,\s*\(Cint,\s*Ref\{Cdouble\}\)", src)
    assert re.search(r"_ktangent\(k::PeriodicKernel,", src)
    assert re.search(r"unequal entries of r", src)                 # a vector r with unequal entries is an error(...)
