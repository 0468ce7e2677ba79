"""Host-only checks of locally periodic latent kernels (SE x Periodic as one base kind; include/lmm_hip.h
LMM_KERNEL_LOCALLY_PERIODIC): the tag registry entry points lmm_kernel_tag_create_locally_periodic / lmm_kernel_tag_decay_grad,
locally periodic terms of lmm_kernel_sum_create, the Python mirror's LocallyPeriodicKernel, `*` and descriptors, and the Julia shim's
methods.  No GPU and no lmm_init needed."""
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
PER, LP = 7, 10


def _lp_tag(lib, rho, decay, ard=None):
    t = C.c_int(0)
    if ard is None:
        rc = lib.lmm_kernel_tag_create_locally_periodic(0, None, C.c_double(rho), C.c_double(decay), C.byref(t))
    else:
        a = np.ascontiguousarray(ard, dtype=np.float64)
        rc = lib.lmm_kernel_tag_create_locally_periodic(int(a.size), a.ctypes.data_as(DP), C.c_double(rho), C.c_double(decay), C.byref(t))
    return rc, t.value


def _sum(lib, *ts):
    arr = (L.GpT * len(ts))()
    for i, (kind, v, l) in enumerate(ts):
        arr[i].kind, arr[i].variance, arr[i].lengthscale, arr[i].mean = kind, v, l, 0.0
    t = C.c_int(0)
    return lib.lmm_kernel_sum_create(len(ts), arr, C.byref(t)), t.value


def test_symbols_declared_and_exported():
    lib = lmm_amd.load()
    for s in ("lmm_kernel_tag_create_locally_periodic", "lmm_kernel_tag_decay_grad"):
        assert hasattr(lib, s) and s in L.SYMBOLS
    src = open(HEADER).read()
    assert re.search(r"#define\s+LMM_KERNEL_LOCALLY_PERIODIC\s+10\b", src)
    assert "int lmm_kernel_tag_create_locally_periodic(int d, const double* ard, double rho, double decay, int* tag);" in src
    assert "int lmm_kernel_tag_decay_grad(int tag, double* out);" in src
    enum = re.search(r"typedef enum \{([^}]*)\} lmm_kernel_kind;", src).group(1)
    assert "PERIODIC" not in enum
    assert L.KERNEL_LOCALLY_PERIODIC == LP and LP not in L.KERNEL_KINDS.values() and "locally_periodic" not in L.KERNEL_KINDS


def test_tag_create_validation_and_readout():
    lib = lmm_amd.load()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _lp_tag(lib, bad, 1.0)[0] == L.LMM_ERR_ARG, bad          # rho
        assert _lp_tag(lib, 1.0, bad)[0] == L.LMM_ERR_ARG, bad          # decay
    assert lib.lmm_kernel_tag_create_locally_periodic(0, None, C.c_double(1.0), C.c_double(1.0), None) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_create_locally_periodic(2, None, C.c_double(1.0), C.c_double(1.0), C.byref(C.c_int())) == L.LMM_ERR_ARG
    assert _lp_tag(lib, 1.0, 1.0, [1.0, -2.0])[0] == L.LMM_ERR_ARG
    rc, t = _lp_tag(lib, 0.7, 2.5, [1.0, 2.0, 0.5])
    assert rc == L.LMM_OK and t > 0
    out = C.c_double(-1.0)
    assert lib.lmm_kernel_tag_decay_grad(t, C.byref(out)) == L.LMM_OK and out.value == 0.0       # no gradient call yet
    out = C.c_double(-1.0)
    assert lib.lmm_kernel_tag_rho_grad(t, C.byref(out)) == L.LMM_OK and out.value == 0.0         # rho is served as for a periodic tag
    assert lib.lmm_kernel_tag_decay_grad(t, None) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_alpha_grad(t, C.byref(out)) == L.LMM_ERR_ARG
    g = np.full(3, -1.0)
    assert lib.lmm_ard_grad(t, g.ctypes.data_as(DP)) == L.LMM_OK and np.all(g == 0.0)
    assert lib.lmm_ard_destroy(t) == L.LMM_OK
    assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_tag_decay_grad(t, C.byref(out)) == L.LMM_ERR_ARG
    # a periodic (rho only), an alpha and a factor tag have no decay
    tr, ta, tf = C.c_int(0), C.c_int(0), C.c_int(0)
    f = np.array([1.0, 2.0])
    assert lib.lmm_kernel_tag_create_periodic(0, None, C.c_double(1.2), C.byref(tr)) == L.LMM_OK
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK
    assert lib.lmm_ard_create(2, f.ctypes.data_as(DP), C.byref(tf)) == L.LMM_OK
    for tt in (tr, ta, tf):
        assert lib.lmm_kernel_tag_decay_grad(tt.value, C.byref(out)) == L.LMM_ERR_ARG
        assert lib.lmm_ard_destroy(tt.value) == L.LMM_OK


def test_sum_create_with_locally_periodic_terms_and_tag_rules():
    lib = lmm_amd.load()
    rc, tl = _lp_tag(lib, 0.8, 3.0)
    assert rc == L.LMM_OK
    tr, ta = C.c_int(0), C.c_int(0)
    assert lib.lmm_kernel_tag_create_periodic(0, None, C.c_double(1.2), C.byref(tr)) == L.LMM_OK
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK
    made = []
    rc, t = _sum(lib, (LP, 1.0, 2.0), (1, 0.5, 1.0))                        # untagged: rho = 1, decay = 1
    assert rc == L.LMM_OK; made.append(t)
    rc, t = _sum(lib, (LP | (tl << 8), 1.0, 2.0), (PER, 0.5, 1.0))          # tagged, next to a periodic term
    assert rc == L.LMM_OK; made.append(t)
    g = (L.GpGradT * 2)()
    assert lib.lmm_kernel_sum_grad(t, g) == L.LMM_OK and g[0].variance == 0.0 and g[0].lengthscale == 0.0
    assert _sum(lib, (LP | (ta.value << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG          # an alpha tag on kind 10
    assert _sum(lib, (LP | (tr.value << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG          # a plain rho tag on kind 10
    assert _sum(lib, (0 | (tl << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG                 # a locally periodic tag on kinds 0 and 7
    assert _sum(lib, (PER | (tl << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG
    assert _sum(lib, (4 | (tl << 8), 1.0, 2.0))[0] == L.LMM_ERR_ARG
    for bad in (5, 6, 8, 9, 11):
        assert _sum(lib, (bad, 1.0, 1.0))[0] == L.LMM_ERR_UNSUPPORTED, bad
    for t in made + [tl, tr.value, ta.value]:
        assert lib.lmm_ard_destroy(t) == L.LMM_OK


def test_mirror_locally_periodic_kernel():
    K = lmm_amd.LocallyPeriodicKernel
    k = K(0.9, 2.5, r=0.7, decay=3.0)
    assert k.desc() == {"kind": "locally_periodic", "variance": 0.9, "lengthscale": 2.5, "r": 0.7, "decay": 3.0}
    assert k.period == 2.5 and k.kind == "locally_periodic" and k.decay == 3.0
    assert k.key() == K(0.9, 2.5, r=0.7, decay=3.0).key()
    assert k.key() != K(0.9, 2.5, r=0.7, decay=3.1).key() and k.key() != K(0.9, 2.5, r=0.8, decay=3.0).key()
    assert k.key() != lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7).key()
    assert k == K(0.9, 2.5, r=0.7, decay=3.0) and k != K(0.9, 2.5, r=0.7, decay=3.5) and k != K(0.9, 2.5, r=0.71, decay=3.0)
    assert k != lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7) and lmm_amd.PeriodicKernel(0.9, 2.5, r=0.7) != k
    assert repr(k).startswith("LocallyPeriodicKernel(") and "r=0.7" in repr(k) and "decay=3.0" in repr(k)
    d = K()
    assert (d.variance, d.period, d.r, d.decay) == (1.0, 1.0, 1.0, 1.0)
    assert np.array_equal(K(1.0, [2.0, 3.0], r=[0.5, 0.5]).period, [2.0, 3.0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError):
            K(1.0, 1.0, decay=bad)
    for bad in (0.0, float("nan"), [0.5, 0.6]):
        with pytest.raises(ValueError):
            K(1.0, 1.0, r=bad)
    assert lmm_amd.GP(0.3, k).desc()["decay"] == 3.0
    s = k + lmm_amd.Matern32Kernel(0.4, 1.1)
    assert isinstance(s, lmm_amd.KernelSum) and s.desc()["terms"][0] == k.desc()
    assert s.key() != (K(0.9, 2.5, r=0.7, decay=3.1) + lmm_amd.Matern32Kernel(0.4, 1.1)).key()


def test_mirror_multiplication():
    se, per = lmm_amd.SEKernel(0.5, 4.0), lmm_amd.PeriodicKernel(3.0, [2.0, 2.5], r=0.6)
    want = lmm_amd.LocallyPeriodicKernel(1.5, [2.0, 2.5], r=0.6, decay=4.0)
    assert se * per == want and per * se == want
    assert type(se * per) is lmm_amd.LocallyPeriodicKernel
    assert (se * lmm_amd.PeriodicKernel(1.0, 2.0)).desc() == {"kind": "locally_periodic", "variance": 0.5, "lengthscale": 2.0,
                                                               "r": 1.0, "decay": 4.0}
    with pytest.raises(ValueError):
        lmm_amd.SEKernel(1.0, [1.0, 2.0]) * per                      # a per-dimension decay
    refused = [(se, se), (per, per), (lmm_amd.Matern52Kernel(), per), (per, lmm_amd.Matern32Kernel()), (se, lmm_amd.RationalQuadraticKernel()),
               (want, se), (se, want), (se + per, per), (per, se + per)]
    for a, b in refused:
        with pytest.raises(NotImplementedError, match=r"SEKernel \* PeriodicKernel"):
            a * b
    with pytest.raises(TypeError):
        se * 2.0


def test_mirror_gps_array_kind_word_and_tags():
    # a descriptor without "r" / "decay" and with a scalar period: the bare kind, no tag (rho = 1, decay = 1 in the library)
    arr = L.gps_array([{"kind": "locally_periodic", "variance": 1.0, "lengthscale": 2.0}])
    assert arr[0].kind == LP and arr.ard.tags[0] == 0 and arr[0].lengthscale == 2.0
    # a kernel object always carries r and decay, so that their gradients are reported
    arr = L.gps_array([lmm_amd.LocallyPeriodicKernel(1.0, 2.0, r=0.6, decay=3.0).desc(), lmm_amd.PeriodicKernel(1.0, 2.0, r=0.6).desc()])
    assert arr[0].kind & 0xFF == LP and arr[0].kind >> 8 == arr.ard.tags[0] > 0 and arr[0].lengthscale == 2.0
    assert arr.ard.has_rho[0] and arr.ard.has_decay[0] and not arr.ard.has_ard[0] and not arr.ard.has_alpha[0]
    assert arr.ard.has_rho[1] and not arr.ard.has_decay[1]
    assert arr.ard.rho_grad(0) == 0.0 and arr.ard.decay_grad(0) == 0.0
    # "decay" alone asks for a tag too; a vector period goes into it
    arr = L.gps_array([{"kind": "locally_periodic", "lengthscale": [2.5, 3.0], "decay": 2.0}])
    assert arr.ard.has_ard[0] and arr.ard.has_rho[0] and arr.ard.has_decay[0] and arr[0].lengthscale == 1.0
    assert np.array_equal(arr.ard.grad(0, 2), [0.0, 0.0])
    for bad in ({"decay": -1.0}, {"decay": [1.0, 2.0]}, {"decay": float("inf")}, {"r": [0.5, 0.7]}):
        with pytest.raises(ValueError):
            L.gps_array([dict({"kind": "locally_periodic", "lengthscale": 1.0}, **bad)])
    with pytest.raises(ValueError):
        L.gps_array([{"kind": "periodic", "lengthscale": 1.0, "decay": 2.0}])
    # as a sum term
    arr = L.gps_array([(lmm_amd.LocallyPeriodicKernel(1.0, 2.0, r=0.6, decay=3.0) + lmm_amd.PeriodicKernel(1.0, 1.0, r=0.9)).desc()])
    ta = arr.ard.terms[0]
    assert arr[0].kind & 0xFF == L.KERNEL_SUM and ta.has_rho == [True, True] and ta.has_decay == [True, False]
    g = arr.ard.sum_grad(0, 1)
    assert g[0]["r"] == 0.0 and g[0]["decay"] == 0.0 and g[1]["r"] == 0.0 and "decay" not in g[1]


def test_shim_locally_periodic_methods():
    src = open(SHIM).read()
    assert re.search(r"ccall\(\(:lmm_kernel_tag_create_locally_periodic,\s*liblmm\),\s*Cint,\s*"
                     r"\(Cint,\s*Ptr\{Cdouble\},\s*Cdouble,\s*Cdouble,\s*Ref\{Cint\}\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_decay_grad,\s*liblmm\),\s*Cint,\s*\(Cint,\s*Ref\{Cdouble\}\)", src)
    assert re.search(r"Cint\(10\)", src)
    assert re.search(r"_ktangent\(k::KernelProduct,", src)
    assert re.search(r"KernelProduct.*not served", src)            # every other product is an error(...)
