"""Host-only checks of the Matern12 / RationalQuadratic latent kinds: the tag registry's RQ shape (include/lmm_hip.h
lmm_kernel_tag_create / lmm_kernel_tag_alpha_grad), the kernel-kind enum against the Python mirror, the mirror's descriptors and the
Julia shim's `_kind` methods.  No GPU and no lmm_init needed."""
import ctypes as C
import math
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


def _tag(lib, d, ard, alpha):
    t = C.c_int(0)
    p = None if ard is None else np.ascontiguousarray(ard, dtype=np.float64).ctypes.data_as(DP)
    rc = lib.lmm_kernel_tag_create(d, p, C.c_double(alpha), C.byref(t))
    return rc, t.value


def test_kernel_tag_symbols_exported():
    lib = lmm_amd.load()
    for s in ("lmm_kernel_tag_create", "lmm_kernel_tag_alpha_grad"):
        assert hasattr(lib, s) and s in L.SYMBOLS


@pytest.mark.parametrize("alpha", [-1.0, math.nan, math.inf, -math.inf])
def test_kernel_tag_rejects_bad_alpha(alpha):
    lib = lmm_amd.load()
    rc, t = _tag(lib, 0, None, alpha)
    assert rc == L.LMM_ERR_ARG and t == 0
    rc, t = _tag(lib, 2, [1.0, 2.0], alpha)
    assert rc == L.LMM_ERR_ARG and t == 0


def test_kernel_tag_rejects_bad_shapes():
    lib = lmm_amd.load()
    assert _tag(lib, 0, None, 0.0)[0] == L.LMM_ERR_ARG            # neither factors nor alpha
    assert _tag(lib, 0, [1.0], 2.0)[0] == L.LMM_ERR_ARG           # d = 0 with a non-NULL ard
    assert _tag(lib, 2, None, 2.0)[0] == L.LMM_ERR_ARG            # d > 0 with a NULL ard
    assert _tag(lib, -1, None, 2.0)[0] == L.LMM_ERR_ARG
    assert _tag(lib, 2, [1.0, 0.0], 2.0)[0] == L.LMM_ERR_ARG      # factors are checked as lmm_ard_create checks them
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(2.0), None) == L.LMM_ERR_ARG


def test_kernel_tag_alpha_only_and_both():
    lib = lmm_amd.load()
    rc, ta = _tag(lib, 0, None, 0.5)                              # an RQ shape alone
    assert rc == L.LMM_OK and ta > 0
    rc, tb = _tag(lib, 3, [0.5, 2.0, 1.5], 7.0)                   # factors and an RQ shape in one tag
    assert rc == L.LMM_OK and tb > 0 and tb != ta
    rc, tc = _tag(lib, 2, [1.0, 3.0], 0.0)                        # alpha = 0: a plain ARD tag
    assert rc == L.LMM_OK and tc > 0
    try:
        g = C.c_double(math.nan)
        for t in (ta, tb, tc):                                    # no gradient call has named them yet
            assert lib.lmm_kernel_tag_alpha_grad(t, C.byref(g)) == L.LMM_OK and g.value == 0.0
        out = np.full(3, 7.5)
        assert lib.lmm_ard_grad(ta, out.ctypes.data_as(DP)) == L.LMM_OK
        assert np.array_equal(out, np.full(3, 7.5))               # a tag without factors: nothing written
        assert lib.lmm_ard_grad(tb, out.ctypes.data_as(DP)) == L.LMM_OK
        assert np.array_equal(out, np.zeros(3))
        assert lib.lmm_kernel_tag_alpha_grad(ta, None) == L.LMM_ERR_ARG
    finally:
        for t in (ta, tb, tc):
            assert lib.lmm_ard_destroy(t) == L.LMM_OK                # lmm_ard_destroy frees any tag
    g = C.c_double()
    assert lib.lmm_kernel_tag_alpha_grad(ta, C.byref(g)) == L.LMM_ERR_ARG
    assert lib.lmm_ard_destroy(tb) == L.LMM_ERR_ARG


def test_header_kernel_enum_matches_mirror():
    src = open(HEADER).read()
    body = re.search(r"typedef enum\s*\{([^}]*)\}\s*lmm_kernel_kind;", src).group(1)
    enum = {k: int(v) for k, v in re.findall(r"LMM_KERNEL_(\w+)\s*=\s*(\d+)", body)}
    assert enum == {"SE": 0, "MATERN32": 1, "MATERN52": 2, "MATERN12": 3, "RQ": 4}
    names = {"SE": "se", "MATERN32": "matern32", "MATERN52": "matern52", "MATERN12": "matern12", "RQ": "rq"}
    assert {names[k]: v for k, v in enum.items()} == L.KERNEL_KINDS


def test_mirror_descriptors():
    assert lmm_amd.ExponentialKernel is lmm_amd.Matern12Kernel
    k12 = lmm_amd.Matern12Kernel(1.5, 0.7)
    rq = lmm_amd.RationalQuadraticKernel(0.8, 1.2, alpha=0.5)
    assert lmm_amd.RationalQuadraticKernel().alpha == 2.0
    assert rq == lmm_amd.RationalQuadraticKernel(0.8, 1.2, alpha=0.5) and rq != lmm_amd.RationalQuadraticKernel(0.8, 1.2, alpha=0.6)
    assert rq != lmm_amd.SEKernel(0.8, 1.2) and k12 != lmm_amd.Matern32Kernel(1.5, 0.7)
    assert "alpha=0.5" in repr(rq)
    with pytest.raises(ValueError):
        lmm_amd.RationalQuadraticKernel(alpha=0.0)
    gps = [lmm_amd.GP(k12), lmm_amd.GP(0.3, rq), lmm_amd.GP(lmm_amd.RationalQuadraticKernel(1.0, [0.5, 2.0], alpha=3.0)),
           lmm_amd.GP(lmm_amd.Matern12Kernel(1.0, [1.0, 4.0]))]
    descs = [g.desc() for g in gps]
    assert descs[1]["alpha"] == 0.5 and "alpha" not in descs[0]
    arr = L.gps_array(descs)
    tags, lib = arr.ard.tags, lmm_amd.load()
    base = [a.kind & L.KERNEL_BASE_MASK for a in arr[:4]]
    assert base == [3, 4, 4, 3]
    assert arr[0].kind == 3 and tags[0] == 0                       # an isotropic Matern12 latent needs no tag
    assert tags[1] > 0 and arr[1].kind >> 8 == tags[1] and arr[1].lengthscale == 1.2
    assert arr.ard.has_alpha[1] and not arr.ard.has_ard[1]
    assert tags[2] > 0 and arr.ard.has_alpha[2] and arr.ard.has_ard[2] and arr[2].lengthscale == 1.0   # ARD + RQ: one tag
    assert tags[3] > 0 and arr.ard.has_ard[3] and not arr.ard.has_alpha[3]
    out = np.full(2, -1.0)
    assert lib.lmm_ard_grad(tags[2], out.ctypes.data_as(DP)) == L.LMM_OK and np.array_equal(out, np.zeros(2))
    assert len(set(t for t in tags if t)) == 3
    arr.ard.close()                                               # the array's tags are destroyed with it
    g = C.c_double()
    assert lib.lmm_kernel_tag_alpha_grad(tags[1], C.byref(g)) == L.LMM_ERR_ARG
    assert arr.ard.tags == [0, 0, 0, 0]


def test_shim_kind_methods_and_tag_ccalls():
    src = open(SHIM).read()
    assert re.search(r"^_kind\(k::ExponentialKernel\)\s*=.*Cint\(3\)", src, re.M)
    assert re.search(r"^_kind\(k::RationalQuadraticKernel\)\s*=.*Cint\(4\)", src, re.M)
    assert re.search(r"_alpha\(k::RationalQuadraticKernel\)\s*=\s*Float64\(only\(k\.α\)\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_create, liblmm\), Cint, \(Cint, Ptr\{Cdouble\}, Cdouble, Ref\{Cint\}\)", src)
    assert re.search(r"ccall\(\(:lmm_kernel_tag_alpha_grad, liblmm\), Cint, \(Cint, Ref\{Cdouble\}\)", src)
    assert re.search(r"_ktangent\(k::RationalQuadraticKernel,.*\n.*α=\[gα\]", src)
    assert "Euclidean" in src
