"""Host-only checks of sum kernels (KernelFunctions' KernelSum as a latent kernel): the sum-tag registry (include/lmm_hip.h
lmm_kernel_sum_create / lmm_kernel_sum_grad), the Python mirror's KernelSum and descriptors, and the Julia shim's sum methods.  No GPU
and no lmm_init needed."""
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


def _terms(*ts):
    arr = (L.GpT * max(len(ts), 1))()
    for i, (kind, v, l, mean) in enumerate(ts):
        arr[i].kind, arr[i].variance, arr[i].lengthscale, arr[i].mean = kind, v, l, mean
    return arr


def _sum(lib, *ts, n=None):
    t = C.c_int(0)
    rc = lib.lmm_kernel_sum_create(len(ts) if n is None else n, _terms(*ts), C.byref(t))
    return rc, t.value


def test_sum_symbols_declared_and_exported():
    lib = lmm_amd.load()
    for s in ("lmm_kernel_sum_create", "lmm_kernel_sum_grad"):
        assert hasattr(lib, s) and s in L.SYMBOLS
    src = open(HEADER).read()
    assert re.search(r"#define\s+LMM_KERNEL_SUM\s+5", src)
    assert re.search(r"#define\s+LMM_SUM_MAX_TERMS\s+4", src)
    assert "int lmm_kernel_sum_create(int nterms, const lmm_gp_t* terms, int* tag);" in src
    assert "int lmm_kernel_sum_grad(int tag, lmm_gp_grad_t* out);" in src
    assert L.KERNEL_SUM == 5


def test_sum_create_grad_destroy_roundtrip():
    lib = lmm_amd.load()
    rc, t = _sum(lib, (2, 1.0, 0.5, 0.0), (0, 0.3, 2.0, 0.0))
    assert rc == L.LMM_OK and t > 0
    g = (L.GpGradT * 2)()
    assert lib.lmm_kernel_sum_grad(t, g) == L.LMM_OK            # no gradient call yet: zeros
    assert all(g[c].variance == 0.0 and g[c].lengthscale == 0.0 for c in range(2))
    out = np.zeros(1)
    assert lib.lmm_ard_grad(t, out.ctypes.data_as(DP)) == L.LMM_OK and out[0] == 0.0     # no factors: writes nothing
    assert lib.lmm_ard_destroy(t) == L.LMM_OK
    assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_sum_grad(t, g) == L.LMM_ERR_ARG


def test_sum_create_validation():
    lib = lmm_amd.load()
    ok = (2, 1.0, 1.0, 0.0)
    assert _sum(lib, n=0)[0] == L.LMM_ERR_ARG                                      # term count
    assert _sum(lib, ok, ok, ok, ok, ok)[0] == L.LMM_ERR_ARG
    assert _sum(lib, ok, ok, ok, ok)[0] == L.LMM_OK
    assert _sum(lib, ok, (5, 1.0, 1.0, 0.0))[0] == L.LMM_ERR_UNSUPPORTED           # nested sum
    assert _sum(lib, (6, 1.0, 1.0, 0.0))[0] == L.LMM_ERR_UNSUPPORTED               # bad base kind
    assert _sum(lib, (0, 0.0, 1.0, 0.0))[0] == L.LMM_ERR_ARG                       # non-positive variance
    assert _sum(lib, (0, 1.0, -1.0, 0.0))[0] == L.LMM_ERR_ARG                      # non-positive lengthscale
    assert _sum(lib, (0, 1.0, 1.0, 0.5))[0] == L.LMM_ERR_ARG                       # a term has no mean
    assert lib.lmm_kernel_sum_create(1, _terms(ok), None) == L.LMM_ERR_ARG
    assert lib.lmm_kernel_sum_create(1, None, C.byref(C.c_int())) == L.LMM_ERR_ARG


def test_sum_terms_with_tags():
    lib = lmm_amd.load()
    ta = C.c_int(0)
    assert lib.lmm_kernel_tag_create(0, None, C.c_double(3.0), C.byref(ta)) == L.LMM_OK     # an RQ alpha
    tb = C.c_int(0)
    ard = np.array([1.0, 2.0])
    assert lib.lmm_ard_create(2, ard.ctypes.data_as(DP), C.byref(tb)) == L.LMM_OK
    assert _sum(lib, (0 | ta.value << 8, 1.0, 1.0, 0.0))[0] == L.LMM_ERR_ARG            # alpha on a non-RQ term
    rc, s = _sum(lib, (4 | ta.value << 8, 1.0, 1.0, 0.0), (2 | tb.value << 8, 1.0, 1.0, 0.0))
    assert rc == L.LMM_OK
    assert _sum(lib, (2 | s << 8, 1.0, 1.0, 0.0))[0] == L.LMM_ERR_ARG                  # a sum tag as a term tag
    for t in (s, ta.value, tb.value):
        assert lib.lmm_ard_destroy(t) == L.LMM_OK
    assert _sum(lib, (2 | tb.value << 8, 1.0, 1.0, 0.0))[0] == L.LMM_ERR_ARG           # a destroyed term tag
    # ... and the tag numbers are reused: destroy and recreate
    rc, s2 = _sum(lib, (1, 1.0, 1.0, 0.0))
    assert rc == L.LMM_OK and lib.lmm_ard_destroy(s2) == L.LMM_OK


def test_sum_tags_count_against_the_tag_limit():
    lib = lmm_amd.load()
    tags = []
    try:
        while True:
            rc, t = _sum(lib, (0, 1.0, 1.0, 0.0))
            if rc != L.LMM_OK:
                assert rc == L.LMM_ERR_UNSUPPORTED
                break
            tags.append(t)
            assert len(tags) <= 4096
        assert len(tags) >= 4000                # the bound is 4096 live tags (a few may be held elsewhere in this process)
        ard = np.array([1.0])
        t = C.c_int(0)
        assert lib.lmm_ard_create(1, ard.ctypes.data_as(DP), C.byref(t)) == L.LMM_ERR_UNSUPPORTED
    finally:
        for t in tags:
            lib.lmm_ard_destroy(t)
    rc, t = _sum(lib, (0, 1.0, 1.0, 0.0))
    assert rc == L.LMM_OK and lib.lmm_ard_destroy(t) == L.LMM_OK


def test_mirror_kernel_sum():
    k = lmm_amd.SEKernel() + lmm_amd.Matern52Kernel(variance=0.5, lengthscale=2.0)
    assert isinstance(k, lmm_amd.KernelSum) and len(k.kernels) == 2
    k3 = k + lmm_amd.RationalQuadraticKernel(alpha=3.0)                       # flattened: the inner sum has unit scale
    assert len(k3.kernels) == 3 and isinstance(k3.kernels[2], lmm_amd.RationalQuadraticKernel)
    assert lmm_amd.KernelSum(k, lmm_amd.Matern12Kernel()).kernels == k.kernels + (lmm_amd.Matern12Kernel(),)
    with pytest.raises(ValueError):
        lmm_amd.KernelSum(lmm_amd.KernelSum(lmm_amd.SEKernel(), variance=2.0), lmm_amd.SEKernel())
    with pytest.raises(ValueError):
        k3 + lmm_amd.SEKernel() + lmm_amd.SEKernel()                          # 5 terms
    with pytest.raises(ValueError):
        lmm_amd.KernelSum(lmm_amd.SEKernel(), lengthscale=np.array([1.0, 2.0]))
    assert k == lmm_amd.SEKernel() + lmm_amd.Matern52Kernel(variance=0.5, lengthscale=2.0)
    assert k != lmm_amd.Matern52Kernel(variance=0.5, lengthscale=2.0) + lmm_amd.SEKernel()
    assert k != lmm_amd.KernelSum(*k.kernels, variance=2.0)
    d = lmm_amd.GP(1.5, lmm_amd.KernelSum(*k3.kernels, variance=2.0, lengthscale=0.5)).desc()
    assert d["kind"] == "sum" and d["variance"] == 2.0 and d["lengthscale"] == 0.5 and d["mean"] == 1.5
    assert [t["kind"] for t in d["terms"]] == ["se", "matern52", "rq"] and d["terms"][2]["alpha"] == 3.0


def test_gps_array_encodes_sum_tags_and_releases_them():
    lib = lmm_amd.load()
    ks = lmm_amd.SEKernel(lengthscale=np.array([1.0, 2.0])) + lmm_amd.RationalQuadraticKernel(alpha=1.5)
    gps = [lmm_amd.GP(lmm_amd.Matern52Kernel()).desc(), lmm_amd.GP(0.25, lmm_amd.KernelSum(*ks.kernels, variance=3.0)).desc()]
    arr = L.gps_array(gps)
    assert arr[0].kind == 2
    assert arr[1].kind & 0xFF == 5 and arr[1].kind >> 8 > 0
    assert arr[1].variance == 3.0 and arr[1].lengthscale == 1.0 and arr[1].mean == 0.25
    sum_tag = arr[1].kind >> 8
    terms = arr.ard.terms[1]
    assert terms is not None and terms.has_ard == [True, False] and terms.has_alpha == [False, True]
    term_tags = list(terms.tags)
    g = (L.GpGradT * 2)()
    assert lib.lmm_kernel_sum_grad(sum_tag, g) == L.LMM_OK
    arr.ard.close()
    assert lib.lmm_kernel_sum_grad(sum_tag, g) == L.LMM_ERR_ARG
    for t in term_tags:
        assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG               # already destroyed with the array's tags


def test_shim_sum_methods():
    src = open(SHIM).read()
    assert "lmm_kernel_sum_create" in src and "lmm_kernel_sum_grad" in src
    assert re.search(r"_desc\(k::KernelSum\)\s*=", src)
    assert re.search(r"_ktangent\(k::KernelSum", src)
    assert "Tangent{typeof(k)}(; kernels=" in src


def test_shim_ktangent_methods_take_the_term_gradients():
    """Every _ktangent method accepts the 6-argument form (…, ga, gα, gt) that _fstangent and the wrapper methods pass on: a method
    with fewer arguments would be skipped for the catch-all `_ktangent(k::Kernel, …) = NoTangent()` and lose its tangent silently."""
    src = open(SHIM).read()
    heads = re.findall(r"^(?:function\s+)?_ktangent\((k::.*?)\)(?:\s*=|\s*$)", src, flags=re.M)
    assert len(heads) >= 6
    for h in heads:
        parts, depth, cur = [], 0, ""
        for ch in h:                                   # split on the commas outside {}
            depth += (ch == "{") - (ch == "}")
            if ch == "," and depth == 0:
                parts.append(cur.strip()); cur = ""
            else:
                cur += ch
        parts.append(cur.strip())
        assert parts[1:] == ["gv", "gl", "ga=nothing", "gα=nothing", "gt=nothing"], parts
    # the wrappers pass gt on
    for kind in ("ScaledKernel", "ScaleTransform", "ARDTransform"):
        body = src[src.index("_ktangent(k::" + ("TransformedKernel{<:Kernel,<:" + kind + "}" if kind != "ScaledKernel" else kind)):]
        body = body[:body.index("\nend")]
        assert re.search(r"_ktangent\(k\.kernel,[^\n]*gt\)", body), kind
