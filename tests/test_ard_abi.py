"""Host-only checks of the per-dimension (ARD) lengthscale registry (include/lmm_hip.h lmm_ard_*) and of the Python mirror's vector
lengthscales: no GPU and no lmm_init needed."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import lmm_amd
from lmm_amd import _lib as L

DP = C.POINTER(C.c_double)


def _create(lib, ls):
    a = np.ascontiguousarray(ls, dtype=np.float64)
    t = C.c_int(0)
    rc = lib.lmm_ard_create(int(a.size), a.ctypes.data_as(DP), C.byref(t))
    return rc, t.value


def test_ard_symbols_exported():
    lib = lmm_amd.load()
    for s in ("lmm_ard_create", "lmm_ard_destroy", "lmm_ard_grad"):
        assert hasattr(lib, s) and s in L.SYMBOLS


def test_ard_create_destroy_grad_roundtrip():
    lib = lmm_amd.load()
    rc, tag = _create(lib, [0.5, 2.0, 1.5])
    assert rc == L.LMM_OK and tag > 0
    out = np.full(3, np.nan)
    assert lib.lmm_ard_grad(tag, out.ctypes.data_as(DP)) == L.LMM_OK
    assert np.array_equal(out, np.zeros(3))                     # no gradient call has named the tag yet
    rc2, tag2 = _create(lib, [1.0])
    assert rc2 == L.LMM_OK and tag2 > 0 and tag2 != tag
    assert lib.lmm_ard_destroy(tag) == L.LMM_OK
    assert lib.lmm_ard_destroy(tag2) == L.LMM_OK
    assert lib.lmm_ard_destroy(tag) == L.LMM_ERR_ARG            # already destroyed
    assert lib.lmm_ard_grad(tag, out.ctypes.data_as(DP)) == L.LMM_ERR_ARG


@pytest.mark.parametrize("ls", [[], [1.0, 0.0], [1.0, -2.0], [math.nan, 1.0], [1.0, math.inf]])
def test_ard_create_rejects_bad_lengthscales(ls):
    lib = lmm_amd.load()
    rc, tag = _create(lib, ls)           # [] -> d = 0
    assert rc == L.LMM_ERR_ARG and tag == 0


def test_ard_create_rejects_null_arguments():
    lib = lmm_amd.load()
    t = C.c_int(0)
    assert lib.lmm_ard_create(2, None, C.byref(t)) == L.LMM_ERR_ARG
    a = np.ones(2)
    assert lib.lmm_ard_create(2, a.ctypes.data_as(DP), None) == L.LMM_ERR_ARG
    assert lib.lmm_ard_create(-1, a.ctypes.data_as(DP), C.byref(t)) == L.LMM_ERR_ARG
    assert lib.lmm_ard_grad(1, None) == L.LMM_ERR_ARG


def test_ard_destroy_unknown_tag():
    lib = lmm_amd.load()
    for t in (0, -3, 1 << 22):
        assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG


def test_ard_live_tag_bound():
    lib = lmm_amd.load()
    tags = []
    try:
        while True:
            rc, t = _create(lib, [1.0, 2.0])
            if rc != L.LMM_OK:
                break
            tags.append(t)
            assert len(tags) <= 4096
        assert rc == L.LMM_ERR_UNSUPPORTED
        assert len(tags) >= 4000                # the bound is 4096 live tags (a few may be held elsewhere in this process)
        assert len(set(tags)) == len(tags) and all(0 < t < (1 << 23) for t in tags)
        assert lib.lmm_ard_destroy(tags.pop()) == L.LMM_OK
        rc, t = _create(lib, [1.0])             # room again after a destroy
        assert rc == L.LMM_OK
        tags.append(t)
    finally:
        for t in tags:
            lib.lmm_ard_destroy(t)


def test_python_kernels_accept_vector_lengthscales():
    k = lmm_amd.Matern52Kernel(1.3, [0.5, 2.0])
    assert isinstance(k.lengthscale, np.ndarray) and k.lengthscale.tolist() == [0.5, 2.0]
    assert k == lmm_amd.Matern52Kernel(1.3, np.array([0.5, 2.0]))
    assert k != lmm_amd.Matern52Kernel(1.3, [0.5, 2.5])
    assert k != lmm_amd.Matern32Kernel(1.3, [0.5, 2.0])
    assert k != lmm_amd.Matern52Kernel(1.3, 0.5)
    assert "[0.5, 2.0]" in repr(k)
    iso = lmm_amd.SEKernel(1.0, 0.7)
    assert isinstance(iso.lengthscale, float) and repr(iso) == "SEKernel(variance=1.0, lengthscale=0.7)"


def test_gps_array_encodes_tags_and_releases_them():
    lib = lmm_amd.load()
    descs = [{"kind": "matern32", "variance": 1.1, "lengthscale": [0.5, 2.0, 1.0], "mean": 0.2},
             {"kind": "se", "variance": 0.9, "lengthscale": 0.8, "mean": 0.0},
             {"kind": "matern52", "variance": 1.0, "lengthscale": np.array([3.0, 3.0, 3.0]), "mean": 0.0}]
    arr = L.gps_array(descs)
    tags = [arr[l].kind >> 8 for l in range(3)]
    assert arr[0].kind & L.KERNEL_BASE_MASK == L.KERNEL_KINDS["matern32"] and tags[0] > 0 and arr[0].lengthscale == 1.0
    assert arr[1].kind == L.KERNEL_KINDS["se"] and tags[1] == 0 and arr[1].lengthscale == 0.8
    assert arr[2].kind & L.KERNEL_BASE_MASK == L.KERNEL_KINDS["matern52"] and tags[2] > 0 and tags[2] != tags[0]
    assert arr.ard.tags == tags
    out = np.empty(3)
    for t in (tags[0], tags[2]):
        assert lib.lmm_ard_grad(t, out.ctypes.data_as(DP)) == L.LMM_OK      # live while the array is
    del arr
    gc.collect()
    for t in (tags[0], tags[2]):
        assert lib.lmm_ard_destroy(t) == L.LMM_ERR_ARG                       # gone with it
