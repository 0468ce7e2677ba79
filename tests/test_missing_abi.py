"""Host-only checks of missing observations (NaN in y; include/lmm_hip.h "missing observations"): the five entry points are
declared and exported, lmm_missing_patterns groups host data by mask and gives the p_t < m refusals, and the Python mirror's
dropping of points without any observation is a pure function of its arrays.  No GPU and no lmm_init needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lmm_amd
from lmm_amd import _lib as L
from lmm_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SYMS = ("lmm_missing_patterns", "lmm_oilmm_project_missing", "lmm_oilmm_logpdf_missing", "lmm_oilmm_posterior_create_missing",
        "lmm_oilmm_logpdf_grad_missing")


def patterns(y_np, m):
    """y_np: (p, n) host array (row o = output o: the by-outputs vector reshaped).  Returns (rc, pattern_of_point, npatterns, n_observed)."""
    lib = lmm_amd.load()
    p, n = y_np.shape
    y = np.ascontiguousarray(y_np, dtype=np.float64)
    pat, npat, nobs = (C.c_int * n)(), C.c_int(-1), C.c_int(-1)
    rc = lib.lmm_missing_patterns(y.ctypes.data_as(C.c_void_p), n, p, m, pat, C.byref(npat), C.byref(nobs))
    return rc, list(pat), npat.value, nobs.value


def detail():
    lat, info = C.c_int(), C.c_int()
    lmm_amd.load().lmm_last_error_detail(C.byref(lat), C.byref(info))
    return lat.value, info.value


def test_missing_symbols_declared_and_exported():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
    # the gradient entry point has no grad_S / grad_U / grad_x arguments
    proto = re.search(r"int\s+lmm_oilmm_logpdf_grad_missing\s*\(([^)]*)\)", src).group(1)
    assert "grad_y" in proto and "grad_sigma2" in proto and "grad_gps" in proto
    assert "grad_S" not in proto and "grad_U" not in proto and "grad_x" not in proto


def test_no_nan_is_one_pattern():
    y = np.random.default_rng(0).normal(size=(5, 9))
    rc, pat, npat, nobs = patterns(y, 3)
    assert rc == L.LMM_OK and npat == 1 and pat == [0] * 9 and nobs == 45


def test_equal_masks_share_a_pattern():
    y = np.random.default_rng(1).normal(size=(5, 6))
    y[1, 2] = np.nan
    y[4, 3] = np.nan
    y[1, 5] = np.nan           # the mask of point 2
    rc, pat, npat, nobs = patterns(y, 3)
    assert rc == L.LMM_OK and npat == 3
    assert pat == [0, 0, 1, 2, 0, 1]          # numbered by first appearance
    assert nobs == 30 - 3


def test_distinct_masks_give_n_patterns():
    n, p = 8, 8
    y = np.random.default_rng(2).normal(size=(p, n))
    for t in range(n):
        y[t, t] = np.nan
    rc, pat, npat, nobs = patterns(y, 3)
    assert rc == L.LMM_OK and npat == n and pat == list(range(n)) and nobs == n * p - n


def test_two_mask_words():
    """p = 70: outputs 64.. live in the second mask word; a NaN there must be seen, and must differ from the same bit of word 0."""
    y = np.random.default_rng(3).normal(size=(70, 5))
    y[64, 1] = np.nan
    y[69, 2] = np.nan
    y[0, 3] = np.nan           # bit 0 of word 0, against bit 0 of word 1 at point 1
    y[64, 4] = np.nan
    rc, pat, npat, nobs = patterns(y, 4)
    assert rc == L.LMM_OK and npat == 4 and pat == [0, 1, 2, 3, 1] and nobs == 350 - 4


def test_too_few_observations_are_refused_with_the_point_index():
    y = np.random.default_rng(4).normal(size=(5, 7))
    y[:3, 4] = np.nan          # p_t = 2 = m - 1 at point 4
    rc, _, _, _ = patterns(y, 3)
    assert rc == L.LMM_ERR_UNSUPPORTED and detail()[1] == 4
    assert b"point 4" in lmm_amd.load().lmm_last_error_string()
    y = np.random.default_rng(5).normal(size=(5, 7))
    y[:, 6] = np.nan           # p_t = 0 at point 6
    y[0, 2] = np.nan           # fine: 4 >= m
    rc, _, _, _ = patterns(y, 3)
    assert rc == L.LMM_ERR_UNSUPPORTED and detail()[1] == 6
    # exactly m observed is served
    y = np.random.default_rng(6).normal(size=(5, 7))
    y[:2, 1] = np.nan
    assert patterns(y, 3)[0] == L.LMM_OK


def test_infinities_are_data():
    y = np.random.default_rng(7).normal(size=(4, 5))
    y[0, 1], y[3, 2] = np.inf, -np.inf
    rc, pat, npat, nobs = patterns(y, 2)
    assert rc == L.LMM_OK and npat == 1 and nobs == 20


def test_bad_arguments():
    lib = lmm_amd.load()
    assert lib.lmm_missing_patterns(None, 3, 2, 1, None, None, None) == L.LMM_ERR_ARG
    y = np.zeros(6)
    assert lib.lmm_missing_patterns(y.ctypes.data_as(C.c_void_p), 0, 2, 1, None, None, None) == L.LMM_ERR_ARG
    assert lib.lmm_missing_patterns(y.ctypes.data_as(C.c_void_p), 3, 2, 1, None, None, None) == L.LMM_OK      # outputs are optional


def test_mirror_drops_points_without_observations():
    p, n = 3, 6
    rng = np.random.default_rng(8)
    Y = rng.normal(size=(p, n))
    Y[:, 1] = np.nan
    Y[:, 4] = np.nan
    Y[0, 2] = np.nan           # partly observed: kept
    x1 = np.arange(n, dtype=np.float64)
    xo, yo, keep = M._drop_unobserved(x1, Y.reshape(-1), p)
    assert keep.tolist() == [True, False, True, True, False, True]
    np.testing.assert_array_equal(xo, x1[[0, 2, 3, 5]])
    np.testing.assert_array_equal(yo.reshape(p, -1), Y[:, [0, 2, 3, 5]])
    assert yo.flags.c_contiguous and np.isnan(yo).sum() == 1
    x2 = rng.normal(size=(2, n))                       # (d, n) inputs: columns are dropped
    xo, _, _ = M._drop_unobserved(x2, Y.reshape(-1), p)
    np.testing.assert_array_equal(xo, x2[:, [0, 2, 3, 5]])
    # nothing to drop: the arrays come back as they are
    Y2 = rng.normal(size=(p, n))
    Y2[1, 3] = np.nan
    y2 = Y2.reshape(-1)
    xo, yo, keep = M._drop_unobserved(x1, y2, p)
    assert xo is x1 and yo is y2 and keep.all()


def test_mirror_drops_points_on_torch_tensors():
    torch = pytest.importorskip("torch")
    p, n = 2, 4
    Y = torch.arange(8, dtype=torch.float64).reshape(p, n).clone()
    Y[:, 2] = float("nan")
    x = np.arange(n, dtype=np.float64)                 # host inputs next to a tensor y
    xo, yo, keep = M._drop_unobserved(x, Y.reshape(-1), p)
    assert keep.tolist() == [True, True, False, True]
    np.testing.assert_array_equal(xo, [0.0, 1.0, 3.0])
    assert yo.is_contiguous() and yo.tolist() == [0.0, 1.0, 3.0, 4.0, 5.0, 7.0]


def test_mirror_refuses_missing_data_where_it_is_not_served():
    """Everything but a vector y on a prior OILMM raises NotImplementedError before any device work (no GPU needed)."""
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.SEKernel())])
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2)
    y = np.zeros(8)
    y[3] = np.nan
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    oilmm = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0])))(x, 0.1)
    Ymat = np.zeros((8, 2))
    Ymat[0, 0] = np.nan
    saved = L.ensure_init
    L.ensure_init = lambda: None                       # the refusals come before the library is touched
    try:
        for fn in (lmm_amd.logpdf, lmm_amd.posterior, lmm_amd.logpdf_and_gradient):
            with pytest.raises(NotImplementedError, match="do not take missing data"):
                fn(dense, y)
            with pytest.raises(NotImplementedError, match="do not take missing data"):
                fn(mogp, y[:4])
        with pytest.raises(NotImplementedError, match="do not take missing data"):
            lmm_amd.logpdf(oilmm, Ymat)
        with pytest.raises(NotImplementedError, match="inputs"):
            lmm_amd.logpdf_and_gradient(oilmm, y, inputs=True)
    finally:
        L.ensure_init = saved
