"""Host-only checks of inducing-point (VFE) inference (include/lmm_hip.h "inducing points"): the entry points are declared, exported
and bound with matching arity, VFE validates its arguments, every refusal of the Python mirror comes before any library call, and the
two NumPy restatements of tests/test_gpu_sparse.py (the dense formula and the library's low-rank algebra) agree on the GPU test cases:
their disagreement delta is what fixes the GPU tolerances, max(1e-10, 100 delta).  No GPU and no lmm_init needed."""
import os
import re

import numpy as np
import pytest

import lmm_amd
from lmm_amd import _lib as L

import test_gpu_sparse as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SYMS = ("lmm_oilmm_elbo", "lmm_oilmm_sparse_posterior_create", "lmm_sparse_post_destroy", "lmm_oilmm_sparse_mean_and_var",
        "lmm_dev_sparse_moments")


def test_sparse_symbols_declared_exported_and_bound():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert proto, s
        params = [a.strip() for a in proto.group(1).split(",")]
        types = L.SPARSE_ARGTYPES[s]
        assert len(params) == len(types), (s, len(params), len(types))
        assert getattr(lib, s).argtypes == types
        for a, t in zip(params, types):            # int <-> c_int, double <-> c_double, anything with * or [] <-> c_void_p
            want = L._P if ("*" in a or "[" in a) else (L._D if a.startswith("double") else L._I)
            assert t is want, (s, a)
    proto = re.search(r"int\s+lmm_oilmm_elbo\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "d", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "z", "nz", "jitter",
                     "with_regulariser", "elbo", "dtc"]


def test_vfe_validates_its_arguments():
    with pytest.raises(ValueError, match="non-empty"):
        lmm_amd.VFE(np.zeros(0))
    with pytest.raises(ValueError, match="non-empty"):
        lmm_amd.VFE(np.zeros((2, 0)))
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="jitter"):
            lmm_amd.VFE(np.arange(3.0), bad)
    v = lmm_amd.VFE(np.zeros((2, 7)))
    assert (v.dim, v.nz, v.jitter) == (2, 7, 1e-6)
    assert lmm_amd.VFE([0.0, 1.0]).dim == 1
    # wrong d: checked against the model's inputs, before the library is touched
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.SEKernel())])
    oilmm = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0])))
    fx = oilmm(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2), 0.1)
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        for fn in (lmm_amd.elbo, lmm_amd.dtc, lmm_amd.approx_posterior):
            with pytest.raises(ValueError, match="d = 2"):
                fn(v, fx, np.zeros(8))
    finally:
        L.ensure_init = saved


def _no_library():
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.SEKernel())])
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2)
    H = lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0]))
    y = np.zeros(8)
    vfe = lmm_amd.VFE(np.arange(3.0))
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    sharded = lmm_amd.ILMM(fs, H, shard=(0, 0))(x, 0.1)
    M = lmm_amd.model
    post = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._PostHandle(None, 0, 1)), H)(x, 0.1)
    sparse = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._SparsePostHandle(None, 0, 1)), H)(x, 0.1)
    ynan = y.copy()
    ynan[3] = np.nan
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        for fn in (lmm_amd.elbo, lmm_amd.dtc, lmm_amd.approx_posterior):
            for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                                 (sparse, y, "posterior model"), (oilmm, np.zeros((8, 2)), "matrix Y"), (oilmm, ynan, "NaN"),
                                 (sharded, y, "sharded")):
                with pytest.raises(NotImplementedError, match=what):
                    fn(vfe, fx, yy)
        rng = np.random.default_rng(0)
        for call in (lambda: lmm_amd.rand(rng, sparse), lambda: lmm_amd.mean_and_cov(sparse), lambda: lmm_amd.cov(sparse),
                     lambda: lmm_amd.logpdf(sparse, y), lambda: lmm_amd.logpdf_and_gradient(sparse, y),
                     lambda: lmm_amd.mean_and_var_vjp(sparse, dmean=y), lambda: lmm_amd.posterior(sparse, y),
                     # the latent model of a sparse posterior handed to cov as it is: its handle is no lmm_post_t*
                     lambda: lmm_amd.cov(lmm_amd.get_latent_gp(sparse.f), x), lambda: lmm_amd.cov(lmm_amd.get_latent_gp(sparse.f), x, x),
                     lambda: lmm_amd.cov(sparse.f)):
            with pytest.raises(NotImplementedError, match="inducing-point posterior"):
                call()
    finally:
        L.ensure_init = saved
    assert lmm_amd.posterior.__code__.co_argcount == 2          # posterior keeps its two-argument signature


@pytest.mark.parametrize("n,M", G.ELBO_SHAPES + [(96, 96)])
def test_lowrank_restatement_agrees_with_dense(n, M):
    P, ref = G.reference(n, M)
    for wr in (True, False):
        (de, dt), (le, lt) = ref[wr]
        assert G.rel(le, de) <= 1e-9 and G.rel(lt, dt) <= 1e-9, (n, M, wr)
        assert le <= lt * (1 - 1e-12) if lt < 0 else le <= lt * (1 + 1e-12)
    if (n, M) == (96, 96):
        ex = G.model_values(P, G.dense_latent, True, exact=True)[1]
        assert G.rel(ref[True][0][0], ex) <= 1e-9 and G.rel(ref[True][0][1], ex) <= 1e-9


@pytest.mark.parametrize("ns", G.NSTAR)
def test_lowrank_predictions_agree_with_dense(ns):
    P, _ = G.reference(333, 70)
    xs = np.linspace(-0.5, 10.5, ns) + 0.013
    (rm, rv), (lm, lv) = G.predict(P, xs, True, False), G.predict(P, xs, True, True)
    assert np.abs(lm - rm).max() <= 1e-9 * np.abs(rm).max() and np.abs(lv - rv).max() <= 1e-9 * np.abs(rv).max()
    assert (rv > 0).all()


@pytest.mark.parametrize("d", [1, 2, 3])
def test_moment_cases_are_well_posed(d):
    for n, M in G.MOMENT_SHAPES:
        k, x, z, w, r = G.moment_problem(n, M, d)
        Phi, b, s, kap, lam = G.moments_ref(k, x, z, w, r)
        assert Phi.shape == (M, M) and np.isfinite(Phi).all() and np.abs(Phi).max() > 0 and np.isfinite(b).all()
        assert n == 1 or w.min() < 0.9 * w.max()            # w is non-constant
        assert s > 0 and kap > 0 and lam < 0
