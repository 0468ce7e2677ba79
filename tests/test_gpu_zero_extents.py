"""GPU checks of the zero extents (DESIGN.md 4.17 "Rows whose panel is exactly zero", csrc/lmm_emul.h): the Gram launch of a
per-latent logpdf keeps, per block of 64 rows, the number of leading columns it stored as +0, and the factorisation leaves out the
region row tasks, f64 update items and emulated tiles whose rows are zero across their whole panel.  None of that may show in a
result, and it must really happen:

(a) lmm_dev_train_gram (the training Gram launch, one matrix and a batch of two) returns the extents a NumPy pass over the matrix
    the same call wrote finds -- Matern12 / 32 / 52, SE, RQ; d = 1 and 2; variance 1 and 1e-300; 0, 1 and 24 rider rows; scalar noise
    and a noisevec; sorted, mostly sorted and permuted inputs -- and all zeros for a sum and a periodic latent;
(b) lmm_dev_potrf_zext with the true extents and with the true extents halved gives the factor, rider rows, inverse diagonal blocks,
    info word and failing pivot of lmm_dev_potrf, bit for bit, at n = 2304 + 64 riders and n = 1152, l / spacing 0.6 and 2.1 and a
    flat matrix, under the default plan, with the region kernel off, with 512-column regions, and with the emulation on from K = 256;
    the void counters equal the NumPy counts for the step shapes the library reports, are 0 for the flat matrix and positive for
    the decaying ones -- except n = 1152, l = 2.1 under the plans with region launches, where no item can be void and the NumPy count
    is 0 as well; a fifth plan, regions off and strict progress off, runs the builds with fused bulk rows;
(c) the five-latent logpdf of tests/test_gpu_f64_screen.py, its splits, two right-hand sides and a y with NaNs: `==` with the switch
    on and off, and void work in the batch that holds l = 0.02.

Switches that are read once from the environment go into a fresh child process per configuration
(`python tests/test_gpu_zero_extents.py child <configuration>`), which prints JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_zero_extents_host as ZH      # noqa: E402

pytestmark = pytest.mark.gpu

NONE = ZH.NONE
UPDATE_LEAF, EMUL_UPDATE_LEAF, REGION = 5, 6, 7      # PotrfStepKind (lmm_dev_potrf_plan)


def setup(lib):
    from lmm_amd import _lib as L
    lib.lmm_dev_set_zero_extents.argtypes = [C.c_int]
    lib.lmm_dev_set_zero_extents_min_cols.argtypes = [C.c_int]
    lib.lmm_dev_zero_extent_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_zero_extent_stats.restype = C.c_int
    lib.lmm_dev_potrf_zext.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.lmm_dev_train_gram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(L.GpT), C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.lmm_dev_set_deterministic.argtypes = [C.c_int]
    lib.lmm_dev_set_f64_emul.argtypes = [C.c_int, C.c_int, C.c_int]
    return lib


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = setup(lmm_amd.load())
    yield lmm_amd
    lib.lmm_dev_set_zero_extents(-1)
    lib.lmm_dev_set_zero_extents_min_cols(-1)
    lib.lmm_dev_zero_extent_stats(0, None, 0)
    lib.lmm_dev_set_deterministic(0)


def stats(lib):
    out = (C.c_int * (7 * 256))()
    n = lib.lmm_dev_zero_extent_stats(1, out, 256)
    assert 0 <= n <= 256
    return [list(out[7 * i:7 * i + 7]) for i in range(n)]


def expected_void(ext, NR, rec):
    """the NumPy count of one record of lmm_dev_zero_extent_stats (one matrix)"""
    kind, j0, h, N, M, _, word = rec
    if kind == REGION:
        return ZH.void_row_tasks(ext, NR, j0, N // 128, n128=word)[0]
    if kind == UPDATE_LEAF:
        rest, _, col0 = ZH.void_update_tiles(ext, NR, j0, h, N, strip=(word >> 1) != 0)
        return rest + (0 if word & 1 else col0)
    assert kind == EMUL_UPDATE_LEAF
    return ZH.void_emul_tiles(ext, j0, h, N, M)[0]


# ---- (a) extents from the Gram entry ----
N_GRAM = 1100      # not a multiple of 128: the last 52 columns are identity padding
KERNELS = {"matern12": 0.6, "matern32": 0.6, "matern52": 0.6, "se": 5.0, "rq": 0.6}      # lengthscale / spacing: zeros from 450, 260, 200 and 195 columns on; RQ has none


def gram_x(order, d):
    x = ZH.inputs(N_GRAM, order, 7)
    return x if d == 1 else np.ascontiguousarray(np.stack([x, 0.5 * x], axis=1))      # [n][d]


def train_gram(lmm, descs, x, d, nrider, noisevec, seed):
    """(matrices [nb][NR][NC] as the launch stored them (upper tiles of the buffer are zero), extents [nb][NR / 64])"""
    import torch
    from lmm_amd import _lib as L
    lib = lmm.load()
    nb, n = len(descs), N_GRAM
    NC = (n + 127) // 128 * 128
    NR = (NC + nrider + 63) // 64 * 64
    rng = np.random.default_rng(seed)
    A = torch.zeros(nb * NC * NR, dtype=torch.float64, device="cuda")
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    noise = np.full(nb, 0.1)
    nv = torch.from_numpy(0.05 + rng.random(nb * n)).cuda() if noisevec else None
    rid = torch.from_numpy(rng.standard_normal(nb * max(nrider, 1) * n)).cuda()
    ext = np.full(nb * (NR // 64), -7, dtype=np.int32)
    gps = L.gps_array(descs)
    torch.cuda.synchronize()
    rc = lib.lmm_dev_train_gram(C.c_void_p(A.data_ptr()), NR, NR, NC, C.c_void_p(xd.data_ptr()), d, n, gps, nb, C.c_void_p(noise.ctypes.data),
                                C.c_void_p(nv.data_ptr()) if noisevec else None, C.c_void_p(rid.data_ptr()) if nrider else None, nrider, C.c_void_p(ext.ctypes.data))
    assert rc == 0, lib.lmm_last_error_string()
    return A.cpu().numpy().reshape(nb, NC, NR).transpose(0, 2, 1), ext.reshape(nb, NR // 64).astype(np.int64)


@pytest.mark.parametrize("kind", list(KERNELS))
def test_gram_extents_equal_numpy(lmm, kind):
    case = 0
    for d in (1, 2):
        for order in ("sorted", "mostly_sorted", "permuted"):
            x = gram_x(order, d)
            for nb in (1, 2):
                nrider = (0, 1, 24)[case % 3]
                noisevec = case % 2 == 1
                case += 1
                descs = [{"kind": kind, "variance": v, "lengthscale": KERNELS[kind]} for v in ((1.0, 1e-300) if nb == 2 else ((1.0, 1e-300)[case % 2],))]
                A, ext = train_gram(lmm, descs, x, d, nrider, noisevec, case)
                for j in range(nb):
                    want = ZH.extents(A[j], A.shape[2])
                    assert np.array_equal(ext[j], want), (kind, d, order, nb, nrider, noisevec, j, ext[j], want)
                    void = int((want > 0).sum())
                    print(f"{kind}, d = {d}, {order}, batch of {nb}, {nrider} riders, noisevec {noisevec}, variance {descs[j]['variance']}: {void} of {want.size} row blocks have zeros")
                    if nrider:
                        assert want[A.shape[2] // 64] == 0                      # the rider block holds data from column 0 on
                    if order == "sorted" and kind != "rq":
                        assert void > 0
                    if kind == "rq" and descs[j]["variance"] == 1.0:
                        assert not want[:N_GRAM // 64].any()                    # RQ never reaches zero
    assert case == 12


@pytest.mark.parametrize("kind,scale", [("matern12", 1.0), ("matern32", np.sqrt(3.0)), ("matern52", np.sqrt(5.0))])
def test_separable_path_stores_zero_where_the_kernel_underflows(lmm, kind, scale):
    """Sorted d = 1 inputs take the separable form exp(-a |xi - xj|) = E_i F_j; its reference exponent is clamped to +-700, so far tiles
    take the direct form (|D| > 700) or are stored as zeros (|D| >= 830): every entry with a |xi - xj| >= 750 is +0, bit for bit, as
    exp_nonpos gives it, and nothing beyond 700 exceeds exp(-700) times the polynomial."""
    x = gram_x("sorted", 1)
    A, ext = train_gram(lmm, [{"kind": kind, "variance": 1.0, "lengthscale": 0.6}], x, 1, 0, False, 2)
    K = A[0][:N_GRAM, :N_GRAM]
    s = scale * np.abs(x[:, None] - x[None, :]) / 0.6
    low = np.tril(np.ones_like(s, dtype=bool))
    assert (s[low] >= 750.0).sum() > 10 ** 5
    assert not K.view(np.int64)[low & (s >= 750.0)].any()
    assert (np.abs(K[low & (s >= 700.0)]) <= np.exp(-700.0) * (1.0 + 800.0 + 800.0 ** 2 / 3.0)).all()
    near = low & (s <= 600.0)
    ref = {"matern12": 1.0, "matern32": 1.0 + s, "matern52": 1.0 + s + s * s / 3.0}[kind] * np.exp(-s) + 0.1 * np.eye(N_GRAM)
    assert np.allclose(K[near], ref[near], rtol=1e-12, atol=0.0)
    assert ext[0][N_GRAM // 64 - 1] > 0


def test_sum_and_periodic_latents_report_no_zeros(lmm):
    x = gram_x("sorted", 1)
    terms = [{"kind": "matern52", "lengthscale": 0.6}, {"kind": "se", "variance": 0.5, "lengthscale": 5.0}]
    for descs in ([{"kind": "sum", "terms": terms}], [{"kind": "sum", "terms": terms}] * 2, [{"kind": "periodic", "lengthscale": 3.0}],
                  [{"kind": "periodic", "lengthscale": 3.0}, {"kind": "periodic", "lengthscale": 5.0, "variance": 2.0}]):
        A, ext = train_gram(lmm, descs, x, 1, 1, False, 3)
        assert not ext.any(), (descs, ext)
        assert (ZH.extents(A[0], A.shape[2])[:-1] > 0).any() or descs[0]["kind"] == "periodic"      # the sum's matrix does hold zero tiles


def test_switch_off_keeps_no_extents(lmm):
    lib = lmm.load()
    try:
        assert lib.lmm_dev_set_zero_extents(0) == 0
        _, ext = train_gram(lmm, [{"kind": "matern52", "lengthscale": 0.6}], gram_x("sorted", 1), 1, 1, False, 1)
        assert (ext == -1).all()
    finally:
        lib.lmm_dev_set_zero_extents(-1)


# ---- (b) factorisations: the child ----
CONFIGS = {
    "default": ({}, False),
    "region_off": ({"LMM_REGION": "0"}, False),
    "region_512": ({"LMM_REGION": "512", "LMM_REGION_ALL": "1"}, False),      # region launches of at most 512 columns (P = 2, 3, 4) as the base case
    "emul_from_256": ({}, True),
    # strict progress off: the update launches carry the next panel's bulk rows (potrf_node_kernel<*, true>: column-0 items never leave)
    "region_off_fused": ({"LMM_REGION": "0", "LMM_STRICT_PROGRESS": "0"}, False),
}
FACT_SHAPES = ((2304, 64), (1152, 0))
MATRICES = ("l0.6", "l2.1", "flat")


def factor_inputs(n, riders, which):
    rng = np.random.default_rng(n + len(which))
    ell = {"l0.6": 0.6, "l2.1": 2.1, "flat": 50.0 * n}[which]
    return ZH.matern52(np.arange(n, dtype=np.float64), ell) + 0.1 * np.eye(n), rng.standard_normal((riders, n))


def potrf(lmm_amd, Kmat, R, ext):
    import torch
    lib = lmm_amd.load()
    n, nr = Kmat.shape[0], Kmat.shape[0] + R.shape[0]
    full = np.vstack([np.tril(Kmat), R])
    A = torch.from_numpy(np.ascontiguousarray(full.T)).cuda()
    W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    zx = None if ext is None else torch.from_numpy(ext.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_potrf_zext(C.c_void_p(A.data_ptr()), nr, n, nr, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr()), None if zx is None else C.c_void_p(zx.data_ptr()))
    assert rc == 0, lib.lmm_last_error_string()
    return A.cpu().numpy().T, W.cpu().numpy(), int(info.item())


def child(config):
    sys.path.insert(0, ROOT)
    import lmm_amd
    lmm_amd.init(0)
    lib = setup(lmm_amd.load())
    assert lib.lmm_dev_set_deterministic(1) == 0
    if CONFIGS[config][1]:
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
    assert lib.lmm_dev_zero_extent_stats(1, None, 0) >= 0
    res = {}
    for n, riders in FACT_SHAPES:
        for which in MATRICES:
            Kmat, R = factor_inputs(n, riders, which)
            NR = n + riders
            tri = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((riders, n), dtype=bool)])
            bad_at = n - 52
            Kbad = Kmat.copy()
            Kbad[bad_at, bad_at] = -5.0
            true = ZH.extents(np.vstack([np.tril(Kmat), R]), n)
            exts = {"none": None, "true": true, "half": np.where(true == NONE, NONE, true // 128 * 64)}
            got, counts = {}, {}
            for name, ext in exts.items():
                F, W, info = potrf(lmm_amd, Kmat, R, ext)
                st = stats(lib)
                _, _, pivot = potrf(lmm_amd, Kbad, R, None if ext is None else ZH.extents(np.vstack([np.tril(Kbad), R]), n) if name == "true" else ext)
                got[name] = (F, W, info, pivot)
                counts[name] = [[r, expected_void(ext, NR, r)] for r in st] if ext is not None else st
            same = lambda a, b: bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
            L = np.linalg.cholesky(Kmat)
            res[f"{n}_{which}"] = {
                "factor_equal": [same(got[k][0][tri], got["none"][0][tri]) for k in ("true", "half")],
                "inverse_equal": [same(got[k][1], got["none"][1]) for k in ("true", "half")],
                "info": [got[k][2] for k in exts], "pivots": [got[k][3] for k in exts], "bad_at": bad_at,
                "counts_none": counts["none"], "counts_true": counts["true"], "counts_half": counts["half"],
                "void_blocks": int((true[:n // 64] > 0).sum()),
                "err": float(np.linalg.norm((got["true"][0][:n] - L)[tri[:n]]) / np.linalg.norm(L)),
            }
    print(json.dumps(res))


_FOUND = {}


def found(config):
    if config not in _FOUND:
        env = dict(os.environ, LMM_DETERMINISTIC="1", **CONFIGS[config][0])
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", config], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        _FOUND[config] = json.loads(out.stdout.strip().splitlines()[-1])
    return _FOUND[config]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("n,riders", FACT_SHAPES)
@pytest.mark.parametrize("which", MATRICES)
def test_factorisation_same_with_and_without_extents(config, n, riders, which):
    r = found(config)[f"{n}_{which}"]
    for name in ("counts_true", "counts_half"):
        print(f"{config}, n = {n} + {riders}, {which}, {name}: (kind, j0, h, N, M, void, shape word) -> NumPy {r[name]}")
    assert r["factor_equal"] == [True, True] and r["inverse_equal"] == [True, True]
    assert r["info"] == [0, 0, 0] and r["pivots"] == [r["bad_at"] + 1] * 3
    assert r["err"] <= 1e-9                                               # the bar of the other factorisation tests against LAPACK
    assert r["counts_none"] == []                                         # no extents: no record, nothing counted
    for name in ("counts_true", "counts_half"):
        assert len(r[name]) >= 1
        for rec, want in r[name]:
            assert rec[5] == want, (name, rec, want)                      # the device left out what the arithmetic says
    total = sum(rec[5] for rec, _ in r["counts_true"])
    kinds = {rec[0] for rec, _ in r["counts_true"]}
    if config == "default":
        assert REGION in kinds
    if config in ("region_off", "region_off_fused"):
        assert kinds == {UPDATE_LEAF}
        assert any(rec[6] & 1 for rec, _ in r["counts_true"]) == (config == "region_off_fused")      # fused bulk rows in that plan only
    if config == "region_512":
        assert {rec[2] for rec, _ in r["counts_true"] if rec[0] == REGION} == {256, 384, 512}
    if config == "emul_from_256" and n == 2304:
        assert EMUL_UPDATE_LEAF in kinds
    if which == "flat":
        assert r["void_blocks"] == 0 and total == 0
    else:
        assert r["void_blocks"] > 0
        # One case has no item that CAN be void: at n = 1152 and l = 2.1 the extents reach 448 columns, and with region launches the
        # only panels that end below that lie inside the first launch, whose row tasks need 512 or 640.  The count is then 0 on the
        # device as in NumPy (asserted above); every other decaying case must leave work out.
        if not (n == 1152 and which == "l2.1" and config in ("default", "emul_from_256", "region_512")):
            assert total > 0
        assert sum(rec[5] for rec, _ in r["counts_half"]) <= total


# ---- (c) five latents, lengthscales 0.02 .. 200 ----
ELLS = (200.0, 0.02, 0.5, 0.2, 0.7)


@pytest.mark.parametrize("case", ["vector", "two_rhs", "nan"])
def test_logpdf_same_with_extents_on_and_off(lmm, case):
    import torch
    lib = lmm.load()
    n = 1152
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    xt = torch.from_numpy(x).cuda()
    try:
        assert lib.lmm_dev_set_deterministic(1) == 0
        assert lib.lmm_dev_zero_extent_stats(1, None, 0) >= 0
        assert lib.lmm_dev_set_zero_extents_min_cols(0) == 0              # the size gate (2048 columns by default) would keep no extents at n = 1152
        for group in ((0, 1, 2, 3, 4), (0, 1), (2, 3), (4,)) if case == "vector" else ((0, 1, 2, 3, 4),):
            m = len(group)
            p = m + 3 if case == "nan" else m                             # missing data needs at least m observed outputs per point
            U = np.linalg.qr(np.random.default_rng(9).standard_normal((p, m)))[0] if case == "nan" else np.eye(m)
            y = np.random.default_rng(m).standard_normal(n * p)
            if case == "two_rhs":
                y = np.stack([y, np.random.default_rng(m + 10).standard_normal(n * p)], axis=1)
            if case == "nan":
                y[::37] = np.nan                                          # n = 31 x 37 + 5: at most one missing output per point
            yt = torch.from_numpy(y).cuda()
            fs = lmm.independent_mogp([lmm.GP(0.0, lmm.Matern52Kernel(1.0, ELLS[k])) for k in group])
            fx = lmm.ILMM(fs, lmm.Orthogonal(U, 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(xt, p), 0.1)
            vals = {}
            for on in (1, 0):
                assert lib.lmm_dev_set_zero_extents(on) == 0
                vals[on] = np.asarray(lmm.logpdf(fx, yt), dtype=np.float64)
                st = stats(lib)
                if on:
                    print(f"{case}, latents {group}: (kind, j0, h, N, M, void, shape word) {st}")
                    assert len(st) >= 1
                    if 1 in group:
                        assert sum(s[5] for s in st) > 0                  # l = 0.02: rows that are zero across whole panels
                else:
                    assert st == []
            assert np.isfinite(vals[1]).all() and np.array_equal(vals[1], vals[0]), (case, group, vals)
    finally:
        lib.lmm_dev_set_zero_extents(-1)
        lib.lmm_dev_set_zero_extents_min_cols(-1)
        lib.lmm_dev_set_deterministic(0)
        lib.lmm_dev_zero_extent_stats(0, None, 0)


def test_size_gate_keeps_no_extents_at_1152(lmm):
    """By default a per-latent logpdf keeps extents only above 2048 columns (LMM_ZERO_EXTENTS_MINCOLS): at n = 1152 no step reports."""
    import torch
    lib = lmm.load()
    n = 1152
    xt = torch.from_numpy(np.sort(np.random.default_rng(5).uniform(0.0, 40.0, n))).cuda()
    yt = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
    fx = lmm.ILMM(lmm.independent_mogp([lmm.GP(0.0, lmm.Matern52Kernel(1.0, 0.02))]), lmm.Orthogonal(np.eye(1), np.ones(1)))(lmm.MOInputIsotopicByOutputs(xt, 1), 0.1)
    try:
        assert lib.lmm_dev_zero_extent_stats(1, None, 0) >= 0
        vals = []
        for cols in (-1, 0):
            assert lib.lmm_dev_set_zero_extents_min_cols(cols) == 0
            vals.append(float(lmm.logpdf(fx, yt)))
            st = stats(lib)
            assert (st == []) == (cols < 0), (cols, st)
        assert vals[0] == vals[1]
    finally:
        lib.lmm_dev_set_zero_extents_min_cols(-1)
        lib.lmm_dev_zero_extent_stats(0, None, 0)


if __name__ == "__main__":
    child(sys.argv[2])
