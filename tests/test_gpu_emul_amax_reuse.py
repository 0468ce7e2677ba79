"""GPU check of the row maxima kept across the emulated updates of a factorisation (emul_amax_cover): an update
reads the maxima of the part of its panel that earlier emulated updates scanned from their kept arrays and scans only the rest.
lmm_dev_set_emul_amax_reuse(0) makes every update scan its whole panel, so the two paths are compared within one build: the factor
must be the same in every bit.

Three nested levels are emulated at small n with lmm_dev_set_f64_emul(1, 128, 16) and the region kernel off (LMM_REGION=0: it would
take a matrix of at most 1024 columns in one launch).  The switches are read once per process, so the GPU work runs in ONE child
process (`python tests/test_gpu_emul_amax_reuse.py child`) that prints its findings as JSON; the tests below read them.

* n = 1024 (+ 64 rider rows): 512 | 512, 256 | 256, 128 | 128 -- the K = 512 update takes [0, 256) from the K = 256 update's array,
  [256, 384) from the K = 128 update at column 256 and scans [384, 512).
* n = 1152 (+ 64): 640 | 512, 384 | 256, 256 | 128 -- uneven halves: the K = 640 update takes [0, 384) and [384, 512) and scans
  [512, 640).
* The matrices carry one large coupling per row below the top update, placed by column range, so that the row maximum of the top
  panel lies in each of the three sources for about a third of the rows: checked on the LAPACK factor before anything is trusted.
* A matrix that is not positive definite in its second half reports the same pivot on both paths.
* Five matrices walked in groups of 2 + 2 + 1 read the kept arrays at group offsets other than 0."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER, STEP, CAP = 8, 14, 1024
EMUL_UPDATE_LEAF = 6
SHAPES = {"even": (1088, 1024), "uneven": (1216, 1152)}
CHAINS = {"even": (512, [(0, 256), (256, 384)], 384), "uneven": (640, [(0, 384), (384, 512)], 512)}      # top K, kept column ranges, first scanned column


# ---- the child: everything that touches the GPU ----
def emulated_steps(lib, NR, NC):
    out = (C.c_longlong * (HEADER + STEP * CAP))()
    lib.lmm_dev_potrf_plan.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    n = lib.lmm_dev_potrf_plan(NR, NC, 1, -1, 1, 256, 0, 1, out, CAP)
    assert 0 < n <= CAP, lib.lmm_last_error_string()
    rows = [out[HEADER + STEP * i: HEADER + STEP * (i + 1)] for i in range(n)]
    return [(r[1], r[2]) for r in rows if r[0] == EMUL_UPDATE_LEAF]      # (j0, h) in launch order


def cover(steps, si):
    """emul_amax_cover in Python: kept (j0, h) ranges of steps before si that cover a prefix of step si's panel, and where the scan begins"""
    j0, h = steps[si]
    at, kept = j0, []
    while True:
        cand = [(hh, jj) for jj, hh in steps[:si] if jj == at and jj + hh <= j0 + h]
        if not cand:
            return kept, at
        hh, jj = max(cand)
        kept.append((jj, jj + hh))
        at += hh


def coupled_matrix(NR, NC, top_h, ranges, seed, bad=None):
    """lower triangle + rider rows of an SPD matrix: G G' / (n + 8) + 2 I (off-diagonal entries ~ 0.03) plus one coupling of 0.4 per row
    below the top update, in the column range its row number picks (at most two per column: the couplings' norm is at most 0.8 < 2)"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((NC, NC + 8))
    K = G @ G.T / (NC + 8) + 2.0 * np.eye(NC)
    R = 0.03 * rng.standard_normal((NR - NC, NC))
    for i in range(top_h, NR):
        lo, hi = ranges[i % 3]
        c = lo + (i // 3) % (hi - lo)
        if i < NC:
            K[i, c] += 0.4
            K[c, i] += 0.4
        else:
            R[i - NC, c] += 0.4
    if bad is not None:
        K[bad, bad] = -5.0
    full = np.zeros((NR, NC))
    full[:NC] = np.tril(K)
    full[NC:] = R
    return K, R, full


def potrf(lmm, full, reuse):
    import torch
    lib = lmm.load()
    NR, NC = full.shape
    ld = NR + 16
    Ah = np.full((NC, ld), np.nan)
    Ah[:, :NR] = full.T
    iu = np.triu_indices(NC, 1)
    Ah[iu[1], iu[0]] = np.nan                                         # the never-read upper triangle
    A = torch.from_numpy(Ah).cuda()
    W = torch.zeros(NC // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.lmm_dev_set_emul_amax_reuse(reuse) == 0
    try:
        rc = lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), NR, NC, ld, C.c_void_p(W.data_ptr()), NC, C.c_void_p(info.data_ptr()))
    finally:
        lib.lmm_dev_set_emul_amax_reuse(1)
    assert rc == 0, lib.lmm_last_error_string()
    return A.cpu().numpy(), W.cpu().numpy(), int(info.item())


def child():
    import scipy.linalg as sla
    import torch
    sys.path.insert(0, ROOT)
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_emul_amax_reuse.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    assert lib.lmm_dev_set_f64_emul(1, 128, 16) == 0
    res = {}
    for name, (NR, NC) in SHAPES.items():
        steps = emulated_steps(lib, NR, NC)
        top = max(range(len(steps)), key=lambda i: (steps[i][0] == 0, steps[i][1]))
        kept, scan0 = cover(steps, top)
        top_h = steps[top][1]
        ranges = kept + [(scan0, top_h)]
        r = {"steps": steps, "top_h": top_h, "kept": kept, "scan0": scan0}
        if len(ranges) == 3:
            K, R, full = coupled_matrix(NR, NC, top_h, ranges, NR)
            L = np.linalg.cholesky(K)
            X = sla.solve_triangular(L, R.T, lower=True).T            # R L^-T
            panel = np.abs(np.vstack([L[top_h:], X])[:, :top_h])
            where = panel.argmax(axis=1)
            r["share"] = [float(np.mean((where >= lo) & (where < hi))) for lo, hi in ranges]
            on, Won, info_on = potrf(lmm_amd, full, 1)
            off, Woff, info_off = potrf(lmm_amd, full, 0)
            r["info"] = [info_on, info_off]
            r["factor_bits_equal"] = bool(np.array_equal(on.view(np.int64), off.view(np.int64)) and np.array_equal(Won.view(np.int64), Woff.view(np.int64)))
            got = on.T[:NR]
            il = np.tril_indices(NC)
            r["err_L"] = float(np.abs(got[:NC][il] - L[il]).max())
            r["max_L"] = float(np.abs(L).max())
            r["err_X"] = float(np.abs(got[NC:] - X).max())
            r["max_X"] = float(np.abs(X).max())
            bad = NC // 2 + 290                                       # inside the second half, after every update of the first
            _, _, fullb = coupled_matrix(NR, NC, top_h, ranges, NR, bad)
            onb, _, ib_on = potrf(lmm_amd, fullb, 1)
            offb, _, ib_off = potrf(lmm_amd, fullb, 0)
            r["bad"] = bad
            r["bad_info"] = [ib_on, ib_off]
            r["bad_bits_equal"] = bool(np.array_equal(onb[:bad].view(np.int64), offb[:bad].view(np.int64)))      # the columns before the pivot
        res[name] = r
    # five matrices in groups of 2 + 2 + 1: the high-level path (one lock-step batch of five latents), n = 1024
    m, n = 5, 1024
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    y = rng.standard_normal(n * m)
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel()) for _ in range(m)])
    fx = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(np.eye(m), 0.5 + np.arange(m) / m))(lmm_amd.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), m), 0.1)
    yt = torch.from_numpy(y).cuda()
    vals = {}
    assert lib.lmm_dev_set_f64_emul(0, 128, 16) == 0
    vals["f64"] = float(lmm_amd.logpdf(fx, yt))
    assert lib.lmm_dev_set_f64_emul(1, 128, 16) == 0
    for g in (2, 0):
        assert lib.lmm_dev_set_emul_group(g) == 0
        for reuse in (1, 0):
            assert lib.lmm_dev_set_emul_amax_reuse(reuse) == 0
            vals[f"g{g}_reuse{reuse}"] = float(lmm_amd.logpdf(fx, yt)).hex()
    lib.lmm_dev_set_emul_amax_reuse(1)
    lib.lmm_dev_set_emul_group(0)
    res["batch"] = vals
    print(json.dumps(res))


# ---- the tests ----
@pytest.fixture(scope="module")
def found():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, LMM_REGION="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    return res


@pytest.mark.parametrize("name", list(SHAPES))
def test_three_levels_are_chained(found, name):
    """the plan the child factored with: the top update reads two kept arrays and scans the last part of its panel"""
    r = found[name]
    top_h, kept, scan0 = CHAINS[name]
    assert r["top_h"] == top_h and [tuple(k) for k in r["kept"]] == kept and r["scan0"] == scan0


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_source_holds_row_maxima(found, name):
    """on the LAPACK factor: each of the two kept arrays and the scanned columns holds the maximum of at least 10 % of the top panel's rows"""
    share = found[name]["share"]
    print(name, "share of the rows whose maximum lies in kept array 1 / kept array 2 / the scanned columns:", share)
    assert len(share) == 3 and min(share) >= 0.10 and sum(share) == pytest.approx(1.0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_factor_is_the_same_in_every_bit(found, name):
    r = found[name]
    assert r["info"] == [0, 0]
    assert r["factor_bits_equal"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_factor_against_lapack(found, name):
    """the bounds of tests/test_gpu_r3.py::test_panel_factorisation_vs_lapack (the emulated updates are no less exact than the f64 ones)"""
    r = found[name]
    print(name, f"|L - LAPACK| = {r['err_L']:.3e} (max |L| = {r['max_L']:.3f}), |riders - LAPACK| = {r['err_X']:.3e} (max = {r['max_X']:.3f})")
    assert r["err_L"] <= 2e-12 * r["max_L"]
    assert r["err_X"] <= 1e-10 * max(1.0, r["max_X"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_failing_pivot_report_is_unchanged(found, name):
    r = found[name]
    assert r["bad_info"] == [r["bad"] + 1, r["bad"] + 1]
    assert r["bad_bits_equal"]


def test_groups_read_the_kept_arrays_at_their_offsets(found):
    """five latents in groups of 2 + 2 + 1 and in one group, with and without the kept maxima: one value, the f64 path's to rounding"""
    v = found["batch"]
    emu = {k: float.fromhex(s) for k, s in v.items() if k != "f64"}
    print("5 latents:", v)
    assert len(set(emu.values())) == 1
    assert emu["g2_reuse1"] == pytest.approx(v["f64"], rel=1e-12)


if __name__ == "__main__":
    child()
