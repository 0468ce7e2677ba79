"""GPU check of the block maxima as the only source of the scanning updates' row maxima (plan_block_maxima): the
region launches' row tasks store them, an update folds them.  lmm_dev_set_bmax_source(0) makes every update scan as before, so the
two sources are compared within one build.

Shapes: NR = 2112, NC = 2048 -- with 512-column block columns (LMM_REGION=512, LMM_REGION_ALL=1) and lmm_dev_set_f64_emul(1, 1024, 16),
lmm_dev_set_f64_screen(1, 512) the plan has region launches (kind 7), screened f64 updates (kind 5: K = 512 at columns 0 and 1024)
and an emulated update outside them (kind 6: K = 1024 at column 0); the 64 rider rows make the last row tile 64 high -- and NR =
1600, NC = 1536 with lmm_dev_set_f64_emul(1, 512, 16), lmm_dev_set_f64_screen(1, 384): block columns of 384, screened K = 384 updates at
columns 0 and 768 and the K = 768 update at column 0 emulated, so kinds 5, 6 and 7 are present there too.  On every input and
both settings:
 (a) at the default, the array read back equals max |L[i, 128 b : 128 b + 128]| of the factor the device returned, bit for bit, for
     every block b a writer is listed for and every row from that writer's first row (with source 0 nothing is listed: nothing to read);
 (b) L, W and info are identical in every bit between the two settings;
 (c) so are the f64 screen's counters and the zero-extent counters.
Inputs: a Matern52 Gram on the benchmark's grid spacing with lengthscale 0.05 and its true zero extents; the coupled matrices of
test_gpu_emul_amax_reuse.py; a NaN, an infinity, and -0.0 with subnormals in a panel row; a matrix that does not decay (the vote is
0) with the emulation's scratch poisoned; a matrix that is not positive definite in its second half.  Then three different matrices
(Matern, coupled, -0.0 / subnormals) as ONE batch through lmm_dev_potrf_batch, walked in emulation groups of 2 + 1
(lmm_dev_set_emul_group(2)): (a) for every matrix against its own factor, (b) and (c) for the batch -- the per-matrix strides of the
array, of the scans and of the fold are only reached there.  Three latents in emulation groups of 2 + 1 also go through the
high-level path: one logpdf value, in every bit, at both settings.  The child runs with
lmm_dev_set_deterministic(1) (no split-K atomics), and every factorisation at the default is run twice, so that a difference between
the settings is not mistaken for the run-to-run difference of atomic sums.
All GPU work runs in one child process; nothing here provokes a fault: a wrong store shows up as a differing value."""
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
SHAPES = {"2048": (2112, 2048), "1536": (1600, 1536)}
SWITCHES = {"2048": (1024, 512), "1536": (512, 384)}      # lmm_dev_set_f64_emul(1, ., 16), lmm_dev_set_f64_screen(1, .)
ABS = np.uint64(0x7FFFFFFFFFFFFFFF)


def plan_kinds(lib, NR, NC, nb):
    out = (C.c_longlong * (8 + 14 * 1024))()
    lib.lmm_dev_potrf_plan.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    n = lib.lmm_dev_potrf_plan(NR, NC, nb, -1, 1, 256, 0, 1, out, 1024)
    assert 0 < n <= 1024
    return [int(out[8 + 14 * i]) for i in range(n)]


def writers(lib, NR, NC, nb=1):
    """block -> first row its writer covers (the plan lmm_dev_potrf runs: nb matrices, all rows real, strict progress)"""
    buf = (C.c_longlong * (5 * 4096))()
    lib.lmm_dev_potrf_block_writers.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    n = lib.lmm_dev_potrf_block_writers(NR, NC, nb, -1, 1, 256, 0, 1, buf, 4096)
    assert 0 <= n <= 4096
    return {int(buf[5 * i + 1]): int(buf[5 * i + 3]) for i in range(n) if buf[5 * i] == buf[5 * i + 2]}


def matern_matrix(NR, NC):
    x = np.arange(NC) * 20.0 / 575.0
    r = np.abs(x[:, None] - x[None, :]) / 0.05
    K = (1.0 + np.sqrt(5.0) * r + 5.0 * r * r / 3.0) * np.exp(-np.sqrt(5.0) * r) + 0.1 * np.eye(NC)
    full = np.zeros((NR, NC))
    full[:NC] = np.tril(K)
    full[NC, NC - 300:] = np.random.default_rng(1).standard_normal(300)                         # one rider row, +0 in its leading columns
    ext = np.zeros(NR // 64, dtype=np.int32)
    bits = full.view(np.uint64)
    for q in range(NR // 64):
        nz = np.nonzero(bits[64 * q: 64 * q + 64].any(axis=0))[0]
        ext[q] = 0x7F7F7F7F if nz.size == 0 else (nz[0] // 64) * 64
    return full, ext


def run(lmm, lib, full, source, ext=None):
    """one matrix through lmm_dev_potrf_zext, or a list of matrices (ext: a list too, None entries = no extents known) as one batch
    through lmm_dev_potrf_batch; A, W, info and bmax of the result have the matrix as their first axis in that case"""
    import torch
    batch = isinstance(full, list)
    fulls = full if batch else [full]
    nb = len(fulls)
    NR, NC = fulls[0].shape
    ld = NR + 16
    Ah = np.full((nb, NC, ld), np.nan)
    iu = np.triu_indices(NC, 1)
    for j, f in enumerate(fulls):
        Ah[j, :, :NR] = f.T
        Ah[j, iu[1], iu[0]] = np.nan
    A = torch.from_numpy(Ah).cuda()
    W = torch.zeros(nb, NC // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(nb, dtype=torch.int32, device="cuda")
    if batch:
        ext = None if all(e is None for e in ext) else np.stack([np.zeros(NR // 64, dtype=np.int32) if e is None else e for e in ext])
    zx = None if ext is None else torch.from_numpy(ext).cuda()
    torch.cuda.synchronize()
    assert lib.lmm_dev_set_bmax_source(source) == 0
    lib.lmm_dev_f64_screen_stats(1, None, 0)
    lib.lmm_dev_zero_extent_stats(1, None, 0)
    lib.lmm_dev_potrf_block_maxima(1, None, 0, None)
    try:
        zp = None if zx is None else C.c_void_p(zx.data_ptr())
        if batch:
            rc = lib.lmm_dev_potrf_batch(C.c_void_p(A.data_ptr()), nb, NR, NC, ld, C.c_void_p(W.data_ptr()), NC, C.c_void_p(info.data_ptr()), zp)
        else:
            rc = lib.lmm_dev_potrf_zext(C.c_void_p(A.data_ptr()), NR, NC, ld, C.c_void_p(W.data_ptr()), NC, C.c_void_p(info.data_ptr()), zp)
        assert rc == 0, lib.lmm_last_error_string()
        s1 = (C.c_int * (5 * 64))()
        n1 = lib.lmm_dev_f64_screen_stats(0, s1, 64)
        s2 = (C.c_int * (7 * 64))()
        n2 = lib.lmm_dev_zero_extent_stats(0, s2, 64)
        dims = (C.c_int * 3)()
        nw = lib.lmm_dev_potrf_block_maxima(1, None, 0, dims)
        bm = np.zeros(max(nw, 1), dtype=np.uint64)
        lib.lmm_dev_potrf_block_maxima(0, bm.ctypes.data_as(C.POINTER(C.c_ulonglong)), nw, dims)
    finally:
        lib.lmm_dev_set_bmax_source(1)
    Ah, Wh, ih = A.cpu().numpy(), W.cpu().numpy(), info.cpu().numpy()
    return {"A": Ah if batch else Ah[0], "W": Wh if batch else Wh[0], "info": [int(v) for v in ih] if batch else int(ih[0]), "screen": list(s1[: 5 * n1]),
            "zext": list(s2[: 7 * n2]), "dims": list(dims), "bmax": bm[:nw].reshape(dims[0], dims[1], dims[2]) if nw > 0 else None}


def readback_ok(r, wr, NR, NC, m=None):
    """(a): every listed word against the returned factor (of matrix m of a batch); returns (words compared, mismatches)"""
    if r["bmax"] is None:
        return 0, 0 if not wr else -1
    Am = r["A"] if m is None else r["A"][m]
    bits = Am.view(np.uint64) & ABS                                   # [column][row]
    want = bits.reshape(NC // 128, 128, -1).max(axis=1)               # [block][row]
    n = bad = 0
    for cb, row0 in wr.items():
        got = r["bmax"][0 if m is None else m, cb, row0:NR]
        n += got.size
        bad += int((got != want[cb, row0:NR]).sum())
    return n, bad


def same(a, b, upto=None):
    A, B = (a["A"], b["A"]) if upto is None else (a["A"][:upto], b["A"][:upto])
    return bool(np.array_equal(A.view(np.int64), B.view(np.int64)) and (upto is not None or np.array_equal(a["W"].view(np.int64), b["W"].view(np.int64))))


def child():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import lmm_amd
    import test_gpu_emul_amax_reuse as AR
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_bmax_source.argtypes = [C.c_int]
    lib.lmm_dev_f64_screen_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_zero_extent_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_potrf_block_maxima.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_longlong, C.POINTER(C.c_int)]
    lib.lmm_dev_potrf_block_maxima.restype = C.c_longlong
    lib.lmm_dev_potrf_zext.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.lmm_dev_set_f64_screen.argtypes = [C.c_int, C.c_int]
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    lib.lmm_dev_potrf_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.lmm_dev_set_zero_extents(1) == 0 and lib.lmm_dev_set_zero_extents_min_cols(0) == 0
    assert lib.lmm_dev_set_deterministic(1) == 0                                    # no split-K atomics: a factor is the same from run to run
    res = {}
    for name, (NR, NC) in SHAPES.items():
        assert lib.lmm_dev_set_f64_emul(1, SWITCHES[name][0], 16) == 0 and lib.lmm_dev_set_f64_screen(1, SWITCHES[name][1]) == 0
        wr = writers(lib, NR, NC)
        r = {"kinds": sorted(set(plan_kinds(lib, NR, NC, 1))), "blocks_written": len(wr), "cases": {}}
        top = NC // 2
        ranges = [(0, 128), (top // 2, top // 2 + 128), (top - 128, top)]            # three different blocks of the top panel
        inputs = {}
        inputs["matern"] = matern_matrix(NR, NC)
        _, _, coupled = AR.coupled_matrix(NR, NC, top, ranges, NR)
        inputs["coupled"] = (coupled, None)
        for kind, val in (("nan", np.nan), ("inf", np.inf)):
            f = coupled.copy()
            f[top + 200, 40] = val                                                  # a panel row of the top update
            inputs[kind] = (f, None)
        f = coupled.copy()
        f[top + 130, :128] = -0.0
        f[top + 131, :256] = 5e-324 * (1 + np.arange(256) % 7)
        f[NC, :64] = -0.0
        inputs["negzero_subnormal"] = (f, None)
        _, _, bad = AR.coupled_matrix(NR, NC, top, ranges, NR, NC // 2 + 290)
        inputs["not_pd"] = (bad, None)
        for key, (full, ext) in inputs.items():
            if key == "coupled":
                lib.lmm_dev_set_emul_scratch_poison(1)                              # the matrix does not decay: the vote is 0
            new, old, again = run(lmm_amd, lib, full, 1, ext), run(lmm_amd, lib, full, 0, ext), run(lmm_amd, lib, full, 1, ext)
            lib.lmm_dev_set_emul_scratch_poison(0)
            n, badw = readback_ok(new, wr, NR, NC)
            upto = NC // 2 + 290 if key == "not_pd" else None                        # beyond a failed pivot the factor is unspecified
            r["cases"][key] = {"info": [new["info"], old["info"]], "bits_equal": same(new, old, upto), "repeat_equal": same(new, again, upto), "screen_equal": new["screen"] == old["screen"],
                               "zext_equal": new["zext"] == old["zext"], "screen": new["screen"], "zext_void": [new["zext"][7 * i + 5] for i in range(len(new["zext"]) // 7)],
                               "words": n, "bad_words": badw, "old_has_array": old["bmax"] is not None}
        # three different matrices as one batch, in emulation groups of 2 + 1: every matrix's words against its own factor
        trio = ["matern", "coupled", "negzero_subnormal"]
        fulls, exts = [inputs[k][0] for k in trio], [inputs[k][1] for k in trio]
        wr3 = writers(lib, NR, NC, 3)
        assert lib.lmm_dev_set_emul_group(2) == 0
        new, old, again = run(lmm_amd, lib, fulls, 1, exts), run(lmm_amd, lib, fulls, 0, exts), run(lmm_amd, lib, fulls, 1, exts)
        assert lib.lmm_dev_set_emul_group(0) == 0
        per = [readback_ok(new, wr3, NR, NC, m) for m in range(3)]
        r["batch"] = {"kinds": sorted(set(plan_kinds(lib, NR, NC, 3))), "blocks_written": len(wr3), "dims": new["dims"], "info": [new["info"], old["info"]],
                      "bits_equal": same(new, old), "repeat_equal": same(new, again), "screen_equal": new["screen"] == old["screen"], "zext_equal": new["zext"] == old["zext"],
                      "screen": new["screen"], "words": [p[0] for p in per], "bad_words": [p[1] for p in per],
                      "matrices_differ": not np.array_equal(new["bmax"][0], new["bmax"][1]) and not np.array_equal(new["bmax"][1], new["bmax"][2])}
        res[name] = r
    assert lib.lmm_dev_set_f64_emul(1, 1024, 16) == 0 and lib.lmm_dev_set_f64_screen(1, 512) == 0
    # three latents in emulation groups of 2 + 1, n = 2048: the high-level path
    m, n = 3, 2048
    x = torch.arange(n, dtype=torch.float64, device="cuda") * (20.0 / 575.0)
    y = torch.from_numpy(np.random.default_rng(7).standard_normal(n * m)).cuda()
    vals = {}
    for ls in (0.05, 50.0):
        fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel(lengthscale=ls)) for _ in range(m)])
        fx = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(np.eye(m), 0.5 + np.arange(m) / m))(lmm_amd.MOInputIsotopicByOutputs(x, m), 0.1)
        for g in (2, 0):
            assert lib.lmm_dev_set_emul_group(g) == 0
            for source in (1, 0):
                assert lib.lmm_dev_set_bmax_source(source) == 0
                vals[f"ls{ls}_g{g}_source{source}"] = float(lmm_amd.logpdf(fx, y)).hex()
    lib.lmm_dev_set_bmax_source(1)
    lib.lmm_dev_set_emul_group(0)
    res["batch"] = vals
    res["batch_kinds"] = sorted(set(plan_kinds(lib, n + 64, n, m)))
    print(json.dumps(res))


@pytest.fixture(scope="module")
def found():
    env = dict(os.environ, LMM_REGION="512", LMM_REGION_ALL="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    return res


CASES = ["matern", "coupled", "nan", "inf", "negzero_subnormal", "not_pd"]


def test_plan_has_region_screened_and_emulated_steps(found):
    for name in SHAPES:
        assert {5, 6, 7} <= set(found[name]["kinds"]) and {5, 6, 7} <= set(found[name]["batch"]["kinds"]), name
    assert {5, 6, 7} <= set(found["batch_kinds"])
    # every 128-column block up to the last scanning step's panel (2048: K = 512 at column 1024; 1536: K = 384 at column 768) has a writer
    assert found["2048"]["blocks_written"] == 12 and found["1536"]["blocks_written"] == 9
    assert found["2048"]["batch"]["blocks_written"] == 12 and found["1536"]["batch"]["blocks_written"] == 9


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("case", CASES)
def test_read_back_equals_block_maxima_of_the_factor(found, name, case):
    c = found[name]["cases"][case]
    print(name, case, c["words"], "words compared,", c["bad_words"], "differ")
    assert c["words"] > 0 and c["bad_words"] == 0


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("case", CASES)
def test_results_do_not_depend_on_the_source(found, name, case):
    c = found[name]["cases"][case]
    assert c["repeat_equal"], "the factor is not reproducible at one setting: nothing can be said about the other"
    assert c["bits_equal"] and c["info"][0] == c["info"][1]
    assert c["screen_equal"] and c["zext_equal"]
    if case == "not_pd":
        assert c["info"][0] == int(name) // 2 + 290 + 1
    if case in ("matern", "coupled", "negzero_subnormal"):
        assert c["info"] == [0, 0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_inputs_reach_the_paths_they_are_meant_for(found, name):
    """the Matern matrix has dead tiles and void work items; the matrix without decay has a vote of 0 where a vote is taken"""
    m, c = found[name]["cases"]["matern"], found[name]["cases"]["coupled"]
    assert len(m["screen"]) > 0 and sum(m["screen"][3::5]) > 0 and sum(m["zext_void"]) > 0
    assert sum(c["screen"][3::5]) == 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_of_three_in_groups_of_two_and_one(found, name):
    """(a) per matrix against its own factor, (b) and (c) for the batch: a wrong matrix offset in the stores, the scans or the fold
    shows as another matrix's words (the three matrices' arrays differ) or as a differing factor or counter"""
    c = found[name]["batch"]      # dims: matrices, blocks, rows of the array read back
    print(name, "batch", c["dims"], c["words"], "words compared,", c["bad_words"], "differ")
    assert c["dims"][0] == 3 and c["dims"][2] == SHAPES[name][0] and c["matrices_differ"]
    assert all(w > 0 for w in c["words"]) and c["bad_words"] == [0, 0, 0]
    assert c["repeat_equal"], "the factors are not reproducible at one setting: nothing can be said about the other"
    assert c["bits_equal"] and c["info"] == [[0, 0, 0], [0, 0, 0]]
    assert c["screen_equal"] and c["zext_equal"] and len(c["screen"]) > 0


def test_three_latents_in_groups_of_two_and_one(found):
    v = found["batch"]
    for ls in ("0.05", "50.0"):
        assert len({s for k, s in v.items() if k.startswith(f"ls{ls}_")}) == 1, v


if __name__ == "__main__":
    child()
