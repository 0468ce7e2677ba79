"""Host-only check of who writes the block maxima of a factorisation (csrc/lmm_potrf_plan.h, plan_block_maxima),
through lmm_dev_potrf_block_writers: for NC = 128 .. 16384 in steps of 64, NR = NC + 64 and nb in {1, 4, 16},

* every block a step folds has exactly one earlier writer, and that writer's rows begin no later than the reader's;
* no block is scanned or stored twice;
* plan_potrf_check passes (the hook refuses a plan that violates an invariant).

The sweep runs under the default switches and, on a coarser grid, with explicit thresholds that put screened f64 updates and emulated
updates into plans whose block columns are not region launches, where scans remain."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 16


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import lmm_amd
    L = lmm_amd.load()
    L.lmm_dev_potrf_block_writers.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    L.lmm_dev_potrf_block_writers.restype = C.c_int
    return L


def records(lib, NR, NC, nb, buf):
    n = lib.lmm_dev_potrf_block_writers(NR, NC, nb, NC + 1, 1, 256, 0, 0, buf, CAP)
    assert 0 <= n <= CAP, (NR, NC, nb, n, lib.lmm_last_error_string())
    return [tuple(buf[5 * i: 5 * i + 5]) for i in range(n)]


def check(recs, where):
    own = {}                                                         # block -> (writer step, first row)
    folds = 0
    for step, cb, writer, wrow, rrow in recs:                        # in step order
        if writer == step:
            assert cb not in own, (where, "block written twice", cb, own[cb], step)
            own[cb] = (step, wrow)
            assert wrow == rrow or wrow <= rrow, (where, cb)
        else:
            folds += 1
            assert cb in own, (where, "folds a block nobody wrote", step, cb)
            assert own[cb][0] == writer and writer < step, (where, step, cb, writer, own[cb])
            assert own[cb][1] == wrow and wrow <= rrow, (where, "writer's rows begin below the reader's", step, cb, wrow, rrow)
    return len(own), folds


def test_every_folded_block_has_one_earlier_writer(lib):
    buf = (C.c_longlong * (5 * CAP))()
    written = folded = plans = 0
    for NC in range(128, 16384 + 1, 64):
        for nb in (1, 4, 16):
            w, f = check(records(lib, NC + 64, NC, nb, buf), (NC, nb))
            written += w
            folded += f
            plans += 1
    print(plans, "plans,", written, "blocks written,", folded, "folds")
    assert written > 0 and folded > 0
    # C2 as the benchmark runs it: every block is a region launch's, nothing is scanned
    n = lib.lmm_dev_potrf_block_writers(16448, 16384, 16, 16385, 2, 256, 0, 1, buf, CAP)
    assert 0 < n <= CAP
    plan = (C.c_longlong * (8 + 14 * 4096))()
    lib.lmm_dev_potrf_plan.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    ns = lib.lmm_dev_potrf_plan(16448, 16384, 16, 16385, 2, 256, 0, 1, plan, 4096)
    kinds = [plan[8 + 14 * i] for i in range(ns)]
    recs = [tuple(buf[5 * i: 5 * i + 5]) for i in range(n)]
    assert all(kinds[r[2]] == 7 for r in recs), "a block of C2 is scanned"
    assert any(kinds[r[0]] == 5 for r in recs) and any(kinds[r[0]] == 6 for r in recs)


def kinds_of(lib, NR, NC, nb):
    plan = (C.c_longlong * (8 + 14 * 8192))()
    lib.lmm_dev_potrf_plan.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    ns = lib.lmm_dev_potrf_plan(NR, NC, nb, NC + 1, 1, 256, 0, 0, plan, 8192)
    assert 0 < ns <= 8192
    return [plan[8 + 14 * i] for i in range(ns)]


def test_scans_remain_where_no_region_launch_writes(lib):
    """widths of 64 mod 128 keep the panel recursion: their blocks are scanned, once each, by update steps (kinds 5 and 6)"""
    lib.lmm_dev_set_f64_screen.argtypes = [C.c_int, C.c_int]
    lib.lmm_dev_set_f64_emul.argtypes = [C.c_int] * 3
    buf = (C.c_longlong * (5 * CAP))()
    scanned = stored = folded = 0
    try:
        assert lib.lmm_dev_set_f64_emul(1, 1024, 16) == 0 and lib.lmm_dev_set_f64_screen(1, 256) == 0
        for NC in list(range(128, 4096 + 1, 64)) + [8192, 8192 + 64, 16384]:
            for nb in (1, 4, 16):
                recs = records(lib, NC + 64, NC, nb, buf)
                check(recs, (NC, nb))
                kinds = kinds_of(lib, NC + 64, NC, nb)
                for step, cb, writer, wrow, rrow in recs:
                    assert kinds[step] in (5, 6, 7) and kinds[writer] in (5, 6, 7)
                    assert kinds[step] != 7 or writer == step
                    if writer != step:
                        folded += 1
                    elif kinds[step] == 7:
                        stored += 1
                    else:
                        scanned += 1
    finally:
        lib.lmm_dev_set_f64_emul(-1, 0, 16)
        lib.lmm_dev_set_f64_screen(-1, 0)
    print(scanned, "blocks scanned,", stored, "stored by region launches,", folded, "folded")
    assert scanned > 0 and stored > 0 and folded > 0


def test_source_zero_plans_no_writers(lib):
    lib.lmm_dev_set_bmax_source.argtypes = [C.c_int]
    buf = (C.c_longlong * (5 * CAP))()
    try:
        assert lib.lmm_dev_set_bmax_source(0) == 0
        assert records(lib, 16448, 16384, 16, buf) == []
    finally:
        lib.lmm_dev_set_bmax_source(1)
    assert len(records(lib, 16448, 16384, 16, buf)) > 0
