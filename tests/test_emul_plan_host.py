"""Host-only checks of the emulation plan through lmm_dev_emul_plan: which trailing updates of a factorisation the
shape rule sends to the int8 emulation, how many matrices go through the scratch block at a time, and that the block the factorisation
asks for holds every group it will form.  The entry walks the recursion, asks the predicate and sizes the groups with the code the
factorisation itself runs; no GPU and no lmm_init are needed."""
import ctypes as C

import pytest

import lmm_amd
from lmm_amd import _lib as L

CAP = 512
# (NR, NC) of a logpdf factorisation: n columns and one 64-row block of riders
C2, C1, SMALL, C3 = (16384 + 64, 16384), (4096 + 64, 4096), (2048 + 64, 2048), (8192 + 64, 8192)
SHAPES = [C2, C1, SMALL, C3, (2304 + 64, 2304), (1152 + 64, 1152), (2304, 2304)]


@pytest.fixture()
def lib():
    lib = lmm_amd.load()
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    lib.lmm_dev_emul_plan.restype = C.c_int
    lib.lmm_dev_set_f64_emul_rule.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.lmm_dev_set_f64_emul_rule.restype = C.c_int
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    assert lib.lmm_dev_set_f64_emul(-1, 0, 0) == 0
    assert lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0) == 0
    assert lib.lmm_dev_set_emul_group(0) == 0
    yield lib
    lib.lmm_dev_set_f64_emul(-1, 0, 0)
    lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0)
    lib.lmm_dev_set_emul_group(0)


def plan(lib, shape, nb):
    """(block bytes, the G the block is sized for, [(M, N, K, emulated, group, bytes), ...])"""
    out = (C.c_longlong * (2 + 6 * CAP))()
    n = lib.lmm_dev_emul_plan(shape[0], shape[1], nb, out, CAP)
    assert 0 <= n <= CAP, lib.lmm_last_error_string()
    return out[0], out[1], [tuple(out[2 + 6 * i: 8 + 6 * i]) for i in range(n)]


def legal(M, N, K):
    return M >= N >= 1 and K >= 128 and K % 128 == 0 and K <= 16384


def pays(M, N, K, nb, always, shape, min_outputs):
    if K >= always:
        return True
    if K < shape:
        return False
    return nb * (N * (N + 1) / 2 + (M - N) * N) >= min_outputs


def test_walk_is_the_recursion_of_the_factorisation(lib):
    """n = 2304 + riders: 1152 | 1152, each half 640 | 512 -- the updates tests/test_gpu_f64_emul.py names."""
    _, _, recs = plan(lib, (2368, 2304), 2)
    big = [(M, N, K) for M, N, K, *_ in recs if K >= 640]
    assert big == [(1728, 512, 640), (1216, 1152, 1152), (576, 512, 640)]
    assert all(N >= 128 for _, N, *_ in recs)


def test_defaults_c2(lib):
    _, _, recs = plan(lib, C2, 16)
    k2048 = [r for r in recs if r[2] == 2048]
    assert sorted(r[0] for r in k2048) == [2112, 6208, 10304, 14400]
    assert [r[2] for r in recs if r[2] >= 4096] == [4096, 8192, 4096]
    for M, N, K, em, *_ in recs:
        if K >= 4096:
            assert em == 1
        if K == 2048 and M >= 6208:
            assert em == 1
        if K <= 1024:
            assert em == 0


@pytest.mark.parametrize("shape,nb", [(C1, 8), (SMALL, 8)])
def test_defaults_emulate_nothing_at_c1_and_small(lib, shape, nb):
    bytes_, G, recs = plan(lib, shape, nb)
    assert bytes_ == 0 and G == 0
    assert recs and all(r[3] == 0 and r[4] == 0 and r[5] == 0 for r in recs)


def test_defaults_c3(lib):
    _, _, recs = plan(lib, C3, 8)
    top = [r for r in recs if r[2] == 4096]
    assert len(top) == 1 and top[0][3] == 1


@pytest.mark.parametrize("nb", [1, 3, 4, 16, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_groups_fit_the_block(lib, shape, nb):
    for rule in (None, (512, 256, 2.0e5)):
        if rule is not None:
            assert lib.lmm_dev_set_f64_emul_rule(*rule) == 0
        bytes_, G, recs = plan(lib, shape, nb)
        emulated = [r for r in recs if r[3]]
        assert (bytes_ > 0) == bool(emulated)
        if emulated:
            assert 1 <= G <= min(4, nb)
        for M, N, K, em, group, need in emulated:
            assert legal(M, N, K)
            assert need <= bytes_
            assert 1 <= group <= nb
            assert group >= G


def test_group_cap(lib):
    _, G, recs = plan(lib, C2, 16)
    assert max(r[4] for r in recs if r[3]) > G      # a level below the widest holds more matrices per group
    assert lib.lmm_dev_set_emul_group(3) == 0
    _, _, capped = plan(lib, C2, 16)
    assert all(r[4] <= 3 for r in capped if r[3]) and [r[:4] for r in capped] == [r[:4] for r in recs]
    assert lib.lmm_dev_set_emul_group(-1) == L.LMM_ERR_ARG


@pytest.mark.parametrize("rule", [(1152, 640, 8.0e5), (512, 256, 2.0e5), (1024, 128, 0.0), (256, 256, 1.0e30), (2048, 384, 3.0e6)])
@pytest.mark.parametrize("shape,nb", [((2368, 2304), 2), ((2304, 2304), 1), (C1, 8), ((1216, 1152), 12)])
def test_scaled_rule_matches_the_predicate(lib, rule, shape, nb):
    assert lib.lmm_dev_set_f64_emul_rule(*rule) == 0
    _, _, recs = plan(lib, shape, nb)
    assert recs
    for M, N, K, em, *_ in recs:
        assert em == int(legal(M, N, K) and pays(M, N, K, nb, *rule)), (M, N, K)


def test_explicit_threshold_overrides_the_rule(lib):
    assert lib.lmm_dev_set_f64_emul_rule(4096, 4096, 1.0e30) == 0
    assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
    for shape, nb in [((2368, 2304), 2), (C1, 8)]:
        _, _, recs = plan(lib, shape, nb)
        assert any(r[2] >= 256 for r in recs)
        for M, N, K, em, *_ in recs:
            assert em == int(K >= 256 and legal(M, N, K)), (M, N, K)
    assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
    assert plan(lib, C2, 16)[0] == 0


def test_bad_arguments(lib):
    out = (C.c_longlong * 8)()
    assert lib.lmm_dev_emul_plan(4160, 4096, 0, out, 1) == -L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_plan(4000, 4096, 8, out, 1) == -L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_plan(4160, 4096, 8, out, 1) > 1      # counted beyond cap, not written
    assert lib.lmm_dev_set_f64_emul_rule(256, 512, 0.0) == L.LMM_ERR_ARG
