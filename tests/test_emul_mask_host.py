"""Host-only checks of the live-mask helpers of the int8 emulation's GEMM (csrc/lmm_emul.h, DESIGN.md 4.17, "zero skip"): the stage
list of a tile is the set bits of (mask of its A rows) & (mask of its B rows) below K / 128, in increasing k, and block 0 alone when
that is empty.  The kernel's staging cursor walks the list and its MFMA loop counts it; both must agree, or the pipeline's two sides
run out of step.  Checked through the host entry lmm_dev_emul_stage_list (the very helpers, compiled into the library) and through the
stand-alone tests/c/emul_mask_check.cpp (the header compiles without HIP).  No GPU, no lmm_init."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ONES = (1 << 64) - 1


def stage_list(a, b, nk):
    """(walk, count) for 128-bit Python integers a, b."""
    import lmm_amd
    lib = lmm_amd.load()
    lib.lmm_dev_emul_stage_list.restype = C.c_int
    lib.lmm_dev_emul_stage_list.argtypes = [C.c_ulonglong] * 4 + [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    out, count = (C.c_int * 129)(), C.c_int(-1)
    n = lib.lmm_dev_emul_stage_list(a & ONES, a >> 64, b & ONES, b >> 64, nk, out, 129, C.byref(count))
    assert 0 <= n <= 128, lib.lmm_last_error_string()
    return list(out[:n]), count.value


def expected(a, b, nk):
    bits = [k for k in range(nk) if (a >> k) & (b >> k) & 1]
    return bits or [0]


ALL = (1 << 128) - 1
MASKS = {
    "word 0 only": 0x00F0_0000_0000_8421,
    "word 1 only": 0x0000_0000_0000_8421 << 64 | 0,
    "both words": (0x8000_0000_0000_0003 << 64) | 0xC000_0000_0000_0001,
    "none": 0,
    "all": ALL,
    "one bit, first": 1,
    "one bit, 63": 1 << 63,
    "one bit, 64": 1 << 64,
    "one bit, last": 1 << 127,
}


@pytest.mark.parametrize("name", list(MASKS))
def test_stage_list_is_the_increasing_intersection(name):
    a = MASKS[name]
    for b in list(MASKS.values()) + [a, ALL ^ a]:
        for nk in (1, 2, 5, 9, 63, 64, 65, 128):
            walk, count = stage_list(a, b, nk)
            want = expected(a, b, nk)
            assert walk == want, (name, hex(b), nk, walk, want)
            assert count == len(walk)                                     # the MFMA loop's count is the cursor's walk
            assert all(x < y for x, y in zip(walk, walk[1:])) and walk[-1] < nk


def test_empty_intersection_walks_block_zero():
    assert stage_list(MASKS["word 0 only"], MASKS["word 1 only"], 128) == ([0], 1)
    assert stage_list(0, ALL, 65) == ([0], 1)
    assert stage_list(1 << 70, 1 << 70, 70) == ([0], 1)                   # live only beyond K
    assert stage_list(ALL, ALL, 65) == (list(range(65)), 65)              # all-ones masks: every block, today's walk


def test_bad_arguments_are_refused():
    import lmm_amd
    lib = lmm_amd.load()
    lib.lmm_dev_emul_stage_list.restype = C.c_int
    lib.lmm_dev_emul_stage_list.argtypes = [C.c_ulonglong] * 4 + [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    for nk in (0, 129, -1):
        assert lib.lmm_dev_emul_stage_list(1, 0, 1, 0, nk, None, 0, None) < 0
    assert lib.lmm_dev_emul_stage_list(3, 0, 3, 0, 2, None, 0, None) == 2  # cap 0: counted, not written


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "emul_mask_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "emul_mask_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout.strip())
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]
    assert int(out.stdout.split()[0]) > 100000
