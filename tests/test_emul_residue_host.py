"""CPU checks of the residue step of the int8 emulation's convert kernel through the host-only entry
lmm_dev_emul_residues: it runs the scalar functions of lmm_emul.h that the kernel runs, on an array of int64."""
import ctypes as C

import numpy as np

import lmm_amd
from lmm_amd import _lib as L

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193]


def residues(values, nmod=16, exhaustive=False):
    lib = lmm_amd.load()
    v = np.array(values, dtype=np.int64)
    out = np.zeros((len(v), nmod), dtype=np.int8)
    ex = np.zeros(2, dtype=np.int64)
    lib.lmm_dev_emul_residues.restype = C.c_int
    rc = lib.lmm_dev_emul_residues(v.ctypes.data_as(C.POINTER(C.c_longlong)), len(v), nmod, out.ctypes.data_as(C.POINTER(C.c_byte)),
                                   ex.ctypes.data_as(C.POINTER(C.c_longlong)) if exhaustive else None)
    assert rc == L.LMM_OK, lib.lmm_last_error_string()
    return out, ex


def test_reduction_is_congruent_and_in_range_for_every_input_it_can_see():
    """Every odd modulus p, every x in [0, 255 sum_i (256^i mod p)] (the largest sum of the eight byte products) and both signs: the
    result is congruent to +-x and lies in [-(p - 1) / 2, (p - 1) / 2].  The loop runs in C++ behind the entry."""
    _, ex = residues([0], exhaustive=True)
    want = sum(255 * sum(pow(256, i, p) for i in range(8)) + 1 for p in MODULI[1:])
    assert int(ex[0]) == want and want < 10 ** 7
    assert int(ex[1]) == 0


def test_residues_agree_with_python_integers():
    rng = np.random.default_rng(3)
    vals = [0, 1, -1, (1 << 58) - 1, -((1 << 58) - 1), 1 << 58, -(1 << 58)]
    for i in range(8):
        for d in (-1, 1):
            x = 256 ** i + d
            if 0 < x <= 1 << 58:
                vals += [x, -x]
    vals += [int(x) * int(s) for x, s in zip(rng.integers(1 << 57, 1 << 58, size=5000), rng.choice([-1, 1], size=5000))]
    vals += [int(x) * int(s) for x, s in zip(rng.integers(0, 1 << 58, size=5000) >> rng.integers(0, 58, size=5000), rng.choice([-1, 1], size=5000))]
    for nmod in (16, 8):
        out, _ = residues(vals, nmod)
        for t in range(nmod):
            p = MODULI[t]
            want = np.array([v % p for v in vals], dtype=np.int64)
            got = out[:, t].astype(np.int64)
            assert np.array_equal(got % p, want), (nmod, p)
            if p != 256:
                assert np.all(np.abs(got) <= (p - 1) // 2), (nmod, p)


def test_bad_arguments_are_refused():
    lib = lmm_amd.load()
    v = np.array([(1 << 58) + 1], dtype=np.int64)
    out = np.zeros(16, dtype=np.int8)
    lib.lmm_dev_emul_residues.restype = C.c_int
    args = (v.ctypes.data_as(C.POINTER(C.c_longlong)), 1, 16, out.ctypes.data_as(C.POINTER(C.c_byte)), None)
    assert lib.lmm_dev_emul_residues(*args) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_residues(args[0], 1, 7, args[3], None) == L.LMM_ERR_ARG
