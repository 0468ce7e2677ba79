"""CPU checks of the reduction in the epilogue of the int8 emulation's GEMM through the host-only entry
lmm_dev_emul_acc_residues: it runs the scalar functions of lmm_emul.h that the kernel runs, on an array of int32 accumulators."""
import ctypes as C

import numpy as np

import lmm_amd
from lmm_amd import _lib as L

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193]
XMAX = 16384 * 128 ** 2                                               # the largest |accumulator|: K = 16384 products of two int8


def residues(values, nmod=16, exhaustive=False):
    lib = lmm_amd.load()
    x = np.array(values, dtype=np.int32)
    out = np.zeros((len(x), nmod), dtype=np.int8)
    ex = np.zeros(2, dtype=np.int64)
    lib.lmm_dev_emul_acc_residues.restype = C.c_int
    rc = lib.lmm_dev_emul_acc_residues(x.ctypes.data_as(C.POINTER(C.c_int)), len(x), nmod, out.ctypes.data_as(C.POINTER(C.c_byte)),
                                       ex.ctypes.data_as(C.POINTER(C.c_longlong)) if exhaustive else None)
    assert rc == L.LMM_OK, lib.lmm_last_error_string()
    return out, ex


def fold_const(p):
    r = 65536 % p
    return r - p if r > p // 2 else r


def check_against_python(vals, nmod):
    out, _ = residues(vals, nmod)
    x = np.array(vals, dtype=np.int64)
    for t in range(nmod):
        p = MODULI[t]
        got = out[:, t].astype(np.int64)
        assert np.array_equal(got % p, x % p), (nmod, p)              # numpy's % on int64 is Python's: the result has the sign of p
        lo = -(p // 2)
        assert np.all((got >= lo) & (got <= lo + p - 1)), (nmod, p)


def test_float_step_is_exact_for_every_folded_value_it_can_see():
    """Every modulus p and every y with |y| <= 4096 |2^16 mod p| + 65535, the folded form of an accumulator |x| <= 2^28: the byte is y's
    residue in [-(p - 1) / 2, (p - 1) / 2] ([-128, 127] for 256).  The loop runs in C++ behind the entry."""
    _, ex = residues([0], exhaustive=True)
    want = sum(2 * (4096 * abs(fold_const(p)) + 65535) + 1 for p in MODULI)
    assert int(ex[0]) == want and want < 3 * 10 ** 7
    assert int(ex[1]) == 0


def test_extremes_and_fold_boundaries():
    vals = [0, 1, -1, XMAX, -XMAX, XMAX - 1, -(XMAX - 1)]
    for h in (-4096, -4095, -1, 0, 1, 4095):                          # the ends of the high and the low half
        for lo in (0, 1, 127, 128, 129, 255, 256, 32767, 32768, 65535):
            vals.append(h * 65536 + lo)
    for p in MODULI:                                                  # multiples of p and the ties of the symmetric range around them
        for k in (1, 1000, XMAX // p):
            vals += [s * k * p + d for s in (1, -1) for d in (-(p // 2) - 1, -(p // 2), -1, 0, 1, p // 2, p // 2 + 1) if abs(s * k * p + d) <= XMAX]
    for nmod in (16, 8):
        check_against_python(vals, nmod)


def test_random_accumulators_agree_with_python_integers():
    rng = np.random.default_rng(11)
    vals = rng.integers(-XMAX, XMAX + 1, size=10 ** 6)
    check_against_python(vals, 16)


def test_bad_arguments_are_refused():
    lib = lmm_amd.load()
    x = np.array([XMAX + 1], dtype=np.int32)
    out = np.zeros(16, dtype=np.int8)
    lib.lmm_dev_emul_acc_residues.restype = C.c_int
    args = (x.ctypes.data_as(C.POINTER(C.c_int)), 1, 16, out.ctypes.data_as(C.POINTER(C.c_byte)), None)
    assert lib.lmm_dev_emul_acc_residues(*args) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_acc_residues(args[0], 1, 7, args[3], None) == L.LMM_ERR_ARG
