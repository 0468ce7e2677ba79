"""The blocked schedule of the Toeplitz path (DESIGN.md 4.22 "Blocked schedule") without a GPU: its symbols, prototypes and caps."""
import ctypes as C
import os

import lmm_amd as lmm
from lmm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME_ARGS = {"lmm_oilmm_logpdf_toeplitz_blocked": "lmm_oilmm_logpdf_toeplitz", "lmm_oilmm_logpdf_grad_toeplitz_blocked": "lmm_oilmm_logpdf_grad_toeplitz",
             "lmm_oilmm_toeplitz_posterior_create_blocked": "lmm_oilmm_toeplitz_posterior_create",
             "lmm_dev_toeplitz_factor_blocked": "lmm_dev_toeplitz_factor", "lmm_toeplitz_blocked_max_n": "lmm_toeplitz_max_n"}


def test_symbols_prototypes_and_caps():
    hdr = open(os.path.join(ROOT, "include", "lmm_hip.h")).read()
    lib = lmm.load()
    for s, base in SAME_ARGS.items():
        assert s in lmm.SYMBOLS and f"int {s}(" in hdr
        assert getattr(lib, s).argtypes == getattr(lib, base).argtypes
    assert "lmm_toeplitz_blocked_shape" in lmm.SYMBOLS and lib.lmm_toeplitz_blocked_shape.argtypes == [L._P, L._P]
    assert lib.lmm_toeplitz_blocked_max_n() == 131072 and lib.lmm_toeplitz_max_n() == 8192
    steps, rows = C.c_int(), C.c_int()
    assert lib.lmm_toeplitz_blocked_shape(C.byref(steps), C.byref(rows)) == 0
    assert 0 < steps.value < rows.value
