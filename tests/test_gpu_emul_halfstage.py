"""Bit-exact GPU check of the half-stage staging of the emulation's GEMM: lmm_dev_syrk_emul on C = 0 against minus
the product of the host entry lmm_dev_emul_host.  The kernel restages the B half and the A half of an LDS buffer separately, one
phase apart, piece by piece between the MFMAs, and waits for them with a counted vmcnt that leaves the youngest half in flight, so
what can go wrong is a half read before it has landed or restaged while it is still read (at either buffer parity, which K / 128
odd flips between tiles), and the counts at the head and the tail of a workgroup's walk and after an epilogue.  All of them show
as mismatching bits.  Operands, canaries and helpers are those of tests/test_gpu_emul_persistent.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
CANARY = 7.25
CAPS = [1, 2, 3, 5, 7, 0]      # lmm_dev_set_emul_gemm_workgroups: 0 is the default grid


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def operands(M, K, seed):
    """2^-20 .. 2^20 between rows, 2^-12 .. 1 inside a row, both signs, plus an all-zero row, a row whose largest entry is an exact
    power of two and a row spanning 60 binades (rows 5, 7, 9: inside every N used here)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) * np.exp2(rng.integers(-20, 21, size=(M, 1))) * np.exp2(-rng.uniform(0, 12, size=(M, K)))
    A[5] = 0.0
    A[7, 3 % K] = -np.exp2(np.ceil(np.log2(np.abs(A[7]).max())) + 1.0)
    A[9] = rng.standard_normal(K) * np.exp2(-rng.uniform(0, 60, size=K))
    A[9, 0] = 1.0
    A[9, K - 1] = 2.0 ** -60
    return A


_CASES = {}


def case(lmm, M, N, K, nmod=16):
    """(A, minus the host-emulated A A[:N]'), computed once per shape and left unchanged."""
    key = (M, N, K, nmod)
    if key not in _CASES:
        lib = lmm.load()
        A = operands(M, K, M + N + K)
        Af = np.asfortranarray(A)
        Bf = np.asfortranarray(A[:N])
        out = np.zeros((M, N), order="F")
        lib.lmm_dev_emul_host.restype = C.c_int
        rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), M, Bf.ctypes.data_as(DP), N, M, N, K, nmod, K, out.ctypes.data_as(DP), M, None)
        assert rc == 0, lib.lmm_last_error_string()
        want = -out
        want.setflags(write=False)
        A.setflags(write=False)
        _CASES[key] = (A, want)
    return _CASES[key]


def run_syrk(lmm, A, N, nmod=16, pad_a=3, pad_c=5):
    """C (zero on and below the diagonal, CANARY elsewhere, pad rows included) after lmm_dev_syrk_emul, with lda = M + pad_a (NaN in the
    pad rows) and ldc = M + pad_c: (the M x N block, everything else of the buffer)."""
    import torch
    lib = lmm.load()
    M, K = A.shape
    lda, ldc = M + pad_a, M + pad_c
    Ah = np.full((K, lda), np.nan)
    Ah[:, :M] = A.T                                                   # (K, lda) row-major = column-major with leading dimension lda
    Ch = np.full((N, ldc), CANARY)
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    Ch[:, :M][lower.T] = 0.0
    At, Ct = torch.from_numpy(Ah).cuda(), torch.from_numpy(Ch).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_syrk_emul(C.c_void_p(Ct.data_ptr()), ldc, C.c_void_p(At.data_ptr()), lda, M, N, K, nmod)
    assert rc == 0, lib.lmm_last_error_string()
    got = Ct.cpu().numpy()
    return got[:, :M].T, got[:, M:], lower


def check(lmm, M, N, K, cap, nmod=16):
    A, want = case(lmm, M, N, K, nmod)
    lib = lmm.load()
    try:
        assert lib.lmm_dev_set_emul_gemm_workgroups(cap) == 0, lib.lmm_last_error_string()
        got, pad, lower = run_syrk(lmm, A, N, nmod)
    finally:
        lib.lmm_dev_set_emul_gemm_workgroups(0)
    assert np.all(pad == CANARY) and np.all(got[~lower] == CANARY)      # nothing outside i >= j is written
    bad = lower & (got != want)
    print(f"syrk_emul {M}x{N}x{K}, nmod = {nmod}, at most {cap} workgroups: {int(bad.sum())} of {int(lower.sum())} entries differ")
    assert not bad.any(), np.argwhere(bad)[:8]
    assert np.all(got[5, :6] == 0.0) and np.all(got[5:, 5] == 0.0)      # the all-zero row


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 9])
def test_ring_wraps_at_every_phase(lmm, nk, cap):
    """M = N = 512: 3 tiles x 16 moduli = 48 work ids.  A tile is 2 nk half-stages in the four halves of the two buffers: nk = 1, 3,
    5, 9 start every other tile in the other buffer, nk = 1 has the cursor two tiles ahead of the MFMAs (every wait follows an
    epilogue), nk = 2 is exactly one turn, and the caps put the ends of the walks (where the counted wait becomes vmcnt(0)) and the
    item boundaries at other ids."""
    check(lmm, 512, 512, 128 * nk, cap)


@pytest.mark.parametrize("cap", CAPS)
def test_off_diagonal_tiles(lmm, cap):
    check(lmm, 768, 512, 384, cap)                                    # a 3 x 2 tile grid: 5 tiles x 16 moduli = 80 work ids


@pytest.mark.parametrize("nmod", [8, 16])
@pytest.mark.parametrize("cap", CAPS)
def test_ragged_shape(lmm, cap, nmod):
    check(lmm, 300, 200, 256, cap, nmod)                              # 2 tiles, both ragged


@pytest.mark.parametrize("cap", [0, 1])
def test_head_and_tail_of_the_walk(lmm, cap):
    """M = N = 256, K = 128, 8 moduli: 8 work ids of two half-stages each.  On the default grid every workgroup's walk is one tile, so
    the prologue issues all there is and the loop is head and tail at once; one workgroup walks the same 8 tiles in a row."""
    check(lmm, 256, 256, 128, cap, 8)
