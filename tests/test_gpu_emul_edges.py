"""Bit-exact GPU check of the edge tiles of the emulation's GEMM: the last tile row of an update whose M is not a
multiple of 256 holds rows M .. Mp - 1 of zero residues, which the kernel multiplies like any others today.  A kernel that leaves
their MFMAs out (DESIGN.md 8.2 has one that was measured and not kept) has to pass this file: lmm_dev_syrk_emul on C = 0 against
minus the product of the host entry lmm_dev_emul_host, every bit, and nothing outside i >= j written.  What could go wrong there is a
live fragment left out, or a count taken for the wrong tile, wave or phase: the number of live rows of the last tile row sits on
either side of a fragment (16), a phase (64) and a wave (128) boundary, both buffer parities start the edge tile (K / 128 odd flips
them), and one workgroup walks full tile -> edge tile -> full tile with the staging cursor two stages ahead across the change.  An
all-zero row and a NaN row lie among the live rows of the edge tile.  Operands, canaries and the check are those of
tests/test_gpu_emul_halfstage.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
CANARY = 7.25
CAPS = [1, 3, 0]      # lmm_dev_set_emul_gemm_workgroups: 0 is the default grid
EDGE_ROWS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255]


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


def host_product(lmm, A, B, nmod):
    """the host-emulated A B' (rows are scaled one by one, so a block of rows of A against B is that block of the whole product)"""
    lib = lmm.load()
    M, K = A.shape
    N = B.shape[0]
    Af, Bf = np.asfortranarray(A), np.asfortranarray(B)
    out = np.zeros((M, N), order="F")
    lib.lmm_dev_emul_host.restype = C.c_int
    rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), M, Bf.ctypes.data_as(DP), N, M, N, K, nmod, K, out.ctypes.data_as(DP), M, None)
    assert rc == 0, lib.lmm_last_error_string()
    return out


_BASE, _CASES = {}, {}


def planted(A, first):
    """A with an all-zero row and a NaN row among the rows first .. M - 1 (the live rows of the edge tile), where there is room for
    them beside ordinary rows: the last live row stays an ordinary one"""
    M, K = A.shape
    r = M - first
    rows = {}
    if r >= 15:
        rows = {"zero": first + r // 2, "nan": first + r // 4}
        A[rows["zero"]] = 0.0
        A[rows["nan"], (7 * r) % K] = np.nan
    return A, rows


def edge_case(lmm, r, K, nmod):
    """(A, minus the host-emulated A A[:256]', planted rows) for M = 256 + r, N = 256: the product of the first 256 rows is computed once
    per (K, nmod), that of the r edge rows per case"""
    key = (r, K, nmod)
    if key not in _CASES:
        A, rows = planted(operands(511, K, 1000 + K)[:256 + r].copy(), 256)      # rows of one matrix for every r: the first 256 are the same
        if (K, nmod) not in _BASE:
            _BASE[(K, nmod)] = (A[:256].copy(), host_product(lmm, A[:256], A[:256], nmod))
        top, top_out = _BASE[(K, nmod)]
        assert np.array_equal(top, A[:256])
        want = -np.vstack([top_out, host_product(lmm, A[256:], A[:256], nmod)])
        want.setflags(write=False)
        A.setflags(write=False)
        _CASES[key] = (A, want, rows)
    return _CASES[key]


def full_case(lmm, M, N, K, nmod, first):
    key = (M, N, K, nmod)
    if key not in _CASES:
        A, rows = planted(operands(M, K, M + N + K), first)
        want = -host_product(lmm, A, A[:N], nmod)
        want.setflags(write=False)
        A.setflags(write=False)
        _CASES[key] = (A, want, rows)
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


def check(lmm, A, want, rows, N, cap, nmod):
    lib = lmm.load()
    M, K = A.shape
    try:
        assert lib.lmm_dev_set_emul_gemm_workgroups(cap) == 0, lib.lmm_last_error_string()
        got, pad, lower = run_syrk(lmm, A, N, nmod)
    finally:
        lib.lmm_dev_set_emul_gemm_workgroups(0)
    assert np.all(pad == CANARY) and np.all(got[~lower] == CANARY)      # nothing outside i >= j is written
    bad = lower & (got != want) & ~(np.isnan(got) & np.isnan(want))     # every bit (a NaN for a NaN)
    print(f"syrk_emul {M}x{N}x{K}, nmod = {nmod}, at most {cap} workgroups: {int(bad.sum())} of {int(lower.sum())} entries differ")
    assert not bad.any(), np.argwhere(bad)[:8]
    assert np.all(got[5, :6] == 0.0) and np.all(got[5:, 5][~np.isnan(got[5:, 5])] == 0.0)      # the all-zero row 5
    if rows:
        z, q = rows["zero"], rows["nan"]
        zr = got[z, :min(z + 1, N)]
        assert np.all(zr[~np.isnan(want[z, :min(z + 1, N)])] == 0.0) and np.all(np.isnan(got[q, :min(q + 1, N)]))      # 0 x NaN (column q) is NaN
        assert np.isnan(want[q, 0]) and not np.isnan(want[M - 1, :1]).any()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nmod", [8, 16])
@pytest.mark.parametrize("nk", [1, 2, 3])
@pytest.mark.parametrize("r", EDGE_ROWS)
def test_live_rows_on_both_sides_of_every_boundary(lmm, r, nk, nmod, cap):
    """M = 256 + r, N = 256: a full tile and an edge tile with r live rows per modulus.  r = 1 .. 17 and 63 .. 65: the first wave row
    holds 1, 1, 1, 2, 4, 4, 5 live fragments (the lower four only, then one of the upper four); 127 .. 129: the second wave row goes
    from none to one; 255: one dead row."""
    A, want, rows = edge_case(lmm, r, 128 * nk, nmod)
    check(lmm, A, want, rows, 256, cap, nmod)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("K", [256, 384])
def test_edge_row_beside_and_off_the_diagonal(lmm, K, cap):
    """M = 576, N = 512: the edge tile row (64 live rows, as every update of a matrix with 64 rider rows has) holds two off-diagonal
    tiles below a full tile row with a diagonal tile"""
    A, want, rows = full_case(lmm, 576, 512, K, 16, 512)
    check(lmm, A, want, rows, 512, cap, 16)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("M,N,K", [(64, 64, 256), (300, 200, 128), (300, 200, 384)])
def test_one_tile_ragged_both_ways(lmm, M, N, K, cap):
    """M = N = 64: the only tile is a diagonal tile with 64 live rows and columns (the NaN row is a column too); 300 x 200: a diagonal
    tile ragged in its columns above an edge tile with 44 live rows"""
    A, want, rows = full_case(lmm, M, N, K, 16, 0 if M == 64 else 256)
    check(lmm, A, want, rows, N, cap, 16)
