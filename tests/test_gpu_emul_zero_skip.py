"""GPU checks of the zero skip of the int8 emulation's GEMM: the convert records per 256 rows of a panel which 128-wide
K blocks hold a non-zero truncated integer, and a tile walks only the blocks that are live in both of its operands.  A skipped block
multiplies exact zeros, so lmm_dev_syrk_emul must still equal the host entry lmm_dev_emul_host (which knows nothing of masks) in every
bit, for operands whose live pattern differs per 256-row block, and a factorisation must give the same factor with the skip on and
off."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
CANARY = 7.25
GRIDS = (1, 2, 3, 5, 7, 0)                                               # workgroups of the persistent GEMM; 0: the default
ZERO_ROW, NAN_ROW, PIECE = 5, 11, range(32, 48)                          # in the first 256-row block, inside every N used here


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_f64_emul_rule.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    yield lmm_amd
    lib.lmm_dev_set_emul_zero_skip(-1)
    lib.lmm_dev_set_emul_gemm_workgroups(0)
    lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0)


def bit_budget(lmm, nmod, K):
    """b of depth K, from the host entry's constants."""
    lib = lmm.load()
    one = np.ones((1, 1), order="F")
    out, consts = np.zeros((1, 1), order="F"), np.zeros(68)
    assert lib.lmm_dev_emul_host(one.ctypes.data_as(DP), 1, one.ctypes.data_as(DP), 1, 1, 1, 1, nmod, K, out.ctypes.data_as(DP), 1, consts.ctypes.data_as(DP)) == 0
    return int(consts[67])


def live_blocks(A, b):
    """[256-row block][K block] -> some truncated integer of the block is not zero (the convert's rule, in NumPy; a NaN row is zeros)."""
    M, K = A.shape
    amax = np.abs(A).max(axis=1)
    ok = np.isfinite(amax) & (amax > 0)
    e = np.zeros(M, dtype=np.int64)
    e[ok] = np.ceil(np.log2(amax[ok])).astype(np.int64)
    ints = np.zeros_like(A)
    ints[ok] = np.trunc(np.ldexp(A[ok], (b - e[ok])[:, None]))
    nz = ints != 0
    return [[bool(nz[r:r + 256, k:k + 128].any()) for k in range(0, K, 128)] for r in range(0, M, 256)]


def pattern(M, nk, variant):
    """Per 256-row block: the K blocks meant to be live, the block that holds only entries at 2^-(b+1) of the row maximum (they
    truncate away: dead) and the block that holds one entry at 2^-(b-1) (it survives as the integer 2: live).
    block 0: every K block (variant 0), or exactly those that block 1 does not have (variants 1, 2: tile (1, 0) has no common block);
    block 1: ONE live K block -- the first, the middle or the last one for variant 0, 1, 2 -- beside the two boundary blocks;
    block 2: the last K block alone.
    With block 0 all live, the tiles (0, 0), (1, 0), (2, 0) of a walk have all, 2 (1 when nk < 3) and 1 stages."""
    pos = (0, nk // 2, nk - 1)[variant]
    others = [k for k in range(nk) if k != pos]
    gone = others[0] if others else None
    kept = others[1] if len(others) > 1 else None
    s1 = {pos} | ({kept} if kept is not None else set())
    s0 = set(range(nk)) - s1 if variant and len(s1) < nk else set(range(nk))
    spec = [dict(live=s0, gone=None, kept=None), dict(live={pos}, gone=gone, kept=kept), dict(live={nk - 1}, gone=None, kept=None)]
    return spec[:(M + 255) // 256]


def operands(M, K, b, variant, seed):
    """Rows scaled 2^-20 .. 2^20 against each other and 2^-12 .. 2^-1/2 inside a row, both signs; entries outside a row block's live K
    blocks are 2^-(b + 20) of that: not zero in Float64, zero once truncated.  Plus, in the first row block: an all-zero row, a NaN
    row, and a 16-row piece that is dead in a K block where the other rows of the block are live."""
    rng = np.random.default_rng(seed)
    nk = K // 128
    q = rng.integers(-20, 21, size=M)
    U = rng.choice([-1.0, 1.0], size=(M, K)) * np.exp2(-rng.uniform(0.5, 12, size=(M, K)))
    spec = pattern(M, nk, variant)
    for r, s in enumerate(spec):
        rows = slice(256 * r, min(256 * r + 256, M))
        for k in range(nk):
            if k not in s["live"]:
                U[rows, 128 * k:128 * k + 128] *= 2.0 ** -(b + 20)
        if s["gone"] is not None or s["kept"] is not None:
            first = 128 * min(s["live"])
            U[rows, first + 17] = -1.0                                     # the row maximum, an exact power of two: e_i = q_i
        if s["gone"] is not None:
            U[rows, 128 * s["gone"]:128 * s["gone"] + 128] = 0.0
            U[rows, 128 * s["gone"] + 3] = 2.0 ** -(b + 1)                 # trunc(1 / 2) = 0, in every row of the block
        if s["kept"] is not None:
            U[rows, 128 * s["kept"]:128 * s["kept"] + 128] = 0.0
            U[256 * r + 3, 128 * s["kept"] + 127] = -(2.0 ** -(b - 1))     # trunc(-2) = -2, in one row
    live0 = sorted(spec[0]["live"])
    if len(live0) > 1:
        U[PIECE.start:PIECE.stop, 128 * live0[0]:128 * live0[0] + 128] *= 2.0 ** -(b + 20)
    A = U * np.exp2(q)[:, None]
    A[ZERO_ROW] = 0.0
    A[NAN_ROW, 128 * live0[-1] + 9] = np.nan
    return A, spec


_CASES = {}


def case(lmm, M, N, K, nmod):
    """(A, minus the host-emulated A A[:N]', the live pattern), computed once per case and left unchanged."""
    key = (M, N, K, nmod)
    if key not in _CASES:
        lib = lmm.load()
        nk = K // 128
        variant = (nk + nmod // 8 + M // 256) % 3                         # every variant occurs at both shapes and both nmod
        b = bit_budget(lmm, nmod, K)
        A, spec = operands(M, K, b, variant, M + N + K + nmod)
        live = live_blocks(A, b)
        for r, s in enumerate(spec):                                      # the operands do have the pattern they are meant to have
            want_live = set(s["live"]) | ({s["kept"]} if s["kept"] is not None else set())
            assert {k for k in range(nk) if live[r][k]} == want_live, (r, live[r], want_live)
        Af, Bf = np.asfortranarray(A), np.asfortranarray(A[:N])
        out = np.zeros((M, N), order="F")
        lib.lmm_dev_emul_host.restype = C.c_int
        rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), M, Bf.ctypes.data_as(DP), N, M, N, K, nmod, K, out.ctypes.data_as(DP), M, None)
        assert rc == 0, lib.lmm_last_error_string()
        want = -out
        want.setflags(write=False)
        A.setflags(write=False)
        _CASES[key] = (A, want, live, variant)
    return _CASES[key]


def run_syrk(lmm, A, N, nmod=16, pad_a=3, pad_c=5):
    """tests/test_gpu_emul_exact.py's: C (zero on and below the diagonal, CANARY elsewhere) after lmm_dev_syrk_emul, lda = M + pad_a
    (NaN in the pad rows), ldc = M + pad_c: (the M x N block, everything else of the buffer, the lower mask)."""
    import torch
    lib = lmm.load()
    M, K = A.shape
    lda, ldc = M + pad_a, M + pad_c
    Ah = np.full((K, lda), np.nan)
    Ah[:, :M] = A.T
    Ch = np.full((N, ldc), CANARY)
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    Ch[:, :M][lower.T] = 0.0
    At, Ct = torch.from_numpy(Ah).cuda(), torch.from_numpy(Ch).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_syrk_emul(C.c_void_p(Ct.data_ptr()), ldc, C.c_void_p(At.data_ptr()), lda, M, N, K, nmod)
    assert rc == 0, lib.lmm_last_error_string()
    got = Ct.cpu().numpy()
    return got[:, :M].T, got[:, M:], lower


def same_bits(got, want, where):
    """entries of `where` that differ in any bit (a NaN for a NaN)"""
    return where & (got != want) & ~(np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("nmod", [8, 16])
@pytest.mark.parametrize("nk", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("M,N", [(320, 320), (768, 256)])
def test_patterned_operands_bit_for_bit(lmm, M, N, nk, nmod):
    """Every grid, skip on, against the host entry; and skip off once, against the same bits."""
    lib = lmm.load()
    K = 128 * nk
    A, want, live, variant = case(lmm, M, N, K, nmod)
    print(f"syrk_emul {M}x{N}x{K}, nmod = {nmod}, variant {variant}: live K blocks per 256-row block {[sum(r) for r in live]} of {nk}")
    assert np.isnan(want[NAN_ROW, 0]) and np.isnan(want[M - 1, NAN_ROW]) and not np.isnan(want[M - 1, 0])
    try:
        for on, grids in ((1, GRIDS), (0, (3,))):
            assert lib.lmm_dev_set_emul_zero_skip(on) == 0
            for wgs in grids:
                assert lib.lmm_dev_set_emul_gemm_workgroups(wgs) == 0
                got, pad, lower = run_syrk(lmm, A, N, nmod)
                assert np.all(pad == CANARY) and np.all(got[~lower] == CANARY)
                bad = same_bits(got, want, lower)
                assert not bad.any(), (on, wgs, int(bad.sum()), np.argwhere(bad)[:8])
                assert np.all(got[ZERO_ROW, :ZERO_ROW + 1] == 0.0)          # the all-zero row (column NAN_ROW lies right of its diagonal)
                assert np.all(np.isnan(got[NAN_ROW, :NAN_ROW + 1])) and np.all(np.isnan(got[NAN_ROW:, NAN_ROW]))
    finally:
        lib.lmm_dev_set_emul_zero_skip(-1)
        lib.lmm_dev_set_emul_gemm_workgroups(0)


def test_second_mask_word_on_against_off(lmm):
    """K = 8320: 65 K blocks, bit 0 of the second mask word.  Block 64 and two blocks of the first word are live, the others dead."""
    lib = lmm.load()
    M = N = 256
    K, nmod = 8320, 16
    b = bit_budget(lmm, nmod, K)
    rng = np.random.default_rng(8320)
    A = rng.choice([-1.0, 1.0], size=(M, K)) * np.exp2(-rng.uniform(0.5, 12, size=(M, K))) * np.exp2(rng.integers(-20, 21, size=(M, 1)))
    keep = np.zeros(K, dtype=bool)
    for k in (7, 63, 64):
        keep[128 * k:128 * k + 128] = True
    A[:, ~keep] *= 2.0 ** -(b + 20)
    live = live_blocks(A, b)
    assert [k for k in range(65) if live[0][k]] == [7, 63, 64]
    ref = -(A @ A[:N].T)                                                  # Float64: a coarse reference, to see that block 64 is in the product
    try:
        res = {}
        for on in (0, 1):
            assert lib.lmm_dev_set_emul_zero_skip(on) == 0
            res[on], pad, lower = run_syrk(lmm, A, N, nmod)
            assert np.all(pad == CANARY) and np.all(res[on][~lower] == CANARY)
    finally:
        lib.lmm_dev_set_emul_zero_skip(-1)
    assert np.array_equal(res[0].view(np.int64), res[1].view(np.int64))
    scale = np.abs(A).max(axis=1)[:, None] * np.abs(A[:N]).max(axis=1)[None, :]
    # Against Float64: the truncation is 4 K 2^-b < 1e-12 of amax_i amax_j, the Float64 dot product's rounding at most K u times the
    # 384 live terms < 4e-10; block 64 alone adds sum_k a_ik^2 > 1e-6 amax_i^2 to every diagonal entry, so leaving it out would show.
    assert np.all(np.abs(res[1] - ref)[lower] <= 1e-9 * scale[lower])
    assert np.all((A[:, 128 * 64:] ** 2).sum(axis=1) > 1e-6 * np.diag(scale))


# ---- one factorisation: n = 1152 and 64 rider rows, the rule scaled down so that its K = 640 update is emulated ----
RULE = (512, 256, 2.0e5)
N_FACT, RIDERS = 1152, 64


def matern52(x, ell):
    r = np.abs(x[:, None] - x[None, :]) / ell
    return (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)


def factor_inputs(decaying):
    rng = np.random.default_rng(1152 + decaying)
    x = np.linspace(0.0, 1.0, N_FACT)
    Kmat = matern52(x, 0.02 if decaying else 50.0) + 0.1 * np.eye(N_FACT)
    R = rng.standard_normal((RIDERS, N_FACT))
    return Kmat, R


def potrf(lmm, Kmat, R):
    """(factor with the rider rows below it, info) from lmm_dev_potrf"""
    import torch
    lib = lmm.load()
    n, nr = Kmat.shape[0], Kmat.shape[0] + R.shape[0]
    full = np.vstack([np.tril(Kmat), R])                                  # nr x n
    A = torch.from_numpy(np.ascontiguousarray(full.T)).cuda()             # [col][row], ld = nr
    W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), nr, n, nr, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0, lib.lmm_last_error_string()
    out = A.cpu().numpy().T
    return out, int(info.item())


def emulated_updates(lmm, NR, NC):
    lib = lmm.load()
    out = (C.c_longlong * (2 + 6 * 64))()
    n = lib.lmm_dev_emul_plan(NR, NC, 1, out, 64)
    assert 0 <= n <= 64
    return [tuple(out[2 + 6 * i: 5 + 6 * i]) for i in range(n) if out[2 + 6 * i + 3]]


@pytest.mark.parametrize("decaying", [1, 0])
def test_factorisation_same_with_skip_on_and_off(lmm, decaying):
    """The factor (rider rows included) is identical with the skip on and off; it matches LAPACK within the bars of
    test_factorisation_emulated_against_f64_and_oracle (1e-9 relative, and no worse than twice the f64 kernels' own error); and a matrix
    that is not positive definite reports the same pivot either way."""
    import scipy.linalg as sla
    lib = lmm.load()
    Kmat, R = factor_inputs(decaying)
    L = np.linalg.cholesky(Kmat)
    want = np.vstack([L, sla.solve_triangular(L, R.T, lower=True).T])
    tri = np.vstack([np.tril(np.ones((N_FACT, N_FACT), dtype=bool)), np.ones((RIDERS, N_FACT), dtype=bool)])
    bad_at = 1100
    Kbad = Kmat.copy()
    Kbad[bad_at, bad_at] = -5.0
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64, info = potrf(lmm, Kmat, R)
        assert info == 0
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
        assert lib.lmm_dev_set_f64_emul_rule(*RULE) == 0
        ups = emulated_updates(lmm, N_FACT + RIDERS, N_FACT)
        assert (N_FACT + RIDERS - 640, 512, 640) in ups, ups              # the K = 640 update above the failing pivot is emulated
        got, pivots = {}, {}
        for on in (1, 0):
            assert lib.lmm_dev_set_emul_zero_skip(on) == 0
            got[on], info = potrf(lmm, Kmat, R)
            assert info == 0
            _, pivots[on] = potrf(lmm, Kbad, R)
    finally:
        lib.lmm_dev_set_emul_zero_skip(-1)
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
        lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0)
    assert np.array_equal(got[1][tri].view(np.int64), got[0][tri].view(np.int64))
    assert pivots == {1: bad_at + 1, 0: bad_at + 1}
    nrm = np.linalg.norm(want[tri])
    e_emu, e_f64 = np.linalg.norm((got[1] - want)[tri]) / nrm, np.linalg.norm((f64 - want)[tri]) / nrm
    b = bit_budget(lmm, 16, 640)
    panel = got[1][640:, :640]
    dead = [sum(1 for v in row if not v) for row in live_blocks(panel, b)]
    print(f"decaying = {decaying}: |emulated - LAPACK| / |LAPACK| = {e_emu:.3e}, f64 kernels {e_f64:.3e}; dead K blocks of 5 per 256-row block of the K = 640 panel: {dead}")
    assert e_emu <= 1e-9
    assert e_emu <= 2.0 * e_f64
    assert (sum(dead) > 0) == bool(decaying)                              # the decaying matrix does have blocks to skip, the other none
