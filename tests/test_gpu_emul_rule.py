"""GPU checks of what decides and drives the int8-emulated updates: a factorisation in which the shape rule sends one
of two updates of the same K to the emulation and the other to the f64 kernel, the batch walked in groups of several sizes, and the
combine at a shape whose grid has workgroups above, across and below the diagonal, bit for bit against the host entry."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
CANARY = 7.25
# n = 2304: 1152 | 1152, each half 640 | 512.  The K = 640 updates have 512 columns and 1728 / 576 rows with the riders' 64-row block
# (1664 / 512 without it, lmm_dev_potrf): 753920 / 164096 outputs per matrix (721152 / 131328).  Two latents per batch and 4e5 outputs
# put the tall one above the bar and the short one below it, as does one matrix; the K = 1152 update between them is always emulated.
RULE = (1152, 640, 4.0e5)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    lib.lmm_dev_emul_plan.restype = C.c_int
    lib.lmm_dev_set_f64_emul_rule.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.lmm_dev_set_f64_emul_rule.restype = C.c_int
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    return lmm_amd


def reset(lib):
    lib.lmm_dev_set_f64_emul(-1, 0, 0)
    lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0)
    lib.lmm_dev_set_emul_group(0)


def plan(lib, NR, NC, nb, cap=256):
    out = (C.c_longlong * (2 + 6 * cap))()
    n = lib.lmm_dev_emul_plan(NR, NC, nb, out, cap)
    assert 0 <= n <= cap, lib.lmm_last_error_string()
    return [tuple(out[2 + 6 * i: 8 + 6 * i]) for i in range(n)]


def _logpdf(lmm, P, m, p):
    import torch
    fs = lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel()) for _ in range(m)])
    fx = lmm.ILMM(fs, lmm.Orthogonal(P["U"], P["S"]))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(P["x"]).cuda(), p), 0.1)
    return float(lmm.logpdf(fx, torch.from_numpy(P["y"]).cuda()))


def test_mixed_levels_against_f64_and_oracle(lmm):
    """Among the two K = 640 updates exactly the tall one is emulated (and the K = 1152 update between them); the bars are those of
    test_factorisation_emulated_against_f64_and_oracle."""
    lib = lmm.load()
    n, m = 2304, 2
    p = m + 2
    P = O.synthetic_problem(m, p, n, "matern52", True, s2=0.1, seed=n + m)
    want = O.oilmm_logpdf(P["gps"], P["U"], P["S"], P["x"], 0.1, P["y"])
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = _logpdf(lmm, P, m, p)
        reset(lib)
        assert lib.lmm_dev_set_f64_emul_rule(*RULE) == 0
        big = {(M, N, K): em for M, N, K, em, *_ in plan(lib, n + 64, n, m) if K >= 640}
        assert big == {(1728, 512, 640): 1, (1216, 1152, 1152): 1, (576, 512, 640): 0}
        emu = _logpdf(lmm, P, m, p)
        again = _logpdf(lmm, P, m, p)
    finally:
        reset(lib)
    e_f64, e_emu = abs(f64 - want) / abs(want), abs(emu - want) / abs(want)
    print(f"n = {n}, m = {m}, mixed levels: |f64 - oracle| / |oracle| = {e_f64:.3e}, |emulated - oracle| / |oracle| = {e_emu:.3e}, "
          f"|emulated - f64| / |oracle| = {abs(emu - f64) / abs(want):.3e}")
    assert e_emu <= 1e-9
    assert e_emu <= 2.0 * e_f64
    assert again == pytest.approx(emu, rel=1e-12)


def test_mixed_levels_report_the_failing_pivot(lmm):
    """The matrix of test_not_pd_reports_the_same_pivot under the same rule: pivot 2201 comes after an emulated K = 640 update, the
    emulated K = 1152 update and an f64 K = 640 update."""
    import torch
    lib = lmm.load()
    n, bad = 2304, 2200
    rng = np.random.default_rng(5)
    G = rng.standard_normal((n, n + 8))
    Kmat = G @ G.T / n + 0.5 * np.eye(n)
    Kmat[bad, bad] = -5.0
    try:
        reset(lib)
        assert lib.lmm_dev_set_f64_emul_rule(*RULE) == 0
        big = {(M, N, K): em for M, N, K, em, *_ in plan(lib, n, n, 1) if K >= 640}
        assert big == {(1664, 512, 640): 1, (1152, 1152, 1152): 1, (512, 512, 640): 0}
        A = torch.from_numpy(np.tril(Kmat).T.copy()).cuda()      # [col][row], ld = n
        W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), n, n, n, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0
        assert int(info.item()) == bad + 1
    finally:
        reset(lib)


def test_group_sizes_agree(lmm):
    """12 latents with distinct mixing scales at n = 1100 are one lock-step batch; its emulated updates walk it in groups of 1, of 4, of
    5 (5 + 5 + 2: a ragged last group) and of as many as the scratch block holds.  A group that read another's residues or scales would
    be off by far more than the tolerance of test_batches_of_one_stream_share_the_scratch."""
    import torch
    lib = lmm.load()
    m, n = 12, 1100
    p = m
    rng = np.random.default_rng(12)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    y = rng.standard_normal(n * p)
    fs = lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel()) for _ in range(m)])
    fx = lmm.ILMM(fs, lmm.Orthogonal(np.eye(p), 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p), 0.1)
    yt = torch.from_numpy(y).cuda()
    vals = {}
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = float(lmm.logpdf(fx, yt))
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        for g in (1, 4, 5, 0):
            assert lib.lmm_dev_set_emul_group(g) == 0
            groups = {r[4] for r in plan(lib, 1152 + 64, 1152, m) if r[3]}
            assert groups and all((1 <= s <= g) if g else (4 <= s <= m) for s in groups)
            vals[g] = float(lmm.logpdf(fx, yt))
    finally:
        reset(lib)
    print("12 latents, groups of 1 / 4 / 5 / default: " + ", ".join(f"{abs(v - f64) / abs(f64):.3e}" for v in vals.values()) + " from f64")
    for g, v in vals.items():
        assert v == pytest.approx(f64, rel=1e-12), g
        assert v == pytest.approx(vals[1], rel=1e-12), g


# ---- the combine's grid: operands and helpers as in tests/test_gpu_emul_persistent.py ----
def operands(M, K, seed):
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


@pytest.mark.parametrize("M,N", [(1100, 1100), (1100, 600)])
def test_combine_grid_bit_for_bit(lmm, M, N):
    """Rows come in chunks of 1024.  1100 x 1100: the chunk of rows 0 .. 1023 has no work in the columns 1024 .. 1099 (workgroups
    wholly above the diagonal), the chunk of rows 1024 .. 1099 is ragged and reaches the diagonal in those columns only partly covered.
    1100 x 600: the columns end before the second chunk begins, which then lies wholly below the diagonal."""
    K = 128
    A, want = case(lmm, M, N, K)
    got, pad, lower = run_syrk(lmm, A, N)
    assert np.all(pad == CANARY) and np.all(got[~lower] == CANARY)      # nothing outside i >= j is written
    bad = lower & (got != want)
    print(f"syrk_emul {M}x{N}x{K}: {int(bad.sum())} of {int(lower.sum())} entries differ")
    assert not bad.any(), np.argwhere(bad)[:8]
    assert np.all(got[5, :6] == 0.0) and np.all(got[5:, 5] == 0.0)      # the all-zero row
