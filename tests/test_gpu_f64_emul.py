"""GPU checks of the int8 modular emulation of the large Float64 Cholesky updates: the update kernels through
lmm_dev_syrk_emul against a host long-double product, and the factorisation with several emulated levels against the f64 path and
the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import lmm_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 128), (320, 192, 384), (576, 320, 640)]     # one tile; ragged 64-row / 64-column edges of 256 tiles; K = 3, 5 K tiles


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


def operands(M, N, K, seed):
    """Asymmetric data with a per-row dynamic range (2^-20 .. 2^20 between rows, 2^-12 .. 1 inside a row), and a C of the product's size."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) * np.exp2(rng.integers(-20, 21, size=(M, 1))) * np.exp2(-rng.uniform(0, 12, size=(M, K)))
    amax = np.abs(A).max(axis=1)
    C0 = rng.standard_normal((M, N)) * math.sqrt(K) * np.outer(amax, amax[:N])
    return A, C0, amax


_REF = {}


def reference(M, N, K):
    """(A, C0, amax, C0 - A A[:N]' in long double), computed once per shape."""
    if (M, N, K) not in _REF:
        A, C0, amax = operands(M, N, K, M + N + K)
        Al = A.astype(np.longdouble)
        _REF[(M, N, K)] = (A, C0, amax, C0.astype(np.longdouble) - Al @ Al[:N].T)
    return _REF[(M, N, K)]


def run_syrk(lmm, A, C0, nmod=16):
    import torch
    lib = lmm.load()
    M, K = A.shape
    N = C0.shape[1]
    At = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()          # (K, M) row-major = M x K column-major, lda = M
    Ct = torch.from_numpy(np.ascontiguousarray(C0.T)).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_syrk_emul(C.c_void_p(Ct.data_ptr()), M, C.c_void_p(At.data_ptr()), M, M, N, K, nmod)
    assert rc == 0, lib.lmm_last_error_string()
    return Ct.cpu().numpy().T


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_syrk_emul_against_long_double(lmm, M, N, K):
    """|err_ij| <= 4 K 2^-b amax_i amax_j + 4 u |C_ij| (truncation of both operands to b bits below their row's power of two, one
    rounding of the reconstructed integer and one of the subtraction), for i >= j; entries with i < j are not written."""
    A, C0, amax, want = reference(M, N, K)
    got = run_syrk(lmm, A, C0)
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    assert np.array_equal(got[~lower], C0[~lower])                  # canaries above the diagonal
    b = min(58, math.floor((math.log2(math.prod([256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193])) - 1 - math.log2(K)) / 2))
    u = 2.0 ** -53
    bound = 4.0 * K * 2.0 ** -b * np.outer(amax, amax[:N]) + 4.0 * u * np.abs(want).astype(np.float64)
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f"syrk_emul {M}x{N}x{K}: b = {b}, worst err / bound = {np.max(err[lower] / bound[lower]):.3f}")
    assert np.all(err[lower] <= bound[lower])
    assert np.array_equal(run_syrk(lmm, A, C0), got)                # integer sums: bit-identical runs


def test_syrk_emul_nan_row(lmm):
    M, N, K = 320, 192, 384
    A, C0, _, _ = reference(M, N, K)
    A = A.copy()
    r = 70
    A[r, 5] = np.nan
    got = run_syrk(lmm, A, C0)
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    hit = np.zeros((M, N), dtype=bool)
    hit[r, :] = True
    hit[:, r] = True
    assert np.array_equal(np.isnan(got), hit & lower)


def _logpdf(lmm, P, m, p):
    import torch
    fs = lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel()) for _ in range(m)])
    fx = lmm.ILMM(fs, lmm.Orthogonal(P["U"], P["S"]))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(P["x"]).cuda(), p), 0.1)
    return float(lmm.logpdf(fx, torch.from_numpy(P["y"]).cuda()))


@pytest.mark.parametrize("n,m", [(1100, 3), (2304, 2)])
def test_factorisation_emulated_against_f64_and_oracle(lmm, n, m):
    """logpdf with every update of K >= 256 emulated, against the f64 path and the oracle's LAPACK factorisation: the emulated path's
    error is at most twice the f64 path's on the same problem and at most 1e-9 relative.  n = 1100 (1152 columns = 640 | 512, the halves
    one region launch each) has one emulated update per latent, K = 640; n = 2304 has three (K = 640, 1152, 640)."""
    lib = lmm.load()
    p = m + 2
    P = O.synthetic_problem(m, p, n, "matern52", True, s2=0.1, seed=n + m)
    want = O.oilmm_logpdf(P["gps"], P["U"], P["S"], P["x"], 0.1, P["y"])
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = _logpdf(lmm, P, m, p)
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        emu = _logpdf(lmm, P, m, p)
        again = _logpdf(lmm, P, m, p)
    finally:
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
    e_f64, e_emu = abs(f64 - want) / abs(want), abs(emu - want) / abs(want)
    print(f"n = {n}, m = {m}: |f64 - oracle| / |oracle| = {e_f64:.3e}, |emulated - oracle| / |oracle| = {e_emu:.3e}, "
          f"|emulated - f64| / |oracle| = {abs(emu - f64) / abs(want):.3e}")
    assert e_emu <= 1e-9
    assert e_emu <= 2.0 * e_f64
    assert again == pytest.approx(emu, rel=1e-12)


def test_batches_of_one_stream_share_the_scratch(lmm):
    """160 latents at n = 1100 are five lock-step batches of 32 on four streams: one stream factors two batches through the same
    scratch block, one after the other.  Every latent has its own mixing scale S, hence its own noise level and matrix, so a batch that
    read another's residues would show."""
    import torch
    lib = lmm.load()
    m, n = 160, 1100
    p = m
    rng = np.random.default_rng(11)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    y = rng.standard_normal(n * p)
    fs = lmm.independent_mogp([lmm.GP(lmm.Matern52Kernel()) for _ in range(m)])
    fx = lmm.ILMM(fs, lmm.Orthogonal(np.eye(p), 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p), 0.1)
    yt = torch.from_numpy(y).cuda()
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = float(lmm.logpdf(fx, yt))
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        emu = float(lmm.logpdf(fx, yt))
    finally:
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
    print(f"160 latents: |emulated - f64| / |f64| = {abs(emu - f64) / abs(f64):.3e}")
    assert emu == pytest.approx(f64, rel=1e-12)      # both are a few ulp from the exact value (the tests above); a wrong batch is off by far more


def test_not_pd_reports_the_same_pivot(lmm):
    """A well conditioned matrix with one diagonal entry made negative: that pivot fails whatever the rounding of the updates before
    it; the emulated and the f64 path both report it.  n = 2304 splits as 1152 | 1152 and each half as 640 | 512, so pivot 2201 comes
    after three emulated updates (K = 640, 1152, 640)."""
    import torch
    lib = lmm.load()
    n, bad = 2304, 2200
    rng = np.random.default_rng(5)
    G = rng.standard_normal((n, n + 8))
    Kmat = G @ G.T / n + 0.5 * np.eye(n)
    Kmat[bad, bad] = -5.0
    info_seen = []
    try:
        for on in (0, 1):
            assert lib.lmm_dev_set_f64_emul(on, 256, 16) == 0
            A = torch.from_numpy(np.tril(Kmat).T.copy()).cuda()      # [col][row], ld = n
            W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), n, n, n, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0
            info_seen.append(int(info.item()))
    finally:
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
    assert info_seen == [bad + 1, bad + 1]
