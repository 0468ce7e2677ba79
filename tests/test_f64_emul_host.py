"""CPU checks of the int8 modular emulation of Float64 products against Python integers, through the host-only entry
lmm_dev_emul_host: it runs row scaling, residues and the CRT combine with the constants and scalar steps the GPU kernels use."""
import ctypes as C
import math

import numpy as np
import pytest

import lmm_amd
from lmm_amd import _lib as L

DP = C.POINTER(C.c_double)


def emul(A, B, k_bound, nmod=16):
    """(emulated A B', consts) for row-major A (M x K), B (N x K)."""
    lib = lmm_amd.load()
    M, K = A.shape
    N = B.shape[0]
    Af, Bf = np.asfortranarray(A, dtype=np.float64), np.asfortranarray(B, dtype=np.float64)
    out = np.zeros((M, N), order="F")
    consts = np.zeros(68)
    lib.lmm_dev_emul_host.restype = C.c_int
    rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), M, Bf.ctypes.data_as(DP), N, M, N, K, nmod, k_bound, out.ctypes.data_as(DP), M,
                               consts.ctypes.data_as(DP))
    assert rc == L.LMM_OK
    return out, consts


def constants(nmod=16, k_bound=1):
    _, c = emul(np.ones((1, 1)), np.ones((1, 1)), k_bound, nmod)
    p = [int(v) for v in c[:nmod]]
    w = [int(c[16 + t]) + int(c[32 + t]) + int(c[48 + t]) for t in range(nmod)]
    P = int(c[64]) + int(c[65]) + int(c[66])
    return p, w, P, int(c[67]), c


def truncated(X, b):
    """Python-integer rows a' = trunc(a 2^(b - e)), e = ceil(log2 max |a|), and the exponents e (None for an all-zero row)."""
    rows, es = [], []
    for r in X:
        amax = float(np.max(np.abs(r)))
        if amax == 0.0:
            rows.append([0] * len(r)); es.append(None); continue
        f, q = math.frexp(amax)
        e = q - 1 if f == 0.5 else q
        rows.append([int(math.ldexp(float(a), b - e)) for a in r]); es.append(e)
    return rows, es


def check_exact(A, B, k_bound, ulps=2):
    out, c = emul(A, B, k_bound)
    b = int(c[67])
    ra, ea = truncated(A, b)
    rb, eb = truncated(B, b)
    worst = 0.0
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            if ea[i] is None or eb[j] is None:
                assert out[i, j] == 0.0
                continue
            dot = sum(x * y for x, y in zip(ra[i], rb[j]))
            want = math.ldexp(float(dot), ea[i] + eb[j] - 2 * b)      # int -> float is correctly rounded, the scaling exact
            err = abs(out[i, j] - want)
            assert err <= ulps * math.ulp(want), (i, j, out[i, j], want)
            if want != 0.0:
                worst = max(worst, err / math.ulp(want))
    return worst


def test_moduli_are_pairwise_coprime_and_the_largest():
    p, _, P, _, _ = constants()
    assert p == [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193]
    for s in range(16):
        for t in range(s + 1, 16):
            assert math.gcd(p[s], p[t]) == 1
    assert P == math.prod(p) and 125.0 < math.log2(P) < 126.0


@pytest.mark.parametrize("nmod", [8, 14, 15, 16])
def test_chunked_weights_sum_to_the_crt_weights(nmod):
    p, w, P, _, c = constants(nmod)
    assert P == math.prod(p)
    for t in range(nmod):
        assert 0 < w[t] < P
        for s in range(nmod):
            assert w[t] % p[s] == (1 if s == t else 0)
        # the chunks are cut at bits 85 and 44: exact in Float64, and the first two are multiples of their cut
        assert int(c[16 + t]) % (1 << 85) == 0 and int(c[32 + t]) % (1 << 44) == 0 and int(c[32 + t]) < (1 << 85) and int(c[48 + t]) < (1 << 44)


def test_dot_products_are_determined_by_their_residues_for_every_depth():
    for nmod in (14, 15, 16):
        p = constants(nmod)[0]
        P = math.prod(p)
        for K in list(range(128, 16384 + 1, 128)):
            b = constants(nmod, K)[3]
            assert b <= 58 and 2 * P > 4 * K * (1 << (2 * b)), (nmod, K, b)      # P / 2 > K 2^(2b)
            assert b == 58 or 2 * P <= 4 * K * (1 << (2 * (b + 1)))              # and b is the largest such
    assert constants(16, 8192)[3] == 55 and constants(16, 2048)[3] == 56


def test_random_products_with_per_row_dynamic_range():
    rng = np.random.default_rng(1)
    for (M, N, K) in [(64, 64, 256), (7, 5, 33), (1, 64, 128)]:
        A = rng.standard_normal((M, K)) * np.exp2(rng.integers(-40, 40, size=(M, 1)))
        B = rng.standard_normal((N, K)) * np.exp2(rng.integers(-40, 40, size=(N, 1)))
        check_exact(A, B, 8192)


def test_zero_rows_and_rows_spanning_sixty_binades():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((16, 64)) * np.exp2(-rng.uniform(0, 60, size=(16, 64)))
    A[:, 0] = 1.0                                     # 2^-60 ... 1 inside every row
    B = rng.standard_normal((12, 64)) * np.exp2(-rng.uniform(0, 60, size=(12, 64)))
    A[3] = 0.0
    B[5] = 0.0
    check_exact(A, B, 8192)
    out, _ = emul(A, B, 8192)
    assert np.all(out[3] == 0.0) and np.all(out[:, 5] == 0.0)


def test_residue_extremes():
    """Entries x 2^-b with the row maximum 1 truncate to the integer x: x = +-128 (residue -128 modulo 256), +-127, and x with residues
    at both ends of every modulus's symmetric range."""
    p, _, _, b, _ = constants(16, 8192)
    xs = [128, -128, 127, -127, 384, -384, 1 << b, -(1 << b), (1 << b) - (1 << 8)]      # (every x has at most 53 significant bits)
    for q in p:
        xs += [q // 2, -(q // 2), q // 2 + q * 12345, (q - 1) // 2 + q * 99, -((q - 1) // 2) - q * 77]
    K = len(xs) + 1
    A = np.zeros((3, K))
    A[0, :-1] = [math.ldexp(x, -b) for x in xs]
    A[1, :-1] = [math.ldexp(-x, -b) for x in xs]
    A[2, :-1] = [math.ldexp(x, -b) for x in reversed(xs)]
    A[:, -1] = 1.0
    ra, _ = truncated(A, b)
    assert ra[0][:-1] == xs
    check_exact(A, A, 8192)


def test_sums_near_plus_and_minus_half_the_modulus_product():
    """K = 256, b = 58: rows of +-1 give dot products of +-K 2^(2b) = 0.76 P / 2, the largest |sum| / (P / 2) a depth can reach."""
    p, _, P, b, _ = constants(16, 256)
    assert b == 58 and 0.7 < 256 * (1 << (2 * b)) / (P / 2) < 1.0
    A = np.ones((2, 256))
    A[1] = -1.0
    A[1, ::7] = -0.999
    check_exact(A, A, 256)
    out, _ = emul(A, A, 256)
    assert out[0, 0] == 256.0 and out[0, 1] < -255.0 and out[1, 0] == out[0, 1]


def test_non_finite_rows_give_nan():
    A = np.ones((3, 8))
    A[1, 2] = np.nan
    A[2, 3] = np.inf
    out, _ = emul(A, A, 128)
    assert out[0, 0] == 8.0 and np.isnan(out[1]).all() and np.isnan(out[:, 1]).all() and np.isnan(out[2]).all()
