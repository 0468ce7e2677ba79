"""Host-only check of the int8 emulation's screen predicate (DESIGN.md 4.17 "negligible tiles", emul_negligible in csrc/lmm_emul.h).
lmm_dev_emul_negligible runs the library's own predicate; exact rational arithmetic (fractions.Fraction) is the reference: whenever
the predicate says "negligible", the correctly rounded C - T has the bits of C for T = +-K 2^(e_i + e_j) (1 + 2^-52), the largest
update the GEMM and the combine can form for rows with the exponents e_i, e_j.  No GPU."""
import ctypes as C
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from lmm_amd import _lib as L

DP = C.POINTER(C.c_double)
MARGIN = 56
KS = [128, 256, 384, 640, 1024, 1152, 2048, 4096, 8192, 12288, 16384]


@pytest.fixture(scope="module")
def lib():
    lib = L.load()
    lib.lmm_dev_emul_negligible.argtypes = [C.c_int, DP, DP, DP, C.c_int, C.POINTER(C.c_int)]
    lib.lmm_dev_emul_negligible.restype = C.c_int
    return lib


def negligible(lib, K, ri, rj, c):
    ri, rj, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.broadcast(ri, rj, c).shape)).ravel() for v in (ri, rj, c))
    out = np.full(c.size, -1, dtype=np.int32)
    rc = lib.lmm_dev_emul_negligible(K, ri.ctypes.data_as(DP), rj.ctypes.data_as(DP), c.ctypes.data_as(DP), c.size, out.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def row_exp(a):      # ceil(log2 a) for a finite a > 0, in integers
    m, q = math.frexp(a)
    return q - 1 if m == 0.5 else q


def clog2(K):
    return (K - 1).bit_length()


def bits(x):
    return struct.pack("<d", x)


def keeps_bits(K, ei, ej, c):
    """fl(c - T) has the bits of c for both signs of T = K 2^(ei + ej) (1 + 2^-52), in exact arithmetic rounded once."""
    T = Fraction(K) * Fraction(2) ** (ei + ej) * (1 + Fraction(1, 2 ** 52))
    return all(bits(float(Fraction(c) - s * T)) == bits(c) for s in (1, -1))


def pow2(e):
    return math.ldexp(1.0, e)


def rows_for(rng, e):
    """a row maximum with ceil(log2) = e: the power of two itself or something in (2^(e - 1), 2^e)"""
    return pow2(e) if rng.random() < 0.3 else float(np.nextafter(pow2(e - 1), np.inf)) + rng.random() * (pow2(e) - pow2(e - 1)) * 0.999


def test_python_rounding_is_the_reference():
    # float(Fraction) rounds to nearest, ties to even, subnormals included: the reference this file leans on
    assert float(Fraction(1) + Fraction(1, 2 ** 53)) == 1.0 and float(Fraction(1) + Fraction(3, 2 ** 54)) == 1.0 + 2.0 ** -52
    assert float(Fraction(1) - Fraction(1, 2 ** 54)) == 1.0 and float(Fraction(1) - Fraction(1, 2 ** 54) - Fraction(1, 2 ** 80)) == 1.0 - 2.0 ** -53
    assert float(Fraction(3, 2 ** 1075)) == 2 * 5e-324 and float(Fraction(1, 2 ** 1075)) == 0.0
    assert not keeps_bits(128, 0, 0, pow2(7 + 53)) and keeps_bits(128, 0, 0, pow2(7 + 55))


def test_random_cases_negligible_implies_unchanged(lib):
    rng = np.random.default_rng(20)
    seen = {True: 0, False: 0}
    for K in KS:
        ei = rng.integers(-80, 80, size=160)
        ej = rng.integers(-80, 80, size=160)
        off = rng.integers(-4, 5, size=160)      # binades of C around the threshold
        ri = np.array([rows_for(rng, int(e)) for e in ei])
        rj = np.array([rows_for(rng, int(e)) for e in ej])
        q = clog2(K) + ei + ej + MARGIN + off
        c = np.ldexp(1.0 + rng.random(160), q) * rng.choice([-1.0, 1.0], size=160)
        c[::7] = np.ldexp(1.0, q[::7])      # exact powers of two among them
        neg = negligible(lib, K, ri, rj, c)
        for t in range(160):
            assert row_exp(ri[t]) == ei[t] and row_exp(rj[t]) == ej[t]
            assert neg[t] == (off[t] >= 0), (K, ei[t], ej[t], c[t])      # the rule as stated: bound <= ilogb(C)
            if neg[t]:
                assert keeps_bits(K, int(ei[t]), int(ej[t]), float(c[t])), (K, ei[t], ej[t], c[t])
            seen[bool(neg[t])] += 1
    assert seen[True] > 500 and seen[False] > 500


@pytest.mark.parametrize("K", KS)
def test_power_of_two_and_its_neighbours_at_the_threshold(lib, K):
    for ei, ej in [(0, 0), (-3, 7), (40, -90), (-500, -500), (400, 500)]:
        bound = clog2(K) + ei + ej + MARGIN
        if not -1022 < bound < 1022:
            continue
        for dq, want in [(0, True), (1, True), (-1, False)]:      # at the threshold, one binade above it, one below
            p = pow2(bound + dq)
            below, above = float(np.nextafter(p, 0.0)), float(np.nextafter(p, np.inf))
            for sign in (1.0, -1.0):
                got = negligible(lib, K, pow2(ei), pow2(ej), np.array([p, above, below]) * sign)
                # the lower neighbour of a power of two is one binade down
                assert list(got) == [want, want, dq == 1], (K, ei, ej, dq, sign, got)
                for c, g in zip((p, above, below), got):
                    if g:
                        assert keeps_bits(K, ei, ej, sign * c), (K, ei, ej, c)
        # the rule is not loose by more than its stated slack: K > 2^(L - 1), so T exceeds half the gap below 2^(bound - 3)
        assert not keeps_bits(K, ei, ej, pow2(bound - 3))


def test_subnormal_and_largest_c(lib):
    tiny = 5e-324
    for K in (128, 4096, 16384):
        Lk = clog2(K)
        # subnormal C: ilogb of the value, -1074 .. -1023
        for m, q in [(1, -1074), (2, -1073), (3, -1073), (2 ** 51, -1023), (2 ** 52 - 1, -1023)]:
            c = m * tiny
            assert math.frexp(c)[1] - 1 == q
            for d, want in [(0, True), (1, False)]:
                e_sum = q - MARGIN - Lk + d
                ei = e_sum // 2
                ej = e_sum - ei
                for sign in (1.0, -1.0):
                    got = negligible(lib, K, pow2(ei), pow2(ej), sign * c)[0]
                    assert got == want, (K, m, d, sign)
                    if got:
                        assert keeps_bits(K, ei, ej, sign * c)
        # subnormal row maxima: any finite non-zero C is far above the update
        for c in (tiny, -tiny, 1.0, 2.2250738585072014e-308, -1.7976931348623157e308):
            assert negligible(lib, K, tiny, 3 * tiny, c)[0]
            assert keeps_bits(K, -1074, row_exp(3 * tiny), c)
        # the largest finite C
        big = 1.7976931348623157e308
        e_sum = 1023 - MARGIN - Lk
        for d, want in [(0, True), (1, False)]:
            ei, ej = 300, e_sum - 300 + d
            for sign in (1.0, -1.0):
                got = negligible(lib, K, pow2(ei), pow2(ej), sign * big)[0]
                assert got == want
                if got:
                    assert keeps_bits(K, ei, ej, sign * big)


def test_special_values(lib):
    inf, nan = math.inf, math.nan
    for K in (128, 1152, 16384):
        # +-0, +-inf and NaN in C are never negligible, not even under all-zero rows
        for ri, rj in [(1.0, 1.0), (0.0, 0.0), (0.0, 1.0), (1e-300, 1e-300), (5e-324, 5e-324)]:
            got = negligible(lib, K, ri, rj, np.array([0.0, -0.0, inf, -inf, nan, -nan]))
            assert not got.any(), (K, ri, rj, got)
        # a NaN or an infinity among a row's entries: never negligible, whatever C and the other row are
        for bad in (nan, inf, -inf, -nan):
            for other in (0.0, 1.0, 1e-300, 5e-324):
                for c in (1.0, -1e300, 1.7976931348623157e308, 5e-324):
                    assert not negligible(lib, K, bad, other, c)[0] and not negligible(lib, K, other, bad, c)[0]
        # an all-zero row: the update is exactly zero, every finite non-zero C is negligible; signs of the maxima are ignored
        for c in (1.0, -1.0, 5e-324, -5e-324, 1.7976931348623157e308, 2.0 ** -1022):
            assert negligible(lib, K, 0.0, 1e300, c)[0] and negligible(lib, K, 1e300, -0.0, c)[0] and negligible(lib, K, 0.0, 0.0, c)[0]
        assert negligible(lib, K, -1.0, -1.0, pow2(clog2(K) + MARGIN))[0] and not negligible(lib, K, -1.0, -1.0, pow2(clog2(K) + MARGIN - 1))[0]


def test_arguments(lib):
    a = np.ones(1)
    out = np.zeros(1, dtype=np.int32)
    p, op = a.ctypes.data_as(DP), out.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lmm_dev_emul_negligible(0, p, p, p, 1, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_negligible(16385, p, p, p, 1, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_negligible(128, p, p, p, -1, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_negligible(128, None, p, p, 1, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_negligible(128, p, p, p, 0, None) == 0


def test_not_vacuous_on_a_decaying_factor(lib):
    """Matern52 (lengthscale 1) on ordered inputs with the flagship's spacing (x_i = 20 i / 575), noise 0.05: the first block column
    of the factor, K = 512 wide, against the trailing matrix it updates.  A panel row's maximum decays with its distance d below the
    panel like exp(-sqrt(5) d / 28.75), an e-fold per 12.9 rows, and C_ij decays at the same rate in |i - j|; the bound asks for
    amax_i amax_j 2^(56 + 9) <= |C_ij|, i.e. 45 e-folds: (d_i + d_j) / 12.9 - 45 >= (d_i - d_j) / 12.9, so d_j >= ~290 rows -- the
    columns further than about 300 below the panel's edge are negligible whatever the row: ((1536 - 300) / 1536)^2 = 0.65 of the
    trapezoid.  The assertion asks for a half."""
    n, K = 2048, 512
    x = np.arange(n) * 20.0 / 575.0
    r = np.abs(x[:, None] - x[None, :])
    s = math.sqrt(5.0) * r
    Kmat = (1.0 + s + s * s / 3.0) * np.exp(-s) + 0.05 * np.eye(n)
    Lf = np.linalg.cholesky(Kmat)
    P = Lf[K:, :K]
    Cm = Kmat[K:, K:]
    amax = np.abs(P).max(axis=1)
    M = n - K
    ii, jj = np.tril_indices(M)
    c = Cm[ii, jj]
    neg = negligible(lib, K, amax[ii], amax[jj], c)
    # the same rule in NumPy
    e = np.array([row_exp(a) if a > 0 else 0 for a in amax])
    ref = (c != 0) & np.isfinite(c) & ((amax[ii] == 0) | (amax[jj] == 0) | (clog2(K) + e[ii] + e[jj] + MARGIN <= np.frexp(c)[1] - 1))
    assert np.array_equal(neg, ref)
    share = neg.mean()
    print(f"negligible outputs: {share:.3f} of {c.size}")
    assert share > 0.5
    # and the screened outputs do keep their bits under the f64 update
    T = (P @ P.T)[ii, jj]
    assert np.array_equal((c - T)[neg].view(np.uint64), c[neg].view(np.uint64))
