"""Host-only checks of the f64 update launches' screen (DESIGN.md 4.17 "the f64 kernel", csrc/lmm_emul.h): the predicate is the
emulation's (emul_negligible, margin 56), reached through lmm_dev_emul_negligible; what differs is the update it has to cover.  The
f64 MFMA kernel forms acc = sum_k a_ik a_jk with one rounding per term, |acc| <= K 2^(e_i + e_j) (1 + 2^-52)^K <= K 2^(e_i + e_j)
(1 + 2^-31), and stores fl(C - acc), or with split-K adds -acc_part atomically once per part, every part within the same bound.
Exact rational arithmetic (fractions.Fraction) is the reference: whenever the predicate says "negligible", the correctly rounded
C -+ T has the bits of C for T = K 2^(e_i + e_j) (1 + 2^-31), and it still has them after 2 and 4 successive subtractions of parts
within the bound.  The stand-alone tests/c/f64_screen_check.cpp (flag indexing, the extended emul_amax_cover) is built and run
here too.  No GPU."""
import ctypes as C
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from lmm_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
DP = C.POINTER(C.c_double)
MARGIN = 56
KS = [128, 256, 384, 512, 640, 1024, 1152, 2048]
SLACK = 1 + Fraction(1, 2 ** 31)


@pytest.fixture(scope="module")
def lib():
    lib = L.load()
    lib.lmm_dev_emul_negligible.argtypes = [C.c_int, DP, DP, DP, C.c_int, C.POINTER(C.c_int)]
    lib.lmm_dev_emul_negligible.restype = C.c_int
    return lib


def negligible(lib, K, ri, rj, c):
    ri, rj, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.broadcast(ri, rj, c).shape)).ravel() for v in (ri, rj, c))
    out = np.full(c.size, -1, dtype=np.int32)
    assert lib.lmm_dev_emul_negligible(K, ri.ctypes.data_as(DP), rj.ctypes.data_as(DP), c.ctypes.data_as(DP), c.size, out.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def row_exp(a):      # ceil(log2 a) for a finite a > 0, in integers
    m, q = math.frexp(a)
    return q - 1 if m == 0.5 else q


def clog2(K):
    return (K - 1).bit_length()


def bits(x):
    return struct.pack("<d", x)


def pow2(e):
    return math.ldexp(1.0, e)


def bound_T(K, ei, ej):
    return Fraction(K) * Fraction(2) ** (ei + ej) * SLACK


def keeps_bits(K, ei, ej, c):
    """fl(c - T) has the bits of c for both signs of the largest acc the f64 kernel can form"""
    T = bound_T(K, ei, ej)
    return all(bits(float(Fraction(c) - s * T)) == bits(c) for s in (1, -1))


def keeps_bits_in_parts(K, ei, ej, c, parts, rng):
    """c after `parts` successive correctly rounded subtractions (the split-K atomic adds), each of any size and sign within the bound
    -- the bound itself among them -- has the bits of c after every one of them"""
    T = bound_T(K, ei, ej)
    for signs in ([1] * parts, [-1] * parts, [(-1) ** p for p in range(parts)]):
        v = c
        for p, s in enumerate(signs):
            t = T if p % 2 == 0 else T * Fraction(int(rng.integers(1, 2 ** 30)), 2 ** 30)
            v = float(Fraction(v) - s * t)
            if bits(v) != bits(c):
                return False
    return True


def rows_for(rng, e):
    """a row maximum with ceil(log2) = e: the power of two itself or something in (2^(e - 1), 2^e)"""
    return pow2(e) if rng.random() < 0.3 else float(np.nextafter(pow2(e - 1), np.inf)) + rng.random() * (pow2(e) - pow2(e - 1)) * 0.999


def test_python_rounding_is_the_reference():
    assert float(Fraction(1) + Fraction(1, 2 ** 53)) == 1.0 and float(Fraction(1) + Fraction(3, 2 ** 54)) == 1.0 + 2.0 ** -52
    assert float(Fraction(1) - Fraction(1, 2 ** 54)) == 1.0 and float(Fraction(1) - Fraction(1, 2 ** 54) - Fraction(1, 2 ** 80)) == 1.0 - 2.0 ** -53
    assert float(Fraction(3, 2 ** 1075)) == 2 * 5e-324 and float(Fraction(1, 2 ** 1075)) == 0.0
    # (1 + 2^-52)^K <= 1 + 2^-31 for every K the kernel takes: the slack the reference uses covers the kernel's roundings
    assert (1 + Fraction(1, 2 ** 52)) ** 16384 <= SLACK


def test_random_cases_around_the_threshold(lib):
    rng = np.random.default_rng(61)
    seen = {True: 0, False: 0}
    for K in KS:
        n = 120
        ei, ej, off = rng.integers(-80, 80, size=n), rng.integers(-80, 80, size=n), rng.integers(-4, 5, size=n)
        ri = np.array([rows_for(rng, int(e)) for e in ei])
        rj = np.array([rows_for(rng, int(e)) for e in ej])
        q = clog2(K) + ei + ej + MARGIN + off
        c = np.ldexp(1.0 + rng.random(n), q) * rng.choice([-1.0, 1.0], size=n)
        c[::7] = np.ldexp(1.0, q[::7])
        neg = negligible(lib, K, ri, rj, c)
        for t in range(n):
            assert row_exp(ri[t]) == ei[t] and row_exp(rj[t]) == ej[t]
            assert neg[t] == (off[t] >= 0), (K, ei[t], ej[t], c[t])
            if neg[t]:
                assert keeps_bits(K, int(ei[t]), int(ej[t]), float(c[t])), (K, ei[t], ej[t], c[t])
                for parts in (2, 4):
                    assert keeps_bits_in_parts(K, int(ei[t]), int(ej[t]), float(c[t]), parts, rng), (K, ei[t], ej[t], c[t], parts)
            seen[bool(neg[t])] += 1
    assert seen[True] > 300 and seen[False] > 300


@pytest.mark.parametrize("K", KS)
def test_powers_of_two_and_their_neighbours_at_the_threshold(lib, K):
    rng = np.random.default_rng(K)
    for ei, ej in [(0, 0), (-3, 7), (40, -90), (-500, -500), (400, 500)]:
        bound = clog2(K) + ei + ej + MARGIN
        if not -1022 < bound < 1022:
            continue
        for dq, want in [(0, True), (1, True), (-1, False)]:
            p = pow2(bound + dq)
            below, above = float(np.nextafter(p, 0.0)), float(np.nextafter(p, np.inf))
            for sign in (1.0, -1.0):
                got = negligible(lib, K, pow2(ei), pow2(ej), np.array([p, above, below]) * sign)
                assert list(got) == [want, want, dq == 1], (K, ei, ej, dq, sign, got)      # the lower neighbour of a power of two is one binade down
                for c, g in zip((p, above, below), got):
                    if g:
                        assert keeps_bits(K, ei, ej, sign * c), (K, ei, ej, c)
                        assert keeps_bits_in_parts(K, ei, ej, sign * c, 2, rng) and keeps_bits_in_parts(K, ei, ej, sign * c, 4, rng)
        # three binades below the threshold the update does change C: K > 2^(L - 1), so T exceeds half the gap below 2^(bound - 3)
        assert not keeps_bits(K, ei, ej, pow2(bound - 3))
        assert not negligible(lib, K, pow2(ei), pow2(ej), pow2(bound - 3))[0]


def test_subnormal_c_largest_c_and_subnormal_row_maxima(lib):
    rng = np.random.default_rng(7)
    tiny, big = 5e-324, float(np.finfo(np.float64).max)
    for K in (128, 512, 1024, 2048):
        Lk = clog2(K)
        # subnormal C (ilogb of the value: -1074 .. -1023) with row maxima small enough for the rule to hold, and just too large
        for m, q in [(1, -1074), (2, -1073), (3, -1073), (2 ** 51, -1023), (2 ** 52 - 1, -1023)]:
            c = m * tiny
            e_sum = q - MARGIN - Lk
            ei = e_sum // 2
            ej = e_sum - ei
            for d, want in [(0, True), (1, False)]:
                got = negligible(lib, K, pow2(ei + d), pow2(ej), np.array([c, -c]))
                assert list(got) == [want, want], (K, m, q, d, got)
                if want:
                    assert keeps_bits(K, ei + d, ej, c) and keeps_bits_in_parts(K, ei + d, ej, c, 4, rng)
        # the largest C
        for ei, ej in [(0, 0), (400, 500), (480, 480)]:
            want = Lk + ei + ej + MARGIN <= 1023
            got = negligible(lib, K, pow2(ei), pow2(ej), np.array([big, -big]))
            assert list(got) == [want, want]
            if want:
                assert keeps_bits(K, ei, ej, big) and keeps_bits_in_parts(K, ei, ej, -big, 4, rng)
        # subnormal row maxima: ceil(log2) of the value
        for mi, ei in [(1, -1074), (3, -1072), (2 ** 51 + 1, -1022), (2 ** 52 - 1, -1022)]:
            ri = mi * tiny
            assert row_exp(ri) == ei
            for ej in (0, 900):
                bound = Lk + ei + ej + MARGIN
                for dq, want in [(0, True), (-1, False)]:
                    q = bound + dq
                    if not -1074 <= q <= 1023:
                        continue
                    c = pow2(q)
                    assert negligible(lib, K, ri, pow2(ej), c)[0] == want, (K, mi, ej, dq)
                    if want:
                        assert keeps_bits(K, ei, ej, c) and keeps_bits_in_parts(K, ei, ej, c, 2, rng)


def test_cases_the_rule_keeps_live(lib):
    for K in (128, 1024):
        one = 1.0
        assert not negligible(lib, K, pow2(-600), pow2(-600), np.array([0.0, -0.0, np.inf, -np.inf, np.nan])).any()
        assert not negligible(lib, K, np.nan, pow2(-600), one)[0] and not negligible(lib, K, pow2(-600), np.inf, one)[0]
        assert negligible(lib, K, 0.0, 1.0e300, np.array([one, 5e-324, -1.0e308])).all()      # an all-zero row: acc = 0 exactly
        assert not negligible(lib, K, 0.0, np.nan, one)[0]


def test_flag_indexing_and_cover_stand_alone(tmp_path):
    exe = str(tmp_path / "f64_screen_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(os.path.dirname(HERE), "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "f64_screen_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout
