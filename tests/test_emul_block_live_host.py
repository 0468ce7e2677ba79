"""Host-only check of the liveness decision of the int8 emulation's convert (emul_block_live in csrc/lmm_emul.h): the
row scan keeps, per row and 128-wide K block, the largest |entry| of the block, and the convert reads a piece only when that maximum
truncates to a non-zero integer.  lmm_dev_emul_block_live runs the library's own predicate on (row maximum, block maximum) pairs; the
reference truncates EVERY entry of the block in NumPy and asks whether one is left."""
import ctypes as C

import numpy as np
import pytest

from lmm_amd import _lib as L

DP = C.POINTER(C.c_double)
BITS = (58, 57, 53, 40, 24, 1)                                           # 58 = the budget of 16 moduli at K = 128; 8 moduli at K = 16384: 24


@pytest.fixture(scope="module")
def lib():
    import lmm_amd
    lib = lmm_amd.load()
    lib.lmm_dev_emul_block_live.argtypes = [DP, DP, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.lmm_dev_emul_block_live.restype = C.c_int
    return lib


def decide(lib, rowmax, blockmax, bits):
    rowmax, blockmax = np.ascontiguousarray(rowmax, dtype=np.float64), np.ascontiguousarray(blockmax, dtype=np.float64)
    out = np.full(rowmax.size, -1, dtype=np.int32)
    rc = lib.lmm_dev_emul_block_live(rowmax.ctypes.data_as(DP), blockmax.ctypes.data_as(DP), rowmax.size, bits, out.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0, lib.lmm_last_error_string()
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def row_exp(amax):
    """ceil(log2 amax) for finite amax > 0, from the exact mantissa / exponent split (subnormals included)"""
    f, q = np.frexp(amax)
    return np.where(f == 0.5, q - 1, q).astype(np.int64)


def truncate_all(rowmax, block, bits):
    """[row] -> some entry of the row's block is not zero after trunc(a 2^(bits - e_row)); rows whose maximum is zero or not finite:
    False.  np.ldexp is exact whenever its result is a normal number or zero, and a result in the subnormals truncates to zero whether
    it was rounded or not."""
    ok = np.isfinite(rowmax) & (rowmax > 0)
    live = np.zeros(rowmax.size, dtype=bool)
    sh = bits - row_exp(np.where(ok, rowmax, 1.0))
    with np.errstate(over="ignore", under="ignore"):
        scaled = np.ldexp(block, sh[:, None].astype(np.int32))
    live[ok] = (np.trunc(scaled[ok]) != 0).any(axis=1)
    return live


@pytest.mark.parametrize("bits", BITS)
def test_random_blocks_against_truncating_every_entry(lib, bits):
    """Rows scaled over 2^-300 .. 2^300; blocks from well above the threshold 2^(e - bits) to well below it, both signs.  About half of
    the blocks straddle the threshold within a few binades, where the decision is not obvious."""
    rng = np.random.default_rng(1000 + bits)
    rows, k = 4096, 128
    scale = np.exp2(rng.integers(-300, 301, size=rows).astype(np.float64))
    rowmax = scale * rng.uniform(0.5, 1.0, size=rows)
    drop = np.maximum(rng.integers(bits - 4, bits + 5, size=rows), 0)    # the block's largest entry sits near 2^(e - drop), at or below the row's
    far = rng.random(rows) < 0.5
    drop[far] = rng.integers(0, 2 * bits + 40, size=int(far.sum()))
    block = rng.choice([-1.0, 1.0], size=(rows, k)) * rng.uniform(0.0, 1.0, size=(rows, k)) * (rowmax * np.exp2(-drop.astype(np.float64)))[:, None]
    blockmax = np.abs(block).max(axis=1)
    assert np.all(blockmax <= rowmax)
    want = truncate_all(rowmax, block, bits)
    got = decide(lib, rowmax, blockmax, bits)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    near = ~far
    assert 0.1 < want[near].mean() < 0.9                                  # the near-threshold half is decided both ways
    # the sign of either argument does not matter
    assert np.array_equal(decide(lib, -rowmax, -blockmax, bits), want)


@pytest.mark.parametrize("bits", BITS)
def test_threshold_edges(lib, bits):
    """Exactly at the threshold 2^(e - bits) (live: the integer 1), one ulp below it (dead), for row maxima that are exact powers of two
    (e = log2, not log2 + 1), just above one, and just below the next."""
    es = np.array([-1000, -300, -1, 0, 1, 52, 300, 1000], dtype=np.int64)
    rowmax, blockmax, want = [], [], []
    for e in es:
        for rm, e_row in ((np.ldexp(1.0, int(e)), e), (np.nextafter(np.ldexp(1.0, int(e)), np.inf), e + 1), (np.nextafter(np.ldexp(1.0, int(e) + 1), 0.0), e + 1)):
            thr = np.ldexp(1.0, int(e_row) - bits)
            for bm, lv in ((thr, True), (np.nextafter(thr, 0.0), False), (np.nextafter(thr, np.inf), True), (0.5 * thr, False), (rm, True), (0.0, False)):
                rowmax.append(rm); blockmax.append(bm); want.append(lv)
    rowmax, blockmax, want = np.array(rowmax), np.array(blockmax), np.array(want)
    assert np.array_equal(row_exp(np.array([1.0, 2.0, 3.0, 0.75, 0.5])), [0, 1, 2, 0, -1])
    ref = truncate_all(rowmax, blockmax[:, None], bits)
    assert np.array_equal(ref, want)
    got = decide(lib, rowmax, blockmax, bits)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("bits", BITS)
def test_extreme_scales(lib, bits):
    """Subnormal row maxima (the shift bits - e then exceeds 1022), subnormal block maxima under normal row maxima, the largest finite
    row maximum (e = 1024), and rows that are zeros to the GEMM: all zeros, an infinity, a NaN."""
    tiny = np.ldexp(1.0, -1074)
    rowmax, blockmax = [], []
    for rm in (tiny, 3 * tiny, np.ldexp(1.0, -1060), np.nextafter(np.ldexp(1.0, -1022), 0.0), np.ldexp(1.0, -1022), np.ldexp(1.5, -1000)):
        e = int(row_exp(np.array([rm]))[0])
        for bm in (rm, 0.0, tiny, np.ldexp(1.0, max(e - bits, -1074)), np.ldexp(1.0, max(e - bits - 1, -1074)), np.ldexp(1.0, max(e - bits + 1, -1074))):
            if bm <= rm:
                rowmax.append(rm); blockmax.append(bm)
    big = np.finfo(np.float64).max
    for bm in (big, np.ldexp(1.0, 1024 - bits), np.nextafter(np.ldexp(1.0, 1024 - bits), 0.0), np.ldexp(1.0, 1023 - bits), 1.0, tiny, 0.0):
        rowmax.append(big); blockmax.append(bm)
    rowmax, blockmax = np.array(rowmax), np.array(blockmax)
    want = truncate_all(rowmax, blockmax[:, None], bits)
    # what the rule says, spelled out without any scaling: live iff blockmax >= 2^(e - bits), which is exact in Float64 down to the
    # smallest subnormal (below it no non-zero blockmax exists and the threshold is not reachable)
    thr_exp = row_exp(rowmax) - bits
    spelled = np.array([bm > 0 and (te < -1074 or bm >= np.ldexp(1.0, int(te))) for bm, te in zip(blockmax, thr_exp)])
    assert np.array_equal(want, spelled)
    got = decide(lib, rowmax, blockmax, bits)
    assert np.array_equal(got, want), [(rowmax[i], blockmax[i]) for i in np.flatnonzero(got != want)[:8]]
    assert want.any() and not want.all()
    dead_rows = np.array([0.0, np.inf, np.nan, np.inf, np.nan])
    their_blocks = np.array([0.0, 1.0, 1.0, np.inf, np.nan])
    assert not decide(lib, dead_rows, their_blocks, bits).any()


def test_bad_arguments(lib):
    one = np.ones(1)
    out = np.zeros(1, dtype=np.int32)
    args = (one.ctypes.data_as(DP), one.ctypes.data_as(DP))
    op = out.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lmm_dev_emul_block_live(*args, 1, 0, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_block_live(*args, 1, 59, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_block_live(*args, -1, 40, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_block_live(None, args[1], 1, 40, op) == L.LMM_ERR_ARG
    assert lib.lmm_dev_emul_block_live(*args, 0, 40, None) == 0
