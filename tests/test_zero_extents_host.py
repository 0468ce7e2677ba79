"""Host-only checks of the zero extents (csrc/lmm_emul.h "zero extents", DESIGN.md 4.17 "Rows whose panel is exactly zero").

The ZERO EXTENT of a block of 64 rows of a factor matrix is the number of leading columns, in whole 64-column blocks of the lower
triangle, in which every entry of those rows is stored as +0.  The claim the kernels rely on: for a finite factor, L[block, :ext] is
zero as well, so an update item, an emulated tile or a region row task whose rows have ext >= the end of its panel only rewrites
zeros.  Here the induction is checked on LAPACK's factor (np.linalg.cholesky) of Matern52 + 0.1 I matrices, and the void-item
arithmetic (which row tasks and update tiles are void for given extents) against counts worked out by hand.  No GPU.

The helpers are shared with tests/test_gpu_zero_extents.py."""
import numpy as np
import pytest

NONE = 0x7F7F7F7F      # LMM_ZERO_EXT_NONE: a row block without a stored bit


def matern52(x, ell):
    r = np.abs(x[:, None] - x[None, :]) / ell
    s = np.sqrt(5.0) * r
    return (1.0 + s + s * s / 3.0) * np.exp(-s)


def extents(A, ncols):
    """Per 64-row block of A (rows x >= ncols columns, the lower triangle and rider rows as stored): 64 x the leading run of all-zero
    64 x 64 tiles among the tiles tj <= ti, tj < ncols / 64 -- on the bit pattern, so -0 counts as an entry; NONE when all are zero."""
    bits = np.ascontiguousarray(A).view(np.int64)
    out = []
    for ti in range(A.shape[0] // 64):
        ext = NONE
        for tj in range(min(ti + 1, ncols // 64)):
            if bits[64 * ti:64 * ti + 64, 64 * tj:64 * tj + 64].any():
                ext = 64 * tj
                break
        out.append(ext)
    return np.array(out, dtype=np.int64)


def is_void(ext, row, nblk, need):
    """zero_ext_void of lmm_emul.h: the nblk 64-row blocks from `row` are zero left of column `need` (blocks past the matrix count as zero)"""
    b = row // 64
    e = ext[b:b + nblk]
    return bool(e.size == 0 or e.min() >= need)


def void_row_tasks(ext, NR, c0, P, n128=None, rows_real=None):
    """(void, all) row tasks of a region launch over the block column [c0, c0 + 128 P): the first n128 tasks are 128 rows high, the
    rest 64; a task with no real row does not run"""
    M = NR - c0
    real_rows = M if rows_real is None else rows_real - c0
    void = total = 0
    roff, k = 128 * P, 0
    while roff < M:
        tall = n128 is None or k < n128
        if real_rows - roff > 0:
            total += 1
            void += is_void(ext, c0 + roff, 2 if tall else 1, c0 + 128 * P)
        roff += 128 if tall else 64
        k += 1
    return void, total


def void_update_tiles(ext, NR, j0, h, N, strip=False, col0=True):
    """(void rest tiles, all rest tiles, void column-0 items ti >= 1) of the f64 update of the N columns from r0 = j0 + h by the
    panel [j0, j0 + h): 128 x 128 tiles ti >= tj, the ragged last 64 rows (strip) apart"""
    r0 = j0 + h
    M = NR - r0 - (64 if strip else 0)
    MT, NT = (M + 127) // 128, (N + 127) // 128
    v = [is_void(ext, r0 + 128 * ti, 2, r0) for ti in range(MT)]
    rest = sum(v[ti] for tj in range(1, NT) for ti in range(tj, MT))
    total = sum(MT - tj for tj in range(1, NT) if MT > tj)
    return rest, total, (sum(v[1:]) if col0 else 0)


def void_emul_tiles(ext, j0, h, N, M):
    """(void, all) 256 x 256 tiles ti >= tj of an emulated update of M rows and N columns from r0 = j0 + h"""
    r0 = j0 + h
    tm, tn = (M + 255) // 256, (N + 255) // 256
    v = [is_void(ext, r0 + 256 * ti, 4, r0) for ti in range(tm)]
    return sum(v[ti] for tj in range(tn) for ti in range(tj, tm)), sum(tm - tj for tj in range(tn) if tm > tj)


def inputs(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    if kind == "mostly_sorted":
        for i in range(0, n, 97):
            j = int(rng.integers(n))
            x[i], x[j] = x[j], x[i]
    elif kind == "permuted":
        x = rng.permutation(x)
    return x


CASES = [(n, ell, "sorted") for n in (1152, 2304) for ell in (0.6, 2.1)] + [
    (1152, 0.6, "mostly_sorted"), (2304, 2.1, "mostly_sorted"), (1152, 0.6, "permuted"), (2304, 2.1, "permuted"), (1152, 50.0 * 1152, "sorted"), (2304, 50.0 * 2304, "sorted")]


@pytest.mark.parametrize("n,ell,kind", CASES)
def test_factor_is_zero_inside_the_extents(n, ell, kind):
    x = inputs(n, kind, n)
    K = matern52(x, ell) + 0.1 * np.eye(n)
    ext = extents(np.tril(K), n)
    L = np.linalg.cholesky(K)
    assert np.isfinite(L).all()
    covered = 0
    for b, e in enumerate(ext):
        e = min(int(e), 64 * b)                 # a diagonal tile is never zero: e <= 64 b
        assert not L[64 * b:64 * b + 64, :e].any(), (b, e)
        covered += e
    print(f"n = {n}, l = {ell}, {kind}: extents cover {covered * 64} of {n * (n + 1) // 2} entries of the lower triangle")
    if kind == "permuted" or ell > n:
        assert not ext.any()                     # nothing is zero, nothing is void
    elif kind == "sorted":
        first = int(np.argmax(ext > 0))
        assert ext[first:].all() and abs(64 * first - 745.2 / np.sqrt(5.0) * ell) <= 128      # exp underflows to +0 at s = 745.13..
        assert (np.diff(ext) >= 0).all()
    else:
        assert ext.any() and (ext == 0).sum() > (extents(np.tril(matern52(inputs(n, "sorted"), ell)), n) == 0).sum()


def test_void_item_counts_at_2304():
    """n = 2304, l = 2.1 (zero from ~700 columns off the diagonal): 12 of the 32 row tasks of 512-column region launches are void, and
    682 of the 969 tiles of a K = 128 panel recursion"""
    n = 2304
    ext = extents(np.tril(matern52(inputs(n, "sorted"), 2.1) + 0.1 * np.eye(n)), n)
    void = total = 0
    for c0 in range(0, n, 512):
        v, t = void_row_tasks(ext, n, c0, min(4, (n - c0) // 128))
        void, total = void + v, total + t
    assert (void, total) == (12, 32)
    void = total = 0
    for j0 in range(0, n - 128, 128):
        rest, t, c0 = void_update_tiles(ext, n, j0, 128, n - j0 - 128)
        void, total = void + rest + c0 + is_void(ext, j0 + 128, 2, j0 + 128), total + t + (n - j0 - 128) // 128
    assert (void, total) == (682, 969)


def test_void_item_arithmetic_edges():
    ext = np.array([0, 0, 0, 64, 128, 128, NONE, NONE], dtype=np.int64)        # NR = 512
    assert is_void(ext, 256, 2, 128) and not is_void(ext, 192, 2, 128) and is_void(ext, 384, 4, 10 ** 6)      # blocks past the matrix are zero
    assert void_row_tasks(ext, 512, 0, 1) == (2, 3)                            # rows 128.., need 128: tasks at 256 and 384
    assert void_row_tasks(ext, 512, 0, 1, n128=1) == (4, 5)                    # 64-row tasks at 256, 320, 384, 448 are void, the tall one at 128 is not
    assert void_row_tasks(ext, 512, 0, 1, rows_real=300) == (1, 2)             # tasks without a real row do not run
    assert void_update_tiles(ext, 512, 0, 128, 384) == (3, 3, 2)
    ragged = np.append(ext, 0)                                                 # NR = 576: the last 64 rows (a live block) are the strip's, not a tile's
    assert void_update_tiles(ragged, 576, 0, 128, 384, strip=True) == (3, 3, 2) and void_update_tiles(ragged, 576, 0, 128, 384) == (3, 5, 2)
    assert void_emul_tiles(ext, 0, 128, 384, 384) == (2, 3)
    half = ext // 128 * 64
    assert (half <= ext).all() and void_update_tiles(half, 512, 0, 128, 384, col0=False)[0] <= 3
