"""GPU checks of the block maxima of the int8 emulation: the row scan keeps the largest |entry| per row and 128-wide
K block, emul_live_kernel decides from them which 256-row blocks and which 16-row pieces of a panel are live, and the convert loads
the live pieces only and writes zeros into the dead pieces of the blocks the GEMM may stage.  Nothing of that may show in a result:

* lmm_dev_syrk_emul equals the host entry lmm_dev_emul_host (which truncates every entry and knows nothing of maxima, masks or pieces)
  in every bit, with the residue scratch poisoned, for operands whose liveness is set per 16-row piece and K block (below);
* a factorisation whose emulated updates cover one another -- so that the maxima an earlier update scanned, at its own row offset,
  decide a later one's live pieces -- gives the same factor and rider rows with the kept maxima on and off, the poison on and off and
  the group cap at 0 and 2, reports the same failing pivot, and stays within 1e-9 of LAPACK.

The helpers (run_syrk, same_bits, bit_budget, live_blocks, factor_inputs, potrf, matern52) are those of tests/test_gpu_emul_zero_skip.py,
live_pieces is tests/test_gpu_emul_dead_blocks.py's and emulated_steps / cover are tests/test_gpu_emul_amax_reuse.py's.

The factorisations need LMM_REGION=0 (the region kernel would take the small block columns whose updates are emulated here), which
is read once per process: they run in ONE child process (`python tests/test_gpu_emul_block_maxima.py child`) that prints JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_emul_amax_reuse as AR
import test_gpu_emul_dead_blocks as DB
import test_gpu_emul_zero_skip as ZS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DP = C.POINTER(C.c_double)
ZERO_ROW, NAN_ROW, INF_ROW = ZS.ZERO_ROW, ZS.NAN_ROW, 13                 # in the first piece of the first block, inside every N used here
THR_ROW = 2                                                              # the row of a piece that holds its threshold entry
NKS = (1, 2, 3, 5, 9)
SHAPES = ((320, 320), (768, 256))
NMODS = (8, 16)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_emul_scratch_poison.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_scratch_poison.restype = C.c_int
    yield lmm_amd
    reset(lib)


def reset(lib):
    lib.lmm_dev_set_emul_scratch_poison(0)
    lib.lmm_dev_set_emul_zero_skip(-1)
    lib.lmm_dev_set_emul_gemm_workgroups(0)


# ---- operands whose liveness is set per (16-row piece, K block) ----
def live_set(R, nk, every=2):
    """the K blocks meant to be live in the 256-row block R: with more than one K block, blocks R and R + 1 share none"""
    return [k for k in range(nk) if nk == 1 or k % every == R % every]


def states(M, nk, every=2):
    """[piece][K block] -> "live" (random entries), "dead" (random entries that truncate away), "thr" (zeros and ONE entry exactly at
    the threshold 2^(e - b) of its row: the integer 1) or "below" (zeros and one entry per row one ulp below the threshold: all zeros
    once truncated).  The first live K block of a 256-row block holds the row maxima and is live in every piece; its other live
    blocks take all four states in turn over pieces and blocks, so a live block has dead pieces; the other blocks are dead in every
    piece."""
    npc = (M + 15) // 16
    st = np.empty((npc, nk), dtype=object)
    for p in range(npc):
        ls = live_set(p // 16, nk, every)
        for k in range(nk):
            if k == ls[0]:
                st[p, k] = "live"
            elif k in ls:
                st[p, k] = ("live", "dead", "thr", "below")[(p + k // every) % 4]
            else:
                st[p, k] = ("dead", "below")[(p + k) % 2]
    return st


def operands(M, K, b, seed, every=2):
    """Rows scaled 2^-20 .. 2^20 against each other.  The maximum of an even row is 2^q exactly (e = q, the 2^k edge of the exponent),
    that of an odd row 1.5 2^q (e = q + 1); the other entries are 2^-12 .. 2^-1/2 of 2^q, both signs.  Plus an all-zero row, a row with a
    NaN and a row with an infinity, in the first piece."""
    rng = np.random.default_rng(seed)
    nk = K // 128
    q = rng.integers(-20, 21, size=M)
    odd = np.arange(M) % 2 == 1
    e_rel = odd.astype(np.int64)                                          # e - q
    U = rng.choice([-1.0, 1.0], size=(M, K)) * np.exp2(-rng.uniform(0.5, 12, size=(M, K)))
    st = states(M, nk, every)
    thr = np.exp2((e_rel - b).astype(np.float64))                         # relative to 2^q
    for p in range(st.shape[0]):
        rows = np.arange(16 * p, min(16 * p + 16, M))
        for k in range(nk):
            cols = slice(128 * k, 128 * k + 128)
            if st[p, k] == "dead":
                U[rows, cols] *= 2.0 ** -(b + 20)
            elif st[p, k] == "thr":
                U[rows, cols] = 0.0
                U[rows[THR_ROW], 128 * k + 7] = -thr[rows[THR_ROW]]
            elif st[p, k] == "below":
                U[rows, cols] = 0.0
                U[rows, 128 * k + 9] = np.nextafter(thr[rows], 0.0)
    for R in range((M + 255) // 256):
        rows = slice(256 * R, min(256 * R + 256, M))
        U[rows, 128 * live_set(R, nk, every)[0] + 17] = -np.where(odd[rows], 1.5, 1.0)
    A = U * np.exp2(q.astype(np.float64))[:, None]
    home = 128 * live_set(0, nk, every)[0]
    A[ZERO_ROW] = 0.0
    A[NAN_ROW, home + 40] = np.nan
    A[INF_ROW, home + 41] = -np.inf
    want_pieces = np.array([[s in ("live", "thr") for s in row] for row in st])
    return A, st, want_pieces


_CASES = {}


def case(lmm, M, N, K, nmod):
    """(A, minus the host-emulated A A[:N]', the states), computed once per case and left unchanged; the operands do have the liveness
    they are meant to have, by the rule "truncate every entry" in NumPy."""
    key = (M, N, K, nmod)
    if key not in _CASES:
        lib = lmm.load()
        b = ZS.bit_budget(lmm, nmod, K)
        A, st, want_pieces = operands(M, K, b, M + N + K + nmod)
        got_pieces = DB.live_pieces(A, b)
        assert np.array_equal(got_pieces, want_pieces), np.argwhere(got_pieces != want_pieces)[:8]
        Af, Bf = np.asfortranarray(A), np.asfortranarray(A[:N])
        out = np.zeros((M, N), order="F")
        lib.lmm_dev_emul_host.restype = C.c_int
        rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), M, Bf.ctypes.data_as(DP), N, M, N, K, nmod, K, out.ctypes.data_as(DP), M, None)
        assert rc == 0, lib.lmm_last_error_string()
        want = -out
        want.setflags(write=False)
        A.setflags(write=False)
        _CASES[key] = (A, want, st, want_pieces)
    return _CASES[key]


def test_patterns_are_what_they_are_meant_to_be(lmm):
    """Every situation the liveness kernel and the convert must handle occurs in the cases below."""
    seen = set()
    for M, N in SHAPES:
        for nk in NKS:
            for nmod in NMODS:
                A, want, st, pieces = case(lmm, M, N, 128 * nk, nmod)
                npc = pieces.shape[0]
                blocks = np.array([pieces[16 * R:16 * R + 16].any(axis=0) for R in range((npc + 15) // 16)])
                for R in range(blocks.shape[0]):
                    sub = pieces[16 * R:min(16 * R + 16, npc)]
                    if (blocks[R][None, :] & ~sub).any():
                        seen.add("dead piece in a live block")
                    seen.add("block 0 live" if blocks[R, 0] else "block 0 dead")
                    for S in range(min(R + 1, (N + 255) // 256)):
                        if not (blocks[R] & blocks[S]).any():
                            seen.add("two tile rows share no live block")
                for s in ("thr", "below", "dead", "live"):
                    if (st == s).any():
                        seen.add(s)
                if M % 256:
                    seen.add("padding rows")
                if npc % 16:
                    seen.add("padding pieces")
                e = np.ceil(np.log2(np.abs(A[2:4]).max(axis=1)))
                assert np.abs(A[2]).max() == 2.0 ** e[0] and np.abs(A[3]).max() == 1.5 * 2.0 ** (e[1] - 1)      # a power-of-two maximum, and one that is not
                assert not A[ZERO_ROW].any() and np.isnan(A[NAN_ROW]).any() and np.isinf(A[INF_ROW]).any()
    want = {"dead piece in a live block", "block 0 live", "block 0 dead", "two tile rows share no live block", "thr", "below", "dead", "live",
            "padding rows", "padding pieces"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("nmod", NMODS)
@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_piece_patterns_bit_for_bit(lmm, M, N, nk, nmod):
    """Poison on: skip on with the default grid and a capped one, and skip off; poison off, skip on: the host entry's bits each time."""
    lib = lmm.load()
    K = 128 * nk
    A, want, st, pieces = case(lmm, M, N, K, nmod)
    print(f"syrk_emul {M}x{N}x{K}, nmod = {nmod}: live pieces {int(pieces.sum())} of {pieces.size}, states "
          + ", ".join(f"{s}: {int((st == s).sum())}" for s in ("live", "thr", "below", "dead")))
    assert np.isnan(want[NAN_ROW, 0]) and np.isnan(want[INF_ROW, 0]) and np.isnan(want[M - 1, NAN_ROW]) and not np.isnan(want[M - 1, 0])
    try:
        for skip, poison, grids in ((1, 1, (0, 3)), (0, 1, (0,)), (1, 0, (0,))):
            assert lib.lmm_dev_set_emul_zero_skip(skip) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
            for wgs in grids:
                assert lib.lmm_dev_set_emul_gemm_workgroups(wgs) == 0
                got, pad, lower = ZS.run_syrk(lmm, A, N, nmod)
                assert np.all(pad == ZS.CANARY) and np.all(got[~lower] == ZS.CANARY)
                bad = ZS.same_bits(got, want, lower)
                assert not bad.any(), (skip, poison, wgs, int(bad.sum()), np.argwhere(bad)[:8])
                assert np.all(got[ZERO_ROW, :ZERO_ROW + 1] == 0.0)
                for r in (NAN_ROW, INF_ROW):
                    assert np.all(np.isnan(got[r, :r + 1])) and np.all(np.isnan(got[r:, r]))
    finally:
        reset(lib)


def test_second_mask_word_with_piece_patterns(lmm):
    """K = 8320: 65 K blocks, bit 0 of the second mask word.  Blocks 0, 32 and 64 are live (64 and 32 with dead, threshold and
    just-below pieces), the others dead.  The host entry stops at K = 4096: skip on (poisoned scratch) against skip off in every bit,
    and against Float64 to see that block 64 is in the product."""
    lib = lmm.load()
    M = N = 256
    K, nmod = 8320, 16
    b = ZS.bit_budget(lmm, nmod, K)
    A, st, want_pieces = operands(M, K, b, 8320, every=32)
    assert np.array_equal(DB.live_pieces(A, b), want_pieces)
    assert [k for k in range(65) if want_pieces[:, k].any()] == [0, 32, 64] and not want_pieces[:, 64].all()
    finite = np.ones(M, dtype=bool)
    finite[[NAN_ROW, INF_ROW]] = False
    try:
        res = {}
        for on in (0, 1):
            assert lib.lmm_dev_set_emul_zero_skip(on) == 0 and lib.lmm_dev_set_emul_scratch_poison(on) == 0
            res[on], pad, lower = ZS.run_syrk(lmm, A, N, nmod)
            assert np.all(pad == ZS.CANARY) and np.all(res[on][~lower] == ZS.CANARY)
    finally:
        reset(lib)
    assert not ZS.same_bits(res[1], res[0], lower).any()
    Af = np.where(np.isfinite(A), A, 0.0)
    ref = -(Af @ Af[:N].T)
    amax = np.abs(Af).max(axis=1)
    scale = amax[:, None] * amax[None, :]
    ok = lower & finite[:, None] & finite[None, :]
    # Against Float64 (the bound of ZS.test_second_mask_word_on_against_off: three live blocks here too): the truncation is
    # 4 K 2^-b < 1e-12 of amax_i amax_j, the Float64 dot product's rounding at most K u times the 384 live terms < 4e-10; block 64
    # alone adds sum_k a_ik^2 > 1e-6 amax_i^2 to the diagonal entry of a row whose piece is live there, so leaving it out would show.
    assert np.all(np.abs(res[1] - ref)[ok] <= 1e-9 * scale[ok])
    rows64 = np.flatnonzero(np.repeat(st[:, 64] == "live", 16)[:M] & finite)
    assert rows64.size >= 32 and np.all((Af[rows64, 128 * 64:] ** 2).sum(axis=1) > 1e-6 * amax[rows64] ** 2)


# ---- factorisations whose emulated updates cover one another: the child ----
SIZES = (1152, 2304)
RIDERS = ZS.RIDERS
SETTINGS = [(reuse, poison, group) for reuse in (1, 0) for poison in (1, 0) for group in (0, 2)]


def factor_inputs(n):
    """ZS.factor_inputs(1) at n = 1152; the same kernel, lengthscale, point spacing and jitter at another n"""
    if n == ZS.N_FACT:
        return ZS.factor_inputs(1)
    rng = np.random.default_rng(n + 1)
    x = np.arange(n) / (ZS.N_FACT - 1.0)
    return ZS.matern52(x, 0.02) + 0.1 * np.eye(n), rng.standard_normal((RIDERS, n))


def child():
    import scipy.linalg as sla
    sys.path.insert(0, ROOT)
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_emul_amax_reuse.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_scratch_poison.argtypes = [C.c_int]
    res = {}
    for n in SIZES:
        Kmat, R = factor_inputs(n)
        L = np.linalg.cholesky(Kmat)
        want = np.vstack([L, sla.solve_triangular(L, R.T, lower=True).T])
        tri = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((RIDERS, n), dtype=bool)])
        bad_at = n - 52
        Kbad = Kmat.copy()
        Kbad[bad_at, bad_at] = -5.0
        assert lib.lmm_dev_set_f64_emul(0, 128, 16) == 0
        f64, info = ZS.potrf(lmm_amd, Kmat, R)
        assert info == 0
        assert lib.lmm_dev_set_f64_emul(1, 128, 16) == 0
        steps = AR.emulated_steps(lib, n + RIDERS, n)
        covers = [AR.cover(steps, si) for si in range(len(steps))]
        r = {"steps": steps, "covers": covers}
        # on the LAPACK factor: the panels of the updates that read kept maxima, at the kept columns -- dead and live pieces both occur
        mixed = 0
        for (j0, h), (kept, scan0) in zip(steps, covers):
            if kept:
                pieces = DB.live_pieces(np.ascontiguousarray(want[j0 + h:, j0:j0 + h]), ZS.bit_budget(lmm_amd, 16, h))[:, :(scan0 - j0) // 128]
                mixed += int(pieces.any() and not pieces.all())
        r["covering_updates_with_dead_and_live_kept_pieces"] = mixed
        got, pivots = {}, {}
        for s in SETTINGS:
            reuse, poison, group = s
            assert lib.lmm_dev_set_emul_amax_reuse(reuse) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0 and lib.lmm_dev_set_emul_group(group) == 0
            got[s], info = ZS.potrf(lmm_amd, Kmat, R)
            assert info == 0
            _, pivots[s] = ZS.potrf(lmm_amd, Kbad, R)
        lib.lmm_dev_set_emul_amax_reuse(1)
        lib.lmm_dev_set_emul_scratch_poison(0)
        lib.lmm_dev_set_emul_group(0)
        first = got[SETTINGS[0]]
        r["bits_equal"] = [bool(np.array_equal(got[s][tri].view(np.int64), first[tri].view(np.int64))) for s in SETTINGS]
        r["pivots"] = [pivots[s] for s in SETTINGS]
        r["bad_at"] = bad_at
        nrm = np.linalg.norm(want[tri])
        r["e_emu"] = float(np.linalg.norm((first - want)[tri]) / nrm)
        r["e_f64"] = float(np.linalg.norm((f64 - want)[tri]) / nrm)
        res[str(n)] = r
    print(json.dumps(res))


@pytest.fixture(scope="module")
def found():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, LMM_REGION="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    return res


@pytest.mark.parametrize("n", SIZES)
def test_updates_cover_one_another(found, n):
    """the plan the child factored with: emulated updates read maxima that earlier ones scanned from a higher first row, and on the
    LAPACK factor those kept columns hold dead and live pieces"""
    r = found[str(n)]
    offsets = [(j0 + h) - (kept[0][1]) for (j0, h), (kept, scan0) in zip(r["steps"], r["covers"]) if kept]      # our first row - the first kept array's
    print(n, "emulated updates (j0, h):", r["steps"], "row offsets of the first kept array:", offsets)
    assert len(offsets) >= 3 and min(offsets) > 0
    assert r["covering_updates_with_dead_and_live_kept_pieces"] >= 1


@pytest.mark.parametrize("n", SIZES)
def test_factor_is_the_same_in_every_bit(found, n):
    """(reuse, poison, group cap) in {1, 0} x {1, 0} x {0, 2}: factor and rider rows"""
    r = found[str(n)]
    assert r["bits_equal"] == [True] * len(SETTINGS), [s for s, ok in zip(SETTINGS, r["bits_equal"]) if not ok]


@pytest.mark.parametrize("n", SIZES)
def test_failing_pivot_report_is_unchanged(found, n):
    r = found[str(n)]
    assert r["pivots"] == [r["bad_at"] + 1] * len(SETTINGS)


@pytest.mark.parametrize("n", SIZES)
def test_factor_against_lapack(found, n):
    """the bar of ZS.test_factorisation_same_with_skip_on_and_off: 1e-9 relative (the f64 kernels' own error is printed beside it)"""
    r = found[str(n)]
    print(n, f"|emulated - LAPACK| / |LAPACK| = {r['e_emu']:.3e}, f64 kernels {r['e_f64']:.3e}")
    assert r["e_emu"] <= 1e-9


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    child()
