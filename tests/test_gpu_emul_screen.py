"""GPU checks of the screen of the int8 emulation (DESIGN.md 4.17 "negligible tiles"): once the row maxima of a panel exist, a pass
over C marks the 256 x 256 tiles in which every output is negligible -- the update cannot change a bit of it (emul_negligible,
tests/test_emul_negligible_host.py) -- and the GEMM walks, and the combine touches, the other tiles only.  Nothing of that may show
in a result, and it must really happen:

* lmm_dev_syrk_emul equals C - (the host entry lmm_dev_emul_host's product), which knows nothing of tiles, in every bit, with the
  scratch poisoned (residues AND the never-written product bytes of dead tiles), for operands and C built so that given tiles are
  dead, on GEMM grids of 1, 2, 3, 5, 7 workgroups and the default one; the hook's live-tile count EQUALS the count a NumPy pass with
  the same rule finds, so a run in which nothing was skipped fails; the same with the screen off (every tile live) and no poison;
* a factorisation of n = 2304 with 64 rider rows, every update of at least 128 columns emulated, gives the same factor, rider rows
  and failing pivot with the screen on and off and the group cap at 0 and 2, for a decaying and a flat kernel matrix;
* five latents with lengthscales 0.02 .. 200 in groups of 2 + 2 + 1: one logpdf, screen on and off.

The factorisations need LMM_REGION=0, which is read once per process: they run in ONE child process
(`python tests/test_gpu_emul_screen.py child`) that prints JSON, as tests/test_gpu_emul_block_maxima.py's do."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_emul_zero_skip as ZS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DP = C.POINTER(C.c_double)
MARGIN = 56
SHAPES = ((832, 768), (1024, 512))
NKS = (1, 3, 9)
NMODS = (8, 16)
GRIDS = (1, 2, 3, 5, 7, 0)
ZERO_ROW, NAN_ROW = 5, 300          # NAN_ROW: tile row 1 and, as a column, tile column 1, at both shapes
PATTERNS = ("all_dead", "none_dead", "alternating", "first_last", "threshold", "specials", "nan_row")
SUBNORMAL = 3 * 5e-324


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_emul_scratch_poison.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_screen.argtypes = [C.c_int]
    lib.lmm_dev_emul_last_live_tiles.restype = C.c_int
    lib.lmm_dev_emul_host.restype = C.c_int
    yield lmm_amd
    reset(lib)


def reset(lib):
    lib.lmm_dev_set_emul_scratch_poison(0)
    lib.lmm_dev_set_emul_screen(-1)
    lib.lmm_dev_set_emul_gemm_workgroups(0)


def tile_list(M, N):
    """the trapezoid's tiles in the GEMM's order: supertiles of 8 tile rows x 4 tile columns, tile rows outside, tile columns inside"""
    tm, tn = (M + 255) // 256, (N + 255) // 256
    return [(i, j) for I in range(0, tm, 8) for J in range(0, tn, 4) for i in range(I, min(I + 8, tm)) for j in range(J, min(J + 4, tn)) if j <= i]


# ---- the rule in NumPy ----
def row_exps(A):
    """(e_i = ceil(log2 max_k |a_ik|) for a finite non-zero maximum, the row is all zeros, the row holds a NaN or an infinity)"""
    amax = np.abs(A).max(axis=1)
    bad = ~np.isfinite(amax)
    zero = amax == 0
    ok = ~bad & ~zero
    e = np.zeros(A.shape[0], dtype=np.int64)
    m, q = np.frexp(amax[ok])
    e[ok] = np.where(m == 0.5, q - 1, q)
    return e, zero, bad


def bounds(A, N, K):
    """ceil(log2 K) + e_i + e_j + 56 for every output (i, j)"""
    e, zero, bad = row_exps(A)
    return (K - 1).bit_length() + e[:, None] + e[None, :N] + MARGIN, zero[:, None] | zero[None, :N], bad[:, None] | bad[None, :N]


def negligible(A, N, K, Cm):
    bound, zero, bad = bounds(A, N, K)
    fin = np.isfinite(Cm) & (Cm != 0)
    ilogb = np.frexp(np.where(fin, Cm, 1.0))[1] - 1
    return fin & ~bad & (zero | (bound <= ilogb))


def live_tiles(A, N, K, Cm):
    """[(tile row, tile column)] of the tiles holding an output the combine would write that is not negligible"""
    M = A.shape[0]
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    live = lower & ~negligible(A, N, K, Cm)
    return [(i, j) for i, j in tile_list(M, N) if live[256 * i:256 * i + 256, 256 * j:256 * j + 256].any()]


# ---- operands and C with given dead tiles ----
def operand(M, K, seed):
    """Rows scaled 2^-20 .. 2^20 against each other, entries 2^-12 .. 2^-1/2 of the row's scale, both signs; even rows have a maximum
    that is an exact power of two.  One all-zero row."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-20, 21, size=M)
    U = rng.choice([-1.0, 1.0], size=(M, K)) * np.exp2(-rng.uniform(0.5, 12, size=(M, K)))
    U[::2, 17] = -1.0
    A = U * np.exp2(q.astype(np.float64))[:, None]
    A[ZERO_ROW] = 0.0
    return A


def build_c(A, N, K, pattern, seed):
    """(A for this pattern, C, the tiles meant to be live).  A dead tile holds entries 0 .. 3 binades above their bound, both signs; a
    live tile entries of the size of the update itself."""
    M = A.shape[0]
    rng = np.random.default_rng(seed)
    tiles = tile_list(M, N)
    if pattern == "nan_row":
        A = A.copy()
        A[NAN_ROW, K // 2 + 3] = np.nan
    bound, zero, bad = bounds(A, N, K)
    dead_val = rng.choice([-1.0, 1.0], size=(M, N)) * np.ldexp(1.0 + rng.random((M, N)), bound + rng.integers(0, 4, size=(M, N)))
    dead_val[zero] = rng.choice([-1.0, 1.0], size=int(zero.sum())) * 2.0 ** -40      # under an all-zero row anything finite and non-zero is negligible
    e, _, _ = row_exps(A)
    live_val = rng.standard_normal((M, N)) * np.exp2((e[:, None] + e[None, :N]).astype(np.float64))
    dead = {
        "all_dead": set(tiles), "none_dead": set(), "alternating": set(tiles[::2]), "first_last": {tiles[0], tiles[-1]},
        "threshold": set(tiles), "specials": set(tiles), "nan_row": set(tiles),
    }[pattern]
    Cm = live_val.copy()
    for i, j in dead:
        Cm[256 * i:256 * i + 256, 256 * j:256 * j + 256] = dead_val[256 * i:256 * i + 256, 256 * j:256 * j + 256]
    want_live = [t for t in tiles if t not in dead]
    if pattern == "threshold":
        # tile (2, 1) stays dead with one entry exactly at the threshold and one a binade above it; tile (1, 0) is live by ONE entry,
        # the largest double below its threshold, in the last column and row the screen reads of it
        Cm[600, 290] = np.ldexp(1.0, bound[600, 290])
        Cm[601, 291] = -np.ldexp(1.0, bound[601, 291] + 1)
        Cm[511, 255] = np.nextafter(np.ldexp(1.0, bound[511, 255]), 0.0)
        want_live = [(1, 0)]
    elif pattern == "specials":
        # otherwise dead tiles, each live by one entry: 0, -0, a subnormal, an infinity, a NaN
        for (r, c), v in {(256, 0): 0.0, (511, 511): -0.0, (700, 3): SUBNORMAL, (520, 300): -np.inf, (780, 40): np.nan}.items():
            Cm[r, c] = v
        want_live = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0)]
    elif pattern == "nan_row":
        # every tile would be dead: the NaN row makes those of its tile row and of its tile column live
        want_live = [t for t in tiles if t[0] == NAN_ROW // 256 or t[1] == NAN_ROW // 256]
    return A, Cm, want_live


_CASES = {}


def host_product(lib, A, B, nmod, K):
    Af, Bf = np.asfortranarray(A), np.asfortranarray(B)
    out = np.zeros((A.shape[0], B.shape[0]), order="F")
    rc = lib.lmm_dev_emul_host(Af.ctypes.data_as(DP), A.shape[0], Bf.ctypes.data_as(DP), B.shape[0], A.shape[0], B.shape[0], K, nmod, K,
                               out.ctypes.data_as(DP), A.shape[0], None)
    assert rc == 0, lib.lmm_last_error_string()
    return np.ascontiguousarray(out)


def case(lmm, M, N, K, nmod):
    """(A, the host-emulated A A[:N]'), computed once per case and left unchanged, and the same product for the operand of the
    "nan_row" pattern: a row's scaling and residues depend on that row alone, so only row and column NAN_ROW differ, and the host
    entry forms those from the changed operand."""
    key = (M, N, K, nmod)
    if key not in _CASES:
        lib = lmm.load()
        A = operand(M, K, M + N + K + nmod)
        T = host_product(lib, A, A[:N], nmod, K)
        An = A.copy()
        An[NAN_ROW, K // 2 + 3] = np.nan
        Tn = T.copy()
        Tn[NAN_ROW, :] = host_product(lib, An[NAN_ROW:NAN_ROW + 1], An[:N], nmod, K)[0]
        Tn[:, NAN_ROW] = host_product(lib, An, An[NAN_ROW:NAN_ROW + 1], nmod, K)[:, 0]
        for v in (A, T, Tn):
            v.setflags(write=False)
        _CASES[key] = (A, T, Tn)
    return _CASES[key]


CANARY = -0.0      # above the diagonal and in the padding of C: not negligible if the screen looked at it, and any update would show


def run_syrk(lmm, At, lda, M, K, Cm, N, nmod, pad_c=5):
    """C after lmm_dev_syrk_emul, ldc = M + pad_c: (the M x N block, everything else of the buffer)"""
    import torch
    lib = lmm.load()
    ldc = M + pad_c
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    Ch = np.full((N, ldc), CANARY)
    Ch[:, :M] = np.where(lower.T, Cm.T, CANARY)
    Ct = torch.from_numpy(Ch).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_syrk_emul(C.c_void_p(Ct.data_ptr()), ldc, C.c_void_p(At.data_ptr()), lda, M, N, K, nmod)
    assert rc == 0, lib.lmm_last_error_string()
    got = Ct.cpu().numpy()
    return got[:, :M].T, got[:, M:]


def differ(got, want):
    """entries that differ in any bit (a NaN for a NaN; -0 is not +0)"""
    return (np.ascontiguousarray(got).view(np.int64) != np.ascontiguousarray(want).view(np.int64)) & ~(np.isnan(got) & np.isnan(want))


def test_patterns_are_what_they_are_meant_to_be(lmm):
    """A NumPy pass with the rule: the tiles meant to be dead are dead, the others live, at every case; and the situations the screen,
    the compaction, the GEMM's walk and the combine must handle all occur."""
    seen = set()
    for M, N in SHAPES:
        tiles = tile_list(M, N)
        for nk in NKS:
            K = 128 * nk
            A0 = operand(M, K, M + N + K)
            for pattern in PATTERNS:
                A, Cm, want_live = build_c(A0, N, K, pattern, nk)
                live = live_tiles(A, N, K, Cm)
                assert live == want_live, (M, N, K, pattern, live, want_live)
                dead = [t for t in tiles if t not in live]
                if not live:
                    seen.add("all dead")
                if not dead:
                    seen.add("none dead")
                if tiles[0] in dead and tiles[-1] in dead and live:
                    seen.add("first and last id dead")
                if any(tiles[k - 1] in live and tiles[k] in dead and tiles[k + 1] in live for k in range(1, len(tiles) - 1)):
                    seen.add("a dead tile between live ones")
                if any(i == j for i, j in dead):
                    seen.add("a dead diagonal tile")
                if any(i == j for i, j in live) and dead:
                    seen.add("a live diagonal tile beside dead tiles")
                if M % 256 and any(i == M // 256 for i, j in dead):
                    seen.add("a dead tile with rows >= M")
                neg = negligible(A, N, K, Cm)
                bound = bounds(A, N, K)[0]
                if pattern == "threshold":
                    assert neg[600, 290] and neg[601, 291] and not neg[511, 255]
                    assert Cm[600, 290] == 2.0 ** bound[600, 290] and abs(Cm[601, 291]) == 2.0 ** (bound[601, 291] + 1)
                    blk = ~neg[256:512, 0:256]
                    assert blk.sum() == 1 and blk[255, 255]
                    seen.add("threshold")
                if pattern == "specials":
                    for (i, j), (r, c) in zip(want_live, ((256, 0), (511, 511), (700, 3), (520, 300), (780, 40))):
                        blk = ~neg[256 * i:256 * i + 256, 256 * j:256 * j + 256] & (np.arange(256 * i, 256 * i + 256)[:, None] >= np.arange(256 * j, 256 * j + 256)[None, :])[:neg[256 * i:256 * i + 256].shape[0]]
                        assert blk.sum() == 1 and blk[r - 256 * i, c - 256 * j], (i, j, int(blk.sum()))
                    assert np.signbit(Cm[511, 511]) and Cm[511, 511] == 0 and 0 < Cm[700, 3] < 2.0 ** -1022
                    seen.add("specials")
                if pattern == "nan_row":
                    assert np.isnan(A[NAN_ROW]).any() and NAN_ROW < N and len(live) < len(tiles)
                    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
                    assert (neg | bounds(A, N, K)[2] | ~lower).all()      # only the NaN row and column keep tiles alive
                    seen.add("NaN row across tiles that would be dead")
                assert neg[ZERO_ROW, :ZERO_ROW + 1].all() or pattern == "none_dead"
    want = {"all dead", "none dead", "first and last id dead", "a dead tile between live ones", "a dead diagonal tile", "a live diagonal tile beside dead tiles",
            "a dead tile with rows >= M", "threshold", "specials", "NaN row across tiles that would be dead"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("nmod", NMODS)
@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_screened_update_bit_for_bit(lmm, M, N, nk, nmod):
    """Screen on with the poison on, screen off with the poison off: every pattern on every grid against the host entry's bits, and
    the live-tile count against NumPy's."""
    import torch
    lib = lmm.load()
    K = 128 * nk
    A0, T, Tn = case(lmm, M, N, K, nmod)
    tiles = tile_list(M, N)
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    lda = M + 3
    dev = {}
    try:
        for pattern in PATTERNS:
            A, Cm, want_live = build_c(A0, N, K, pattern, nk)
            live = live_tiles(A, N, K, Cm)
            assert live == want_live
            nan = pattern == "nan_row"
            if nan not in dev:
                Ah = np.full((K, lda), np.nan)
                Ah[:, :M] = A.T
                dev[nan] = torch.from_numpy(Ah).cuda()
            with np.errstate(invalid="ignore"):
                want = np.where(lower, Cm - (Tn if nan else T), CANARY)
            # a dead tile's outputs are C itself
            for i, j in tiles:
                if (i, j) not in live:
                    blk = (slice(256 * i, 256 * i + 256), slice(256 * j, 256 * j + 256))
                    assert not (differ(want[blk], Cm[blk]) & lower[blk]).any()
            print(f"syrk_emul {M}x{N}x{K}, nmod = {nmod}, {pattern}: live tiles {len(live)} of {len(tiles)}")
            for screen, poison in ((1, 1), (0, 0)):
                assert lib.lmm_dev_set_emul_screen(screen) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
                for wgs in GRIDS:
                    assert lib.lmm_dev_set_emul_gemm_workgroups(wgs) == 0
                    got, pad = run_syrk(lmm, dev[nan], lda, M, K, Cm, N, nmod)
                    count = lib.lmm_dev_emul_last_live_tiles()
                    assert count == (len(live) if screen else len(tiles)), (pattern, screen, wgs, count, len(live), len(tiles))
                    assert not differ(pad, np.full_like(pad, CANARY)).any()
                    bad = differ(got, want)
                    assert not bad.any(), (pattern, screen, poison, wgs, int(bad.sum()), np.argwhere(bad)[:8])
                    if nan:
                        assert np.all(np.isnan(got[NAN_ROW, :NAN_ROW + 1])) and np.all(np.isnan(got[NAN_ROW:, NAN_ROW]))
    finally:
        reset(lib)


# ---- factorisations with every update of at least 128 columns emulated: the child ----
N_FACT, RIDERS = 2304, ZS.RIDERS
SETTINGS = [(screen, group) for screen in (1, 0) for group in (0, 2)]


def factor_inputs(decaying):
    """tests/test_gpu_emul_block_maxima.py's matrix at n = 2304 (point spacing 1 / 1151, lengthscale 0.02), and a flat one"""
    rng = np.random.default_rng(N_FACT + 1 + decaying)
    x = np.arange(N_FACT) / (ZS.N_FACT - 1.0)
    return ZS.matern52(x, 0.02 if decaying else 50.0) + 0.1 * np.eye(N_FACT), rng.standard_normal((RIDERS, N_FACT))


def child():
    import scipy.linalg as sla
    sys.path.insert(0, ROOT)
    import lmm_amd
    import test_gpu_emul_amax_reuse as AR
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_screen.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_scratch_poison.argtypes = [C.c_int]
    res = {}
    n = N_FACT
    for decaying in (1, 0):
        Kmat, R = factor_inputs(decaying)
        L = np.linalg.cholesky(Kmat)
        want = np.vstack([L, sla.solve_triangular(L, R.T, lower=True).T])
        tri = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((RIDERS, n), dtype=bool)])
        bad_at = n - 52
        Kbad = Kmat.copy()
        Kbad[bad_at, bad_at] = -5.0
        assert lib.lmm_dev_set_f64_emul(1, 128, 16) == 0
        steps = AR.emulated_steps(lib, n + RIDERS, n)
        r = {"steps": steps}
        # on the LAPACK factor, in Float64: the trailing block each emulated update meets (what the columns left of its panel have
        # left of it) and its dead tiles by the rule -- an estimate, good away from the threshold
        dead = []
        full = np.vstack([Kmat, R])
        for j0, h in steps:
            r0 = j0 + h
            P = want[r0:, j0:r0]
            Cb = full[r0:, r0:] - want[r0:, :j0] @ want[r0:n, :j0].T
            M, N = Cb.shape
            live = live_tiles(P, N, h, Cb)
            dead.append([len(tile_list(M, N)) - len(live), len(tile_list(M, N))])
        r["dead_tiles"] = dead
        got, pivots = {}, {}
        assert lib.lmm_dev_set_emul_scratch_poison(1) == 0
        for s in SETTINGS:
            screen, group = s
            assert lib.lmm_dev_set_emul_screen(screen) == 0 and lib.lmm_dev_set_emul_group(group) == 0
            got[s], info = ZS.potrf(lmm_amd, Kmat, R)
            assert info == 0
            _, pivots[s] = ZS.potrf(lmm_amd, Kbad, R)
        lib.lmm_dev_set_emul_screen(-1)
        lib.lmm_dev_set_emul_group(0)
        lib.lmm_dev_set_emul_scratch_poison(0)
        first = got[SETTINGS[0]]
        r["bits_equal"] = [bool(np.array_equal(got[s][tri].view(np.int64), first[tri].view(np.int64))) for s in SETTINGS]
        r["pivots"] = [pivots[s] for s in SETTINGS]
        r["bad_at"] = bad_at
        r["e_emu"] = float(np.linalg.norm((first - want)[tri]) / np.linalg.norm(want[tri]))
        res[str(decaying)] = r
    print(json.dumps(res))


@pytest.fixture(scope="module")
def found():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, LMM_REGION="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    return res


@pytest.mark.parametrize("decaying", [1, 0])
def test_factor_and_pivot_same_with_screen_on_and_off(found, decaying):
    """(screen, group cap) in {1, 0} x {0, 2}, poisoned scratch: factor, rider rows and the failing pivot; 1e-9 of LAPACK, the bar of
    the other emulated factorisations.  The decaying matrix does have tiles to skip (by the rule, on the LAPACK factor)."""
    r = found[str(decaying)]
    print(f"decaying = {decaying}: emulated updates (j0, h) {r['steps']}, dead tiles of each (dead, all) {r['dead_tiles']}, |emulated - LAPACK| / |LAPACK| = {r['e_emu']:.3e}")
    assert len(r["steps"]) >= 3
    assert r["bits_equal"] == [True] * len(SETTINGS), [s for s, ok in zip(SETTINGS, r["bits_equal"]) if not ok]
    assert r["pivots"] == [r["bad_at"] + 1] * len(SETTINGS)
    assert r["e_emu"] <= 1e-9
    assert (sum(d for d, _ in r["dead_tiles"]) > 0) == bool(decaying)      # the flat matrix has none: its panel rows do not decay


# ---- a batch of 5 matrices in groups of 2 + 2 + 1: flags, list and count are rewritten per group ----
ELLS = (200.0, 0.02, 0.5, 0.2, 0.7)


def test_groups_of_a_batch_with_different_dead_tiles(lmm):
    """tests/test_gpu_emul_dead_blocks.py's batch: 5 Matern52 latents with lengthscales from 0.02 to 200 at n = 1100, one lock-step
    batch whose emulated updates walk it in groups of 2 + 2 + 1 (and of as many as fit), with from many dead tiles to none per matrix.
    A group that kept the flags or the list of the group before would skip a live tile or combine poison.  One logpdf whatever the
    screen, the groups and the poison; 1e-9 of the f64 kernels', the bar of that test."""
    import torch
    lib = lmm.load()
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    m, n = len(ELLS), 1100
    p = m
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    y = rng.standard_normal(n * p)
    deads = []
    for ell in ELLS:                                                       # the K = 256 update of the first block column, by the rule
        Km = ZS.matern52(x, ell) + 0.1 * np.eye(n)
        Lc = np.linalg.cholesky(Km)
        live = live_tiles(Lc[256:, :256], n - 256, 256, Km[256:, 256:])
        deads.append(len(tile_list(n - 256, n - 256)) - len(live))
    print(f"dead tiles of the first K = 256 update per latent (of {len(tile_list(n - 256, n - 256))}): {deads}")
    assert deads[0] == 0 and max(deads) >= 3 and len(set(deads)) >= 2
    fs = lmm.independent_mogp([lmm.GP(0.0, lmm.Matern52Kernel(1.0, ell)) for ell in ELLS])
    fx = lmm.ILMM(fs, lmm.Orthogonal(np.eye(p), 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p), 0.1)
    yt = torch.from_numpy(y).cuda()
    vals = {}
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = float(lmm.logpdf(fx, yt))
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        for g, screen, poison in ((2, 1, 1), (2, 0, 1), (0, 1, 1), (0, 0, 0), (2, 1, 0)):
            assert lib.lmm_dev_set_emul_group(g) == 0 and lib.lmm_dev_set_emul_screen(screen) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
            out = (C.c_longlong * (2 + 6 * 64))()
            cnt = lib.lmm_dev_emul_plan(1152 + 64, 1152, m, out, 64)
            groups = {out[2 + 6 * i + 4] for i in range(cnt) if out[2 + 6 * i + 3]}
            assert groups and (groups == {g} if g else min(groups) >= 3), (g, groups)
            vals[g, screen, poison] = float(lmm.logpdf(fx, yt))
    finally:
        lib.lmm_dev_set_emul_group(0)
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
        reset(lib)
    print("5 latents: " + ", ".join(f"{k}: {abs(v - f64) / abs(f64):.3e}" for k, v in vals.items()) + " from f64")
    first = vals[2, 1, 1]
    for k, v in vals.items():
        assert v == first, (k, v, first)
    assert abs(first - f64) <= 1e-9 * abs(f64)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    child()
