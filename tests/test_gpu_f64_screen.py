"""GPU checks of the screen in front of the f64 update launches (DESIGN.md 4.17 "the same screen on the f64 kernel"): a screened
update + leaf step scans its panel for the row maxima, a pass over C marks the 128 x 128 tiles of the launch's tile columns 1.. in
which no entry can change by a bit (emul_negligible, tests/test_f64_screen_rule_host.py), and potrf_node_kernel's work items for
those tiles return at once.  Nothing of that may show in a result, and it must really happen:

(a) lmm_dev_f64_screen_flags (scan + screen of one update shape) returns the flag bytes and the dead count a NumPy pass with the same
    rule finds, for C built so that given tiles are dead; the NumPy pass first asserts the count each pattern was built for;
(b) lmm_dev_potrf with no split-K atomics gives the same factor, rider rows, inverse diagonal blocks and failing pivot with the
    screen on and off, at n = 2304 + 64 rider rows and n = 1152, for a decaying and a flat kernel matrix, under the default plan,
    with the region kernel off (every K = 128 .. 1152 step an update launch: both pipeline depths, the builds with fused bulk
    rows), and with the region kernel off and min_k = 128; the decaying matrix has dead tiles on the device, the flat one has none
    and the vote then makes the later screens return at entry;
(c) five latents with lengthscales 0.02 .. 200 at n = 1152: one logpdf with the screen on and off, for the batch of five and for
    the batches of 2, 2 and 1 latents it splits into (each its own model: a batch's flags belong to it alone).

The emulation is off throughout, so that every update stays on the f64 kernel.  Switches that are read once from the environment go
into a fresh child process per configuration (`python tests/test_gpu_f64_screen.py child <configuration>`), which prints JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MARGIN, T = 56, 128
SHAPES = ((704, 384), (512, 512))
KS = (128, 512, 1024)
PATTERNS = ("all_dead", "none_dead", "alternating", "threshold", "specials", "nan_row")
ZERO_ROW, NAN_ROW = 200, 300      # tile row 1; tile row 2 and, as a column, tile column 2
SUBNORMAL = 3 * 5e-324


def setup(lib):
    lib.lmm_dev_set_f64_screen.argtypes = [C.c_int, C.c_int]
    lib.lmm_dev_set_deterministic.argtypes = [C.c_int]
    lib.lmm_dev_f64_screen_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_f64_screen_stats.restype = C.c_int
    lib.lmm_dev_f64_screen_flags.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = setup(lmm_amd.load())
    yield lmm_amd
    lib.lmm_dev_set_f64_screen(-1, 0)
    lib.lmm_dev_set_deterministic(0)
    lib.lmm_dev_set_f64_emul(-1, 0, 0)


# ---- the rule in NumPy, on 128 x 128 tiles ----
def rest_tiles(M, N):
    return [(i, j) for j in range(1, (N + T - 1) // T) for i in range(j, (M + T - 1) // T)]


def row_exps(A):
    amax = np.abs(A).max(axis=1)
    bad = ~np.isfinite(amax)
    zero = amax == 0
    ok = ~bad & ~zero
    e = np.zeros(A.shape[0], dtype=np.int64)
    m, q = np.frexp(amax[ok])
    e[ok] = np.where(m == 0.5, q - 1, q)
    return e, zero, bad


def bounds(A, N, K):
    e, zero, bad = row_exps(A)
    return (K - 1).bit_length() + e[:, None] + e[None, :N] + MARGIN, zero[:, None] | zero[None, :N], bad[:, None] | bad[None, :N]


def negligible(A, N, K, Cm):
    bound, zero, bad = bounds(A, N, K)
    fin = np.isfinite(Cm) & (Cm != 0)
    ilogb = np.frexp(np.where(fin, Cm, 1.0))[1] - 1
    return fin & ~bad & (zero | (bound <= ilogb))


def live_tiles(A, N, K, Cm):
    M = A.shape[0]
    lower = np.arange(M)[:, None] >= np.arange(N)[None, :]
    live = lower & ~negligible(A, N, K, Cm)
    return [(i, j) for i, j in rest_tiles(M, N) if live[T * i:T * i + T, T * j:T * j + T].any()]


# ---- operands and C with given dead tiles ----
def operand(M, K, seed):
    """Rows scaled 2^-20 .. 2^20 against each other, entries 2^-12 .. 2^-1/2 of the row's scale; even rows have a maximum that is an
    exact power of two.  One all-zero row."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-20, 21, size=M)
    U = rng.choice([-1.0, 1.0], size=(M, K)) * np.exp2(-rng.uniform(0.5, 12, size=(M, K)))
    U[::2, 17] = -1.0
    A = U * np.exp2(q.astype(np.float64))[:, None]
    A[ZERO_ROW] = 0.0
    return A


def build_c(A, N, K, pattern, seed):
    """(C, the live rest tiles the pattern was built for).  A dead tile's entries sit 0 .. 3 binades above their thresholds (the
    zero row's and column's entries 300 binades below: negligible all the same); a live tile's sit 1 .. 4 binades below."""
    M = A.shape[0]
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        bound, zero, _ = bounds(np.where(np.isfinite(A), A, 1.0), N, K)
    up = np.ldexp(1.0 + rng.random((M, N)), bound + rng.integers(0, 4, size=(M, N))) * rng.choice([-1.0, 1.0], size=(M, N))
    up[::3, ::5] = np.ldexp(1.0, bound[::3, ::5])                         # exactly at the threshold
    up[zero] = np.ldexp(1.0 + rng.random(int(zero.sum())), -300)
    down = np.ldexp(1.0 + rng.random((M, N)), bound - 1 - rng.integers(0, 4, size=(M, N)))
    tiles = rest_tiles(M, N)
    Cm = up.copy()
    want = []
    blk = lambda i, j: (slice(T * i, T * i + T), slice(T * j, T * j + T))
    if pattern == "none_dead":
        Cm = np.where(zero, up, down)
        # the tile row of the zero row keeps live entries in its other rows
        want = list(tiles)
    elif pattern == "alternating":
        for k, (i, j) in enumerate(tiles):
            if k % 2 == 0:
                Cm[blk(i, j)] = np.where(zero[blk(i, j)], up[blk(i, j)], down[blk(i, j)])
                want.append((i, j))
    elif pattern == "threshold":
        # ONE entry, the largest double below its threshold, in the last 16-column chunk of an off-diagonal tile; its neighbour in the
        # tile row keeps an entry exactly at the threshold and stays dead
        i, j = tiles[-1][0], 1
        assert i > j + 1 or (i, j + 1) in tiles
        r, c = T * i + 37, T * j + T - 3
        assert not zero[r, c]
        Cm[r, c] = np.nextafter(np.ldexp(1.0, bound[r, c]), 0.0)
        if (i, j + 1) in tiles:
            Cm[r, c + T] = -np.ldexp(1.0, bound[r, c + T])
        want = [(i, j)]
    elif pattern == "specials":
        for (i, j), v in zip(tiles, (0.0, -0.0, SUBNORMAL, np.inf, np.nan)):
            r, c = T * i + T - 1 - 2 * j, T * j + 3 + i                  # on or below the diagonal: row >= column
            if r >= M:
                r = M - 1
            assert r >= c
            Cm[r, c] = v
            want.append((i, j))
    elif pattern == "nan_row":
        want = [(i, j) for i, j in tiles if i == NAN_ROW // T or (j == NAN_ROW // T and NAN_ROW < N)]
    return Cm, sorted(want)


@pytest.mark.parametrize("M,N", SHAPES)
def test_flags_and_dead_count_equal_the_rule(lmm, M, N):
    import torch
    lib = lmm.load()
    MT, NT = (M + T - 1) // T, (N + T - 1) // T
    tiles = rest_tiles(M, N)
    assert len(tiles) >= 6
    for K in KS:
        A0 = operand(M, K, 100 * K + M)
        for pattern in PATTERNS:
            A = A0.copy()
            if pattern == "nan_row":
                A[NAN_ROW, 5] = np.nan
            Cm, want = build_c(A, N, K, pattern, K + M + len(pattern))
            with np.errstate(invalid="ignore"):
                live = sorted(live_tiles(A, N, K, Cm))
            assert live == want, (pattern, K, live, want)                 # the pattern gives what it was built for
            if pattern == "all_dead":
                assert live == []
            Ad = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()       # [k][row], lda = M
            Cd = torch.from_numpy(np.ascontiguousarray(Cm.T)).cuda()
            before = Cd.clone()
            flags = np.zeros(MT * NT, dtype=np.uint8)
            dead = C.c_int(-1)
            torch.cuda.synchronize()
            rc = lib.lmm_dev_f64_screen_flags(C.c_void_p(Cd.data_ptr()), M, C.c_void_p(Ad.data_ptr()), M, M, N, K, C.c_void_p(flags.ctypes.data), C.byref(dead))
            assert rc == 0, lib.lmm_last_error_string()
            flags = flags.reshape(MT, NT)
            expect = np.full((MT, NT), 0xFF, dtype=np.uint8)
            for i, j in tiles:
                expect[i, j] = 1 if (i, j) in live else 0
            print(f"f64 screen {M}x{N}x{K}, {pattern}: dead {dead.value} of {len(tiles)}")
            assert np.array_equal(flags, expect), (pattern, K, flags, expect)
            assert dead.value == len(tiles) - len(live)
            assert torch.equal(Cd.view(torch.int64), before.view(torch.int64))      # the screen only reads C


# ---- factorisations: the child ----
CONFIGS = {
    "default": ({}, 512),
    "region_off": ({"LMM_REGION": "0"}, 512),
    "region_off_min_k_128": ({"LMM_REGION": "0"}, 128),
}
FACT_SHAPES = ((2304, 64), (1152, 0))


def matern52(x, ell):
    r = np.abs(x[:, None] - x[None, :]) / ell
    return (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)


def factor_inputs(n, riders, decaying):
    rng = np.random.default_rng(n + decaying)
    x = np.arange(n) / 1151.0
    return matern52(x, 0.02 if decaying else 50.0) + 0.1 * np.eye(n), rng.standard_normal((riders, n))


def potrf(lmm, Kmat, R):
    """(factor with the rider rows below it, inverse diagonal blocks, info) from lmm_dev_potrf"""
    import torch
    lib = lmm.load()
    n, nr = Kmat.shape[0], Kmat.shape[0] + R.shape[0]
    full = np.vstack([np.tril(Kmat), R])
    A = torch.from_numpy(np.ascontiguousarray(full.T)).cuda()
    W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), nr, n, nr, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0, lib.lmm_last_error_string()
    return A.cpu().numpy().T, W.cpu().numpy(), int(info.item())


def stats(lib):
    out = (C.c_int * (5 * 256))()
    n = lib.lmm_dev_f64_screen_stats(1, out, 256)
    assert 0 <= n <= 256
    return [list(out[5 * i:5 * i + 5]) for i in range(n)]


def child(config):
    sys.path.insert(0, ROOT)
    import lmm_amd
    lmm_amd.init(0)
    lib = setup(lmm_amd.load())
    min_k = CONFIGS[config][1]
    assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0 and lib.lmm_dev_set_deterministic(1) == 0
    assert lib.lmm_dev_f64_screen_stats(1, None, 0) >= 0
    res = {}
    for n, riders in FACT_SHAPES:
        for decaying in (1, 0):
            Kmat, R = factor_inputs(n, riders, decaying)
            tri = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((riders, n), dtype=bool)])
            bad_at = n - 52
            Kbad = Kmat.copy()
            Kbad[bad_at, bad_at] = -5.0
            got = {}
            for on in (1, 0):
                assert lib.lmm_dev_set_f64_screen(on, min_k) == 0
                F, W, info = potrf(lmm_amd, Kmat, R)
                st = stats(lib)
                _, _, pivot = potrf(lmm_amd, Kbad, R)
                got[on] = (F, W, info, st, pivot)
            L = np.linalg.cholesky(Kmat)
            res[f"{n}_{decaying}"] = {
                "factor_equal": bool(np.array_equal(got[1][0][tri].view(np.int64), got[0][0][tri].view(np.int64))),
                "inverse_equal": bool(np.array_equal(got[1][1].view(np.int64), got[0][1].view(np.int64))),
                "info": [got[1][2], got[0][2]], "pivots": [got[1][4], got[0][4]], "bad_at": bad_at,
                "stats_on": got[1][3], "stats_off": got[0][3],
                "err": float(np.linalg.norm((got[1][0][:n] - L)[tri[:n]]) / np.linalg.norm(L)),
            }
    lib.lmm_dev_set_f64_screen(-1, 0)
    print(json.dumps(res))


_FOUND = {}


def found(config):
    if config not in _FOUND:
        env = dict(os.environ, LMM_DETERMINISTIC="1", **CONFIGS[config][0])
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", config], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        _FOUND[config] = json.loads(out.stdout.strip().splitlines()[-1])
    return _FOUND[config]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("n,riders", FACT_SHAPES)
@pytest.mark.parametrize("decaying", [1, 0])
def test_factorisation_same_with_screen_on_and_off(config, n, riders, decaying):
    r = found(config)[f"{n}_{decaying}"]
    print(f"{config}, n = {n} + {riders}, decaying = {decaying}: screened updates (M, N, K, dead, ran) {r['stats_on']}; |factor - LAPACK| / |LAPACK| = {r['err']:.3e}")
    assert r["factor_equal"] and r["inverse_equal"]
    assert r["info"] == [0, 0] and r["pivots"] == [r["bad_at"] + 1] * 2
    assert r["err"] <= 1e-9                                               # the bar of the other factorisation tests against LAPACK
    assert r["stats_off"] == []                                           # off: no step is screened
    st = r["stats_on"]
    assert len(st) >= 1 and all(s[2] >= CONFIGS[config][1] and s[1] > 128 for s in st)
    if config != "default":
        assert {s[2] >= 1024 for s in st} == {True, False} or n < 2304    # both pipeline depths at n = 2304
    wide = [k for k, s in enumerate(st) if (s[1] + T - 1) // T >= 4]      # the vote: the first screened update with 4 tile columns
    assert wide
    v = wide[0]
    if decaying:
        assert st[v][3] > 0 and all(s[4] == 1 for s in st)                # dead tiles on the device, and every screen ran
    else:
        assert all(s[3] == 0 for s in st)                                 # data that does not decay has none ...
        assert all(s[4] == 1 for s in st[:v + 1]) and all(s[4] == 0 for s in st[v + 1:])      # ... and once the vote found that, the later screens returned at entry
        assert n < 2304 or len(st) > v + 1


# ---- (c) five latents, lengthscales 0.02 .. 200 ----
ELLS = (200.0, 0.02, 0.5, 0.2, 0.7)


def test_logpdf_same_with_screen_on_and_off(lmm):
    import torch
    lib = lmm.load()
    n = 1152
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    xt = torch.from_numpy(x).cuda()
    vals = {}
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0 and lib.lmm_dev_set_deterministic(1) == 0
        assert lib.lmm_dev_f64_screen_stats(1, None, 0) >= 0
        for group in ((0, 1, 2, 3, 4), (0, 1), (2, 3), (4,)):
            m = len(group)
            y = torch.from_numpy(np.random.default_rng(m).standard_normal(n * m)).cuda()
            fs = lmm.independent_mogp([lmm.GP(0.0, lmm.Matern52Kernel(1.0, ELLS[k])) for k in group])
            fx = lmm.ILMM(fs, lmm.Orthogonal(np.eye(m), 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(xt, m), 0.1)
            for on in (1, 0):
                assert lib.lmm_dev_set_f64_screen(on, 512) == 0
                vals[group, on] = float(lmm.logpdf(fx, y))
                if on:
                    st = stats(lib)
                    print(f"latents {group}: screened updates (M, N, K, dead, ran) {st}")
                    assert len(st) >= 1
                    if group == (0, 1, 2, 3, 4):
                        assert sum(s[3] for s in st) > 0                  # the short lengthscales have dead tiles
            assert vals[group, 1] == vals[group, 0], (group, vals[group, 1], vals[group, 0])
    finally:
        lib.lmm_dev_set_f64_screen(-1, 0)
        lib.lmm_dev_set_deterministic(0)
        lib.lmm_dev_f64_screen_stats(0, None, 0)
        lib.lmm_dev_set_f64_emul(-1, 0, 0)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    child(sys.argv[2])
