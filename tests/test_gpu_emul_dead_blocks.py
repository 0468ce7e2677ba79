"""GPU checks of "dead blocks are never written" in the int8 emulation's convert: with the zero skip on, a piece of
16 rows x 128 k whose truncated integers are all zero is read once, not turned into residues and not stored, and only the dead pieces
of blocks the GEMM may stage (the live ones, and block 0) get zeros from emul_zero_fill_kernel.  A dead block therefore holds whatever
was in the residue scratch before.  lmm_dev_set_emul_scratch_poison(1) fills that scratch with a non-zero byte before every convert,
so a GEMM stage that read a block nobody wrote would multiply garbage: lmm_dev_syrk_emul must still equal the host entry
lmm_dev_emul_host (which knows nothing of masks) in every bit, on every grid of the persistent GEMM, with the skip and the poison on
and off; a factorisation whose emulated updates share one scratch block, and a batch that goes through it in groups, must not change.

The operands, the reference and the helpers are those of tests/test_gpu_emul_zero_skip.py (one cache of cases for both files)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_emul_zero_skip as ZS

pytestmark = pytest.mark.gpu

GRIDS = (1, 2, 3, 5, 7, 9, 0)                                            # workgroups of the persistent GEMM; 0: the default
NKS = (1, 2, 3, 5, 9)
SHAPES = ((320, 320), (768, 256))
NMODS = (8, 16)


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_set_f64_emul_rule.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    lib.lmm_dev_set_emul_group.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_scratch_poison.argtypes = [C.c_int]
    lib.lmm_dev_set_emul_scratch_poison.restype = C.c_int
    yield lmm_amd
    reset(lib)


def reset(lib):
    lib.lmm_dev_set_emul_scratch_poison(0)
    lib.lmm_dev_set_emul_zero_skip(-1)
    lib.lmm_dev_set_emul_gemm_workgroups(0)
    lib.lmm_dev_set_emul_group(0)
    lib.lmm_dev_set_f64_emul(-1, 0, 0)
    lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0)


def live_pieces(A, b):
    """[16-row piece][K block] -> some truncated integer of the piece is not zero (ZS.live_blocks at the convert's own granularity)."""
    M, K = A.shape
    amax = np.abs(A).max(axis=1)
    ok = np.isfinite(amax) & (amax > 0)
    e = np.zeros(M, dtype=np.int64)
    e[ok] = np.ceil(np.log2(amax[ok])).astype(np.int64)
    ints = np.zeros_like(A)
    ints[ok] = np.trunc(np.ldexp(A[ok], (b - e[ok])[:, None]))
    nz = ints != 0
    return np.array([[bool(nz[r:r + 16, k:k + 128].any()) for k in range(0, K, 128)] for r in range(0, M, 16)])


def features(lmm, M, N, K, nmod):
    """What the operands of a case hold, found in NumPy from the matrix alone (the convert's rule)."""
    A, want, live, variant = ZS.case(lmm, M, N, K, nmod)
    b = ZS.bit_budget(lmm, nmod, K)
    nk = K // 128
    live = np.array(live)                                                 # [256-row block][K block]
    pieces = live_pieces(A, b)
    f = set()
    for r in range(live.shape[0]):
        on = np.flatnonzero(live[r])
        meant = sorted(ZS.pattern(M, nk, variant)[r]["live"])             # beside the block kept alive by one boundary entry
        if len(meant) == 1 and nk >= 3 and live[r, meant[0]]:
            f.add(("only", "first" if meant[0] == 0 else "last" if meant[0] == nk - 1 else "middle"))
        f.add("block 0 live" if live[r, 0] else "block 0 dead")
        for k in on:                                                      # a dead 16-row piece of real rows inside a live block
            rows = range(16 * r, min(16 * r + 16, (M + 15) // 16))
            if any(not pieces[p, k] for p in rows):
                f.add("dead piece in a live block")
    stages = {}
    for i in range(live.shape[0]):
        for j in range(min(i + 1, (N + 255) // 256)):
            both = int((live[i] & live[j]).sum())
            if both == 0:
                f.add("empty intersection")
            stages[(i, j)] = max(1, both)
    if len(set(stages.values())) > 1:
        f.add("unequal tile lengths")
    if {1, 2, nk} <= set(stages.values()) and nk > 2:
        f.add("1, 2 and all stages")
    if M % 256:
        f.add("padding rows")
    assert not A[ZS.ZERO_ROW].any() and np.isnan(A[ZS.NAN_ROW]).any()
    return f


def test_patterns_are_what_they_are_meant_to_be(lmm):
    """Every situation the convert and the fill must handle occurs in the cases below (each case is also checked against its own
    specification by ZS.case).  The boundary entries 2^-(b+1) (gone) and 2^-(b-1) (kept) of the row maximum are part of every case
    with more than one K block: ZS.operands puts them there and ZS.case checks that the blocks holding them are dead / live."""
    seen = set()
    for M, N in SHAPES:
        for nk in NKS:
            for nmod in NMODS:
                seen |= features(lmm, M, N, 128 * nk, nmod)
    want = {("only", "first"), ("only", "middle"), ("only", "last"), "block 0 live", "block 0 dead", "dead piece in a live block",
            "empty intersection", "unequal tile lengths", "1, 2 and all stages", "padding rows"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("nmod", NMODS)
@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_poisoned_scratch_bit_for_bit(lmm, M, N, nk, nmod):
    """Poison and skip on: every grid.  Then skip off (poison on) and poison off (skip on), one capped grid and the default each: the
    same bits."""
    lib = lmm.load()
    K = 128 * nk
    A, want, live, variant = ZS.case(lmm, M, N, K, nmod)
    assert np.isnan(want[ZS.NAN_ROW, 0]) and np.isnan(want[M - 1, ZS.NAN_ROW]) and not np.isnan(want[M - 1, 0])
    try:
        for skip, poison, grids in ((1, 1, GRIDS), (0, 1, (3, 0)), (1, 0, (3, 0)), (0, 0, (3,))):
            assert lib.lmm_dev_set_emul_zero_skip(skip) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
            for wgs in grids:
                assert lib.lmm_dev_set_emul_gemm_workgroups(wgs) == 0
                got, pad, lower = ZS.run_syrk(lmm, A, N, nmod)
                assert np.all(pad == ZS.CANARY) and np.all(got[~lower] == ZS.CANARY)
                bad = ZS.same_bits(got, want, lower)
                assert not bad.any(), (skip, poison, wgs, int(bad.sum()), np.argwhere(bad)[:8])
                assert np.all(got[ZS.ZERO_ROW, :ZS.ZERO_ROW + 1] == 0.0)
                assert np.all(np.isnan(got[ZS.NAN_ROW, :ZS.NAN_ROW + 1])) and np.all(np.isnan(got[ZS.NAN_ROW:, ZS.NAN_ROW]))
    finally:
        reset(lib)


# ---- one factorisation: n = 1152 and 64 rider rows.  ZS.RULE emulates its K = 640 update; with the output bar of the rule at 0 the
# K = 256, 384, 640 and 256 updates are all emulated and go through ONE scratch block one after the other, so a later, shallower update
# finds the deeper one's residues (or the poison) in the blocks it does not write. ----
RULES = (ZS.RULE, (ZS.RULE[0], ZS.RULE[1], 0.0))


@pytest.mark.parametrize("rule", RULES, ids=["one level", "four levels"])
@pytest.mark.parametrize("decaying", [1, 0])
def test_factorisation_same_with_poisoned_scratch(lmm, decaying, rule):
    """The factor (rider rows included) is identical with the skip on / off and the poison on / off, matches LAPACK within the bars of
    ZS.test_factorisation_same_with_skip_on_and_off (1e-9 relative, and no worse than twice the f64 kernels' own error), and a matrix
    that is not positive definite reports the same pivot in all four settings."""
    import scipy.linalg as sla
    lib = lmm.load()
    Kmat, R = ZS.factor_inputs(decaying)
    n, riders = ZS.N_FACT, ZS.RIDERS
    L = np.linalg.cholesky(Kmat)
    want = np.vstack([L, sla.solve_triangular(L, R.T, lower=True).T])
    tri = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((riders, n), dtype=bool)])
    bad_at = 1100
    Kbad = Kmat.copy()
    Kbad[bad_at, bad_at] = -5.0
    settings = ((1, 1), (1, 0), (0, 1), (0, 0))                           # (skip, poison)
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64, info = ZS.potrf(lmm, Kmat, R)
        assert info == 0
        lib.lmm_dev_set_f64_emul(-1, 0, 0)
        assert lib.lmm_dev_set_f64_emul_rule(*rule) == 0
        ups = ZS.emulated_updates(lmm, n + riders, n)
        assert (n + riders - 640, 512, 640) in ups, ups
        assert len(ups) == (1 if rule == ZS.RULE else 4), ups
        got, pivots = {}, {}
        for skip, poison in settings:
            assert lib.lmm_dev_set_emul_zero_skip(skip) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
            got[skip, poison], info = ZS.potrf(lmm, Kmat, R)
            assert info == 0
            _, pivots[skip, poison] = ZS.potrf(lmm, Kbad, R)
    finally:
        reset(lib)
    for s in settings[1:]:
        assert np.array_equal(got[s][tri].view(np.int64), got[1, 1][tri].view(np.int64)), s
    assert pivots == {s: bad_at + 1 for s in settings}
    nrm = np.linalg.norm(want[tri])
    e_emu, e_f64 = np.linalg.norm((got[1, 1] - want)[tri]) / nrm, np.linalg.norm((f64 - want)[tri]) / nrm
    dead = [sum(1 for v in row if not v) for row in ZS.live_blocks(got[1, 1][640:, :640], ZS.bit_budget(lmm, 16, 640))]
    print(f"decaying = {decaying}, emulated updates {ups}: |emulated - LAPACK| / |LAPACK| = {e_emu:.3e}, f64 kernels {e_f64:.3e}; "
          f"dead K blocks of 5 per 256-row block of the K = 640 panel: {dead}")
    assert e_emu <= 1e-9
    assert e_emu <= 2.0 * e_f64
    assert (sum(dead) > 0) == bool(decaying)


# ---- a batch of 5 matrices in groups of 2 + 2 + 1: masks and bitmap are rewritten per group ----
ELLS = (200.0, 0.02, 0.5, 0.2, 0.7)


def test_groups_of_a_batch_with_different_live_patterns(lmm):
    """5 Matern52 latents with lengthscales from 0.02 to 200 at n = 1100 are one lock-step batch whose K = 640 panels have from many
    dead blocks to none; its emulated updates walk it in groups of 2 + 2 + 1 (and of 1, and of as many as fit).  A group that kept the
    masks or the unwritten-piece bits of the group before would stage poison, or leave a live block out.  Integer sums are exact: the
    logpdf is the same Float64 whatever the groups, the skip and the poison; against the f64 kernels it is held to 1e-9, the bar of the
    emulated factorisations against LAPACK."""
    import torch
    lib = lmm.load()
    m, n = len(ELLS), 1100
    p = m
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    y = rng.standard_normal(n * p)
    b = ZS.bit_budget(lmm, 16, 640)
    deads = []
    for ell in ELLS:                                                       # the patterns do differ per matrix
        Lc = np.linalg.cholesky(ZS.matern52(x, ell) + 0.1 * np.eye(n))
        deads.append(sum(1 for row in ZS.live_blocks(Lc[640:, :640], b) for v in row if not v))
    print(f"dead K blocks of the K = 640 panel per latent (of 10): {deads}")
    assert deads[0] == 0 and max(deads) >= 8 and len(set(deads)) >= 4
    fs = lmm.independent_mogp([lmm.GP(0.0, lmm.Matern52Kernel(1.0, ell)) for ell in ELLS])
    fx = lmm.ILMM(fs, lmm.Orthogonal(np.eye(p), 0.5 + np.arange(m) / m))(lmm.MOInputIsotopicByOutputs(torch.from_numpy(x).cuda(), p), 0.1)
    yt = torch.from_numpy(y).cuda()
    vals = {}
    try:
        assert lib.lmm_dev_set_f64_emul(0, 256, 16) == 0
        f64 = float(lmm.logpdf(fx, yt))
        assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        for g, skip, poison in ((2, 1, 1), (2, 1, 0), (2, 0, 1), (1, 1, 1), (0, 1, 1), (0, 0, 0)):
            assert lib.lmm_dev_set_emul_group(g) == 0 and lib.lmm_dev_set_emul_zero_skip(skip) == 0 and lib.lmm_dev_set_emul_scratch_poison(poison) == 0
            out = (C.c_longlong * (2 + 6 * 64))()
            cnt = lib.lmm_dev_emul_plan(1152 + 64, 1152, m, out, 64)
            groups = {out[2 + 6 * i + 4] for i in range(cnt) if out[2 + 6 * i + 3]}
            assert groups and (groups == {g} if g else min(groups) >= 3), (g, groups)
            vals[g, skip, poison] = float(lmm.logpdf(fx, yt))
    finally:
        reset(lib)
    print("5 latents: " + ", ".join(f"{k}: {abs(v - f64) / abs(f64):.3e}" for k, v in vals.items()) + " from f64")
    first = vals[2, 1, 1]
    for k, v in vals.items():
        assert v == first, (k, v, first)
    assert abs(first - f64) <= 1e-9 * abs(f64)
