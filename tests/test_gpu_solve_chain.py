"""-m gpu: the chain behind every dense gradient and every posterior -- potrf_batch -> launch_backsolve (alpha = L^-T z) ->
trsm_rec(tri) (R = L^-T) -> launch_syrk_upper_set (K^-1) -> grad_reduce -- element-wise against float64 host references, through the
building blocks lmm_dev_backsolve and lmm_dev_factor_inverse (include/lmm_hip.h), and then on a busy device through the library's own
entry points.

Inputs of the building blocks: tests/test_gpu_parity.py::test_potrf_vs_lapack's K = G G' / n + I / 2 (condition number about 9), ld =
NC + 2, padding diagonal 1; the factor and the inverse diagonal blocks come from lmm_dev_potrf and the factor is read back, so that the
reference solves with the GPU's own L and only the solve is under test.  Errors are relative to max|reference|; the tolerance is
max(1e-10, 100 DELTA) with the host floors DELTA of tests/test_solve_chain_host.py (5.9e-16 and 2.3e-15, so 1e-10).  Every test prints
its largest error in a line beginning `solve_chain:` (profiles/solve_chain/errors.txt is those lines of one run).

Back substitution.  n = 1, 64, 65, 256, 300, 320, 333, 1088, 2112 give 1, 1, 2, 4, 5, 5, 6, 17, 33 blocks of 64: the launches with one
workgroup per matrix (steps b <= 4), the `col < 64 b` guard of a last, partly filled workgroup (b = 1, 2, 3, 5, ...), the first step
with two workgroups (b = 5) and sizes that are no multiple of 64; nb = 1, 3, 32 matrices (three distinct factors, matrix j of a batch
holding a copy of factor j mod 3, every matrix with its own right-hand side, every alpha checked).  The words of z from n on -- zero up
to 64 nblk, as every caller leaves them, arbitrary beyond -- and the guard words around every z are bitwise what they were.  One
oversubscribed case: 32 right-hand sides on ONE 16384-column factor (stride 0), 64 x 32 workgroups in the largest step launch, where
workgroups of one launch start at visibly different times.

Inverse.  R = L^-T: its upper triangle against the host's, its strict lower triangle exactly 0; lower(A) against (L L')^-1; the two
padding rows of every column of A and R bitwise untouched.  trsm_rec(tri = true) calls launch_gemm_nt with lower = 0, M = j0 + h rows,
N = w - h columns and K = h, h = potrf_split(w) (a multiple of 128 once w >= 256).  Branches of launch_gemm_nt and the cases that
launch them (nb = 1 / nb = 3 unless stated; 256 CUs):

| branch of launch_gemm_nt                                   | first reached at                                                    |
|---|---|
| `set`: in-place 64-column leaf, gemm44_kernel<64, true>    | NC = 64 (the only launch), every larger NC                           |
| narrow N <= 64, gemm44_kernel<64, false>, no split         | NC = 128 (64 x 64 x 64)                                              |
| narrow, split-K                                            | NC = 192 (128 x 64 x 128, split 2), NC = 320 (256 x 64 x 256, split 4) |
| gemm16p_kernel<1> (K < 1024), split-K                      | NC = 256 (128 x 128 x 128, split 2); NC = 1088 (640 x 448 x 640, split 10 at nb = 1) |
| gemm16p_kernel<1>, no split, partial last column tile      | NC = 2112, nb = 3 (1664 x 448 x 512) and NC = 1088, nb = 32          |
| gemm16p_kernel<2> (K >= 1024)                              | NC = 2112 (1152 x 960 x 1152: split 3 at nb = 1, none at nb = 3)     |
| LMM_DETERMINISTIC=1 (no split anywhere)                    | NC = 256 and 1088, nb = 1 and 3, in a child process (the switch is read once) |
| ragged rows, gemm16h_kernel<true> (M % 128 == 64, K >= 1024) | not reachable: M = j0 + h is an odd multiple of 64 only below a split of w < 256, where K = h <= 128 |
| underfilled 64 x 128 tiles, gemm16h_kernel<false>          | not reachable: it needs lower != 0 and the triangular solve passes lower = 0 (the factorisation's updates reach it) |

(nb = 32 at NC = 128: a full batch in blockIdx.y.  The two unreachable branches are covered where they are reachable, by
tests/test_gpu_potrf_plan.py and tests/test_gpu_parity.py through lmm_dev_potrf.)

Busy device (one child process, LMM_NSTREAMS=4 LMM_BATCH=16): 64 latents over d = 1 cycling Matern12 / Matern32 / Matern52, p = 64,
n = 4096 sorted inputs, sigma2 = 0.2 -- four concurrent batches of 16.  logpdf_and_gradient, posterior -> lmm_latent_marginals and
mean_and_var at 64 new inputs, against (a) the state-space path (statespace_logpdf_and_gradient, statespace_mean_and_var(xs=)), which
shares no kernel with the chain, with the error measure and tolerance of tests/test_gpu_statespace_grad.py, and (b) a float64 NumPy
reference of latents 0, 15, 16 and 63 alone: alpha = C^-1 delta (recovered from the "y" gradient: U is square and orthogonal, so
alpha_l = -sqrt(S_l) U_l' dy), sum(alpha), (alpha' K alpha - tr C^-1 K) / (2 v), the lengthscale term and the posterior marginals.
Tolerance of (b): 1e-10, of max|reference| for arrays and of the sum of the absolute values of the terms for the three scalars.  The
chain's rounding error is of order eps cond(C); here the spacing is 0.05, v, l <= 2 and the noise sigma2 / S_l >= 0.1, so
cond(C) <= (v l sqrt(2 pi) / 0.05 + 0.1) / 0.1 ~ 2e3 and eps cond(C) ~ 5e-13, two hundred times below.

Measured on an MI355X (profiles/solve_chain/errors.txt): back substitution <= 2.7e-15, 16384 columns x 32 included; inverse <= 5.4e-16
(R) and <= 4.8e-15 (K^-1); busy device <= 2.9e-14 against the state-space path in every array and <= 4.9e-11 in the per-latent scalars
(relative to each scalar itself), <= 2.5e-14 against the host.  With the back substitution of the build before (one workgroup stored
alpha_b over the z_b that the other workgroups of the launch load; profiles/solve_chain/parent.txt) the busy gradient was off by 0.15
of max|y-gradient|, latent alphas by 0.08 to 0.31, and the oversubscribed single-stream case by 1.1e-2."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_solve_chain_host as H

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BACKSOLVE_N = (1, 64, 65, 256, 300, 320, 333, 1088, 2112)
INVERSE_NC = (64, 128, 192, 256, 320, 1088, 2112)
INVERSE_CASES = [(nc, nb) for nc in INVERSE_NC for nb in (1, 3)] + [(128, 32)]
DETERMINISTIC_CASES = [(256, 1), (256, 3), (1088, 1), (1088, 3)]
GUARD = 8


@pytest.fixture(scope="module")
def lmm():
    import lmm_amd
    lmm_amd.init(0)
    return lmm_amd


@pytest.fixture(scope="module")
def tol():
    return H.tolerance()


# ---------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------
_FACTORS = {}


def factors(lmm, n):
    """Three distinct matrices of size n factored by lmm_dev_potrf: (A (3, NC, ld) on the device, column-major per matrix;
    W (3, NC / 64 * 4096); the n x n factors read back), computed once per n and never modified."""
    import torch
    if n not in _FACTORS:
        lib = lmm.load()
        NC = (n + 63) // 64 * 64
        ld = NC + 2
        A = torch.zeros(3, NC, ld, dtype=torch.float64, device="cuda")
        W = torch.zeros(3, NC // 64 * 4096, dtype=torch.float64, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        Lh = []
        for j in range(3):
            full = np.zeros((NC, NC))
            full[:n, :n] = np.tril(H.spd(n, j))
            full[np.arange(n, NC), np.arange(n, NC)] = 1.0
            A[j, :, :NC] = torch.from_numpy(full.T.copy()).cuda()
            torch.cuda.synchronize()      # raw pointers cross the ABI: torch's asynchronous producers of these tensors must be done
            rc = lib.lmm_dev_potrf(C.c_void_p(A[j].data_ptr()), NC, NC, ld, C.c_void_p(W[j].data_ptr()), n, C.c_void_p(info.data_ptr()))
            assert rc == 0, lib.lmm_last_error_string()
            assert int(info.item()) == 0
            Lh.append(np.tril(A[j, :, :NC].T.cpu().numpy()[:n, :n]))
        _FACTORS[n] = (A, W, Lh)
    return _FACTORS[n]


def batch_of(lmm, n, nb):
    """(A (nb, NC, ld), W, host factors, factor index of each matrix): matrix j holds a copy of factor j mod 3."""
    A3, W3, Lh = factors(lmm, n)
    idx = [j % 3 for j in range(nb)]
    return A3[idx].clone(), W3[idx].clone(), Lh, idx


def run_backsolve(lmm, A, W, nblk, ld, Z, n, shared=False):
    """alpha (nb, n) of lmm_dev_backsolve for the right-hand sides Z (nb, n), after asserting that nothing but z's first n words
    changed: the buffer holds GUARD arbitrary words before, between and after the vectors, zeros from n to 64 nblk."""
    import torch
    lib = lmm.load()
    nb, NC = Z.shape[0], 64 * nblk
    stride = NC + GUARD
    buf = np.random.default_rng([n, nb, 11]).standard_normal(GUARD + nb * stride)
    for j in range(nb):
        buf[GUARD + j * stride: GUARD + j * stride + n] = Z[j]
        buf[GUARD + j * stride + n: GUARD + j * stride + NC] = 0.0
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_backsolve(A.data_ptr(), 0 if shared else A.stride(0), ld, W.data_ptr(), 0 if shared else W.stride(0), nblk,
                               dev.data_ptr() + 8 * GUARD, stride, nb)
    assert rc == 0, lib.lmm_last_error_string()
    got = dev.cpu().numpy()
    keep = np.ones(buf.size, dtype=bool)
    for j in range(nb):
        keep[GUARD + j * stride: GUARD + j * stride + n] = False
    assert np.array_equal(got.view(np.int64)[keep], buf.view(np.int64)[keep])      # bitwise, the zeros' signs included
    return np.stack([got[GUARD + j * stride: GUARD + j * stride + n] for j in range(nb)])


@pytest.mark.parametrize("nb", [1, 3, 32])
@pytest.mark.parametrize("n", BACKSOLVE_N)
def test_backsolve_vs_host(lmm, tol, n, nb):
    A, W, Lh, idx = batch_of(lmm, n, nb)
    nblk = A.shape[1] // 64
    Z = np.random.default_rng([n, nb, 7]).standard_normal((nb, n))
    got = run_backsolve(lmm, A, W, nblk, A.shape[2], Z, n)
    worst = 0.0
    for f in set(idx):
        js = [j for j in range(nb) if idx[j] == f]
        ref = H.backsolve_ref(Lh[f], Z[js].T).T
        for j, r in zip(js, ref):
            worst = max(worst, float(np.abs(got[j] - r).max() / np.abs(r).max()))
    print(f"solve_chain: backsolve n={n} nblk={nblk} nb={nb}: largest error {worst:.3e} of max|alpha|")
    assert np.isfinite(got).all() and worst <= tol[0], worst


def test_backsolve_oversubscribed(lmm, tol):
    """32 right-hand sides on one shared 16384-column factor: up to 64 x 32 workgroups per step launch, more than the device holds at
    once.  The matrix is assembled and factored on the device; the reference is torch's triangular solve on the CPU, with the factor
    read back."""
    import torch
    lib = lmm.load()
    n, nb = 16384, 32
    ld = n + 2
    gen = torch.Generator(device="cuda").manual_seed(n)
    G = torch.randn(n, n + 8, dtype=torch.float64, device="cuda", generator=gen)
    A = torch.zeros(n, ld, dtype=torch.float64, device="cuda")
    A[:, :n] = torch.triu(G @ G.T / n + 0.5 * torch.eye(n, dtype=torch.float64, device="cuda"))      # column-major lower triangle
    del G
    W = torch.zeros(n // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), n, n, ld, C.c_void_p(W.data_ptr()), n, C.c_void_p(info.data_ptr())) == 0, lib.lmm_last_error_string()
    assert int(info.item()) == 0
    Z = np.random.default_rng([n, nb, 7]).standard_normal((nb, n))
    got = run_backsolve(lmm, A, W, n // 64, ld, Z, n, shared=True)
    U = torch.triu(A[:, :n].cpu())                    # L' as it lies: row c of the buffer is column c of L
    ref = torch.linalg.solve_triangular(U, torch.from_numpy(Z.T.copy()), upper=True).numpy().T
    worst = max(float(np.abs(got[j] - ref[j]).max() / np.abs(ref[j]).max()) for j in range(nb))
    print(f"solve_chain: backsolve n={n} nblk={n // 64} nb={nb} shared factor: largest error {worst:.3e} of max|alpha|")
    assert np.isfinite(got).all() and worst <= tol[0], worst


def inverse_errors(lmm, NC, nb):
    """(largest error of upper(R), largest |strict lower(R)|, largest error of lower(A), padding rows untouched, A and R) of
    lmm_dev_factor_inverse on a batch of nb factors of size NC."""
    import torch
    lib = lmm.load()
    A, W, Lh, idx = batch_of(lmm, NC, nb)
    ld = A.shape[2]
    R = torch.from_numpy(np.random.default_rng([NC, nb, 13]).standard_normal((nb, NC, ld))).cuda()
    A0pad, R0pad = A[:, :, NC:].clone(), R[:, :, NC:].clone()
    torch.cuda.synchronize()
    rc = lib.lmm_dev_factor_inverse(A.data_ptr(), A.stride(0), ld, NC, W.data_ptr(), W.stride(0), R.data_ptr(), R.stride(0), nb)
    assert rc == 0, lib.lmm_last_error_string()
    pads = bool(torch.equal(A[:, :, NC:].view(torch.int64), A0pad.view(torch.int64)) and
                torch.equal(R[:, :, NC:].view(torch.int64), R0pad.view(torch.int64)))
    Ah, Rh = A.cpu().numpy(), R.cpu().numpy()
    refs = {f: H.inverse_ref(Lh[f]) for f in set(idx)}
    eR = eL = eA = 0.0
    for j in range(nb):
        Rref, Kinv = refs[idx[j]]
        Rg, Ag = Rh[j, :, :NC].T, Ah[j, :, :NC].T
        assert np.isfinite(Rg).all() and np.isfinite(np.tril(Ag)).all()
        eR = max(eR, float(np.abs(np.triu(Rg) - Rref).max() / np.abs(Rref).max()))
        eL = max(eL, float(np.abs(np.tril(Rg, -1)).max()))
        eA = max(eA, float(np.abs(np.tril(Ag) - np.tril(Kinv)).max() / np.abs(Kinv).max()))
    return eR, eL, eA, pads, Ah, Rh


@pytest.mark.parametrize("NC,nb", INVERSE_CASES)
def test_factor_inverse_vs_host(lmm, tol, NC, nb):
    eR, eL, eA, pads, _, _ = inverse_errors(lmm, NC, nb)
    print(f"solve_chain: inverse NC={NC} nb={nb}: upper(R) {eR:.3e} of max|L^-T|, strict lower(R) {eL:.1e}, lower(A) {eA:.3e} of max|K^-1|")
    assert eL == 0.0
    assert pads
    assert eR <= tol[1] and eA <= tol[1], (eR, eA)


def test_building_blocks_refuse_bad_arguments(lmm):
    import torch
    from lmm_amd import _lib as L
    lib = lmm.load()
    a = torch.zeros(64 * 66 * 2, dtype=torch.float64, device="cuda")
    p = a.data_ptr()
    for args in [(None, 0, 66, p, 0, 1, p, 64, 1), (p, 0, 66, p, 0, 0, p, 64, 1), (p, 0, 62, p, 0, 1, p, 64, 1), (p, 0, 65, p, 0, 1, p, 64, 1),
                 (p, 0, 66, p, 0, 1, p, 64, 33), (p, 0, 66, p, 0, 1, p, 63, 2)]:
        assert lib.lmm_dev_backsolve(*args) == L.LMM_ERR_ARG, args
    for args in [(p, 0, 66, 64, p, 0, None, 0, 1), (p, 0, 66, 96, p, 0, p, 0, 1), (p, 0, 62, 64, p, 0, p, 0, 1), (p, 0, 66, 64, p, 0, p, 0, 33),
                 (p, 64, 66, 64, p, 4096, p, 64 * 66, 2)]:
        assert lib.lmm_dev_factor_inverse(*args) == L.LMM_ERR_ARG, args


# ---------------------------------------------------------------------------------------------------
# child processes: LMM_DETERMINISTIC=1 (read once per process), and the busy device
# ---------------------------------------------------------------------------------------------------
def _child_deterministic():
    import lmm_amd as lmm
    lmm.init(0)
    out = []
    for NC, nb in DETERMINISTIC_CASES:
        eR, eL, eA, pads, A1, R1 = inverse_errors(lmm, NC, nb)
        _, _, _, _, A2, R2 = inverse_errors(lmm, NC, nb)
        same = bool(np.array_equal(A1.view(np.int64), A2.view(np.int64)) and np.array_equal(R1.view(np.int64), R2.view(np.int64)))
        out.append({"NC": NC, "nb": nb, "eR": eR, "eL": eL, "eA": eA, "pads": pads, "repeat_bitwise": same})
    print(json.dumps(out))


def test_factor_inverse_deterministic_switch(tol):
    """LMM_DETERMINISTIC=1: the same inverse without split-K atomics; two runs are bitwise equal."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "deterministic"], env=dict(os.environ, LMM_DETERMINISTIC="1"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = json.loads(out.stdout.strip().splitlines()[-1])
    assert [(r["NC"], r["nb"]) for r in rows] == DETERMINISTIC_CASES
    for r in rows:
        print(f"solve_chain: inverse NC={r['NC']} nb={r['nb']} LMM_DETERMINISTIC=1: upper(R) {r['eR']:.3e}, strict lower(R) {r['eL']:.1e}, "
              f"lower(A) {r['eA']:.3e}, repeat bitwise {r['repeat_bitwise']}")
        assert r["eL"] == 0.0 and r["pads"] and r["repeat_bitwise"]
        assert r["eR"] <= tol[1] and r["eA"] <= tol[1], r


BUSY_M, BUSY_P, BUSY_N, BUSY_NS, BUSY_S2 = 64, 64, 4096, 64, 0.2
BUSY_KINDS = ("matern12", "matern32", "matern52")
BUSY_HOST_LATENTS = (0, 15, 16, 63)


def busy_problem():
    rng = np.random.default_rng(2718)
    gps = [{"kind": BUSY_KINDS[l % 3], "variance": float(rng.uniform(0.5, 2.0)), "lengthscale": float(rng.uniform(0.5, 2.0)),
            "mean": float(rng.normal())} for l in range(BUSY_M)]
    U = np.linalg.qr(rng.standard_normal((BUSY_P, BUSY_M)))[0]
    S = rng.uniform(0.5, 2.0, BUSY_M)
    x = np.cumsum(0.05 * (0.5 + rng.uniform(size=BUSY_N)))
    xs = np.sort(rng.uniform(x[0], x[-1], BUSY_NS))
    y = rng.standard_normal(BUSY_N * BUSY_P)
    return dict(gps=gps, U=np.ascontiguousarray(U), S=S, x=x, xs=xs, y=y)


def _child_busy(path):
    import lmm_amd as lmm
    from lmm_amd import _lib as L
    lmm.init(0)
    Q = busy_problem()
    K = {"matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    mogp = lmm.independent_mogp([lmm.GP(g["mean"], K[g["kind"]](g["variance"], g["lengthscale"])) for g in Q["gps"]])
    fx = lmm.ILMM(mogp, lmm.Orthogonal(Q["U"], Q["S"]))(lmm.MOInputIsotopicByOutputs(Q["x"], BUSY_P), BUSY_S2)
    xsin = lmm.MOInputIsotopicByOutputs(Q["xs"], BUSY_P)
    out = {}

    def put(tag, G):
        for k in ("y", "S", "U"):
            out[f"{tag}_{k}"] = np.asarray(G[k], dtype=np.float64)
        out[f"{tag}_scalars"] = np.array([G["value"], G["sigma2"]])
        out[f"{tag}_gps"] = np.array([[g["variance"], g["lengthscale"], g["mean"]] for g in G["gps"]])

    put("chain", lmm.logpdf_and_gradient(fx, Q["y"]))
    put("ss", lmm.statespace_logpdf_and_gradient(fx, Q["y"]))
    post = lmm.posterior(fx, Q["y"])
    ml, vl = np.empty(BUSY_M * BUSY_NS), np.empty(BUSY_M * BUSY_NS)
    L.check(lmm.load().lmm_latent_marginals(post.f._post.ptr, None, BUSY_M, L.Arr(Q["xs"]).ptr, 1, BUSY_NS, L.Arr(ml, True).ptr, L.Arr(vl, True).ptr))
    out["chain_latent_mean"], out["chain_latent_var"] = ml, vl
    out["chain_mean"], out["chain_var"] = (np.asarray(a, dtype=np.float64) for a in lmm.mean_and_var(post(xsin, BUSY_S2)))
    out["ss_mean"], out["ss_var"] = (np.asarray(a, dtype=np.float64) for a in lmm.statespace_mean_and_var(fx, Q["y"], xs=Q["xs"]))
    np.savez(path, **out)


@pytest.fixture(scope="module")
def busy():
    """The child's outputs: one run, no retry."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "busy.npz")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "busy", path], env=dict(os.environ, LMM_NSTREAMS="4", LMM_BATCH="16"),
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


def _grad_dict(busy, tag):
    return {"value": float(busy[f"{tag}_scalars"][0]), "sigma2": float(busy[f"{tag}_scalars"][1]), "y": busy[f"{tag}_y"], "S": busy[f"{tag}_S"],
            "U": busy[f"{tag}_U"], "gps": [{"variance": r[0], "lengthscale": r[1], "mean": r[2]} for r in busy[f"{tag}_gps"]]}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_busy_gradient_vs_state_space(busy):
    import test_gpu_statespace_grad as TGG
    import test_statespace_grad_abi as TG
    tol = max(1e-10, 100.0 * TG.delta_grad())
    got, ref = _grad_dict(busy, "chain"), _grad_dict(busy, "ss")
    for k in ("y", "S", "U"):
        print(f"solve_chain: busy gradient {k}: {_rel(got[k], ref[k]):.3e} of max|state space|")
    print(f"solve_chain: busy gradient value {abs(got['value'] - ref['value']) / abs(ref['value']):.3e}, sigma2 "
          f"{abs(got['sigma2'] - ref['sigma2']) / abs(ref['sigma2']):.3e} (relative)")
    for i, key in enumerate(("variance", "lengthscale", "mean")):
        e = np.abs(busy["chain_gps"][:, i] - busy["ss_gps"][:, i]) / np.abs(busy["ss_gps"][:, i])
        print(f"solve_chain: busy gradient gps {key}: largest relative difference {e.max():.3e} (latent {int(e.argmax())})")
    TGG.check_dict(got, ref, tol)


def test_busy_posterior_vs_state_space(busy):
    import test_gpu_statespace as GS
    import test_statespace_abi as T
    tol = max(1e-10, 100.0 * T.delta())
    for k in ("mean", "var"):
        print(f"solve_chain: busy posterior {k}: {_rel(busy['chain_' + k], busy['ss_' + k]):.3e} of max|state space|")
    GS.close(busy["chain_mean"], busy["ss_mean"], tol)
    GS.close(busy["chain_var"], busy["ss_var"], tol)


def _kernel(kind, v, ell, r):
    from oracle import lmm_oracle as O
    return v * np.exp(-r / ell) if kind == "matern12" else O.kernel_eval(kind, v, ell, r)


def _dkernel_dell(kind, v, ell, r):
    from oracle import lmm_oracle as O
    return v * np.exp(-r / ell) * r / ell ** 2 if kind == "matern12" else O.kernel_dlengthscale(kind, v, ell, r)


@pytest.mark.parametrize("l", BUSY_HOST_LATENTS)
def test_busy_latent_vs_host(busy, l):
    """Latent l alone in float64 NumPy: the first and the last latent of a batch (0, 15; 16, 63), of the first and the last stream."""
    import scipy.linalg as sla
    from oracle import lmm_oracle as O
    TOL = 1e-10
    Q = busy_problem()
    g, n = Q["gps"][l], BUSY_N
    v, ell = g["variance"], g["lengthscale"]
    T, ST = O.project_orthogonal(Q["U"], Q["S"], BUSY_S2)
    delta = T[l] @ O.reshape_y(Q["y"], n) - g["mean"]
    r = O.pairwise_dist(Q["x"])
    K = _kernel(g["kind"], v, ell, r)
    Lc = np.linalg.cholesky(K + ST[l] * np.eye(n))
    alpha = sla.cho_solve((Lc, True), delta)
    Kinv = sla.cho_solve((Lc, True), np.eye(n))
    aa = np.outer(alpha, alpha)
    dK = _dkernel_dell(g["kind"], v, ell, r)
    ref = {"mean": (alpha.sum(), np.abs(alpha).sum()),
           "variance": (0.5 * np.sum((aa - Kinv) * K) / v, 0.5 * (np.abs(aa * K).sum() + np.abs(Kinv * K).sum()) / v),
           "lengthscale": (0.5 * np.sum((aa - Kinv) * dK), 0.5 * (np.abs(aa * dK).sum() + np.abs(Kinv * dK).sum()))}
    got_alpha = -np.sqrt(Q["S"][l]) * (Q["U"][:, l] @ O.reshape_y(busy["chain_y"], n))
    e_alpha = _rel(got_alpha, alpha)
    errs = {}
    for i, key in enumerate(("variance", "lengthscale", "mean")):
        errs[key] = abs(float(busy["chain_gps"][l, i]) - ref[key][0]) / ref[key][1]
    Ks = _kernel(g["kind"], v, ell, O.pairwise_dist(Q["x"], Q["xs"]))
    mref = g["mean"] + Ks.T @ alpha
    Am = sla.solve_triangular(Lc, Ks, lower=True)
    vref = v - np.sum(Am * Am, axis=0)
    ml = busy["chain_latent_mean"].reshape(BUSY_M, BUSY_NS)[l]
    vl = busy["chain_latent_var"].reshape(BUSY_M, BUSY_NS)[l]
    e_m, e_v = _rel(ml, mref), _rel(vl, vref)
    print(f"solve_chain: busy latent {l} ({g['kind']}): alpha {e_alpha:.3e} of max|alpha|; of the sum of |terms|: mean {errs['mean']:.3e}, variance "
          f"{errs['variance']:.3e}, lengthscale {errs['lengthscale']:.3e}; marginal mean {e_m:.3e}, var {e_v:.3e} of max|reference|")
    assert e_alpha <= TOL
    assert all(e <= TOL for e in errs.values()), errs
    assert e_m <= TOL and e_v <= TOL, (e_m, e_v)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if sys.argv[1] == "deterministic":
        _child_deterministic()
    else:
        _child_busy(sys.argv[2])
