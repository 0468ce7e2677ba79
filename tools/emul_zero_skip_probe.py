"""Two measurements for the zero skip of the int8 emulation's GEMM, on C2's shapes (bench.py's default workload: OILMM,
32 Matern52 latents, n = 16384, x_i = i 20 / 575) with the latents' lengthscale as a parameter:

    python tools/emul_zero_skip_probe.py time [--lengthscale L] [--steps K] [--warmup W]
        logpdf timed the way bench.py times it (warm-up, fence, K evaluations, fence); one JSON line.  --lengthscale 50 is the control
        without decay: nothing truncates to zero, every mask is all ones, and what is left of the difference to the parent build
        (LMM_HIP_LIB) is the price of the masks and of the scalar cursor.

    python tools/emul_zero_skip_probe.py live [--lengthscale L] [--noise S]
        the live K blocks the GEMM walks, per emulated level: the Cholesky factor of ONE latent's matrix K + S I (torch, Float64), the
        convert's rule applied to every emulated update's panel (a 256-row block is live in a 128-wide K block when one of its
        truncated integers is not zero), and per tile (I, J) of the update the number of blocks live in both operands -- the K steps
        the kernel runs for it -- beside K / 128, the K steps without the skip.  Rider rows (y) are left out: they are one tile row.

    python tools/emul_zero_skip_probe.py screen [--lengthscale L]
        one logpdf, then the counters the screen of the f64 update launches kept on the device (lmm_dev_f64_screen_stats): per
        screened update of the last batch, the dead 128 x 128 tiles of its rest tiles, and whether its screen ran or returned at
        entry after the vote.

    python tools/emul_zero_skip_probe.py void [--lengthscale L]
        one logpdf, then the work items the zero extents ("Rows whose panel is exactly zero") left out in the last
        batch's factorisation (lmm_dev_zero_extent_stats): per region launch its void row tasks, per f64 update its void items, per
        emulated update its void 256 x 256 tiles, all matrices of the batch together.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

M_LAT, P_OUT, N = 32, 64, 16384


def split(w):      # potrf_split (csrc/lmm_potrf_plan.h)
    return (w // 2 + 127) // 128 * 128 if w >= 256 else (128 if w == 192 else 64)


def updates(NR, j0, w, out):
    """(j0, M, N, K) of the trailing updates with N >= 128 of the columns [j0, j0 + w), in launch order"""
    if w < 256:
        return
    h = split(w)
    updates(NR, j0, h, out)
    if w - h >= 128:
        out.append((j0, NR - j0 - h, w - h, h))
    updates(NR, j0 + h, w - h, out)


def timed(args):
    import torch
    import lmm_amd
    from lmm_amd.workloads import synthetic_problem
    lmm_amd.init(0)
    P = synthetic_problem(M_LAT, P_OUT, N, "matern52", True, s2=0.1, seed=0)
    fs = lmm_amd.independent_mogp([lmm_amd.GP(0.0, lmm_amd.Matern52Kernel(1.0, args.lengthscale)) for _ in range(M_LAT)])
    f = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(P["U"], P["S"]), shard=lmm_amd.latent_shard(M_LAT, 0, 1))
    xd, yd = torch.from_numpy(P["x"]).cuda(), torch.from_numpy(P["y"]).cuda()
    fx = f(lmm_amd.MOInputIsotopicByOutputs(xd, P_OUT), 0.1)
    val = None
    for _ in range(args.warmup):
        val = lmm_amd.logpdf(fx, yd, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        val = lmm_amd.logpdf(fx, yd, True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"workload": "C2's shapes", "lengthscale": args.lengthscale, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": 1e3 * dt / max(args.steps, 1), "logpdf": val, "lib": os.environ.get("LMM_HIP_LIB", "in-tree")}))


def screen(args):
    """The f64 update launches' screen on the device: per screened update of the last batch's factorisation, the dead
    tiles its screen counted of the rest tiles of one matrix x the batch"""
    import torch
    import lmm_amd
    from lmm_amd.workloads import synthetic_problem
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_f64_screen_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_f64_screen_stats.restype = C.c_int
    P = synthetic_problem(M_LAT, P_OUT, N, "matern52", True, s2=0.1, seed=0)
    fs = lmm_amd.independent_mogp([lmm_amd.GP(0.0, lmm_amd.Matern52Kernel(1.0, args.lengthscale)) for _ in range(M_LAT)])
    f = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(P["U"], P["S"]), shard=lmm_amd.latent_shard(M_LAT, 0, 1))
    xd, yd = torch.from_numpy(P["x"]).cuda(), torch.from_numpy(P["y"]).cuda()
    fx = f(lmm_amd.MOInputIsotopicByOutputs(xd, P_OUT), 0.1)
    assert lib.lmm_dev_f64_screen_stats(1, None, 0) >= 0
    val = lmm_amd.logpdf(fx, yd, True)
    out = (C.c_int * (5 * 256))()
    n = lib.lmm_dev_f64_screen_stats(0, out, 256)
    print(f"lengthscale {args.lengthscale}: logpdf {val!r}; screened f64 updates of the last batch ({M_LAT // 2} matrices), in launch order: M N K | dead tiles of rest tiles | screen ran")
    tot = {}
    for i in range(n):
        M, Nc, K, dead, ran = out[5 * i:5 * i + 5]
        mt, nt = (M - (64 if M % 128 == 64 and K >= 1024 else 0) + 127) // 128, (Nc + 127) // 128
        rest = (M_LAT // 2) * sum(mt - tj for tj in range(1, nt))
        tot.setdefault(K, [0, 0])
        tot[K][0] += dead
        tot[K][1] += rest
        print(f"  {M:6d} {Nc:5d} {K:5d} | {dead:6d} of {rest:6d} | {ran}")
    print("per K (dead, rest tiles): " + str({k: tuple(v) for k, v in sorted(tot.items())}))


def void(args):
    """The zero extents on the device: per step of the last batch's factorisation, the work items left out"""
    import torch
    import lmm_amd
    from lmm_amd.workloads import synthetic_problem
    lmm_amd.init(0)
    lib = lmm_amd.load()
    lib.lmm_dev_zero_extent_stats.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.lmm_dev_zero_extent_stats.restype = C.c_int
    P = synthetic_problem(M_LAT, P_OUT, N, "matern52", True, s2=0.1, seed=0)
    fs = lmm_amd.independent_mogp([lmm_amd.GP(0.0, lmm_amd.Matern52Kernel(1.0, args.lengthscale)) for _ in range(M_LAT)])
    f = lmm_amd.ILMM(fs, lmm_amd.Orthogonal(P["U"], P["S"]), shard=lmm_amd.latent_shard(M_LAT, 0, 1))
    xd, yd = torch.from_numpy(P["x"]).cuda(), torch.from_numpy(P["y"]).cuda()
    fx = f(lmm_amd.MOInputIsotopicByOutputs(xd, P_OUT), 0.1)
    assert lib.lmm_dev_zero_extent_stats(1, None, 0) >= 0
    val = lmm_amd.logpdf(fx, yd, True)
    out = (C.c_int * (7 * 512))()
    n = lib.lmm_dev_zero_extent_stats(0, out, 512)
    names = {5: "f64 update", 6: "emulated update", 7: "region"}
    print(f"lengthscale {args.lengthscale}: logpdf {val!r}; steps of the last batch ({M_LAT // 2} matrices) that take the zero extents, in launch order: "
          "step | j0 h N M | void items | shape word (region: 128-row row tasks; update: fused + 2 strip mode)")
    tot = {}
    for i in range(min(n, 512)):
        kind, j0, h, Nc, M, cnt, word = out[7 * i:7 * i + 7]
        key = (names.get(kind, str(kind)), h)
        tot[key] = tot.get(key, 0) + cnt
        print(f"  {names.get(kind, kind):15s} | {j0:6d} {h:5d} {Nc:6d} {M:6d} | {cnt:6d} | {word}")
    print("void items per (step, K): " + str({f"{k[0]} K={k[1]}": v for k, v in sorted(tot.items())}))


def live(args):
    import torch
    import lmm_amd
    lib = lmm_amd.load()
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    DP = C.POINTER(C.c_double)
    NR = N + 64
    out = (C.c_longlong * (2 + 6 * 512))()
    cnt = lib.lmm_dev_emul_plan(NR, N, 16, out, 512)
    emulated = {tuple(out[2 + 6 * i: 5 + 6 * i]) for i in range(cnt) if out[2 + 6 * i + 3]}
    seq = []
    updates(NR, 0, N, seq)
    x = torch.arange(N, dtype=torch.float64, device="cuda") * (20.0 / 575.0)
    r = (x[:, None] - x[None, :]).abs() / args.lengthscale
    Kmat = (1.0 + 5.0 ** 0.5 * r + 5.0 / 3.0 * r * r) * torch.exp(-(5.0 ** 0.5) * r)
    del r
    Kmat.diagonal().add_(args.noise)
    L = torch.linalg.cholesky(Kmat)
    del Kmat
    one = np.ones((1, 1), order="F")
    per = {}
    print(f"lengthscale {args.lengthscale}, noise {args.noise}: emulated updates in launch order: j0 M N K | tiles | K steps walked of K steps without the skip | per tile min mean max of K / 128")
    for j0, M, Nn, K in seq:
        if (M, Nn, K) not in emulated:
            continue
        o, consts = np.zeros((1, 1), order="F"), np.zeros(68)
        assert lib.lmm_dev_emul_host(one.ctypes.data_as(DP), 1, one.ctypes.data_as(DP), 1, 1, 1, 1, 16, K, o.ctypes.data_as(DP), 1, consts.ctypes.data_as(DP)) == 0
        b = int(consts[67])
        r0 = j0 + K
        panel = L[r0:N, j0:j0 + K]                                           # the rows of the factor; the 64 rider rows are left out
        amax = panel.abs().amax(dim=1)
        e = torch.ceil(torch.log2(amax)).to(torch.int32)
        nz = torch.trunc(torch.ldexp(panel, (b - e)[:, None])) != 0
        rows = nz.shape[0]
        tr, nk = (rows + 255) // 256, K // 128
        pad = torch.zeros((tr * 256 - rows, K), dtype=torch.bool, device="cuda")
        mask = torch.cat([nz, pad]).reshape(tr, 256, nk, 128).any(dim=3).any(dim=1).cpu().numpy()      # [tile row][K block]
        tn = (Nn + 255) // 256
        steps = np.array([max(1, int((mask[i] & mask[j]).sum())) for i in range(tr) for j in range(min(i + 1, tn))])
        print(f"  j0={j0:5d} M={M:5d} N={Nn:5d} K={K:5d} | {len(steps):4d} | {int(steps.sum()):6d} of {len(steps) * nk:6d} | {steps.min():3d} {steps.mean():6.2f} {steps.max():3d} of {nk}")
        a = per.setdefault(K, [0, 0, 0])
        a[0] += len(steps); a[1] += int(steps.sum()); a[2] += len(steps) * nk
    for K in sorted(per):
        t, s, full = per[K]
        print(f"level K={K}: {t} tiles per matrix and modulus, {s / t:.2f} K steps per tile with the skip, {full / t:.0f} without; dead share of the K steps {1 - s / full:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "live", "screen", "void"])
    ap.add_argument("--lengthscale", type=float, default=1.0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    {"time": timed, "live": live, "screen": screen, "void": void}[a.mode](a)
