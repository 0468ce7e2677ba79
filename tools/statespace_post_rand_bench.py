"""Timings of sampling from the state-space posterior object (DESIGN.md 4.18 "Sampling from the posterior object") ->
profiles/statespace_post_rand_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), data and queries on the device, normals from a
DeviceNormals, n = 16384 / 262144 / 1048576.  One sample and eight samples of post.rand(rng, xs, N) for three windows:
  * forecast: 512 queries behind the data (no training point inside the window);
  * inside:   1024 queries inside a stretch of the data that holds about 1024 training points;
  * spread:   1024 queries over the whole range of x (every training point inside the window);
  * beside each, statespace_rand(rng, fx, y, N, xs=xs) of the same build on the same data and queries in the same run: the route that
    merges xs into the inputs, draws a prior path over all n + ns points and filters and smooths the residual again;
  * and lmm_oilmm_statespace_post_rand alone on normals drawn beforehand (library_call_ms): the mirror draws 33 blocks of normals per
    sample, one library call each, and that is most of a short call.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time (the draws of the normals included, on both routes).  Every size is a child
process of its own with its own time limit (`--step-timeout` seconds); after a step that fails or runs out of time nothing more is
started.  A figure no run produced is "not measured".  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SAMPLES = (1, 8)


def windows(x, gen):
    """{name: queries on the device}"""
    import torch
    n = int(x.shape[0])
    lo, hi = float(x[0]), float(x[-1])
    rand = lambda k: torch.rand(k, dtype=torch.float64, device="cuda", generator=gen)
    i0 = max(0, n // 2 - 512)
    i1 = min(n - 1, i0 + 1024)
    return {"forecast": hi + 0.05 * torch.cumsum(0.5 + rand(512), 0),
            "inside": float(x[i0]) + (float(x[i1]) - float(x[i0])) * rand(1024),
            "spread": lo + (hi - lo) * rand(1024)}


def library_call(post, xs, count, N, m=32, D=3):
    """lmm_oilmm_statespace_post_rand alone on normals drawn beforehand: what of post.rand's time is the library's (the mirror draws
    m + 1 blocks of normals per sample, one library call each)."""
    import torch
    from lmm_amd import _lib as L
    from statespace_bench import P_OUT
    lib = L.load()
    xq = torch.sort(xs).values.contiguous()
    ns = int(xq.shape[0])
    W = ns + count
    z = torch.randn(N, m * D * W, dtype=torch.float64, device="cuda")
    eps = torch.randn(N, ns * P_OUT, dtype=torch.float64, device="cuda")
    out = torch.empty(N, ns * P_OUT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def call():
        L.check(lib.lmm_oilmm_statespace_post_rand(post._ptr, L.Arr(xq).ptr, ns, L.Arr(z).ptr, L.Arr(eps).ptr, N, 1, L.Arr(out, True).ptr))
    return call


def step_size(n, runs):
    """One size: the row of figures."""
    import torch
    import lmm_amd as lmm
    from statespace_bench import P_OUT, S2, make_problem, timed
    lmm.init(0)
    f, x, y = make_problem(lmm, n)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    row = {"n": n, "device": torch.cuda.get_device_name(0)}
    post = lmm.statespace_posterior(fx, y)
    gen = torch.Generator(device="cuda").manual_seed(n)
    for name, xs in windows(x, gen).items():
        torch.cuda.synchronize()
        first, count = post.window(xs)
        cell = {"ns": int(xs.shape[0]), "training_points_in_window": count}
        for N in SAMPLES:
            def handle():
                out = post.rand(lmm.DeviceNormals(1), xs, N)
                return float(out.reshape(-1)[0])

            def route():
                out = lmm.statespace_rand(lmm.DeviceNormals(1), fx, y, N, xs=xs)
                return float(out.reshape(-1)[0])

            th, thr, _ = timed(handle, runs)
            tx, txr, _ = timed(route, runs)
            tc, tcr, _ = timed(library_call(post, xs, count, N), runs)
            cell[f"N{N}"] = {"post_rand_ms": th * 1e3, "post_rand_runs_ms": [q * 1e3 for q in thr], "xs_route_ms": tx * 1e3,
                             "xs_route_runs_ms": [q * 1e3 for q in txr], "xs_route_over_post_rand": tx / th,
                             "library_call_ms": tc * 1e3, "library_call_runs_ms": [q * 1e3 for q in tcr]}
        row[name] = cell
    post.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_post_rand_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=["size"], help="(internal) run one step in this process and print its row")
    ap.add_argument("--n", type=int)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    if a.step:
        print("ROW " + json.dumps(step_size(a.n, a.runs)), flush=True)
        return 0
    res = {"latents": 32, "p": 64, "kernel": "matern52", "sigma2": 0.1, "runs": a.runs, "normals": "DeviceNormals", "sizes": []}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for n in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "size", "--n", str(n), "--runs", str(a.runs)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"step n={n} ran out of its {a.step_timeout} s; nothing more was started"
            print(res["stopped"], flush=True)
            save()
            return 1
        rows = [ln[4:] for ln in done.stdout.splitlines() if ln.startswith("ROW ")]
        if done.returncode != 0 or not rows:
            res["stopped"] = f"step n={n} failed (exit {done.returncode}); nothing more was started: {done.stderr[-2000:]}"
            print(res["stopped"], flush=True)
            save()
            return 1
        row = json.loads(rows[-1])
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
