"""Timings of StateSpacePosterior.predictive_logpdf (DESIGN.md 4.18 "Predictive log density from the posterior object") ->
profiles/statespace_predictive_logpdf_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), data on the device, n = 16384 / 262144 / 1048576 and
ns = 1024 held-out points in three placements:
  * "behind": behind the last input (the window holds no training point);
  * "inside": inside a stretch of about 1000 training points in the middle of the data;
  * "whole": over the whole range of the inputs (the window holds every training point).
Per (n, placement), on one handle built on the n points:
  * post.predictive_logpdf(xs, ys);
  * beside it, in the same process, the difference route's call: statespace_logpdf on all n + ns points (post.logpdf is what it
    subtracts, at no cost).
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call.  Each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  Every size is a child process of its own with its own time limit
(`--step-timeout` seconds); after a step that fails or runs out of time nothing more is started.  A figure no run produced is "not
measured".  No threshold is asserted; the claims to read off the table are that "behind" and "inside" do not grow with n and that
"whole" is O(n) and no slower than the difference route.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NS = 1024
STRETCH = 1000
PLACEMENTS = ("behind", "inside", "whole")


def queries(x, n, placement, gen):
    import torch
    u = torch.rand(NS, dtype=torch.float64, device="cuda", generator=gen)
    if placement == "behind":
        lo, hi = float(x[n - 1]), float(x[n - 1]) + 50.0
    elif placement == "inside":
        lo, hi = float(x[n // 2]), float(x[n // 2 + STRETCH])
    else:
        lo, hi = float(x[0]), float(x[n - 1])
    return torch.sort(lo + (hi - lo) * u)[0].contiguous()


def step_size(n, runs):
    """One size: the row of figures."""
    import torch
    import lmm_amd as lmm
    from statespace_bench import P_OUT, S2, make_problem, timed
    lmm.init(0)
    f, x, y = make_problem(lmm, n)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    Y = y.reshape(P_OUT, n)
    row = {"n": n, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda").manual_seed(n)
    with lmm.statespace_posterior(fx, y) as post:
        for placement in PLACEMENTS:
            xs = queries(x, n, placement, gen)
            ys = torch.randn(NS * P_OUT, dtype=torch.float64, device="cuda", generator=gen)
            xa = torch.cat([x, xs]).contiguous()
            ya = torch.cat([Y, ys.reshape(P_OUT, NS)], dim=1).reshape(-1).contiguous()
            fxa = f(lmm.MOInputIsotopicByOutputs(xa, P_OUT), S2)
            first, count = post.window(xs)
            torch.cuda.synchronize()
            tp, tpr, vp = timed(lambda: post.predictive_logpdf(xs, ys), runs)
            td, tdr, va = timed(lambda: lmm.statespace_logpdf(fxa, ya), runs)
            vd = va - post.logpdf
            row[placement] = {"window_training_points": count,
                              "predictive_logpdf_ms": tp * 1e3, "predictive_logpdf_runs_ms": [q * 1e3 for q in tpr],
                              "difference_route_ms": td * 1e3, "difference_route_runs_ms": [q * 1e3 for q in tdr],
                              "difference_over_predictive": td / tp, "value": vp,
                              "relative_difference_of_the_values": abs(vp - vd) / max(1.0, abs(vd))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_predictive_logpdf_bench.json"))
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
    res = {"latents": 32, "p": 64, "kernel": "matern52", "sigma2": 0.1, "runs": a.runs, "queries": NS, "placements": list(PLACEMENTS),
           "sizes": []}

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
