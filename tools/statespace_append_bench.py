"""Timings of appending observations to the state-space posterior object (DESIGN.md 4.18 "Appending observations") ->
profiles/statespace_append_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), data on the device, n = 16384 / 262144 / 1048576 and
k = 1 / 64 / 4096 new points behind them.  Per (n, k), on a handle built on the n points and given room by reserve(n + 2 k):
  * post.append(x_new, y_new): the front end and the filter over the k points from the stored last state;
  * post.mean_and_var(xs) at 1024 forecast queries (device) right after it, which leaves the smoothed states behind;
  * post.smooth(): the RTS pass over all n + k kept filtered states;
  * a second post.append of the next k points on the same handle, whose predecessor is then not the O(n) conditioning pass but the
    small calls above (what a stream of ticks sees);
  * beside them, what a caller without append does: statespace_posterior(fx, y) on all n + k points, in the same process.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; every timed append starts from a fresh handle on the
n points, so the handle does not grow from one run to the next.  Each call ends in a device synchronise inside the library, so a host
clock around it is the call time.  Every size is a child process of its own with its own time limit (`--step-timeout` seconds); after
a step that fails or runs out of time nothing more is started.  A figure no run produced is "not measured".  No threshold is
asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KS = (1, 64, 4096)
NS_FORECAST = 1024


def step_size(n, runs):
    """One size: the row of figures."""
    import torch
    import lmm_amd as lmm
    from statespace_bench import P_OUT, S2, make_problem, timed
    lmm.init(0)
    f, x, y = make_problem(lmm, n + 2 * max(KS))
    Y = y.reshape(P_OUT, n + 2 * max(KS))
    fx0 = f(lmm.MOInputIsotopicByOutputs(x[:n].contiguous(), P_OUT), S2)
    y0 = Y[:, :n].reshape(-1).contiguous()
    row = {"n": n, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda").manual_seed(n)
    for k in KS:
        xn, yn = x[n:n + k].contiguous(), Y[:, n:n + k].reshape(-1).contiguous()
        xn2, yn2 = x[n + k:n + 2 * k].contiguous(), Y[:, n + k:n + 2 * k].reshape(-1).contiguous()
        xs = float(x[n + k - 1]) + 5.0 * torch.rand(NS_FORECAST, dtype=torch.float64, device="cuda", generator=gen)
        fxa = f(lmm.MOInputIsotopicByOutputs(x[:n + k].contiguous(), P_OUT), S2)
        ya = Y[:, :n + k].reshape(-1).contiguous()
        torch.cuda.synchronize()
        ta, tf, ts, t2nd, val = [], [], [], [], None
        for run in range(runs + 1):                    # the first is the warm-up
            with lmm.statespace_posterior(fx0, y0) as post:
                post.reserve(n + 2 * k)
                t0 = time.perf_counter()
                inc = post.append(xn, yn)
                t1 = time.perf_counter()
                m, _ = post.mean_and_var(xs)
                t2 = time.perf_counter()
                stale = not post.smoothed
                t3 = time.perf_counter()
                post.smooth()
                t4 = time.perf_counter()
                val = post.logpdf
                assert stale and post.smoothed         # the forecasts left the smoothed states behind, smooth() caught up
                t5 = time.perf_counter()
                post.append(xn2, yn2)
                t6 = time.perf_counter()
                if run:
                    ta.append(t1 - t0); tf.append(t2 - t1); ts.append(t4 - t3); t2nd.append(t6 - t5)

        def rebuild():
            with lmm.statespace_posterior(fxa, ya) as post:
                return post.logpdf

        tr, trr, vr = timed(rebuild, runs)
        med = statistics.median
        row[f"k{k}"] = {"append_ms": med(ta) * 1e3, "append_runs_ms": [q * 1e3 for q in ta],
                        "forecast_1024_ms": med(tf) * 1e3, "forecast_runs_ms": [q * 1e3 for q in tf],
                        "second_append_ms": med(t2nd) * 1e3, "second_append_runs_ms": [q * 1e3 for q in t2nd],
                        "smooth_ms": med(ts) * 1e3, "smooth_runs_ms": [q * 1e3 for q in ts],
                        "rebuild_ms": tr * 1e3, "rebuild_runs_ms": [q * 1e3 for q in trr],
                        "rebuild_over_append": tr / med(ta), "rebuild_over_append_and_smooth": tr / (med(ta) + med(ts)),
                        "smooth_over_rebuild": med(ts) / tr, "increment": inc,
                        "logpdf_relative_difference": abs(val - vr) / max(abs(vr), 1e-300)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_append_bench.json"))
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
    res = {"latents": 32, "p": 64, "kernel": "matern52", "sigma2": 0.1, "runs": a.runs, "k": list(KS), "forecast_queries": NS_FORECAST,
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
