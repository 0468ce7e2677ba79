"""Timings of the state-space posterior object (DESIGN.md 4.18 "Posterior object") -> profiles/statespace_posterior_bench.json.

32 Matern52 latents, p = 64, d = 1 (the problem of tools/statespace_bench.py), data on the device, n = 16384 / 262144 / 1048576:
  * statespace_posterior(fx, y): the one conditioning pass (front end, filter, smoother with full states);
  * post.mean_and_var(xs) at ns = 1 / 1024 / 65536 uniform queries over the range of x, with xs on the host and on the device;
  * beside each, statespace_mean_and_var(fx, y, xs=xs) of the same build on the same data: the route that merges xs into the inputs
    and filters and smooths all n + ns points again.
  * the layout experiment (one Matern52 latent, n = 1048576, ns = 65536 and 1048576 device queries): lmm_dev_statespace_interp_layout
    on component-major (comps x n, what the filter writes for itself) against point-major (n x comps, what the library keeps) states,
    alternating, with the two results compared bitwise.
Every figure is the median of `--runs` (>= 3) timed calls after one warm-up call; each call ends in a device synchronise inside the
library, so a host clock around it is the call time.  Every size is a child process of its own with its own time limit
(`--step-timeout` seconds); after a step that fails or runs out of time nothing more is started.  A figure no run produced is
"not measured".  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NS = (1, 1024, 65536)
LAYOUT_NS = (65536, 1048576)


def step_size(n, runs):
    """One size: the row of figures."""
    import torch
    import lmm_amd as lmm
    from statespace_bench import P_OUT, S2, make_problem, timed
    lmm.init(0)
    f, x, y = make_problem(lmm, n)
    fx = f(lmm.MOInputIsotopicByOutputs(x, P_OUT), S2)
    row = {"n": n, "device": torch.cuda.get_device_name(0)}

    def create():
        with lmm.statespace_posterior(fx, y) as post:
            return post.logpdf

    t, tr, v = timed(create, runs)
    row.update(posterior_ms=t * 1e3, posterior_runs_ms=[q * 1e3 for q in tr], logpdf=v)
    post = lmm.statespace_posterior(fx, y)
    gen = torch.Generator(device="cuda").manual_seed(n)
    lo, hi = float(x[0]) - 1.0, float(x[-1]) + 1.0
    for ns in NS:
        xs_dev = lo + (hi - lo) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
        xs_host = xs_dev.cpu().numpy()
        torch.cuda.synchronize()
        for side, xs in (("host", xs_host), ("device", xs_dev)):
            def query():
                m, _ = post.mean_and_var(xs)
                return float(m[0])

            def route():
                m, _ = lmm.statespace_mean_and_var(fx, y, xs=xs)
                return float(m[0])

            tq, tqr, vq = timed(query, runs)
            tx, txr, vx = timed(route, runs)
            row[f"ns{ns}_{side}"] = {"post_mean_and_var_ms": tq * 1e3, "post_runs_ms": [q * 1e3 for q in tqr], "xs_route_ms": tx * 1e3,
                                     "xs_route_runs_ms": [q * 1e3 for q in txr], "xs_route_over_post": tx / tq,
                                     "first_mean_relative_difference": abs(vq - vx) / max(abs(vx), 1e-300)}
    post.close()
    return row


def step_layout(n, runs):
    """Component-major against point-major states, one Matern52 latent."""
    import torch
    import lmm_amd as lmm
    from lmm_amd import _lib as L
    from statespace_bench import S2, timed
    lmm.init(0)
    lib = lmm.load()
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.cumsum(0.05 * (0.5 + torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)), 0)
    w = torch.full((n,), S2, dtype=torch.float64, device="cuda")
    r = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    comps = 9
    fp, sp = (torch.empty((n, comps), dtype=torch.float64, device="cuda") for _ in range(2))
    gp = L.gps_array([dict(lmm.Matern52Kernel(1.0, 1.0).desc(), mean=0.0)])
    torch.cuda.synchronize()
    L.check(lib.lmm_dev_statespace_states(x.data_ptr(), n, gp, w.data_ptr(), r.data_ptr(), 0, fp.data_ptr(), sp.data_ptr()))
    fs, ss = fp.t().contiguous(), sp.t().contiguous()
    row = {"n": n, "latent": "matern52", "state_doubles_per_point": comps, "device": torch.cuda.get_device_name(0)}
    for ns in LAYOUT_NS:
        xs = float(x[0]) - 1.0 + (float(x[-1]) - float(x[0]) + 2.0) * torch.rand(ns, dtype=torch.float64, device="cuda", generator=gen)
        out = [torch.empty(ns, dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()

        def call(point_major):
            f_, s_ = (fp, sp) if point_major else (fs, ss)
            m_, v_ = (out[2], out[3]) if point_major else (out[0], out[1])
            L.check(lib.lmm_dev_statespace_interp_layout(x.data_ptr(), n, gp, f_.data_ptr(), s_.data_ptr(), point_major, xs.data_ptr(), ns,
                                                         m_.data_ptr(), v_.data_ptr()))

        tc, tcr, _ = timed(lambda: call(0), runs)
        tp, tpr, _ = timed(lambda: call(1), runs)
        tc2, tcr2, _ = timed(lambda: call(0), runs)           # once more, for the spread
        row[f"ns{ns}"] = {"component_major_ms": tc * 1e3, "component_major_runs_ms": [q * 1e3 for q in tcr + tcr2], "point_major_ms": tp * 1e3,
                          "point_major_runs_ms": [q * 1e3 for q in tpr], "component_major_again_ms": tc2 * 1e3,
                          "bitwise_equal": bool((out[0] == out[2]).all() and (out[1] == out[3]).all())}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_posterior_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    ap.add_argument("--layout-n", type=int, default=1048576)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=["size", "layout"], help="(internal) run one step in this process and print its row")
    ap.add_argument("--n", type=int)
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    if a.step:
        row = step_size(a.n, a.runs) if a.step == "size" else step_layout(a.n, a.runs)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    res = {"latents": 32, "p": 64, "kernel": "matern52", "sigma2": 0.1, "runs": a.runs, "sizes": [], "layout": "not measured"}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    steps = [("size", n) for n in a.sizes] + [("layout", a.layout_n)]
    for kind, n in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--n", str(n), "--runs", str(a.runs)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"step {kind} n={n} ran out of its {a.step_timeout} s; nothing more was started"
            print(res["stopped"], flush=True)
            save()
            return 1
        rows = [ln[4:] for ln in done.stdout.splitlines() if ln.startswith("ROW ")]
        if done.returncode != 0 or not rows:
            res["stopped"] = f"step {kind} n={n} failed (exit {done.returncode}); nothing more was started: {done.stderr[-2000:]}"
            print(res["stopped"], flush=True)
            save()
            return 1
        row = json.loads(rows[-1])
        if kind == "size":
            res["sizes"].append(row)
        else:
            res["layout"] = row
        print(json.dumps(row), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
