"""Timings of sum latents on the state-space path (DESIGN.md 4.18 "Sum latents") -> profiles/statespace_sum_bench.json.

p = 64, d = 1, the data of tools/statespace_bench.py (sorted inputs, on the device), n = 16384 / 262144 / 1048576, and four models in the
same run:
  * matern32+sho      : 32 latents, each the sum of a Matern32 and an SHO: D = 4, five seeded parameters;
  * matern32+matern32 : 32 latents, each the sum of a short and a long Matern32: D = 4, four seeded parameters;
  * matern52          : 32 plain Matern52 latents (D = 3), the largest one-term model;
  * separate          : 64 latents, the 32 Matern32 and the 32 SHO terms of the first model each a latent of its own, mixed through a
                        64-column H -- the only way to write "trend + oscillation" on this path without sum latents (another model: it
                        spends two latent slots and two columns of H per pair).
Every model is timed through the C ABI's entry points themselves, on L.statespace_gps_array descriptors (the Python state-space functions
refuse a sum with an SHO term, and one route for all four keeps the figures comparable): lmm_oilmm_logpdf_statespace,
lmm_oilmm_logpdf_grad_statespace (every output asked for) and one posterior sample of lmm_oilmm_rand_statespace, whose normals are
drawn on the device inside the timed call, as statespace_rand draws them.  Each figure is the median of `--runs` (>= 3) timed calls
after one warm-up call; each call ends in a device synchronise inside the library, so a host clock around it is the call time.  The
ratios of the two sum models to matern52 and to `separate` are written beside the times.  A figure no run produced is written as "not
measured".  No threshold is asserted.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from statespace_bench import M_LAT, P_OUT, S2, make_problem, timed

MODELS = ("matern32+sho", "matern32+matern32", "matern52", "separate")
SUMS = MODELS[:2]
WHAT = ("logpdf", "logpdf_and_gradient", "rand_posterior")
DIM = {"matern12": 1, "matern32": 2, "matern52": 3, "sho": 2}


def descriptors(name):
    short = [{"kind": "matern32", "variance": 0.5 + 0.03 * l, "lengthscale": 0.8 + 0.02 * l} for l in range(M_LAT)]
    osc = [{"kind": "sho", "variance": 0.3 + 0.01 * l, "lengthscale": 2.0 + 0.05 * l, "quality": 3.0 + 0.1 * l} for l in range(M_LAT)]
    long_ = [{"kind": "matern32", "variance": 0.3 + 0.01 * l, "lengthscale": 6.0 + 0.1 * l} for l in range(M_LAT)]
    sums = lambda second: [{"kind": "sum", "variance": 1.0, "lengthscale": 1.0, "mean": 0.0, "terms": [a, b]} for a, b in zip(short, second)]
    if name == "matern32+sho":
        return sums(osc)
    if name == "matern32+matern32":
        return sums(long_)
    if name == "matern52":
        return [{"kind": "matern52", "variance": 0.5 + 0.03 * l, "lengthscale": 0.8 + 0.02 * l, "mean": 0.0} for l in range(M_LAT)]
    return [dict(g, mean=0.0) for g in short + osc]


def state_dim(g):
    return sum(DIM[t["kind"]] for t in g["terms"]) if g["kind"] == "sum" else DIM[g["kind"]]


def entry_points(lmm, descs, U, S, x, y, n):
    """The three timed calls of one model, each through the library's entry point on device data."""
    import torch
    from lmm_amd import _lib as L
    lib, m = lmm.load(), len(descs)
    ga = L.statespace_gps_array(descs)
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    zl = sum(state_dim(g) for g in descs) * n
    out, val, gs2 = C.c_double(), C.c_double(), C.c_double()
    gy = torch.empty(n * P_OUT, dtype=torch.float64, device="cuda")
    gS, gU, gg = np.empty(m), np.empty(P_OUT * m), (L.GpGradT * m)()
    path = torch.empty(n * P_OUT, dtype=torch.float64, device="cuda")
    normals = lmm.DeviceNormals(3)

    def logpdf():
        L.check(lib.lmm_oilmm_logpdf_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, m, S2, ga, 0, m, 1, C.byref(out)))
        return out.value

    def gradient():
        L.check(lib.lmm_oilmm_logpdf_grad_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, m, S2, ga, 0, m, 1, C.byref(val),
                                                     L.Arr(gy, True).ptr, C.byref(gs2), L.Arr(gS, True).ptr, L.Arr(gU, True).ptr, gg))
        return val.value

    def rand():
        z, xi, eps = normals.standard_normal(zl), normals.standard_normal(m * n), normals.standard_normal(n * P_OUT)
        L.check(lib.lmm_oilmm_rand_statespace(L.Arr(x).ptr, n, L.Arr(y).ptr, P_OUT, Ua.ptr, Sa.ptr, m, S2, ga, 0, m, 1, 1, L.Arr(z).ptr,
                                              L.Arr(xi).ptr, L.Arr(eps).ptr, L.Arr(path, True).ptr))
        return float(path[0])

    return {"logpdf": logpdf, "logpdf_and_gradient": gradient, "rand_posterior": rand}, ga


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace_sum_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144, 1048576])
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be >= 3")
    import torch
    import lmm_amd as lmm
    lmm.init(0)
    res = {"latents": M_LAT, "p": P_OUT, "sigma2": S2, "runs": a.runs, "device": torch.cuda.get_device_name(0), "models": list(MODELS),
           "route": "C ABI entry points on device data", "sizes": []}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for n in a.sizes:
        _, x, y = make_problem(lmm, n)
        rng = np.random.default_rng(1)
        row = {"n": n, "ms": {m: {w: "not measured" for w in WHAT} for m in MODELS}, "runs_ms": {m: {} for m in MODELS}, "values": {}}
        res["sizes"].append(row)
        for name in MODELS:
            descs = descriptors(name)
            m = len(descs)
            U, S = np.linalg.qr(rng.standard_normal((P_OUT, m)))[0], rng.uniform(0.5, 2.0, m)
            calls, ga = entry_points(lmm, descs, U, S, x, y, n)
            for what in WHAT:
                t, tr, v = timed(calls[what], a.runs)
                row["ms"][name][what] = t * 1e3
                row["runs_ms"][name][what] = [q * 1e3 for q in tr]
                if what != "rand_posterior":
                    row["values"].setdefault(name, {})[what] = v
                save()
            del calls, ga
            torch.cuda.empty_cache()
        ms = row["ms"]
        row["ratios"] = {s: {w: {"over_matern52": ms[s][w] / ms["matern52"][w], "over_separate": ms[s][w] / ms["separate"][w]} for w in WHAT}
                         for s in SUMS}
        row["gradient_over_value"] = {m: ms[m]["logpdf_and_gradient"] / ms[m]["logpdf"] for m in MODELS}
        print(json.dumps({k: row[k] for k in ("n", "ms", "ratios", "gradient_over_value")}), flush=True)
        save()
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
