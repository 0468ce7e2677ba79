"""-m gpu: the host-side fan-out that every per-latent loop of the library goes through (lmm_api.hip, FanOut), where its indexing
can go wrong: more batches than slot streams, and a ragged last batch.

m = 70 latents over n = 96 points with LMM_NSTREAMS=2: matrices this small are planned (batch_plan: a working set under 40 MB per
latent lifts the batch to LMM_MAX_BATCH = 32) as batches of 32, 32 and 6 latents on two slot streams, the third batch reusing slot 0
behind the first.  Every verb over the whole latent range is compared with the same verb over the shards [0, 32), [32, 64) and
[64, 70), each of which is ONE batch on ONE slot: values add up, per-latent gradients concatenate (a shard leaves the other latents'
entries zero), and the posterior verbs return partial sums -- what parallel.py adds up across ranks.

Tolerance: relative 1e-12 (scalars: of the whole-range value; arrays: of its largest entry), the figure
test_c2_full_value_equals_sum_of_eight_shares holds the same identity to.  The two sides run the same per-latent launches; they
differ in the order of the sums over latents and in the split-K atomics' order.  Measured on an MI355X: at most 7.2e-16 over every
verb below, the same on the build before the fan-out driver and on the one with it.

The evaluations run once, in a child process (the stream count is read at lmm_init), and are shared by the tests below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M, P, N, D, NS, S2 = 70, 72, 96, 2, 40, 0.2
SHARDS = [(0, 32), (32, 64), (64, 70)]
RTOL = 1e-12


def _problem():
    rng = np.random.default_rng(314)
    kinds = ["se", "matern32", "matern52"]
    gps = [{"kind": kinds[l % 3], "variance": float(rng.uniform(0.5, 2.0)), "lengthscale": float(rng.uniform(0.5, 2.0)),
            "mean": float(rng.normal())} for l in range(M)]
    U, S, _ = np.linalg.svd(rng.uniform(size=(P, M)), full_matrices=False)
    x = rng.uniform(0, 6, size=(D, N))
    xs = rng.uniform(0, 6, size=(D, NS))
    y = rng.standard_normal(N * P)
    Y = y.reshape(P, N)                               # by outputs: y[o * N + i]
    ya = Y.copy(); ya[3, 10:20] = np.nan              # one pattern of missing outputs (and the complete one)
    yb = Y.copy(); yb[3, 10:20] = np.nan; yb[40, 50:60] = np.nan      # two patterns
    dmean, dvar = rng.standard_normal(NS * P), rng.standard_normal(NS * P)
    return dict(gps=gps, U=np.ascontiguousarray(U), S=S, x=x, xs=xs, y=y, ya=ya.reshape(-1), yb=yb.reshape(-1), dmean=dmean, dvar=dvar)


def _child():
    sys.path.insert(0, os.path.dirname(HERE))
    import lmm_amd as lmm
    lmm.init(0)
    Q = _problem()
    K = {"se": lmm.SEKernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    mogp = lmm.independent_mogp([lmm.GP(g["mean"], K[g["kind"]](g["variance"], g["lengthscale"])) for g in Q["gps"]])
    H = lmm.Orthogonal(Q["U"], Q["S"])
    xin, xsin = lmm.MOInputIsotopicByOutputs(Q["x"], P), lmm.MOInputIsotopicByOutputs(Q["xs"], P)

    def flat(G, keys):
        out = {k: np.asarray(G[k], dtype=np.float64).reshape(-1).tolist() for k in keys}
        out["value"] = [float(G["value"])]
        for f in ("variance", "lengthscale", "mean"):
            out["gps_" + f] = [float(g[f]) for g in G["gps"]]
        return out

    def verbs(shard):
        fx = lmm.ILMM(mogp, H, shard=shard)(xin, S2)
        r = {"logpdf": {"value": [lmm.logpdf(fx, Q["y"], False)]},
             "grad": flat(lmm.logpdf_and_gradient(fx, Q["y"], False, inputs=True), ("y", "sigma2", "S", "U", "x")),
             "grad_missing_a": flat(lmm.logpdf_and_gradient(fx, Q["ya"], False), ("y", "sigma2")),
             "grad_missing_b": flat(lmm.logpdf_and_gradient(fx, Q["yb"], False), ("y", "sigma2"))}
        post = lmm.posterior(fx, Q["y"])
        mu, var = lmm.mean_and_var(post(xsin, S2), add_noise=False)
        r["mean_and_var"] = {"mean": np.asarray(mu).reshape(-1).tolist(), "var": np.asarray(var).reshape(-1).tolist()}
        r["mean_and_var_vjp"] = {"x": np.asarray(lmm.mean_and_var_vjp(post(xsin, S2), Q["dmean"], Q["dvar"], add_noise=False)["x"]).reshape(-1).tolist()}
        return r

    out = {"whole": verbs((0, M)), "shards": [verbs(s) for s in SHARDS]}
    out["whole_with_regulariser"] = lmm.logpdf(lmm.ILMM(mogp, H)(xin, S2), Q["y"], True)
    fe = lmm.ILMM(mogp, H, shard=(33, 33))(xin, S2)
    out["empty"] = {"logpdf": lmm.logpdf(fe, Q["y"], True), "logpdf_no_regulariser": lmm.logpdf(fe, Q["y"], False),
                    "grad_value": lmm.logpdf_and_gradient(fe, Q["y"], True)["value"]}
    print(json.dumps(out))


@pytest.fixture(scope="module")
def runs():
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, LMM_NSTREAMS="2"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _check_sums(runs, verb):
    whole = runs["whole"][verb]
    for key, w in whole.items():
        w = np.asarray(w)
        parts = sum(np.asarray(s[verb][key]) for s in runs["shards"])
        scale = np.abs(w).max()
        err = np.abs(parts - w).max()
        print(f"{verb}.{key}: |sum of shards - whole| = {err:.3e}, largest entry {scale:.3e}, relative {err / scale if scale else 0.0:.3e}")
        assert np.isfinite(w).all() and scale > 0.0, (verb, key)
        assert err <= RTOL * scale, (verb, key, err, scale)


@pytest.mark.gpu
def test_logpdf_whole_range_equals_shards(runs):
    """logpdf over three batches on two slots = the sum over its three one-batch shards; and the whole-range value against the
    oracle at the suite's usual 1e-6, so that the identity cannot hold between two wrong values."""
    from oracle import lmm_oracle as O
    _check_sums(runs, "logpdf")
    Q = _problem()
    ref = O.oilmm_logpdf(Q["gps"], Q["U"], Q["S"], Q["x"], S2, Q["y"])
    assert abs(runs["whole_with_regulariser"] - ref) <= 1e-6 * abs(ref), (runs["whole_with_regulariser"], ref)


@pytest.mark.gpu
def test_gradient_whole_range_equals_shards(runs):
    """logpdf_and_gradient with input gradients: value, y, sigma2, S, U and x add up over the shards; each latent's (variance,
    lengthscale, mean) comes from the one shard that holds it."""
    _check_sums(runs, "grad")
    for key in ("gps_variance", "gps_lengthscale", "gps_mean"):
        for (l0, l1), s in zip(SHARDS, runs["shards"]):
            outside = np.delete(np.asarray(s["grad"][key]), np.arange(l0, l1))
            assert not outside.any(), (key, l0, l1)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["a", "b"])
def test_missing_data_gradient_whole_range_equals_shards(runs, pattern):
    """The missing-data gradient (NaN in y; a: one pattern of missing outputs beside the complete one, b: two)."""
    _check_sums(runs, "grad_missing_" + pattern)


@pytest.mark.gpu
def test_posterior_verbs_whole_range_equal_shards(runs):
    """posterior then mean_and_var, and the predictive input gradient: a shard's outputs are partial sums."""
    _check_sums(runs, "mean_and_var")
    _check_sums(runs, "mean_and_var_vjp")


@pytest.mark.gpu
def test_empty_shard_in_a_two_stream_plan(runs):
    """latent_begin == latent_end: the regulariser alone, from logpdf and from the gradient's value (as
    test_empty_shard_returns_regulariser_only asserts for logpdf)."""
    from oracle import lmm_oracle as O
    Q = _problem()
    reg = O.regulariser_oilmm(Q["U"], Q["S"], S2, O.reshape_y(Q["y"], N))
    assert runs["empty"]["logpdf"] == pytest.approx(reg, rel=1e-12)
    assert runs["empty"]["grad_value"] == pytest.approx(reg, rel=1e-12)
    assert runs["empty"]["logpdf_no_regulariser"] == 0.0


if __name__ == "__main__":
    _child()
