"""Error behaviour of the per-latent (OILMM / MOGP) entry points: for every entry point that takes training data or a posterior handle, a
table of defective calls with the code and a piece of lmm_last_error_string() each must give.  The expectations are written out from
the order of the checks in each entry point; the rows with two defects pin that order (the first failing check wins).  A defect an
entry point does not check (sigma2 = 0 in lmm_oilmm_logpdf_multi, lmm_oilmm_posterior_create and the MOGP entry points; S outside the
missing-data entry points; m > p where no p is taken; the shard where a handle brings it) has no row: such a call would run.  Every
call here returns before any launch.  The dense-H training entry points (lmm_ilmm_*) have rows of the same form; theirs were recorded
from the build before their shared front end (profiles/dense_h_refactor/entry_checks_parent.txt).

Shapes: n = 8, p = 3, m = 2, d = 1; one per-latent posterior handle at n = 64 and one dense-H handle (the "other kind") at n = 8.
The inducing-point entry points (the bound's gradient, the sparse posterior handle and its mean_and_var at nz = 4, the two one-latent
building blocks) have rows recorded from the build before their shared front end (profiles/oilmm_grad_backend/entry_checks_parent.txt).
The argument lists are built from the declarations in include/lmm_hip.h; a row names the arguments it spoils."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, NOT_PD, ARG, UNSUP = 1, 3, 5, 6          # LMM_ERR_DIM, LMM_ERR_NOT_PD, LMM_ERR_ARG, LMM_ERR_UNSUPPORTED
N, P, M, D, NS, NZ = 8, 3, 2, 1, 4, 4

# messages
BAD, OUTDIM, SHARD, SIGMA2, SBAD, GPS = "bad arguments", "out dim of x != out dim of f.", "bad latent shard", "sigma2 must be > 0", "S must be finite and > 0 (S[1] = ", "gps is NULL"
DTYPE = "posterior handle was built in the other compute dtype"
HM, HD = "posterior has 2 latents, H has 3", "input dimension mismatch"
PROJECT = "PosDefException in project(H, sigma2)"
HDXS = "input dimension mismatch: posterior has d=1, xs has d=2"

# spoiled arguments
NULLX, NULLU, NULLXS, NULLH = {"x": None}, {"U": None}, {"xs": None}, {"H": None}
MP = {"m": 4}                       # m > p; the shard [0, 2) stays inside [0, m]
SH = {"latent_end": 3}              # shard outside [0, m]
S0 = {"sigma2": 0.0}
SNAN = {"S": "S_nan"}
NOGPS = {"gps": None}
OTHER, PRIOR = {"post": "dense"}, {"post": None}
M3, D2 = {"m": 3}, {"d": 2}
NZBIG, J0 = {"nz": 1025}, {"jitter": 0.0}          # one inducing point more than LMM_SPARSE_MMAX
NZMSG, JITTER = "inducing-point inference is served for at most 1024 inducing points (nz = 1025)", "jitter must be finite and > 0"
SPARSE, NOTSPARSE = {"post": "sparse"}, "not a handle of lmm_oilmm_sparse_posterior_create"
F32 = {"f32": 1}                    # the call is made in the other compute dtype than the handles were built in


def both(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


DENSE = [("NULL x", NULLX, ARG, BAD), ("NULL H", NULLH, ARG, BAD), ("no gps", NOGPS, ARG, GPS), ("NULL x and no gps", both(NULLX, NOGPS), ARG, BAD)]
TRAIN = [("NULL x", NULLX, ARG, BAD), ("m > p", MP, DIM, OUTDIM), ("shard", SH, ARG, SHARD)]
TABLE = {
    # ---- training data: args, m > p, shard, resolve, then sigma2 (S is not checked)
    "lmm_oilmm_logpdf": TRAIN + [("sigma2 = 0", S0, ARG, SIGMA2), ("m > p and shard", both(MP, {"latent_end": 5}), DIM, OUTDIM),
                                 ("shard and sigma2 = 0", both(SH, S0), ARG, SHARD), ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS)],
    "lmm_oilmm_logpdf_grad_x": TRAIN + [("sigma2 = 0", S0, ARG, SIGMA2), ("shard and sigma2 = 0", both(SH, S0), ARG, SHARD),
                                        ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS)],
    # args, m > p, shard, resolve; sigma2 is not checked
    "lmm_oilmm_logpdf_multi": [("NULL Y", {"Y": None}, ARG, BAD), ("ncol = 0", {"ncol": 0}, ARG, BAD), ("m > p", MP, DIM, OUTDIM), ("shard", SH, ARG, SHARD),
                               ("NULL x and m > p", both(NULLX, MP), ARG, BAD), ("m > p and shard", both(MP, {"latent_end": 5}), DIM, OUTDIM)],
    "lmm_oilmm_posterior_create": TRAIN + [("NULL x and m > p", both(NULLX, MP), ARG, BAD), ("shard and no gps", both(SH, NOGPS), ARG, SHARD)],
    # args, m > p, shard, resolve, the batches, then the test points' sigma2
    "lmm_oilmm_post_logpdf_grad_seq_x": [("NULL ys", {"ys": None}, ARG, BAD), ("m > p", MP, DIM, OUTDIM), ("shard", SH, ARG, SHARD),
                                         ("sigma2_s = 0", {"sigma2_s": 0.0}, ARG, SIGMA2), ("batches", {"batch_n": "batch_bad"}, ARG, "batch sizes do not add up to n"),
                                         ("shard and batches", both(SH, {"batch_n": "batch_bad"}), ARG, SHARD),
                                         ("batches and sigma2_s = 0", {"batch_n": "batch_bad", "sigma2_s": 0.0}, ARG, "batch sizes do not add up to n")],
    # args, m > p, sigma2, S, shard, resolve
    **{name: TRAIN + [("sigma2 = 0", S0, ARG, SIGMA2), ("S not finite", SNAN, ARG, SBAD), ("sigma2 = 0 and S", both(S0, SNAN), ARG, SIGMA2),
                      ("S and shard", both(SNAN, SH), ARG, SBAD), ("m > p and sigma2 = 0", both(MP, S0), DIM, OUTDIM)]
       for name in ("lmm_oilmm_logpdf_missing", "lmm_oilmm_posterior_create_missing", "lmm_oilmm_logpdf_grad_missing")},
    # the inducing-point bound: args, m > p, shard, shape (jitter), sigma2, resolve
    "lmm_oilmm_elbo": TRAIN + [("NULL z", {"z": None}, ARG, BAD), ("sigma2 = 0", S0, ARG, SIGMA2), ("shard and jitter = 0", both(SH, {"jitter": 0.0}), ARG, SHARD),
                               ("jitter = 0 and sigma2 = 0", both({"jitter": 0.0}, S0), ARG, "jitter must be finite and > 0"),
                               ("sigma2 = 0 and no gps", both(S0, NOGPS), ARG, SIGMA2)],
    # its gradient tests its own arguments and the shape (nz, d, dtype, jitter) ahead of the shared front end: those come before m > p and the shard
    "lmm_oilmm_elbo_grad": TRAIN + [("NULL z", {"z": None}, ARG, BAD), ("nz above the limit", NZBIG, UNSUP, NZMSG), ("jitter = 0", J0, ARG, JITTER), ("sigma2 = 0", S0, ARG, SIGMA2),
                                    ("NULL z and nz above the limit", both({"z": None}, NZBIG), ARG, BAD), ("nz above the limit and jitter = 0", both(NZBIG, J0), UNSUP, NZMSG),
                                    ("jitter = 0 and m > p", both(J0, MP), ARG, JITTER), ("jitter = 0 and shard", both(J0, SH), ARG, JITTER),
                                    ("nz above the limit and shard", both(NZBIG, SH), UNSUP, NZMSG), ("m > p and shard", both(MP, {"latent_end": 5}), DIM, OUTDIM),
                                    ("shard and sigma2 = 0", both(SH, S0), ARG, SHARD), ("jitter = 0 and sigma2 = 0", both(J0, S0), ARG, JITTER),
                                    ("sigma2 = 0 and no gps", both(S0, NOGPS), ARG, SIGMA2), ("no gps", NOGPS, ARG, GPS)],
    # the handle: its own output, then the bound's order
    "lmm_oilmm_sparse_posterior_create": TRAIN + [("NULL out", {"out": None}, ARG, BAD), ("NULL z", {"z": None}, ARG, BAD), ("nz above the limit", NZBIG, UNSUP, NZMSG),
                                                  ("jitter = 0", J0, ARG, JITTER), ("sigma2 = 0", S0, ARG, SIGMA2), ("m > p and nz above the limit", both(MP, NZBIG), DIM, OUTDIM),
                                                  ("shard and jitter = 0", both(SH, J0), ARG, SHARD), ("jitter = 0 and sigma2 = 0", both(J0, S0), ARG, JITTER),
                                                  ("sigma2 = 0 and no gps", both(S0, NOGPS), ARG, SIGMA2), ("no gps", NOGPS, ARG, GPS)],
    # args, dtype, handle kind, m, d (every row names its handle: the table's `post` is a per-latent one, another kind here)
    "lmm_oilmm_sparse_mean_and_var": [("NULL U", both(SPARSE, NULLU), ARG, BAD), ("no handle", PRIOR, ARG, BAD), ("other kind", {}, ARG, NOTSPARSE), ("other kind (dense-H)", OTHER, ARG, NOTSPARSE),
                                      ("other m", both(SPARSE, M3), DIM, HM), ("other d", both(SPARSE, D2), DIM, HDXS), ("other dtype", both(SPARSE, F32), UNSUP, "inducing-point inference is Float64 only"),
                                      ("NULL U and other kind", NULLU, ARG, BAD), ("other dtype and other kind", F32, UNSUP, "inducing-point inference is Float64 only"),
                                      ("other kind and other m", M3, ARG, NOTSPARSE), ("other m and other d", both(SPARSE, M3, D2), DIM, HM)],
    # the one-latent building blocks: args (ld < nz among them), then the sizes; no dtype and no jitter check
    **{name: [("NULL x", NULLX, ARG, BAD), ("ld < nz", {"ld": NZ - 1}, ARG, BAD), ("nz above the limit", both(NZBIG, {"ld": 1025}), UNSUP, NZMSG),
              ("d above the limit", {"d": 33}, UNSUP, "inducing-point inference is served for d <= 32 (d = 33)"),
              ("ld < nz and nz above the limit", NZBIG, ARG, BAD), ("nz and d above the limit", both(NZBIG, {"ld": 1025, "d": 33}), UNSUP, NZMSG)]
       for name in ("lmm_dev_sparse_moments", "lmm_dev_sparse_grad")},
    # IndependentMOGP: args, shard, resolve
    **{name: [("NULL x", NULLX, ARG, BAD), ("shard", SH, ARG, SHARD), ("NULL x and shard", both(NULLX, SH), ARG, BAD), ("shard and no gps", both(SH, NOGPS), ARG, SHARD)]
       for name in ("lmm_mogp_logpdf", "lmm_mogp_logpdf_diag", "lmm_mogp_posterior_create")},
    # ---- prediction: dtype, args, (entry point's own), handle kind, m, d, or resolve; then the shard
    "lmm_latent_marginals": [("NULL xs", NULLXS, ARG, BAD), ("other kind", OTHER, UNSUP, "use lmm_ilmm_post_mean_and_var"), ("other d", D2, DIM, HDXS),
                             ("other dtype", F32, ARG, DTYPE), ("other dtype and NULL xs", both(F32, NULLXS), ARG, DTYPE), ("NULL xs and other kind", both(NULLXS, OTHER), ARG, BAD)],
    "lmm_oilmm_mean_and_var": [("NULL U", NULLU, ARG, BAD), ("shard", both(PRIOR, SH), ARG, SHARD), ("other kind", OTHER, UNSUP, "dense-H posterior handle: use lmm_ilmm_post_mean_and_var"),
                               ("other m", M3, DIM, HM), ("other d", both(D2, {"var_out": None}), DIM, HDXS), ("other dtype", F32, ARG, DTYPE),
                               ("other dtype and NULL U", both(F32, NULLU), ARG, DTYPE), ("other kind and other m", both(OTHER, M3), UNSUP, "dense-H posterior handle"),
                               ("no gps and shard", both(PRIOR, NOGPS, SH), ARG, GPS)],
    "lmm_oilmm_mean_and_var_grad_xs": [("NULL U", NULLU, ARG, BAD), ("shard", both(PRIOR, SH), ARG, SHARD), ("other kind", OTHER, UNSUP, "of a dense-H posterior (coupled latents) are not served"),
                                       ("other m", M3, DIM, HM), ("other d", D2, DIM, HDXS), ("other dtype", F32, UNSUP, "Float64 compute mode only"),
                                       ("other kind and d > 32", both(OTHER, {"d": 33}), UNSUP, "of a dense-H posterior"), ("other m and other d", both(M3, D2), DIM, HM)],
    "lmm_lmm_mean_and_cov": [("NULL U", NULLU, ARG, BAD), ("shard", both(PRIOR, SH), ARG, SHARD), ("other kind", OTHER, UNSUP, "full covariance of the dense-H posterior is not built"),
                             ("other m", M3, DIM, HM), ("other d", D2, DIM, HD), ("other dtype", F32, ARG, DTYPE),
                             ("too large and other kind", both({"ns": 20000}, OTHER), UNSUP, "too large"), ("other m and other d", both(M3, D2), DIM, HM)],
    "lmm_mogp_cross_cov": [("NULL x", NULLX, ARG, BAD), ("shard", both(PRIOR, SH), ARG, SHARD), ("other kind", OTHER, UNSUP, "cross-covariance of the coupled latents"),
                           ("other m", M3, DIM, "posterior has 2 latents, m = 3"), ("other d", D2, DIM, "input dimension mismatch: posterior has d=1, x has d=2"),
                           ("other dtype", F32, ARG, DTYPE), ("other kind and other m", both(OTHER, M3), UNSUP, "cross-covariance"), ("other m and other d", both(M3, D2), DIM, "m = 3")],
    "lmm_oilmm_post_logpdf": [("NULL U", NULLU, ARG, BAD), ("m > p", {"p": 1}, DIM, OUTDIM), ("sigma2 = 0", S0, ARG, SIGMA2), ("other kind", OTHER, UNSUP, "use lmm_ilmm_post_logpdf"),
                              ("other m", M3, DIM, HM), ("other d", D2, DIM, HD), ("other dtype", F32, ARG, DTYPE),
                              ("other d and m > p", both(D2, {"p": 1}), DIM, HD), ("m > p and sigma2 = 0", both({"p": 1}, S0), DIM, OUTDIM)],
    "lmm_lmm_rand_multi": [("NULL U", NULLU, ARG, BAD), ("shard", both(PRIOR, SH), ARG, SHARD), ("other kind", OTHER, UNSUP, "use lmm_ilmm_post_rand"), ("other m", M3, DIM, HM),
                           ("other d", D2, DIM, HD), ("other dtype", F32, ARG, DTYPE), ("no eps and other kind", both({"add_noise": 1}, OTHER), ARG, "eps is NULL"),
                           ("other kind and other d", both(OTHER, D2), UNSUP, "use lmm_ilmm_post_rand")],
    "lmm_post_condition": [("NULL U", NULLU, ARG, BAD), ("m > p", {"p": 1}, DIM, OUTDIM), ("other kind", OTHER, UNSUP, "sequential conditioning of the dense-H posterior is not built"),
                           ("other m", M3, DIM, HM), ("other d", D2, DIM, HD), ("other dtype", F32, ARG, DTYPE),
                           ("other dtype and NULL U", both(F32, NULLU), ARG, DTYPE), ("other m and m > p", both(M3, {"p": 1}), DIM, HM)],
    # the dense-H handle's own entry points: the dtype check comes first
    **{name: [("other dtype", both(OTHER, F32), ARG, DTYPE), ("other dtype and NULL input", both(OTHER, F32, {"xs": None, "x2": None}), ARG, DTYPE)]
       for name in ("lmm_ilmm_post_mean_and_var", "lmm_ilmm_post_mean_and_cov", "lmm_ilmm_post_condition", "lmm_ilmm_post_logpdf", "lmm_ilmm_post_rand")},
    # ---- dense-H training data (no shard, no m > p): args, resolve, then sigma2 where the entry point tests it; lmm_ilmm_logpdf_ex and
    # lmm_ilmm_posterior_create do not, and project(H, sigma2) refuses sigma2 = 0 on the host
    "lmm_ilmm_logpdf_ex": DENSE + [("sigma2 = 0", S0, NOT_PD, PROJECT), ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS)],
    "lmm_ilmm_logpdf_multi": DENSE + [("NULL Y", {"Y": None}, ARG, BAD), ("ncol = 0", {"ncol": 0}, ARG, BAD), ("sigma2 = 0", S0, ARG, SIGMA2),
                                      ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS), ("ncol = 0 and sigma2 = 0", both({"ncol": 0}, S0), ARG, BAD)],
    "lmm_ilmm_logpdf_grad_x": DENSE + [("sigma2 = 0", S0, ARG, SIGMA2), ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS),
                                       ("NULL H and sigma2 = 0", both(NULLH, S0), ARG, BAD)],
    # args, resolve, the batches, then the test points' sigma2
    "lmm_ilmm_post_logpdf_grad_seq_x": DENSE + [("NULL ys", {"ys": None}, ARG, BAD), ("sigma2_s = 0", {"sigma2_s": 0.0}, ARG, SIGMA2),
                                                ("batches", {"batch_n": "batch_bad"}, ARG, "batch sizes do not add up to n"),
                                                ("no gps and batches", both(NOGPS, {"batch_n": "batch_bad"}), ARG, GPS),
                                                ("batches and sigma2_s = 0", {"batch_n": "batch_bad", "sigma2_s": 0.0}, ARG, "batch sizes do not add up to n")],
    "lmm_ilmm_posterior_create": DENSE + [("sigma2 = 0", S0, NOT_PD, PROJECT), ("no gps and sigma2 = 0", both(NOGPS, S0), ARG, GPS)],
}
CASES = [(name, label, spoil, code, msg) for name, rows in TABLE.items() for label, spoil, code, msg in rows]


@functools.lru_cache(maxsize=None)
def declared(name):
    """[(argument name, 'p' / 'i' / 'd')] of an entry point, from its declaration in the header"""
    text = open(os.path.join(ROOT, "include", "lmm_hip.h")).read()
    args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S).group(1)
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        out.append((a.split()[-1].lstrip("*"), "p" if "*" in a else "d" if a.startswith("double ") else "i"))
    return out


@pytest.fixture(scope="module")
def env():
    from lmm_amd import _lib as L
    L.ensure_init()
    lib = L.load()
    rng = np.random.default_rng(0)
    keep = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in {
        "x": np.linspace(0.0, 1.0, 64), "y": rng.standard_normal(64 * P),
        "S": np.array([1.0, 2.0, 1.5, 1.0]), "S_nan": np.array([1.0, np.nan, 1.5, 1.0]), "xs": np.linspace(0.1, 0.9, 2 * NS), "z": np.linspace(0.0, 1.0, NZ),
        "batch_sigma2": np.array([0.1]), "noise_diag": np.full(N * M, 0.1), "scratch": np.zeros(4096)}.items()}
    keep["U"] = np.array(np.linalg.qr(rng.standard_normal((P, P)))[0].ravel(order="F").tolist() + [0.0] * 7)      # p x 3 orthonormal columns (+ room for m = 4)
    keep["batch_n"], keep["batch_bad"] = np.array([N], dtype=np.int32), np.array([N - 1], dtype=np.int32)
    gps = (L.GpT * 4)(*[L.GpT(0, 1.0, 0.5, 0.0) for _ in range(4)])      # SE latents
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in keep.items()}
    ptr["gps"] = C.cast(gps, C.c_void_p)
    # the handles: per-latent at n = 64, dense-H at n = 8 (both in the Float64 compute dtype)
    post, dense = C.c_void_p(), C.c_void_p()
    L.check(lib.lmm_oilmm_posterior_create(ptr["x"], C.c_int(D), C.c_int(64), ptr["y"], C.c_int(P), ptr["U"], ptr["S"], C.c_int(M), C.c_double(0.1), ptr["gps"],
                                           C.c_int(0), C.c_int(M), C.byref(post)))
    L.check(lib.lmm_ilmm_posterior_create(ptr["x"], C.c_int(D), C.c_int(N), ptr["y"], C.c_int(P), ptr["U"], C.c_int(M), C.c_double(0.1), ptr["gps"], None, C.byref(dense)))
    sparse = C.c_void_p()
    L.check(lib.lmm_oilmm_sparse_posterior_create(ptr["x"], C.c_int(D), C.c_int(64), ptr["y"], C.c_int(P), ptr["U"], ptr["S"], C.c_int(M), C.c_double(0.1), ptr["gps"],
                                                  C.c_int(0), C.c_int(M), ptr["z"], C.c_int(NZ), C.c_double(1e-6), C.byref(sparse)))
    ptr["post"], ptr["dense"], ptr["sparse"] = post, dense, sparse
    yield lib, ptr, (keep, gps)
    lib.lmm_sparse_post_destroy(sparse)
    lib.lmm_set_compute_dtype(C.c_int(0))
    lib.lmm_post_destroy(post)
    lib.lmm_post_destroy(dense)


# what a sound call passes, by argument name; any other pointer is an output (or an optional input) and gets the scratch block
VALUES = {"d": D, "n": N, "p": P, "m": M, "ncol": 2, "ns": NS, "nz": NZ, "n2": NS, "nbatch": 1, "nsamples": 1, "m_shard": M, "latent_begin": 0, "latent_end": M,
          "with_regulariser": 1, "add_noise": 0, "allow_decoupled": 1, "x_by_features": 0, "y_by_features": 0, "sigma2": 0.1, "sigma2_s": 0.1, "jitter": 1e-6,
          "ld": NZ, "chunk": 0}
INPUTS = {"x": "x", "y": "y", "Y": "y", "U": "U", "H": "U", "S": "S", "gps": "gps", "xs": "xs", "ys": "y", "z": "z", "batch_n": "batch_n", "batch_sigma2": "batch_sigma2",
          "noise_diag": "noise_diag", "post": "post", "x2": "xs", "y2": "y", "z_lat": "y", "dmean": "y", "dvar": "y"}
NULLS = {"jit", "eps", "grad_y", "grad_ys", "grad_sigma2", "grad_S", "grad_U", "grad_gps", "grad_x", "grad_batch_sigma2", "grad_sigma2_s", "dtc"}


@pytest.mark.gpu
@pytest.mark.parametrize("name,label,spoil,code,msg", CASES, ids=[f"{c[0]}-{c[1].replace(' ', '_')}" for c in CASES])
def test_defective_call(env, name, label, spoil, code, msg):
    lib, ptr, _ = env
    args = []
    for arg, kind in declared(name):
        if kind == "p":
            v = spoil[arg] if arg in spoil else None if arg in NULLS else INPUTS.get(arg, "scratch")
            args.append(None if v is None else ptr[v])
        else:
            v = spoil.get(arg, VALUES[arg])
            args.append(C.c_double(v) if kind == "d" else C.c_int(v))
    if name == "lmm_mogp_cross_cov":          # its y is a second set of inputs
        args[[a for a, _ in declared(name)].index("y")] = ptr["xs"]
    lib.lmm_set_compute_dtype(C.c_int(spoil.get("f32", 0)))
    try:
        rc = getattr(lib, name)(*args)
    finally:
        lib.lmm_set_compute_dtype(C.c_int(0))
    text = lib.lmm_last_error_string().decode()
    print(f"{name} [{label}]: rc = {rc}, {text!r}")
    assert rc == code and msg in text, (rc, text)
