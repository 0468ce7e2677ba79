"""Host-only checks of the gradient of the inducing-point (VFE) bound (include/lmm_hip.h "inducing points"): the two
entry points are declared, exported and bound, elbo_and_gradient refuses what elbo refuses before any library call, and three Float64
CPU restatements of the gradient of one latent's bound agree on every case of tests/test_gpu_sparse_grad.py:

    dense     torch autograd of the dense formula of tests/test_gpu_sparse.py::dense_latent
    lowrank   torch autograd of the low-rank algebra of lowrank_latent (Phi, b, L_u, B, L_B, c)
    backward  a NumPy restatement of exactly the library's backward algebra: X = L_u^-1, Y = L_B^-1 X, PhiBar, KuuBar, the weights
              g = (2 PhiBar K_uf + beta r') / w, then sum g dk (dk from autograd of the kernel matrix with g held constant)

delta is their largest disagreement per gradient array, max|a - b| / max|b| against the dense one; it fixes the tolerance of the GPU
tests, max(1e-10, 100 delta).  No GPU and no lmm_init needed.  This module also holds the cases and restatements the GPU tests share.

Cases (x uniform on [0, 10]^d, z equispaced plus 0.3 N(0, 1) per coordinate at d > 1, eps = 1e-6, w = 0.1; per-dimension lengthscales
l (1, 1.8, 1.3)); `python tests/test_sparse_grad_abi.py` prints cond(K_uu + eps I) and delta per case."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # run as a script: the package loader lies in the repository root
    sys.path.insert(0, ROOT)

import lmm_amd
from lmm_amd import _lib as L

HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SYMS = ("lmm_oilmm_elbo_grad", "lmm_dev_sparse_grad")
LOG2PI = math.log(2.0 * math.pi)
EPS = 1e-6
ARD = np.array([1.0, 1.8, 1.3])
DT = torch.float64


# ---------------------------------------------------------------------------------------------------
# kernels: ("se" | "matern12" | "matern32" | "matern52", v, ls), ("rq", v, ls, alpha), ("periodic", v, period, r),
# ("lp", v, period, r, decay), ("sum", v0, s0, [terms]); ls / period a float or a length-d list
# ---------------------------------------------------------------------------------------------------
def to_kernel(lmm, k):
    cls = {"se": lmm.SEKernel, "matern12": lmm.Matern12Kernel, "matern32": lmm.Matern32Kernel, "matern52": lmm.Matern52Kernel}
    if k[0] == "sum":
        return lmm.KernelSum(*[to_kernel(lmm, t) for t in k[3]], variance=k[1], lengthscale=k[2])
    if k[0] == "rq":
        return lmm.RationalQuadraticKernel(k[1], k[2], alpha=k[3])
    if k[0] == "periodic":
        return lmm.PeriodicKernel(k[1], k[2], r=k[3])
    if k[0] == "lp":
        return lmm.LocallyPeriodicKernel(k[1], k[2], r=k[3], decay=k[4])
    return cls[k[0]](k[1], k[2])


def tparams(k):
    """The kernel's parameters as torch leaves, named as the library's gradient dicts name them."""
    leaf = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=DT, requires_grad=True)
    if k[0] == "sum":
        return {"variance": leaf(k[1]), "lengthscale": leaf(k[2]), "terms": [tparams(t) for t in k[3]]}
    tp = {"variance": leaf(k[1]), "lengthscale": leaf(k[2])}
    if k[0] == "rq":
        tp["alpha"] = leaf(k[3])
    if k[0] in ("periodic", "lp"):
        tp["r"] = leaf(k[3])
    if k[0] == "lp":
        tp["decay"] = leaf(k[4])
    return tp


def leaves(tp):
    """[(name, leaf)] in a fixed order; a sum's terms as terms.<c>.<name>."""
    out = [(n, tp[n]) for n in ("variance", "lengthscale", "alpha", "r", "decay") if n in tp]
    for c, t in enumerate(tp.get("terms", [])):
        out += [(f"terms.{c}.{n}", v) for n, v in leaves(t)]
    return out


def _kbase_t(k, tp, A, B, v0=1.0, s0=1.0):
    d = A.shape[0]
    ls = (tp["lengthscale"] * s0).expand(d) if tp["lengthscale"].ndim == 0 else tp["lengthscale"] * s0
    dx = A[:, :, None] - B[:, None, :]
    D = dx / ls[:, None, None]
    v = v0 * tp["variance"]
    if k[0] in ("periodic", "lp"):
        e = -0.5 * (torch.sin(math.pi * D) ** 2).sum(0) / tp["r"] ** 2
        if k[0] == "lp":
            e = e - 0.5 * (dx ** 2).sum(0) / (s0 * tp["decay"]) ** 2
        return v * torch.exp(e)
    r2 = (D ** 2).sum(0)
    if k[0] == "se":
        return v * torch.exp(-0.5 * r2)
    if k[0] == "rq":
        return v * (1.0 + r2 / (2.0 * tp["alpha"])) ** (-tp["alpha"])
    pos = r2 > 0                                       # sqrt has no derivative at 0: the Matern32 / 52 gradient is 0 there, and a Matern12 pair
    r = torch.where(pos, torch.sqrt(torch.where(pos, r2, torch.ones_like(r2))), torch.zeros_like(r2))      # at r = 0 contributes 0 (grad_x_kernel)
    if k[0] == "matern12":
        return v * torch.exp(-r)
    if k[0] == "matern32":
        return v * (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    assert k[0] == "matern52", k[0]
    return v * (1.0 + math.sqrt(5.0) * r + 5.0 * r2 / 3.0) * torch.exp(-math.sqrt(5.0) * r)


def kmat_t(k, tp, A, B):
    if k[0] == "sum":
        return sum(_kbase_t(t, tt, A, B, tp["variance"], tp["lengthscale"]) for t, tt in zip(k[3], tp["terms"]))
    return _kbase_t(k, tp, A, B)


def kdiag_t(k, tp):
    return tp["variance"] * sum(tt["variance"] for tt in tp["terms"]) if k[0] == "sum" else tp["variance"]


def tens(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=DT, requires_grad=grad)


def cols_t(x):
    return x[None, :] if x.ndim == 1 else x


# ---------------------------------------------------------------------------------------------------
# one latent's bound, three ways.  x: (d, n), z: (d, M) NumPy; w: scalar; r: (n,)
# ---------------------------------------------------------------------------------------------------
def elbo_dense_t(k, tp, x, z, w, r, eps):
    n, M = x.shape[1], z.shape[1]
    Kuf = kmat_t(k, tp, z, x)
    Lu = torch.linalg.cholesky(kmat_t(k, tp, z, z) + eps * torch.eye(M, dtype=DT))
    A = torch.linalg.solve_triangular(Lu, Kuf, upper=False)
    Q = A.T @ A
    Lc = torch.linalg.cholesky(Q + torch.diag(w.expand(n)))
    v = torch.linalg.solve_triangular(Lc, r[:, None], upper=False)[:, 0]
    dtc = -0.5 * (n * LOG2PI + 2.0 * torch.log(torch.diagonal(Lc)).sum() + v @ v)
    return dtc - 0.5 * ((kdiag_t(k, tp) - torch.diagonal(Q)) / w).sum()


def elbo_lowrank_t(k, tp, x, z, w, r, eps):
    n, M = x.shape[1], z.shape[1]
    Kuf = kmat_t(k, tp, z, x)
    Phi, b, s, kap, lam = (Kuf / w) @ Kuf.T, Kuf @ (r / w), (r * r / w).sum(), n * kdiag_t(k, tp) / w, n * torch.log(w)
    Lu = torch.linalg.cholesky(kmat_t(k, tp, z, z) + eps * torch.eye(M, dtype=DT))
    Cq = torch.linalg.solve_triangular(Lu, torch.linalg.solve_triangular(Lu, Phi, upper=False).T, upper=False)
    LB = torch.linalg.cholesky(torch.eye(M, dtype=DT) + 0.5 * (Cq + Cq.T))
    c = torch.linalg.solve_triangular(LB, torch.linalg.solve_triangular(Lu, b[:, None], upper=False), upper=False)[:, 0]
    dtc = -0.5 * (n * LOG2PI + lam + 2.0 * torch.log(torch.diagonal(LB)).sum() + s - c @ c)
    return dtc - 0.5 * (kap - torch.trace(Cq))


def autograd_latent(fn, k, x, z, w, r, eps):
    """{"value", "theta": {name: array}, "z", "r", "w"} by torch autograd of fn."""
    tp, zt, wt, rt = tparams(k), tens(z, True), tens(w, True), tens(r, True)
    val = fn(k, tp, tens(x), zt, wt, rt, eps)
    names, lv = zip(*leaves(tp))
    g = torch.autograd.grad(val, list(lv) + [zt, rt, wt])
    return {"value": float(val.detach()), "theta": {n: gi.numpy().copy() for n, gi in zip(names, g)}, "z": g[-3].numpy(), "r": g[-2].numpy(),
            "w": float(g[-1])}


def backward_state(k, x, z, w, r, eps):
    """The library's backward algebra in NumPy: (PhiBar, KuuBar, beta, Kuf, kdiag, cond(K_uu + eps I)) with an explicit X and Y."""
    tp = tparams(k)
    with torch.no_grad():
        Kuf, Kuu, kd = kmat_t(k, tp, tens(z), tens(x)).numpy(), kmat_t(k, tp, tens(z), tens(z)).numpy(), float(kdiag_t(k, tp))
    M = Kuu.shape[0]
    Kj = Kuu + eps * np.eye(M)
    Phi, b = (Kuf / w) @ Kuf.T, Kuf @ (r / w)
    Lu = np.linalg.cholesky(Kj)
    X = np.linalg.inv(Lu)
    Q = X @ Phi @ X.T
    LB = np.linalg.cholesky(np.eye(M) + 0.5 * (Q + Q.T))
    Y = np.linalg.inv(LB) @ X
    beta = Y.T @ (Y @ b)
    PhiBar = 0.5 * (X.T @ X - Y.T @ Y - np.outer(beta, beta))
    T2 = X.T @ Q @ X
    return PhiBar, PhiBar - 0.25 * (T2 + T2.T), beta, Kuf, kd, np.linalg.cond(Kj)


def contract(k, x, z, G, Kbar=None, kdw=0.0):
    """sum G . K_uf(theta, z) [+ sum Kbar . K_uu(theta, z) - kdw kdiag(theta)] differentiated with respect to theta and z, G held constant."""
    tp, zt = tparams(k), tens(z, True)
    val = (tens(G) * kmat_t(k, tp, zt, tens(x))).sum()
    if Kbar is not None:
        val = val + (tens(Kbar) * kmat_t(k, tp, zt, zt)).sum() - kdw * kdiag_t(k, tp)
    names, lv = zip(*leaves(tp))
    g = torch.autograd.grad(val, list(lv) + [zt], allow_unused=True)
    g = [torch.zeros_like(v) if gi is None else gi for gi, v in zip(g, list(lv) + [zt])]
    return {n: gi.numpy().copy() for n, gi in zip(names, g)}, g[-1].numpy()


def backward_latent(k, x, z, w, r, eps):
    n = x.shape[1]
    PhiBar, KuuBar, beta, Kuf, kd, cond = backward_state(k, x, z, w, r, eps)
    G = (2.0 * PhiBar @ Kuf + np.outer(beta, r)) / w
    theta, gz = contract(k, x, z, G, KuuBar, 0.5 * n / w)
    b, s, kap = Kuf @ (r / w), np.sum(r * r) / w, n * kd / w
    gw = -(0.5 * np.sum(G * Kuf) + 0.5 * beta @ b - 0.5 * s - 0.5 * kap) / w - n / (2.0 * w)
    return {"theta": theta, "z": gz, "r": (beta @ Kuf - r) / w, "w": gw, "cond": cond}


def relmax(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return float(np.abs(a - b).max() / np.abs(b).max())


def flat(g):
    """The gradient arrays of one latent as {name: array}."""
    out = {"theta." + n: v for n, v in g["theta"].items()}
    out.update(z=g["z"], r=g["r"], w=g["w"])
    return out


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
def ls_of(l, d, ard):
    return [float(v) for v in l * ARD[:d]] if ard else l


def kernel_of(name, l, d, ard=False):
    e = ls_of(l, d, ard)
    if name == "m52":
        return ("matern52", 1.3, e)
    if name == "m52+per":
        return ("sum", 1.2, 1.0, [("matern52", 0.8, e), ("periodic", 0.5, ls_of(2.0, d, ard), 0.9)])
    if name == "rq+lp":
        return ("sum", 1.1, 1.0, [("rq", 0.9, e, 1.5), ("lp", 0.6, ls_of(2.5, d, ard), 0.8, 0.75)])
    assert name == "m12+se+m32", name
    return ("sum", 1.2, 1.0, [("matern12", 0.7, e), ("se", 0.5, e), ("matern32", 0.9, e)])


# (n, M, d, kernel, l, ARD)
CASES = [(1, 1, 1, "m52", 0.5, False), (63, 16, 1, "m52", 0.5, False), (63, 16, 1, "rq+lp", 0.5, False), (333, 70, 1, "m52", 0.2, False),
         (333, 70, 1, "m52+per", 0.2, False), (200, 70, 2, "m52", 0.25, True), (200, 70, 2, "m52+per", 0.25, True),
         (200, 70, 3, "rq+lp", 0.4, True), (200, 70, 3, "m12+se+m32", 0.4, True), (97, 65, 2, "m52", 0.3, True),
         (1000, 130, 1, "m52+per", 0.1, False)]
W = 0.1


def case_problem(n, M, d, name, l, ard):
    rng = np.random.default_rng(7 * n + M + d)
    x = rng.uniform(0.0, 10.0, (d, n))
    z = np.linspace(0.0, 10.0, M)[None, :] * np.ones((d, 1)) + (0.3 * rng.normal(size=(d, M)) if d > 1 else 0.0)
    return kernel_of(name, l, d, ard), x, z, rng.normal(size=n)


_CACHE = {}


def case_reference(case):
    """Computed once per session: (kernel, x, z, r, dense, lowrank, backward, delta per array, cond)."""
    if case not in _CACHE:
        k, x, z, r = case_problem(*case)
        dn, lr, bw = (autograd_latent(elbo_dense_t, k, x, z, W, r, EPS), autograd_latent(elbo_lowrank_t, k, x, z, W, r, EPS),
                      backward_latent(k, x, z, W, r, EPS))
        fd, fl, fb = flat(dn), flat(lr), flat(bw)
        delta = {a: max(relmax(fl[a], fd[a]), relmax(fb[a], fd[a])) for a in fd}
        _CACHE[case] = (k, x, z, r, dn, lr, bw, delta, bw["cond"])
    return _CACHE[case]


# ---------------------------------------------------------------------------------------------------
# the three-latent OILMM of tests/test_gpu_sparse.py::problem with every kind of gradient entry: an RQ latent with a length-1
# lengthscale array, a locally periodic latent with a mean, a Matern52 + Periodic sum
# ---------------------------------------------------------------------------------------------------
def model_gps(l):
    return [(("rq", 1.2, [l], 1.5), 0.0), (("lp", 0.8, 2.5, 0.8, l), 0.3),
            (("sum", 1.1, 1.0, [("matern52", 0.8, l), ("periodic", 0.5, 2.0, 0.9)]), 0.0)]


MODEL_SHAPES = [(63, 16, 0.5), (333, 70, 0.2)]


def model_problem(n, M, l):
    import test_gpu_sparse as G
    P = G.problem(n, M, gps=model_gps(l))
    return P


def model_value_t(P, latent_fn, with_reg, leaf):
    """The model's bound in torch: projection, regulariser and the per-latent bound.  leaf: {"Y", "s2", "S", "U", "z", "gps": [(tp, mean)]}."""
    Y, s2, S, U, z = leaf["Y"], leaf["s2"], leaf["S"], leaf["U"], leaf["z"]
    (p, n), m = Y.shape, S.shape[0]
    Ty = (U / torch.sqrt(S)[None, :]).T @ Y
    val = torch.zeros((), dtype=DT)
    if with_reg:
        R = Y - U @ (U.T @ Y)
        val = val - 0.5 * (n * (torch.log(S).sum() + (p - m) * torch.log(2.0 * math.pi * s2)) + (R * R).sum() / s2)
    x = tens(P["x"])[None, :]
    for l, ((k, _), (tp, mu)) in enumerate(zip(P["gps"], leaf["gps"])):
        val = val + latent_fn(k, tp, x, cols_t(z), s2 / S[l], Ty[l] - mu, P["eps"])
    return val


def model_gradient(P, latent_fn, with_reg):
    """{"value", "y", "sigma2", "S", "U", "z", "gps": [{name: array, "mean"}]} by autograd of model_value_t."""
    leaf = {"Y": tens(P["Y"], True), "s2": tens(P["s2"], True), "S": tens(P["S"], True), "U": tens(P["U"], True), "z": tens(P["z"], True),
            "gps": [(tparams(k), tens(mu, True)) for k, mu in P["gps"]]}
    val = model_value_t(P, latent_fn, with_reg, leaf)
    val.backward()
    gps = []
    for tp, mu in leaf["gps"]:
        e = {n: (np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy()) for n, v in leaves(tp)}
        e["mean"] = 0.0 if mu.grad is None else float(mu.grad)
        gps.append(e)
    return {"value": float(val.detach()), "y": leaf["Y"].grad.numpy().reshape(-1), "sigma2": float(leaf["s2"].grad), "S": leaf["S"].grad.numpy(),
            "U": leaf["U"].grad.numpy(), "z": leaf["z"].grad.numpy(), "gps": gps}


def model_entries(g):
    """The arrays of a model gradient, flat: {name: array}."""
    out = {n: g[n] for n in ("y", "sigma2", "S", "U", "z")}
    for l, e in enumerate(g["gps"]):
        out.update({f"gps.{l}.{n}": v for n, v in e.items()})
    return out


def library_entries(g):
    """The same names from the dict elbo_and_gradient returns (a sum's terms flattened as terms.<c>.<name>)."""
    out = {n: (g[n].cpu().numpy() if L._is_torch(g[n]) else g[n]) for n in ("y", "sigma2", "S", "U", "z")}
    for l, e in enumerate(g["gps"]):
        for n, v in e.items():
            if n == "terms":
                for c, t in enumerate(v):
                    out.update({f"gps.{l}.terms.{c}.{a}": b for a, b in t.items()})
            else:
                out[f"gps.{l}.{n}"] = v
    return out


_MCACHE = {}


def model_reference(n, M, l, with_reg):
    """Computed once per session: (P, dense gradient, delta per entry against the low-rank autograd)."""
    key = (n, M, l, with_reg)
    if key not in _MCACHE:
        P = model_problem(n, M, l)
        dn, lr = model_gradient(P, elbo_dense_t, with_reg), model_gradient(P, elbo_lowrank_t, with_reg)
        ed, el = model_entries(dn), model_entries(lr)
        _MCACHE[key] = (P, dn, {a: relmax(el[a], ed[a]) for a in ed if np.abs(np.atleast_1d(ed[a])).max() > 0})
    return _MCACHE[key]


# ---------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    lib = lmm_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert proto, s
        params = [a.strip() for a in proto.group(1).split(",")]
        types = L.SPARSE_ARGTYPES[s]
        assert len(params) == len(types), (s, len(params), len(types))
        assert getattr(lib, s).argtypes == types
        for a, t in zip(params, types):
            want = L._P if ("*" in a or "[" in a) else (L._D if a.startswith("double") else L._I)
            assert t is want, (s, a)
    proto = re.search(r"int\s+lmm_oilmm_elbo_grad\s*\(([^)]*)\)", src).group(1)
    order = [re.sub(r".*[\s*]", "", a.strip()) for a in proto.split(",")]
    assert order == ["x", "d", "n", "y", "p", "U", "S", "m", "sigma2", "gps", "latent_begin", "latent_end", "z", "nz", "jitter",
                     "with_regulariser", "out_elbo", "grad_y", "grad_sigma2", "grad_S", "grad_U", "grad_gps", "grad_z"]
    assert "elbo_and_gradient" in lmm_amd.__all__ and not hasattr(lmm_amd, "dtc_and_gradient")


def _no_library():
    raise AssertionError("the library was reached")


def test_refusals_come_before_any_library_call():
    fs = lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.SEKernel())])
    x = lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 2)
    H = lmm_amd.Orthogonal(np.array([[1.0], [0.0]]), np.array([1.0]))
    y = np.zeros(8)
    vfe = lmm_amd.VFE(np.arange(3.0))
    dense = lmm_amd.ILMM(fs, np.array([[1.0], [0.5]]))(x, 0.1)
    mogp = fs(lmm_amd.MOInputIsotopicByOutputs(np.arange(4.0), 1), 0.1)
    oilmm = lmm_amd.ILMM(fs, H)(x, 0.1)
    sharded = lmm_amd.ILMM(fs, H, shard=(0, 0))(x, 0.1)
    M = lmm_amd.model
    post = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._PostHandle(None, 0, 1)), H)(x, 0.1)
    sparse = lmm_amd.ILMM(lmm_amd.IndependentMOGP(fs.fs, M._SparsePostHandle(None, 0, 1)), H)(x, 0.1)
    ynan = y.copy()
    ynan[3] = np.nan
    saved = L.ensure_init
    L.ensure_init = _no_library
    try:
        for fx, yy, what in ((dense, y, "dense-H"), (mogp, y[:4], "IndependentMOGP"), (post, y, "posterior model"),
                             (sparse, y, "posterior model"), (oilmm, np.zeros((8, 2)), "matrix Y"), (oilmm, ynan, "NaN"),
                             (sharded, y, "sharded")):
            with pytest.raises(NotImplementedError, match=what):
                lmm_amd.elbo_and_gradient(vfe, fx, yy)
        with pytest.raises(ValueError, match="d = 2"):
            lmm_amd.elbo_and_gradient(lmm_amd.VFE(np.zeros((2, 7))), oilmm, y)
        with pytest.raises(TypeError, match="VFE"):
            lmm_amd.elbo_and_gradient(np.arange(3.0), oilmm, y)
    finally:
        L.ensure_init = saved


def test_two_point_case_fixes_the_factor_of_kuubar():
    """n = 1, M = 2: d elbo / d z_0 of the backward algebra, whose K_uu share is 2 sum_{j != i} KuuBar_ij dk(z_i, z_j) / dz_i, against
    autograd of the dense formula and against a central difference of the dense value."""
    k, x, z, r = ("matern52", 1.3, 0.5), np.array([[0.4]]), np.array([[0.0, 0.7]]), np.array([0.8])
    dn, bw = autograd_latent(elbo_dense_t, k, x, z, W, r, EPS), backward_latent(k, x, z, W, r, EPS)
    assert relmax(bw["z"], dn["z"]) <= 1e-12 and relmax(bw["theta"]["lengthscale"], dn["theta"]["lengthscale"]) <= 1e-12
    assert relmax(bw["theta"]["variance"], dn["theta"]["variance"]) <= 1e-12
    PhiBar, KuuBar, beta, Kuf, kd, _ = backward_state(k, x, z, W, r, EPS)
    G = (2.0 * PhiBar @ Kuf + np.outer(beta, r)) / W
    _, gz_uf = contract(k, x, z, G)
    off = KuuBar - np.diag(np.diag(KuuBar))                        # contract differentiates both triangles: sum_ij = 2 sum_{j != i} per z_i
    _, gz_uu = contract(k, z, z, np.zeros((2, 2)), off, 0.0)
    assert relmax(gz_uf + gz_uu, dn["z"]) <= 1e-12
    assert abs(gz_uu[0, 0]) > 1e-3 * abs(dn["z"][0, 0])              # the K_uu share matters: half of it would miss
    assert relmax(gz_uf + 0.5 * gz_uu, dn["z"]) > 1e-4
    h = 1e-6
    with torch.no_grad():
        f = lambda zz: float(elbo_dense_t(k, tparams(k), tens(x), tens(zz), tens(W), tens(r), EPS))
        fd = (f(z + np.array([[h, 0.0]])) - f(z - np.array([[h, 0.0]]))) / (2.0 * h)
    assert abs(fd - dn["z"][0, 0]) <= 1e-7 * abs(dn["z"][0, 0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_three_restatements_agree(case):
    k, x, z, r, dn, lr, bw, delta, cond = case_reference(case)
    print(f"{case}: cond {cond:.1e}  delta " + "  ".join(f"{a} {v:.1e}" for a, v in delta.items()))
    assert abs(lr["value"] - dn["value"]) <= 1e-9 * abs(dn["value"])
    assert cond <= 1e4
    for a, v in delta.items():
        assert v <= 1e-9, (case, a, v)


@pytest.mark.parametrize("with_reg", [True, False])
@pytest.mark.parametrize("n,M,l", MODEL_SHAPES)
def test_model_restatements_agree(n, M, l, with_reg):
    P, dn, delta = model_reference(n, M, l, with_reg)
    print(f"model ({n}, {M}) reg={with_reg}: delta " + "  ".join(f"{a} {v:.1e}" for a, v in delta.items()))
    for a, v in delta.items():
        assert v <= 1e-9, (a, v)
    for k, _ in P["gps"]:
        tp = tparams(k)
        with torch.no_grad():
            Kj = kmat_t(k, tp, cols_t(tens(P["z"])), cols_t(tens(P["z"]))).numpy() + EPS * np.eye(M)
        assert np.linalg.cond(Kj) <= 1e4


if __name__ == "__main__":
    for case in CASES:
        _, _, _, _, _, _, _, delta, cond = case_reference(case)
        print(f"{str(case):44s} cond {cond:.1e}  delta {max(delta.values()):.1e}  (" + " ".join(f"{a} {v:.0e}" for a, v in delta.items()) + ")")
    for n, M, l in MODEL_SHAPES:
        _, _, delta = model_reference(n, M, l, True)
        print(f"model ({n}, {M}, l = {l})  delta {max(delta.values()):.1e}")
