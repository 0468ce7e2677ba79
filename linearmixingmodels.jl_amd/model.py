"""Host-side mirror of the LinearMixingModels.jl interface for the ILMM/OILMM inference hot path.

Julia is not available in the build image, so this module plays the role of the
Julia shim for tests and benchmarks: the same type names (`ILMM`, `IndependentMOGP`, `independent_mogp`,
`Orthogonal`, `get_latent_gp`; reference src/LinearMixingModels.jl:21-24) and the AbstractGPs verbs the
reference adds methods to (`logpdf`, `posterior`, `rand`, `marginals`, `mean_and_var`, `mean`, `var`),
each body being ONE call into liblmm_hip.so -- exactly what the `ccall` shim in
`linearmixingmodels.jl_amd/julia/LinearMixingModelsHIP.jl` does.  No arithmetic happens here.

Arrays may be NumPy (host) or float64 CUDA/HIP torch tensors (device pointers are passed straight
through the C ABI).
"""
from __future__ import annotations

import ctypes as C
import weakref
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


# ---- kernels / GPs (KernelFunctions.jl + AbstractGPs.jl names) ------------------------------------
def _ls_key(ls):
    """Hashable, comparable form of a lengthscale: the float, or the tuple of a per-dimension (ARD) vector."""
    return ls if isinstance(ls, float) else tuple(ls.tolist())


class _Kernel:
    """variance * kernel(|x - x'| / lengthscale).  A length-d vector lengthscale gives per-dimension lengthscales: KernelFunctions'
    with_lengthscale(k, l::AbstractVector) = k o ARDTransform(1 ./ l)."""
    kind = ""

    def __init__(self, variance: float = 1.0, lengthscale=1.0):
        self.variance = float(variance)
        if np.ndim(lengthscale) == 0:
            self.lengthscale = float(lengthscale)
        else:
            ls = np.array(lengthscale, dtype=np.float64).reshape(-1)
            if ls.size == 0:
                raise ValueError("lengthscale vector is empty")
            self.lengthscale = ls

    def __eq__(self, o):
        return type(self) is type(o) and (self.variance, _ls_key(self.lengthscale)) == (o.variance, _ls_key(o.lengthscale))

    def __repr__(self):
        ls = self.lengthscale if isinstance(self.lengthscale, float) else list(self.lengthscale.tolist())
        return f"{type(self).__name__}(variance={self.variance}, lengthscale={ls})"

    def __add__(self, o):
        """k1 + k2: KernelFunctions' KernelSum (flattened: see KernelSum)."""
        if not isinstance(o, _Kernel):
            return NotImplemented
        return KernelSum(self, o)

    def __mul__(self, o):
        """k1 * k2: only SEKernel * PeriodicKernel (either order), the locally periodic kernel; see LocallyPeriodicKernel."""
        if not isinstance(o, _Kernel):
            return NotImplemented
        se, per = (self, o) if type(self) is SEKernel else (o, self)
        if type(se) is not SEKernel or type(per) is not PeriodicKernel:
            raise NotImplementedError("the only product kernel served is SEKernel * PeriodicKernel (LocallyPeriodicKernel); "
                                      f"got {type(self).__name__} * {type(o).__name__}")
        if not isinstance(se.lengthscale, float):
            raise ValueError("SEKernel * PeriodicKernel needs a scalar SE lengthscale (a per-dimension decay is not supported)")
        return LocallyPeriodicKernel(se.variance * per.variance, per.lengthscale, per.r, se.lengthscale)

    def desc(self) -> dict:
        """Descriptor of this kernel (a latent's, or a term's of a sum kernel)."""
        d = {"kind": self.kind, "variance": self.variance, "lengthscale": self.lengthscale}
        if hasattr(self, "alpha"):
            d["alpha"] = self.alpha
        if hasattr(self, "r"):
            d["r"] = self.r
        if hasattr(self, "decay"):
            d["decay"] = self.decay
        return d

    def key(self) -> tuple:
        """Hashable form of the kernel's values (the latent-array cache key)."""
        if hasattr(self, "decay"):
            return (self.kind, self.variance, _ls_key(self.lengthscale), None, self.r, self.decay)
        if hasattr(self, "r"):
            return (self.kind, self.variance, _ls_key(self.lengthscale), None, self.r)
        return (self.kind, self.variance, _ls_key(self.lengthscale), getattr(self, "alpha", None))


class SEKernel(_Kernel):
    kind = "se"


class Matern32Kernel(_Kernel):
    kind = "matern32"


class Matern52Kernel(_Kernel):
    kind = "matern52"


class Matern12Kernel(_Kernel):
    """variance * exp(-r): KernelFunctions' Matern12Kernel, an alias of ExponentialKernel."""
    kind = "matern12"


ExponentialKernel = Matern12Kernel


class RationalQuadraticKernel(_Kernel):
    """variance * (1 + r^2 / (2 alpha))^(-alpha): KernelFunctions' RationalQuadraticKernel(; alpha=2.0)."""
    kind = "rq"

    def __init__(self, variance: float = 1.0, lengthscale=1.0, alpha: float = 2.0):
        super().__init__(variance, lengthscale)
        self.alpha = float(alpha)
        if not (self.alpha > 0.0 and np.isfinite(self.alpha)):
            raise ValueError("alpha must be finite and > 0")

    def __eq__(self, o):
        return super().__eq__(o) and self.alpha == o.alpha

    def __repr__(self):
        return super().__repr__()[:-1] + f", alpha={self.alpha})"


class PeriodicKernel(_Kernel):
    """variance * exp(-sum_k sin^2(pi (x_k - x'_k) / period_k) / (2 r^2)): KernelFunctions' PeriodicKernel(; r) o ScaleTransform(1 /
    period) (a vector: ARDTransform(1 ./ period)).  `lengthscale` is the period, a float or a length-d vector (`.period` is an alias);
    `r` is one scalar for all dimensions (a vector with equal entries is accepted, unequal entries are refused)."""
    kind = "periodic"

    def __init__(self, variance: float = 1.0, lengthscale=1.0, r=1.0):
        super().__init__(variance, lengthscale)
        if np.ndim(r) != 0:
            rv = np.asarray(r, dtype=np.float64).reshape(-1)
            if rv.size == 0 or not np.all(rv == rv[0]):
                raise ValueError("r must be one scalar for all dimensions (a vector with equal entries is accepted)")
            r = rv[0]
        self.r = float(r)
        if not (self.r > 0.0 and np.isfinite(self.r)):
            raise ValueError("r must be finite and > 0")

    @property
    def period(self):
        return self.lengthscale

    @period.setter
    def period(self, v):
        self.lengthscale = float(v) if np.ndim(v) == 0 else np.array(v, dtype=np.float64).reshape(-1)

    def __eq__(self, o):
        return super().__eq__(o) and self.r == o.r

    def __repr__(self):
        return super().__repr__()[:-1] + f", r={self.r})"


class LocallyPeriodicKernel(PeriodicKernel):
    """variance * exp(-|x - x'|^2 / (2 decay^2) - sum_k sin^2(pi (x_k - x'_k) / period_k) / (2 r^2)): the locally periodic (quasi-periodic)
    kernel, KernelFunctions' (SEKernel() o ScaleTransform(1 / decay)) * (PeriodicKernel(; r) o ScaleTransform(1 / period)); also what
    SEKernel(v1, decay) * PeriodicKernel(v2, period, r) returns (variance v1 v2).  `lengthscale` is the period (float or length-d vector,
    alias `.period`) and `r` as for PeriodicKernel; `decay` is the SE lengthscale, one positive finite scalar.  It is a base kernel (the
    one product the library serves), so it may be a term of a KernelSum, whose outer lengthscale then scales the period and the decay."""
    kind = "locally_periodic"

    def __init__(self, variance: float = 1.0, lengthscale=1.0, r=1.0, decay: float = 1.0):
        super().__init__(variance, lengthscale, r)
        if np.ndim(decay) != 0:
            raise ValueError("decay must be one scalar (a per-dimension decay is not supported)")
        self.decay = float(decay)
        if not (self.decay > 0.0 and np.isfinite(self.decay)):
            raise ValueError("decay must be finite and > 0")

    def __eq__(self, o):
        return super().__eq__(o) and self.decay == o.decay

    def __repr__(self):
        return super().__repr__()[:-1] + f", decay={self.decay})"


class SHOKernel(_Kernel):
    """variance * exp(-a tau) (cos(eta tau) + (a / eta) sin(eta tau)), tau = |x - x'|, w0 = 2 pi / period, a = w0 / (2 quality),
    eta = w0 sqrt(1 - 1 / (4 quality^2)): the stochastically driven damped harmonic oscillator (the celerite "SHO" kernel of
    Foreman-Mackey et al. 2017), a quasi-periodic kernel whose spectrum peaks near 1 / period with a width set by `quality`, and whose
    paths are once differentiable.  `lengthscale` is the undamped period, one scalar (`.period` is an alias, the PeriodicKernel
    convention): the kernel is defined for one-dimensional inputs only, the radial form is not positive definite for d > 1.  `quality`
    is one finite scalar > 1/2 (underdamped).  quality -> 1/2 is Matern32Kernel with sqrt(3) / lengthscale = 2 pi / period; quality <=
    1/2 (critically damped and overdamped) is not served.  It is exactly a two-dimensional linear SDE: the state-space functions
    (statespace_logpdf, statespace_mean_and_var, statespace_logpdf_and_gradient, statespace_rand) serve it alone or mixed with Matern
    latents, in O(n).  The dense verbs serve it too (logpdf, posterior and what is asked of it, logpdf_and_gradient with "quality", NaN
    data; OILMM, IndependentMOGP and dense-H); inputs=True, mean_and_var_vjp, the VFE functions and sum kernels refuse it.  (The C ABI's state-space
    entry points take a two-term sum with an SHO term, through lmm_kernel_sum_create_statespace; the state-space functions here serve
    Matern-only sums.)"""
    kind = "sho"

    def __init__(self, variance: float = 1.0, lengthscale=1.0, quality: float = 1.0):
        if np.ndim(lengthscale) != 0:
            raise ValueError("an SHOKernel's period is one scalar (the kernel is defined for one-dimensional inputs)")
        super().__init__(variance, lengthscale)
        self.quality = L.sho_quality(quality)

    @property
    def period(self):
        return self.lengthscale

    @period.setter
    def period(self, v):
        if np.ndim(v) != 0:
            raise ValueError("an SHOKernel's period is one scalar")
        self.lengthscale = float(v)

    def __eq__(self, o):
        return super().__eq__(o) and self.quality == o.quality

    def __repr__(self):
        return super().__repr__()[:-1] + f", quality={self.quality})"

    def desc(self) -> dict:
        d = super().desc()
        d["quality"] = self.quality
        return d

    def key(self) -> tuple:
        return (self.kind, self.variance, self.lengthscale, None, None, None, self.quality)


class KernelSum(_Kernel):
    """variance * sum_c kernels[c](|x - x'| / lengthscale): KernelFunctions' KernelSum (k1 + k2 + ...), with `variance` and the scalar
    `lengthscale` the ScaledKernel and ScaleTransform around the whole sum (1.0: none).  Each term is a base kernel with its own
    variance, lengthscale (a float, or a length-d vector), and RQ alpha.  A term that is itself a sum with unit variance and
    lengthscale is flattened into its terms; any other nested sum is rejected.  At most 4 terms."""
    kind = "sum"

    def __init__(self, *kernels, variance: float = 1.0, lengthscale: float = 1.0):
        if np.ndim(lengthscale) != 0:
            raise ValueError("per-dimension lengthscales around a whole sum kernel are not supported")
        super().__init__(variance, lengthscale)
        terms = []
        for k in kernels:
            if isinstance(k, KernelSum):
                if k.variance != 1.0 or k.lengthscale != 1.0:
                    raise ValueError("a scaled sum kernel cannot be a term of another sum")
                terms.extend(k.kernels)
            elif isinstance(k, _Kernel):
                terms.append(k)
            else:
                raise TypeError(f"not a kernel: {k!r}")
        if not 1 <= len(terms) <= L.SUM_MAX_TERMS:
            raise ValueError(f"a sum kernel has 1..{L.SUM_MAX_TERMS} terms, got {len(terms)}")
        self.kernels = tuple(terms)

    def __eq__(self, o):
        return super().__eq__(o) and self.kernels == o.kernels

    def __repr__(self):
        return f"KernelSum({', '.join(map(repr, self.kernels))}, variance={self.variance}, lengthscale={self.lengthscale})"

    def desc(self) -> dict:
        return {"kind": "sum", "variance": self.variance, "lengthscale": self.lengthscale,
                "terms": [k.desc() for k in self.kernels]}

    def key(self) -> tuple:
        return ("sum", self.variance, self.lengthscale, tuple(k.key() for k in self.kernels))


class GP:
    """GP(kernel) or GP(mean_const, kernel)."""

    def __init__(self, *args):
        if len(args) == 1:
            self.mean, self.kernel = 0.0, args[0]
        else:
            self.mean, self.kernel = float(args[0]), args[1]

    def desc(self) -> dict:
        d = self.kernel.desc()
        d["mean"] = self.mean
        return d

    def __eq__(self, o):
        return isinstance(o, GP) and self.mean == o.mean and self.kernel == o.kernel


class IndependentMOGP:
    """reference src/independent_mogp.jl:10-12."""

    def __init__(self, fs: Sequence[GP], _post: Optional["_PostHandle"] = None):
        self.fs = list(fs)
        self._post = _post

    def __call__(self, x: "MOInputIsotopicByOutputs", sigma2=1e-18) -> "FiniteGP":
        """f(x, sigma2) or f(x, diag) with the diagonal of a general Diagonal noise (length n*p, ordered like x)."""
        # get_latent_gp(posterior(ilmm_dense(x, s2), y)): the latents of a dense-H posterior are COUPLED (one (mn) x (mn) state,
        # reference src/ilmm.jl:196-197); the verbs below serve them through the handle's latent view (H = I_m)
        if np.isscalar(sigma2) or getattr(sigma2, "ndim", 1) == 0:
            return FiniteGP(self, x, float(sigma2))
        return FiniteGP(self, x, sigma2)

    def __eq__(self, o):
        return isinstance(o, IndependentMOGP) and self.fs == o.fs and self._post is o._post


def independent_mogp(fs: Sequence[GP]) -> IndependentMOGP:
    """reference src/independent_mogp.jl:31."""
    return IndependentMOGP(fs)


class Orthogonal:
    """reference src/orthogonal_matrix.jl:11-34: H = U * sqrt(S); validates U'U ~ I."""

    def __init__(self, U, S, validate_fields: bool = True):
        # U is held column-major (what Julia holds and the C ABI takes): a row-major argument is copied once, here, and the ABI then
        # reads H.U's own buffer on every call (in-place edits of H.U are seen; edits of a row-major original are not)
        self.U = np.asfortranarray(np.asarray(U, dtype=np.float64))
        self.S = np.ascontiguousarray(np.asarray(S, dtype=np.float64).reshape(-1))      # the Diagonal's diag
        self._args = None                                         # (U object, S object, column-major image of U): see abi_args()
        if self.U.ndim != 2 or self.U.shape[1] != self.S.shape[0]:
            raise ValueError("U must be p x m and S of length m")
        if validate_fields:
            p, m = self.U.shape
            L.check(L.load().lmm_orthogonal_validate(L.Arr(L.colmajor(self.U)).ptr, C.c_int(p), C.c_int(m)))

    @property
    def shape(self) -> Tuple[int, int]:
        return self.U.shape

    def abi_args(self):
        """(U column-major, S) as the C ABI takes them.  A U that is already column-major (Fortran order, what Julia holds) goes over
        as it is, with no copy and therefore always current; a row-major U is re-imaged per call."""
        U, S = self.U, self.S
        a = self._args
        if a is not None and a[0] is U and a[1] is S:
            return a[2], a[3]
        Uc = L.colmajor(U)
        Ua, Sa = L.Arr(Uc), L.Arr(S)
        if Uc.base is U or Uc is U:                  # a view of the live buffer: safe to keep (in-place edits of U stay visible)
            self._args = (U, S, Ua, Sa)
        return Ua, Sa

    def collect(self) -> np.ndarray:
        """reference src/orthogonal_matrix.jl:27-30 (materialised H)."""
        return self.U * np.sqrt(self.S)[None, :]

    def __array__(self, dtype=None, copy=None):
        return self.collect()


class MOInputIsotopicByOutputs:
    """KernelFunctions.MOInputIsotopicByOutputs(x, out_dim): x is (n,) or ColVecs-style (d, n)."""

    def __init__(self, x, out_dim: int):
        self.x, self.out_dim = x, int(out_dim)

    @property
    def dim(self) -> int:
        return 1 if len(self.x.shape) == 1 else int(self.x.shape[0])

    @property
    def n(self) -> int:
        return int(self.x.shape[-1])

    def carr(self) -> L.Arr:
        x = self.x
        if len(x.shape) == 2:          # (d, n) -> d x n column-major == (n, d) C-order
            x = x.T.contiguous() if L._is_torch(x) else np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)
        return L.Arr(x)

    def __len__(self):
        return self.n * self.out_dim


class MOInputIsotopicByFeatures:
    """KernelFunctions.MOInputIsotopicByFeatures(x, out_dim): index k -> (x[k // p], k % p) (all outputs of x_1, then x_2, ...).
    The reference supports it for IndependentMOGP only (src/independent_mogp.jl:128-229; ILMM `unpack` rejects it,
    src/ilmm.jl:45)."""

    def __init__(self, x, out_dim: int):
        self.x, self.out_dim = x, int(out_dim)

    @property
    def n(self) -> int:
        return int(self.x.shape[-1])

    def by_outputs(self) -> MOInputIsotopicByOutputs:
        return MOInputIsotopicByOutputs(self.x, self.out_dim)

    def __len__(self):
        return self.n * self.out_dim


def indices_which_reorder_features_to_outputs(x) -> np.ndarray:
    """reference src/independent_mogp.jl:141-145 (1-based, as in test/independent_mogp.jl:86-98): applied to a vector
    ordered by features it orders it by outputs."""
    return np.arange(1, len(x) + 1).reshape(x.n, x.out_dim).T.reshape(-1)


def indices_which_reorder_outputs_to_features(x) -> np.ndarray:
    """reference src/independent_mogp.jl:135-139."""
    return np.arange(1, len(x) + 1).reshape(x.out_dim, x.n).T.reshape(-1)


def _reorder(v, n: int, p: int, to_outputs: bool):
    """lmm_reorder: by-features <-> by-outputs (index permutation done by the library)."""
    L.ensure_init()
    a = L.Arr(v)
    out = _alloc_like(v, n * p)
    L.check(L.load().lmm_reorder(a.ptr, n, p, int(to_outputs), L.Arr(out, True).ptr))
    return out


class _PostHandle:
    """Owns an lmm_post_t* (device-resident posterior state); freed with the Python object, as the Julia
    shim does with a finalizer."""

    def __init__(self, ptr: C.c_void_p, l0: int, l1: int, dense: bool = False, train=None, latent: bool = False, parent=None, mix=None):
        self.ptr, self.l0, self.l1, self.dense = ptr, l0, l1, dense      # dense: coupled (mn) x (mn) state of a dense-H ILMM
        self.mix = mix                # dense only: the H (p x m) the conditioning batches were observed through (gradient of the latent view)
        # the conditioning batches [(x, sigma2, y), ...] the posterior was built from (references, no copies): the gradient of the
        # predictive logpdf is a total derivative through the posterior and needs them (one entry per posterior(...) call)
        self.train = train if (train is None or isinstance(train, list)) else [train]
        self.latent = latent          # dense only: this handle's H is I_m (it IS the latent PosteriorGP{IndependentMOGP})
        # A latent view does NOT reference its parent: the C side keeps the shared device state alive until the last of the two handles
        # is destroyed (either order), and a back-reference would make parent <-> view a cycle of objects with __del__, whose device
        # memory only the cyclic collector would free.
        self._parent = weakref.ref(parent) if parent is not None else None
        self._view = None

    def latent_view(self) -> "_PostHandle":
        """The latent PosteriorGP{IndependentMOGP} of a dense-H posterior (reference src/ilmm.jl:39 on :196-197) as a handle of
        its own: lmm_ilmm_post_latent_view (shares the factor, H = I_m)."""
        if self.latent:
            return self
        if self._view is None:
            h = C.c_void_p()
            L.check(L.load().lmm_ilmm_post_latent_view(self.ptr, C.byref(h)))
            self._view = _PostHandle(h, self.l0, self.l1, dense=True, latent=True, parent=self)
        return self._view

    def __del__(self):
        try:
            if self.ptr:
                L.load().lmm_post_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


class ILMM:
    """reference src/ilmm.jl:16-19.  `ILMM(f, H)` with H a dense p x m matrix or an `Orthogonal` (=> OILMM,
    reference src/oilmm.jl:13).  `shard=(begin, end)` restricts this process to a block of latents
    (one process per GPU); partial results are combined by `parallel.py`."""

    def __init__(self, f: IndependentMOGP, H, shard: Optional[Tuple[int, int]] = None):
        self.f, self.H = f, H if isinstance(H, Orthogonal) else np.asarray(H, dtype=np.float64)
        m = len(f.fs)
        if self.H.shape[1] != m:
            raise ValueError(f"H has {self.H.shape[1]} columns but there are {m} latent processes")
        self.shard = (0, m) if shard is None else (int(shard[0]), int(shard[1]))

    @property
    def is_oilmm(self) -> bool:
        return isinstance(self.H, Orthogonal)

    def __call__(self, x: MOInputIsotopicByOutputs, sigma2: float = 1e-18) -> "FiniteGP":
        return FiniteGP(self, x, float(sigma2))


def OILMM(f: IndependentMOGP, H: Orthogonal, **kw) -> ILMM:
    if not isinstance(H, Orthogonal):
        raise TypeError("OILMM needs an Orthogonal mixing matrix")
    return ILMM(f, H, **kw)


def get_latent_gp(f: ILMM) -> IndependentMOGP:
    """reference src/ilmm.jl:39."""
    return f.f


class Normal:
    def __init__(self, mu, sigma):
        self.mu, self.sigma = mu, sigma


class FiniteGP:
    """AbstractGPs.FiniteGP(f, x, Diagonal(Fill(sigma2, n*p))).  `sigma2` may also be a length n*p vector -- the diagonal of a
    general `Diagonal` noise, ordered like x -- which the reference accepts for IndependentMOGP logpdf only
    (src/independent_mogp.jl:149-159, 222-229; ILMM `noise_var` requires a Fill, src/ilmm.jl:41)."""

    def __init__(self, f, x: MOInputIsotopicByOutputs, sigma2):
        self.f, self.x, self.sigma2 = f, x, sigma2

    @property
    def heteroscedastic(self) -> bool:
        return not np.isscalar(self.sigma2) and getattr(self.sigma2, "ndim", 1) > 0

    def __len__(self):
        return len(self.x)


# ---- helpers ----------------------------------------------------------------------------------------
def noise_var(sigma2):
    """reference src/ilmm.jl:41."""
    return sigma2


def reshape_y(y, n: int):
    """reference src/ilmm.jl:43: reshape(y, N, :)'."""
    return np.asarray(y).reshape(-1, n)


def unpack(fx: FiniteGP):
    """reference src/ilmm.jl:45-54."""
    f = fx.f
    if fx.x.out_dim != f.H.shape[0]:
        raise RuntimeError("out dim of x != out dim of f.")
    return f.f, f.H, fx.sigma2, fx.x.x


def _merged_train(train, p: int):
    """The conditioning batches of a (sequentially conditioned) posterior as ONE set of points: posterior(posterior(f(x1, s1), y1)(x2, s2),
    y2) is the posterior given ([x1 x2], [y1; y2]) under per-batch noise (exact conditioning), which is what the *_post_logpdf_grad_seq
    entry points serve (one noise block per batch + one for the test points).  Returns (x_all, [s2 per batch], y_all, sizes); y is
    by-outputs, so the batches interleave per output."""
    if train is None:
        raise NotImplementedError("this posterior does not carry its training data (built outside posterior(fx, y))")
    if any(np.ndim(t[1]) > 0 for t in train):
        raise NotImplementedError("gradient of the predictive logpdf after conditioning with a per-point (Diagonal) noise is not built "
                                  "(scalar noise variances, one per conditioning batch, are)")
    if len(train) == 1:
        x0, s20, y0 = train[0]
        return x0, [float(s20)], y0, [x0.n]
    if len(train) > 7:
        raise NotImplementedError("gradient of the predictive logpdf after more than 7 conditioning batches is not built")
    xs = [np.asarray(t[0].x.cpu() if L._is_torch(t[0].x) else t[0].x, dtype=np.float64) for t in train]
    ys = [np.asarray(t[2].cpu() if L._is_torch(t[2]) else t[2], dtype=np.float64).reshape(p, -1) for t in train]
    x_all = np.concatenate(xs, axis=-1)
    y_all = np.concatenate(ys, axis=1).reshape(-1)
    return MOInputIsotopicByOutputs(x_all, p), [float(t[1]) for t in train], y_all, [t[0].n for t in train]


def _batch_args(s2b, sizes):
    """(batch_n, batch_sigma2, grad_batch_sigma2) ctypes arrays of a *_post_logpdf_grad_seq call."""
    k = len(sizes)
    return (C.c_int * k)(*sizes), (C.c_double * k)(*s2b), (C.c_double * k)()


def _train_noise_grad(gb, s2b):
    """d/d(training noise): ONE number when the batches share their variance (the derivative w.r.t. that shared value), else one per
    conditioning batch."""
    g = [float(v) for v in gb]
    return sum(g) if len(set(s2b)) == 1 else g


def _split_train_grad(gy, sizes, p: int):
    """d/dy of the merged batch back into one by-outputs vector per conditioning batch."""
    if len(sizes) == 1:
        return gy
    g = np.asarray(gy.cpu() if L._is_torch(gy) else gy).reshape(p, -1)
    out, o = [], 0
    for nb in sizes:
        out.append(np.ascontiguousarray(g[:, o:o + nb]).reshape(-1)); o += nb
    return out


def _gps_arg(mogp):
    """(descs, lmm_gp_t array) of an IndependentMOGP's latents.  The ctypes array is rebuilt only when a hyperparameter changed (the key
    is the tuple of current values: building it costs a third of filling the array, which at m = 20 is 25 us of a 380-us call)."""
    key = tuple((g.kernel.key(), g.mean) for g in mogp.fs)
    hit = getattr(mogp, "_gps_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    descs = [g.desc() for g in mogp.fs]
    arr = L.gps_array(descs)
    mogp._gps_cache = (key, descs, arr)
    return descs, arr


def _H_args(H):
    """(U or dense-H pointer, S pointer or None, p, m) for the C ABI."""
    if isinstance(H, Orthogonal):
        Ua, Sa = H.abi_args()
        return Ua, Sa, H.U.shape[0], H.U.shape[1]
    return L.Arr(L.colmajor(H)), None, H.shape[0], H.shape[1]


def _alloc_like(ref, count: int):
    """Output buffer on the same side (host / device) as `ref`."""
    if L._is_torch(ref) and ref.is_cuda:
        import torch
        return torch.empty(count, dtype=torch.float64, device=ref.device)
    return np.empty(count, dtype=np.float64)


# ---- missing observations (NaN in y) ---------------------------------------------------------------------
# The reference's notebook: "Heterotopic and missing data ... are not supported yet ... using the missing data techniques identified in
# the paper".  logpdf, posterior and logpdf_and_gradient of a PRIOR OILMM take a by-outputs vector y whose missing entries are NaN
# (include/lmm_hip.h, "missing observations"); nothing else does.
def _has_nan(y) -> bool:
    if L._is_torch(y):
        import torch
        return bool(torch.isnan(y).any())
    return bool(np.isnan(y).any())


def _drop_unobserved(xv, y, p: int):
    """Removes the points that have no observed output (a point without observations carries no information, and the C ABI refuses
    it): (x, y, keep) with x (n,) or (d, n), y the by-outputs vector (n * p) and keep the boolean mask of the points kept (on the side
    of y).  Arrays are returned unchanged when every point is kept."""
    tor = L._is_torch(y)
    Y = y.reshape(p, -1)
    if tor:
        import torch
        keep = ~torch.isnan(Y).all(dim=0)
    else:
        keep = ~np.isnan(Y).all(axis=0)
    if bool(keep.all()):
        return xv, y, keep
    kx = keep
    if L._is_torch(xv) and not tor:
        import torch
        kx = torch.as_tensor(keep, device=xv.device)
    elif tor and not L._is_torch(xv):
        kx = keep.cpu().numpy()
    y2 = Y[:, keep].reshape(-1)
    return xv[..., kx], (y2.contiguous() if tor else np.ascontiguousarray(y2)), keep


def _missing_args(fx: "FiniteGP", y, what: str):
    """(x without the unobserved points, y without them, keep) for the *_missing entry points, or NotImplementedError when `fx` is not a
    prior OILMM over by-outputs inputs with a vector y."""
    f, x = fx.f, fx.x
    if not hasattr(y, "shape"):
        y = np.asarray(y, dtype=np.float64)
    if (not isinstance(f, ILMM) or not f.is_oilmm or f.f._post is not None or not isinstance(x, MOInputIsotopicByOutputs)
            or fx.heteroscedastic or (hasattr(y, "shape") and len(y.shape) != 1)):
        raise NotImplementedError(
            f"{what}: missing observations (NaN in y) are served for a vector y on a prior OILMM (logpdf, posterior, "
            "logpdf_and_gradient) over MOInputIsotopicByOutputs only; sequential conditioning (lmm_post_condition), the predictive "
            "logpdf, matrix Y, by-features inputs, per-point noise, dense-H ILMM, IndependentMOGP and rand do not take missing data")
    unpack(fx)
    if y.shape[0] != x.n * x.out_dim:
        raise ValueError("length(y) != n * out_dim")
    xv, y2, keep = _drop_unobserved(x.x, y, x.out_dim)
    return MOInputIsotopicByOutputs(xv, x.out_dim), y2, keep


def _logpdf_missing(fx: "FiniteGP", y, with_regulariser: bool) -> float:
    lib = L.load()
    x, y2, _ = _missing_args(fx, y, "logpdf")
    f = fx.f
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    out = C.c_double()
    L.check(lib.lmm_oilmm_logpdf_missing(x.carr().ptr, x.dim, x.n, L.Arr(y2).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(fx.sigma2), gps,
                                         f.shard[0], f.shard[1], int(with_regulariser), C.byref(out)))
    return out.value


def _posterior_missing(fx: "FiniteGP", y):
    lib = L.load()
    x, y2, _ = _missing_args(fx, y, "posterior")
    f = fx.f
    gps = L.gps_array([g.desc() for g in f.f.fs])
    Ua, Sa, p, m = _H_args(f.H)
    handle = C.c_void_p()
    L.check(lib.lmm_oilmm_posterior_create_missing(x.carr().ptr, x.dim, x.n, L.Arr(y2).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(fx.sigma2),
                                                   gps, f.shard[0], f.shard[1], C.byref(handle)))
    # train=None: the gradient of the predictive logpdf through NaN-carrying training data is not built
    return ILMM(IndependentMOGP(f.f.fs, _PostHandle(handle, f.shard[0], f.shard[1])), f.H, shard=f.shard)


def _gradient_missing(fx: "FiniteGP", y, with_regulariser: bool, inputs: bool) -> dict:
    if inputs:
        raise NotImplementedError("logpdf_and_gradient: the gradient with respect to the inputs is not built for data with NaN")
    lib = L.load()
    x, y2, keep = _missing_args(fx, y, "logpdf_and_gradient")
    f = fx.f
    Ua, Sa, p, m = _H_args(f.H)
    val, gs2 = C.c_double(), C.c_double()
    gy2 = _alloc_like(y2, x.n * p)
    gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in f.f.fs])
    L.check(lib.lmm_oilmm_logpdf_grad_missing(x.carr().ptr, x.dim, x.n, L.Arr(y2).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(fx.sigma2), ga,
                                              f.shard[0], f.shard[1], int(with_regulariser), C.byref(val), L.Arr(gy2, True).ptr,
                                              C.byref(gs2), gg))
    gy = gy2
    if not bool(keep.all()):          # the dropped points' entries are missing ones: 0
        if L._is_torch(gy2):
            import torch
            gy = torch.zeros(p, fx.x.n, dtype=torch.float64, device=gy2.device)
            gy[:, keep.to(gy2.device)] = gy2.reshape(p, -1)
        else:
            gy = np.zeros((p, fx.x.n))
            gy[:, np.asarray(keep.cpu() if L._is_torch(keep) else keep)] = gy2.reshape(p, -1)
        gy = gy.reshape(-1)
    return {"value": val.value, "y": gy, "sigma2": gs2.value, "gps": _gps_grads(gg, ga, m, x.dim)}


class _NoMixingGradient(dict):
    """The gradient dict for data with NaN: "S", "U" (and "x") are not built."""

    def __missing__(self, key):
        if key in ("S", "U", "x"):
            raise NotImplementedError(f"logpdf_and_gradient: the gradient with respect to {key!r} is not built for data with NaN")
        raise KeyError(key)


# ---- inducing points (VFE) -------------------------------------------------------------------------------
# AbstractGPs' VFE(f(z)) with elbo, dtc and posterior(VFE(...), fx, y) on the independent latents of an OILMM (include/lmm_hip.h,
# "inducing points"): linear cost in n.  `posterior` keeps its two-argument form; the sparse one is approx_posterior.
class VFE:
    """VFE(z, jitter=1e-6): the inducing inputs z, shaped like the model's inputs ((M,) or (d, M)), shared by all latents, and the jitter
    added to the diagonal of K_uu (AbstractGPs' VFE(f(z, jitter)))."""

    def __init__(self, z, jitter: float = 1e-6):
        if not hasattr(z, "shape"):
            z = np.asarray(z, dtype=np.float64)
        if len(z.shape) not in (1, 2) or int(z.shape[-1]) == 0 or (len(z.shape) == 2 and int(z.shape[0]) == 0):
            raise ValueError("VFE: z must be a non-empty (M,) or (d, M) array of inducing inputs")
        jitter = float(jitter)
        if not (jitter > 0.0 and np.isfinite(jitter)):
            raise ValueError("VFE: jitter must be finite and > 0")
        self.z, self.jitter = z, jitter

    @property
    def dim(self) -> int:
        return 1 if len(self.z.shape) == 1 else int(self.z.shape[0])

    @property
    def nz(self) -> int:
        return int(self.z.shape[-1])

    def carr(self) -> L.Arr:
        return MOInputIsotopicByOutputs(self.z, 1).carr()


class _SparsePostHandle:
    """Owns an lmm_sparse_post_t* (z, L_u, L_B and c per latent, on the device)."""
    sparse = True

    def __init__(self, ptr: C.c_void_p, l0: int, l1: int):
        self.ptr, self.l0, self.l1, self.dense, self.train = ptr, l0, l1, False, None

    def __del__(self):
        try:
            if self.ptr:
                L.load().lmm_sparse_post_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def _sparse_post(fx) -> Optional[_SparsePostHandle]:
    """The inducing-point handle behind a FiniteGP, or behind a model passed as it is (cov(f::IndependentMOGP, x, y)), else None."""
    f = fx if isinstance(fx, (IndependentMOGP, ILMM)) else getattr(fx, "f", None)
    post = f._post if isinstance(f, IndependentMOGP) else (f.f._post if isinstance(f, ILMM) else None)
    return post if isinstance(post, _SparsePostHandle) else None


def _refuse_sparse(fx, what: str) -> None:
    if _sparse_post(fx) is not None:
        raise NotImplementedError(f"{what} is not served on an inducing-point posterior (approx_posterior): it answers mean_and_var, "
                                  "mean, var and marginals")


def _has_sho(k) -> bool:
    return isinstance(k, SHOKernel) or (isinstance(k, KernelSum) and any(isinstance(t, SHOKernel) for t in k.kernels))


def _sho_latent(fx):
    """(index, kernel) of the first SHO latent of a FiniteGP's (or a model's) latents, else None."""
    f = fx if isinstance(fx, (IndependentMOGP, ILMM)) else getattr(fx, "f", None)
    mogp = f if isinstance(f, IndependentMOGP) else (f.f if isinstance(f, ILMM) else None)
    for l, gp in enumerate(mogp.fs if mogp is not None else ()):
        if _has_sho(gp.kernel):
            return l, gp.kernel
    return None


def _refuse_sho(fx, what: str) -> None:
    """What is not served for SHO latents (gradients with respect to inputs, inducing-point inference) refuses them here, before any
    library call, so no route evaluates another kernel in their place."""
    hit = _sho_latent(fx)
    if hit is not None:
        raise NotImplementedError(f"{what} is not served for SHO latents (latent {hit[0]} is {hit[1]!r})")


def _refuse_sho_dims(fx, what: str, *xs) -> None:
    """An SHO latent is defined over one-dimensional inputs only: d > 1 is refused before any library call.  xs: the inputs of the
    call (default: fx.x)."""
    hit = _sho_latent(fx)
    if hit is None:
        return
    if isinstance(hit[1], KernelSum):
        raise NotImplementedError(f"{what}: an SHO term inside a KernelSum is not served (latent {hit[0]} is {hit[1]!r})")
    for x in (xs or (getattr(fx, "x", None),)):
        d = getattr(x, "dim", 1)
        if d != 1:
            raise NotImplementedError(f"{what}: an SHO latent (latent {hit[0]} is {hit[1]!r}) is served for one-dimensional inputs "
                                      f"only (d = {d})")


def _sparse_args(vfe: VFE, fx: "FiniteGP", y, what: str):
    """Checks of elbo / dtc / approx_posterior, all before any library call."""
    if not isinstance(vfe, VFE):
        raise TypeError(f"{what}: the first argument is a VFE(z, jitter)")
    _refuse_sho(fx, what)
    f, x = fx.f, fx.x
    if isinstance(f, IndependentMOGP):
        raise NotImplementedError(f"{what}: inducing-point inference is not served for an IndependentMOGP (wrap it in an OILMM)")
    if not isinstance(f, ILMM) or not f.is_oilmm:
        raise NotImplementedError(f"{what}: inducing-point inference is not served for a dense-H ILMM (OILMM only)")
    if f.f._post is not None:
        raise NotImplementedError(f"{what}: inducing-point inference is not served on a posterior model (prior OILMM only)")
    if f.shard != (0, len(f.f.fs)):
        raise NotImplementedError(f"{what}: inducing-point inference is not served with latents sharded across processes")
    if not isinstance(x, MOInputIsotopicByOutputs) or fx.heteroscedastic:
        raise NotImplementedError(f"{what}: inducing-point inference takes MOInputIsotopicByOutputs inputs and a scalar noise variance")
    if not hasattr(y, "shape"):
        y = np.asarray(y, dtype=np.float64)
    if len(y.shape) != 1:
        raise NotImplementedError(f"{what}: inducing-point inference is not served for a matrix Y (one vector y)")
    if _has_nan(y):
        raise NotImplementedError(f"{what}: inducing-point inference is not served with missing observations (NaN in y)")
    unpack(fx)
    if y.shape[0] != x.n * x.out_dim:
        raise ValueError("length(y) != n * out_dim")
    if vfe.dim != x.dim:
        raise ValueError(f"{what}: the inducing inputs have d = {vfe.dim}, the inputs d = {x.dim}")
    return y


def _elbo_dtc(vfe: VFE, fx: "FiniteGP", y, with_regulariser: bool, what: str):
    y = _sparse_args(vfe, fx, y, what)
    L.ensure_init()
    f, x = fx.f, fx.x
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    e, t = C.c_double(), C.c_double()
    L.check(L.load().lmm_oilmm_elbo(x.carr().ptr, x.dim, x.n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), gps, 0, m,
                                    vfe.carr().ptr, vfe.nz, vfe.jitter, int(with_regulariser), C.byref(e), C.byref(t)))
    return e.value, t.value


def elbo(vfe: VFE, fx: "FiniteGP", y, with_regulariser: bool = True) -> float:
    """elbo(VFE(f(z)), fx, y) of AbstractGPs (Titsias' collapsed bound) summed over the latents of an OILMM, plus the OILMM
    regulariser (reference src/oilmm.jl:101-113): a lower bound of logpdf(fx, y)."""
    return _elbo_dtc(vfe, fx, y, with_regulariser, "elbo")[0]


def dtc(vfe: VFE, fx: "FiniteGP", y, with_regulariser: bool = True) -> float:
    """dtc(VFE(f(z)), fx, y) of AbstractGPs: the log density under the low-rank prior Q_ff (the bound without its trace term)."""
    return _elbo_dtc(vfe, fx, y, with_regulariser, "dtc")[1]


def elbo_and_gradient(vfe: VFE, fx: "FiniteGP", y, with_regulariser: bool = True) -> dict:
    """Value and gradient of elbo(vfe, fx, y): {"value", "y", "sigma2", "S", "U", "gps", "z"}.  "value" is bitwise elbo(vfe, fx, y);
    "y", "sigma2", "S", "U" and "gps" are as logpdf_and_gradient returns them for a prior OILMM ("gps" through _gps_grads: per-dimension
    lengthscales, alpha, r, decay and sum terms included); "z" is the gradient with respect to the inducing inputs, shaped and typed
    like vfe.z ((M,) or (d, M); NumPy or torch).  There is no gradient of dtc."""
    y = _sparse_args(vfe, fx, y, "elbo_and_gradient")
    L.ensure_init()
    f, x = fx.f, fx.x
    Ua, Sa, p, m = _H_args(f.H)
    val, gs2 = C.c_double(), C.c_double()
    gy, gS, gU = _alloc_like(y if L._is_torch(y) else x.x, x.n * p), np.empty(m), np.empty(p * m)
    gz = _alloc_like(vfe.z, x.dim * vfe.nz)
    gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in f.f.fs])
    L.check(L.load().lmm_oilmm_elbo_grad(x.carr().ptr, x.dim, x.n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), ga, 0, m,
                                         vfe.carr().ptr, vfe.nz, vfe.jitter, int(with_regulariser), C.byref(val), L.Arr(gy, True).ptr,
                                         C.byref(gs2), L.Arr(gS, True).ptr, L.Arr(gU, True).ptr, gg, L.Arr(gz, True).ptr))
    return {"value": val.value, "y": gy, "sigma2": gs2.value, "S": gS, "U": gU.reshape(m, p).T.copy(),
            "gps": _gps_grads(gg, ga, m, x.dim), "z": _x_grad(gz, vfe.z)}


def approx_posterior(vfe: VFE, fx: "FiniteGP", y) -> "ILMM":
    """posterior(VFE(f(z)), fx, y) of AbstractGPs: an OILMM with the same H whose latents are ApproxPosteriorGPs.  mean_and_var, mean,
    var and marginals work on it; nothing else does."""
    y = _sparse_args(vfe, fx, y, "approx_posterior")
    L.ensure_init()
    f, x = fx.f, fx.x
    gps = L.gps_array([g.desc() for g in f.f.fs])
    Ua, Sa, p, m = _H_args(f.H)
    handle = C.c_void_p()
    L.check(L.load().lmm_oilmm_sparse_posterior_create(x.carr().ptr, x.dim, x.n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2),
                                                       gps, 0, m, vfe.carr().ptr, vfe.nz, vfe.jitter, C.byref(handle)))
    return ILMM(IndependentMOGP(f.f.fs, _SparsePostHandle(handle, 0, m)), f.H, shard=f.shard)


def _sparse_mean_and_var(fx: "FiniteGP", add_noise: bool, want_var: bool):
    f, x = fx.f, fx.x
    if not isinstance(f, ILMM) or not isinstance(x, MOInputIsotopicByOutputs):
        raise NotImplementedError("an inducing-point posterior is an OILMM over MOInputIsotopicByOutputs inputs")
    unpack(fx)
    L.ensure_init()
    Ua, Sa, p, m = _H_args(f.H)
    mean = _alloc_like(x.x, x.n * p)
    var = _alloc_like(x.x, x.n * p) if want_var else None
    L.check(L.load().lmm_oilmm_sparse_mean_and_var(f.f._post.ptr, None, Ua.ptr, Sa.ptr, p, m, float(fx.sigma2), int(add_noise),
                                                   x.carr().ptr, x.dim, x.n, L.Arr(mean, True).ptr,
                                                   L.Arr(var, True).ptr if want_var else None))
    return mean, var


# ---- state space (Matern latents over a one-dimensional input) -----------------------------------------------
# Matern12 / 32 / 52 latents over a one-dimensional input are finite-dimensional linear SDEs, so a Kalman filter gives logpdf and an RTS
# smoother the posterior marginals in O(n), exactly (include/lmm_hip.h, "state space").  The library takes sorted
# inputs; the sorting, and the merging of new inputs as points without observations, happen here.
_STATESPACE_DIM = {"matern12": 1, "matern32": 2, "matern52": 3, "sho": 2}
_STATESPACE_MAX_DIM = 4      # the largest state the kernels are built for: a sum of two terms whose dimensions add up to it


def _statespace_dim(k) -> Optional[int]:
    """The state dimension of a latent kernel the state-space functions serve, None for any other: a plain Matern12 / 32 / 52 or SHO
    with a scalar lengthscale, or a KernelSum of exactly two plain Matern terms whose dimensions add up to at most 4 (the sum's own
    variance and lengthscale fold into the terms; the library has one order of the terms, so either order is served).  An SHO term
    inside a KernelSum stays refused here, as on the dense verbs: the library serves it (lmm_kernel_sum_create_statespace,
    L.statespace_gps_array), these functions do not yet."""
    if k.kind in _STATESPACE_DIM:
        return _STATESPACE_DIM[k.kind] if np.ndim(k.lengthscale) == 0 else None
    if k.kind == "sum" and len(k.kernels) == 2:
        dims = [None if t.kind in ("sum", "sho") else _statespace_dim(t) for t in k.kernels]
        if None not in dims and sum(dims) <= _STATESPACE_MAX_DIM:
            return sum(dims)
    return None


def _statespace_refuse_sums(fx: "FiniteGP", what: str) -> None:
    """Gradients with respect to locations are not served for a sum latent: the second component of its state is not f'."""
    for l, gp in enumerate(fx.f.f.fs):
        if gp.kernel.kind == "sum":
            raise NotImplementedError(f"{what}: gradients with respect to locations are not served for a sum latent on the state-space "
                                      f"path; latent {l} is {gp.kernel!r}")


def _statespace_sorted(xv, y, p: int, xs=None):
    """(x sorted, y permuted, perm, n) for inputs xv (n,) and the by-outputs vector y (n * p); with xs (ns,) the new inputs are appended
    as points whose outputs are all NaN before sorting.  The sort is stable; perm[k] is the original index of sorted point k.  NumPy
    arrays unless xv or y is a torch tensor (then tensors on that one's device).  y = None (no xs): only the inputs are sorted, and the
    second value is None."""
    n = int(xv.shape[-1])
    if y is None:
        if L._is_torch(xv):
            import torch
            xa, perm = torch.sort(torch.as_tensor(xv, dtype=torch.float64).reshape(-1), stable=True)
            return xa.contiguous(), None, perm, n
        xa = np.asarray(xv, dtype=np.float64).reshape(-1)
        perm = np.argsort(xa, kind="stable")
        return np.ascontiguousarray(xa[perm]), None, perm, n
    if L._is_torch(xv) or L._is_torch(y):
        import torch
        dev = xv.device if L._is_torch(xv) else y.device
        xa = torch.as_tensor(xv, dtype=torch.float64, device=dev).reshape(-1)
        Y = torch.as_tensor(y, dtype=torch.float64, device=dev).reshape(p, n)
        if xs is not None:
            xn = torch.as_tensor(xs, dtype=torch.float64, device=dev).reshape(-1)
            xa = torch.cat([xa, xn])
            Y = torch.cat([Y, torch.full((p, int(xn.shape[0])), float("nan"), dtype=torch.float64, device=dev)], dim=1)
        xa, perm = torch.sort(xa, stable=True)
        return xa.contiguous(), Y[:, perm].reshape(-1).contiguous(), perm, n
    xa = np.asarray(xv, dtype=np.float64).reshape(-1)
    Y = np.asarray(y, dtype=np.float64).reshape(p, n)
    if xs is not None:
        xn = np.asarray(xs, dtype=np.float64).reshape(-1)
        xa = np.concatenate([xa, xn])
        Y = np.concatenate([Y, np.full((p, xn.shape[0]), np.nan)], axis=1)
    perm = np.argsort(xa, kind="stable")
    return np.ascontiguousarray(xa[perm]), np.ascontiguousarray(Y[:, perm]).reshape(-1), perm, n


def _statespace_unsorted(out, perm, p: int, n: int, only_new: bool):
    """A by-outputs result over the sorted points back in the callers' order: the n training inputs, or (only_new) the inputs
    appended behind them."""
    N = int(perm.shape[0])
    O = out.reshape(p, N)
    if L._is_torch(out):
        import torch
        B = torch.empty_like(O)
        B[:, perm] = O
        return (B[:, n:] if only_new else B[:, :n]).reshape(-1).contiguous()
    B = np.empty_like(O)
    B[:, perm] = O
    return np.ascontiguousarray(B[:, n:] if only_new else B[:, :n]).reshape(-1)


def _statespace_args(fx: "FiniteGP", y, what: str):
    """Checks of statespace_logpdf / statespace_mean_and_var, all before any library call."""
    f, x = fx.f, fx.x
    if isinstance(f, IndependentMOGP):
        raise NotImplementedError(f"{what}: state-space inference is not served for an IndependentMOGP (wrap it in an OILMM)")
    if not isinstance(f, ILMM) or not f.is_oilmm:
        raise NotImplementedError(f"{what}: state-space inference is not served for a dense-H ILMM (OILMM only)")
    if f.f._post is not None:
        raise NotImplementedError(f"{what}: state-space inference is not served on a posterior model (prior OILMM only)")
    if f.shard != (0, len(f.f.fs)):
        raise NotImplementedError(f"{what}: state-space inference is not served with latents sharded across processes")
    if not isinstance(x, MOInputIsotopicByOutputs):
        raise NotImplementedError(f"{what}: state-space inference takes MOInputIsotopicByOutputs inputs")
    if fx.heteroscedastic:
        raise NotImplementedError(f"{what}: state-space inference takes a scalar noise variance (no per-point noise)")
    if x.dim != 1:
        raise NotImplementedError(f"{what}: state-space inference is served for one-dimensional inputs (d = {x.dim})")
    for l, gp in enumerate(f.f.fs):
        k = gp.kernel
        if _statespace_dim(k) is None:
            raise NotImplementedError(f"{what}: state-space inference is served for plain Matern12, Matern32 and Matern52 latents; "
                                      f"latent {l} is {k!r}")
    if not hasattr(y, "shape"):
        y = np.asarray(y, dtype=np.float64)
    if len(y.shape) != 1:
        raise NotImplementedError(f"{what}: state-space inference is not served for a matrix Y (one vector y)")
    unpack(fx)
    if y.shape[0] != x.n * x.out_dim:
        raise ValueError("length(y) != n * out_dim")
    return y


def statespace_logpdf(fx: "FiniteGP", y, with_regulariser: bool = True) -> float:
    """logpdf(fx, y) of a prior OILMM whose latents are Matern12 / 32 / 52 or SHO (in any mixture and order) over one-dimensional inputs, by a
    Kalman filter per latent; a latent may also be a KernelSum of two plain Matern terms whose state dimensions (1 / 2 / 3) add up to
    at most 4 -- "short + long lengthscale" in one latent (_statespace_dim; DESIGN.md 4.18 "Sum latents"):
    the value of logpdf (NaN in y included: the missing-data approximation of logpdf) in O(n).  Points may come in any order (they are
    sorted here, stably); a point whose outputs are all NaN is a predict-only step and leaves the value unchanged."""
    y = _statespace_args(fx, y, "statespace_logpdf")
    f, x = fx.f, fx.x
    xa, ya, _, _ = _statespace_sorted(x.x.reshape(-1), y, x.out_dim)
    L.ensure_init()
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    out = C.c_double()
    L.check(L.load().lmm_oilmm_logpdf_statespace(L.Arr(xa).ptr, x.n, L.Arr(ya).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), gps, 0, m,
                                                 int(with_regulariser), C.byref(out)))
    return out.value


def statespace_mean_and_var(fx: "FiniteGP", y, add_noise: bool = True, xs=None):
    """mean_and_var(posterior(fx, y)(x*, sigma2)) of the same models by a Kalman filter and an RTS smoother per latent, in O(n): at the
    training inputs (xs=None) or at the new inputs xs ((ns,); they are merged into the inputs as points without observations, and only
    their rows are returned).  By-outputs vectors (mean, var), NumPy or torch like the inputs; add_noise adds sigma2 to the variances."""
    y = _statespace_args(fx, y, "statespace_mean_and_var")
    f, x = fx.f, fx.x
    if xs is not None:
        if not hasattr(xs, "shape"):
            xs = np.asarray(xs, dtype=np.float64)
        if len(xs.shape) != 1:
            raise ValueError("statespace_mean_and_var: xs is a (ns,) array of one-dimensional inputs")
        if int(xs.shape[0]) == 0:
            xs = None
    xa, ya, perm, n = _statespace_sorted(x.x.reshape(-1), y, x.out_dim, xs)
    N = int(perm.shape[0])
    L.ensure_init()
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    mean, var = _alloc_like(xa, N * p), _alloc_like(xa, N * p)
    L.check(L.load().lmm_oilmm_mean_and_var_statespace(L.Arr(xa).ptr, N, L.Arr(ya).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), gps, 0, m,
                                                       int(add_noise), L.Arr(mean, True).ptr, L.Arr(var, True).ptr))
    return _statespace_unsorted(mean, perm, p, n, xs is not None), _statespace_unsorted(var, perm, p, n, xs is not None)


class StateSpacePosterior:
    """posterior(fx, y) on the state-space path: owns an lmm_ss_post_t* (the sorted inputs and, per latent, the filtered and the
    smoothed states on the device; include/lmm_hip.h "state space: the posterior object") and answers mean_and_var(post(x*, sigma2))
    at new inputs in O(ns log n) per latent, without touching the data again; rand draws joint samples there from the same states,
    and predictive_logpdf scores held-out observations there.
    Built by statespace_posterior; freed by close(), on leaving a `with` block or with the object."""

    def __init__(self, ptr: C.c_void_p, n: int, p: int, logpdf: float, dims: Optional[Sequence[int]] = None,
                 x_last: Optional[float] = None, sums: Sequence[int] = ()):
        self._ptr, self.n, self.p, self.logpdf = ptr, n, p, logpdf
        self._sums = [int(l) for l in sums]                                  # the sum latents: mean_and_var_vjp refuses them
        self._dims = None if dims is None else [int(D) for D in dims]       # the latents' state dimensions: what rand draws per point
        self._x_last = None if x_last is None else float(x_last)            # the last input, kept on the host for append's check

    def close(self) -> None:
        if self._ptr:
            ptr, self._ptr = self._ptr, None
            L.load().lmm_statespace_post_destroy(ptr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, x_new, y_new) -> float:
        """Conditions the posterior on k LATER observations in O(k), without starting over (include/lmm_hip.h "state space: appending
        observations").  x_new: (k,) inputs in any order (sorted here, stably), NumPy or a torch device tensor, none in front of the
        last input so far (equal to it is served); y_new: (k * p,) by outputs in the caller's order, NaN = missing.  Returns the
        increment log p(y_new | all earlier data) and updates n and logpdf.  The smoothed states fall behind (`smoothed`): forecasts
        stay O(1) per query, and the first query in front of the last input (or smooth()) pays one O(n) pass that does not need the
        data.  Every refusal below comes before any library call."""
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        if not hasattr(x_new, "shape"):
            x_new = np.asarray(x_new, dtype=np.float64)
        if not hasattr(y_new, "shape"):
            y_new = np.asarray(y_new, dtype=np.float64)
        if len(x_new.shape) != 1:
            raise ValueError("StateSpacePosterior.append: x_new is a (k,) array of one-dimensional inputs")
        k = int(x_new.shape[0])
        if len(y_new.shape) != 1 or int(y_new.shape[0]) != k * self.p:
            raise ValueError(f"StateSpacePosterior.append: y_new holds k * p = {k * self.p} values by outputs")
        if self._x_last is None:
            raise ValueError("StateSpacePosterior.append: the handle was built without its last input")
        if k == 0:
            return 0.0
        if L._is_torch(x_new):
            import torch
            x_new = x_new.to(torch.float64)
            finite, lo, hi = bool(torch.isfinite(x_new).all()), float(x_new.min()), float(x_new.max())
        else:
            x_new = np.ascontiguousarray(x_new, dtype=np.float64)
            finite, lo, hi = bool(np.isfinite(x_new).all()), float(x_new.min()), float(x_new.max())
        if not finite:
            raise ValueError("StateSpacePosterior.append: x_new must be finite (no NaN or Inf)")
        if lo < self._x_last:
            raise ValueError(f"StateSpacePosterior.append: appended points lie at or behind the last input ({lo} is in front of "
                             f"{self._x_last})")
        xa, ya, _, _ = _statespace_sorted(x_new, y_new, self.p)
        out = C.c_double()
        L.check(L.load().lmm_oilmm_statespace_post_append(self._ptr, L.Arr(xa).ptr, k, L.Arr(ya).ptr, C.byref(out)))
        self.n += k
        self.logpdf += out.value
        self._x_last = hi
        return out.value

    def smooth(self) -> None:
        """Brings the smoothed states up to date after appends (one O(n) pass over the kept filtered states); else nothing."""
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        L.check(L.load().lmm_statespace_post_smooth(self._ptr))

    def reserve(self, n_total: int) -> None:
        """Room for n_total points in all, so that appends up to there do not grow the buffers; smaller than the capacity: nothing."""
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        if int(n_total) != n_total or n_total < 0 or n_total > 2 ** 31 - 1:
            raise ValueError("StateSpacePosterior.reserve: n_total is a number of points in 0 .. 2^31 - 1")
        L.check(L.load().lmm_statespace_post_reserve(self._ptr, int(n_total)))

    def _size(self):
        n, sn, cap = C.c_int(), C.c_int(), C.c_int()
        L.check(L.load().lmm_statespace_post_size(self._ptr, C.byref(n), C.byref(sn), C.byref(cap)))
        return n.value, sn.value, cap.value

    @property
    def smoothed(self) -> bool:
        """Whether the smoothed states are current (False between an append and the next smooth, explicit or on demand)."""
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        n, sn, _ = self._size()
        return sn == n

    @property
    def capacity(self) -> int:
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        return self._size()[2]

    def _queries(self, xs):
        """xs as a (ns,) float64 array, checked: every refusal comes before any library call."""
        if not self._ptr:
            raise ValueError("StateSpacePosterior: the posterior has been closed")
        if not hasattr(xs, "shape"):
            xs = np.asarray(xs, dtype=np.float64)
        if len(xs.shape) != 1:
            raise ValueError("StateSpacePosterior: xs is a (ns,) array of one-dimensional inputs")
        if L._is_torch(xs):
            import torch
            xs = xs.to(torch.float64)
            finite = bool(torch.isfinite(xs).all())
        else:
            xs = np.ascontiguousarray(xs, dtype=np.float64)
            finite = bool(np.isfinite(xs).all())
        if not finite:
            raise ValueError("StateSpacePosterior: xs must be finite (no NaN or Inf)")
        return xs

    def _query(self, xs, add_noise: bool, want_var: bool):
        xs = self._queries(xs)
        ns = int(xs.shape[0])
        mean = _alloc_like(xs, ns * self.p)
        var = _alloc_like(xs, ns * self.p) if want_var else None
        if ns == 0:
            return mean, var
        L.check(L.load().lmm_oilmm_statespace_post_mean_and_var(self._ptr, L.Arr(xs).ptr, ns, int(add_noise), L.Arr(mean, True).ptr,
                                                                L.Arr(var, True).ptr if want_var else None))
        return mean, var

    def mean_and_var(self, xs, add_noise: bool = True):
        """(mean, var) at the inputs xs ((ns,), in any order): by-outputs vectors of ns * p values, NumPy or torch-device like xs."""
        return self._query(xs, add_noise, True)

    def mean(self, xs):
        return self._query(xs, False, False)[0]

    def var(self, xs, add_noise: bool = True):
        return self._query(xs, add_noise, True)[1]

    def marginals(self, xs) -> "Normal":
        """Normal(mean, sqrt(var)) as marginals builds it."""
        m, v = self._query(xs, True, True)
        return Normal(m, v ** 0.5)

    def mean_and_var_vjp(self, xs, dmean=None, dvar=None) -> dict:
        """Pullback of mean_and_var to the queries: {"x": d/d xs of sum(dmean * mean) + sum(dvar * var)} with mean, var =
        self.mean_and_var(xs), shaped and typed like xs and in the callers' order, in O(ns log n) per latent from the stored states
        (include/lmm_hip.h, lmm_oilmm_statespace_post_mean_and_var_grad_xs).  dmean, dvar: by-outputs cotangents of ns * p values, NumPy
        or torch; dvar=None is the pullback of the mean alone, dmean=None that of the variance.  The sigma2 that add_noise adds does not
        depend on xs, so there is no add_noise argument and no "sigma2" entry.  A query's entry depends on no other query.
        Matern12 latents only: at a query equal to a training input the mean has a kink, and the derivative returned is that of the
        side the query is sorted to (behind the training point); Matern32, Matern52 and SHO latents are differentiable there."""
        if self._sums:
            raise NotImplementedError("StateSpacePosterior.mean_and_var_vjp: gradients with respect to locations are not served for a "
                                      f"sum latent on the state-space path (latent {self._sums[0]})")
        xs = self._queries(xs)
        ns = int(xs.shape[0])
        if dmean is None and dvar is None:
            raise ValueError("StateSpacePosterior.mean_and_var_vjp: dmean and dvar are both None")
        cot = []
        for name, d in (("dmean", dmean), ("dvar", dvar)):
            if d is not None:
                if not hasattr(d, "shape"):
                    d = np.asarray(d, dtype=np.float64)
                if len(d.shape) != 1 or int(d.shape[0]) != ns * self.p:
                    raise ValueError(f"StateSpacePosterior.mean_and_var_vjp: {name} holds ns * p = {ns * self.p} values by outputs")
                if L._is_torch(d):
                    import torch
                    d = d.to(torch.float64)
            cot.append(d)
        gx = _alloc_like(xs, ns)
        if ns == 0:
            return {"x": gx}
        L.check(L.load().lmm_oilmm_statespace_post_mean_and_var_grad_xs(self._ptr, L.Arr(xs).ptr, ns,
                                                                        None if cot[0] is None else L.Arr(cot[0]).ptr,
                                                                        None if cot[1] is None else L.Arr(cot[1]).ptr, L.Arr(gx, True).ptr))
        return {"x": gx}

    def _window(self, lo: float, hi: float):
        first, count = C.c_int(), C.c_int()
        L.check(L.load().lmm_statespace_post_window(self._ptr, float(lo), float(hi), C.byref(first), C.byref(count)))
        return first.value, count.value

    def window(self, xs):
        """(first, count): the training points (of the sorted inputs) that lie between the smallest and the largest of the queries xs,
        first = #{t : x_t <= min xs}.  rand touches these and the queries, W = ns + count points per latent and sample, and nothing
        else.  No queries: (0, 0)."""
        xs = self._queries(xs)
        if int(xs.shape[0]) == 0:
            return 0, 0
        L.ensure_init()
        return self._window(float(xs.min()), float(xs.max()))

    def rand(self, rng, xs, N: Optional[int] = None, add_noise: bool = True):
        """Joint samples of post(xs, sigma2) at the inputs xs ((ns,), in any order; NumPy or a torch device tensor), exact, without
        touching the data again: rand(rng, posterior(fx, y)(x*, sigma2)) in O(ns + count) per latent and sample (window(xs)), by
        sampling the posterior's Markov chain backwards from the largest query (include/lmm_hip.h "state space: sampling from the
        posterior object").  `rng` is a NumPy Generator or a DeviceNormals; buffers and the result live where the normals do.  The
        queries are sorted here, stably.  Draw order, per sample, with W = ns + count window points (the sorted queries merged with the
        training points between them, a training point before an equal query):
          for each latent l in order, standard_normal(D_l * W)     (component-major: component i of window point j at i * W + j);
          then, if add_noise, standard_normal(ns * p)               (by outputs, over the SORTED queries).
        Returns the by-outputs vector (ns * p,) for N=None, else (ns * p, N), in the callers' order of queries; column q of an N-sample
        call is bitwise the one-sample call on the same normals."""
        xs = self._queries(xs)
        if N is not None and (int(N) != N or N < 1):
            raise ValueError("StateSpacePosterior.rand: N is None or a number of samples >= 1")
        if self._dims is None:
            raise ValueError("StateSpacePosterior.rand: the handle was built without its latents' state dimensions")
        ns, Ns, p = int(xs.shape[0]), 1 if N is None else int(N), self.p
        if ns == 0:
            return _empty_for(rng, 0) if N is None else _empty_for(rng, 0, Ns)
        if L._is_torch(xs):
            import torch
            xq, perm = torch.sort(xs, stable=True)
            xq = xq.contiguous()
        else:
            perm = np.argsort(xs, kind="stable")
            xq = np.ascontiguousarray(xs[perm])
        L.ensure_init()
        _, count = self._window(float(xq[0]), float(xq[-1]))
        W = ns + count
        z = _empty_for(rng, Ns, sum(self._dims) * W)
        eps = _empty_for(rng, Ns, ns * p) if add_noise else None
        for q in range(Ns):
            off = 0
            for D in self._dims:
                z[q, off:off + D * W] = rng.standard_normal(D * W)
                off += D * W
            if eps is not None:
                eps[q] = rng.standard_normal(ns * p)
        out = _empty_for(rng, Ns, ns * p)
        L.check(L.load().lmm_oilmm_statespace_post_rand(self._ptr, L.Arr(xq).ptr, ns, L.Arr(z).ptr, None if eps is None else L.Arr(eps).ptr,
                                                        Ns, int(add_noise), L.Arr(out, True).ptr))
        if L._is_torch(out) and not L._is_torch(perm):        # the un-permuting happens where the result lives
            import torch
            perm = torch.as_tensor(perm, device=out.device)
        elif L._is_torch(perm) and not L._is_torch(out):
            perm = perm.cpu().numpy()
        cols = [_statespace_unsorted(out[q], perm, p, ns, False) for q in range(Ns)]
        if N is None:
            return cols[0]
        if L._is_torch(out):
            import torch
            return torch.stack(cols, dim=1)
        return np.stack(cols, axis=1)

    def predictive_logpdf(self, xs, ys, sigma2: Optional[float] = None) -> float:
        """logpdf(post(xs, sigma2), ys): the joint log density of the held-out observations ys at the inputs xs given the training
        data, from the stored states alone, in O(ns + count) per latent (window(xs)) -- a Kalman filter over the posterior's backward
        Markov chain, run from the largest query (include/lmm_hip.h "state space: predictive log density").  (`logpdf` is the
        attribute that holds the training data's value, hence the name.)  xs: (ns,) in any order (sorted here, stably, with ys
        carried along), NumPy or a torch device tensor; ys: (ns * p,) by outputs in the caller's order, NaN = missing (a query
        without any observed output contributes 0; one observing fewer than m outputs is refused by the library, which names it by
        its index among the sorted queries); sigma2: the noise at the queries, None = the handle's own.  The handle is left
        as it was: n, logpdf and every later answer are unchanged.  Every refusal below comes before any library call."""
        xs = self._queries(xs)
        ns = int(xs.shape[0])
        if not hasattr(ys, "shape"):
            ys = np.asarray(ys, dtype=np.float64)
        if len(ys.shape) != 1 or int(ys.shape[0]) != ns * self.p:
            raise ValueError(f"StateSpacePosterior.predictive_logpdf: ys holds ns * p = {ns * self.p} values by outputs")
        if sigma2 is not None:
            sigma2 = float(sigma2)
            if not np.isfinite(sigma2) or not sigma2 > 0.0:
                raise ValueError("StateSpacePosterior.predictive_logpdf: sigma2 must be finite and > 0 (None: the handle's own)")
        if ns == 0:
            return 0.0
        xa, ya, _, _ = _statespace_sorted(xs, ys, self.p)
        out = C.c_double()
        L.check(L.load().lmm_oilmm_statespace_post_logpdf(self._ptr, L.Arr(xa).ptr, ns, L.Arr(ya).ptr, 0.0 if sigma2 is None else sigma2,
                                                          C.byref(out)))
        return out.value


def statespace_posterior(fx: "FiniteGP", y) -> StateSpacePosterior:
    """posterior(fx, y) of the models statespace_logpdf serves, as a reusable object: one O(n) pass (the inputs are sorted here once,
    stably; NaN in y is missing data) conditions on the data, and post.mean_and_var(xs) then answers at any new inputs without it.
    post.logpdf is bitwise statespace_logpdf(fx, y)."""
    y = _statespace_args(fx, y, "statespace_posterior")
    f, x = fx.f, fx.x
    xa, ya, _, _ = _statespace_sorted(x.x.reshape(-1), y, x.out_dim)
    L.ensure_init()
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    ptr, out = C.c_void_p(), C.c_double()
    L.check(L.load().lmm_oilmm_statespace_posterior_create(L.Arr(xa).ptr, x.n, L.Arr(ya).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), gps,
                                                           0, m, C.byref(ptr), C.byref(out)))
    return StateSpacePosterior(ptr, x.n, p, out.value, [_statespace_dim(g.kernel) for g in f.f.fs], float(xa[-1]),
                               [l for l, g in enumerate(f.f.fs) if g.kernel.kind == "sum"])


class _NoStateSpaceMixingGradient(dict):
    """The gradient dict of statespace_logpdf_and_gradient for data with NaN: "S" and "U" are not built (as _NoMixingGradient)."""

    def __missing__(self, key):
        if key in ("S", "U"):
            raise NotImplementedError(f"statespace_logpdf_and_gradient: the gradient with respect to {key!r} is not built for data with NaN")
        raise KeyError(key)


def statespace_logpdf_and_gradient(fx: "FiniteGP", y, with_regulariser: bool = True, inputs: bool = False) -> dict:
    """Value and gradient of statespace_logpdf(fx, y) in O(n): {"value", "y", "sigma2", "S", "U", "gps"}, as logpdf_and_gradient returns
    them for a prior OILMM.  "value" is bitwise statespace_logpdf(fx, y, with_regulariser); "y" is shaped and typed like y, in the
    callers' order of points whatever the order of the inputs, and exactly 0 at NaN entries; "gps" (through _gps_grads) holds every
    latent's "variance", "lengthscale" and "mean", and an SHO latent's "quality" ("lengthscale" is then d / d period).  With NaN in y (points whose outputs are all NaN included) "S" and "U" raise
    NotImplementedError, as after logpdf_and_gradient.  inputs=True adds "x", the gradient with respect to the input locations in O(n)
    (include/lmm_hip.h, lmm_oilmm_logpdf_grad_statespace_x): shaped and typed like fx.x.x, in the callers' order of points, exactly 0
    at points whose outputs are all NaN; every other entry is bitwise that of inputs=False."""
    y = _statespace_args(fx, y, "statespace_logpdf_and_gradient")
    if inputs:
        _statespace_refuse_sums(fx, "statespace_logpdf_and_gradient(inputs=True)")
    f, x = fx.f, fx.x
    nan = _has_nan(y)
    xa, ya, perm, n = _statespace_sorted(x.x.reshape(-1), y, x.out_dim)
    L.ensure_init()
    Ua, Sa, p, m = _H_args(f.H)
    val, gs2 = C.c_double(), C.c_double()
    gy, gS, gU = _alloc_like(ya, n * p), np.empty(m), np.empty(p * m)
    gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in f.f.fs])
    args = (L.Arr(xa).ptr, n, L.Arr(ya).ptr, p, Ua.ptr, Sa.ptr, m, float(fx.sigma2), ga, 0, m, int(with_regulariser), C.byref(val),
            L.Arr(gy, True).ptr, C.byref(gs2), None if nan else L.Arr(gS, True).ptr, None if nan else L.Arr(gU, True).ptr, gg)
    gx = None
    if inputs:
        gx = _alloc_like(xa, n)
        L.check(L.load().lmm_oilmm_logpdf_grad_statespace_x(*args, L.Arr(gx, True).ptr))
        gx = _statespace_unsorted(gx, perm, 1, n, False).reshape(x.x.shape)
        if L._is_torch(gx) and not L._is_torch(x.x):      # NumPy inputs x with a torch y
            gx = gx.cpu().numpy()
    else:
        L.check(L.load().lmm_oilmm_logpdf_grad_statespace(*args))
    gy = _statespace_unsorted(gy, perm, p, n, False)
    if L._is_torch(gy) and not L._is_torch(y):        # torch inputs x with a NumPy y
        gy = gy.cpu().numpy()
    out = {"value": val.value, "y": gy, "sigma2": gs2.value, "gps": _gps_grads(gg, ga, m, 1)}
    if inputs:
        out["x"] = gx
    if nan:
        return _NoStateSpaceMixingGradient(out)
    out.update(S=gS, U=gU.reshape(m, p).T.copy())
    return out


def statespace_rand(rng, fx: "FiniteGP", y=None, N: Optional[int] = None, add_noise: bool = True, xs=None):
    """Joint samples of the same models in O(n), exact: of the prior fx (y=None: rand(rng, fx)), or of the posterior given y
    (rand(rng, posterior(fx, y)(x*, sigma2))) at the training inputs (xs=None) or at the new inputs xs ((ns,); merged into the inputs
    as points without observations, only their rows are returned).  Per latent the prior path is the SDE's recursion driven by D
    standard normals per point (D = 1 / 2 / 3 for Matern12 / 32 / 52, 2 for SHO), run as a scan; a posterior path is the prior path plus the
    smoothed mean of the residual data (pathwise conditioning), through the filter and smoother of statespace_mean_and_var.
    `rng` is a NumPy Generator or a DeviceNormals, as for rand; buffers and the result live where the normals do.  Draw order, per
    sample, all indexed by SORTED point (the stable sort of the inputs; n_all counts the new inputs as well):
      for each latent l in order, standard_normal(D_l * n_all)     (component-major: component i of sorted point t at i * n_all + t);
      then, with y only, standard_normal(m * n_all)                (latent-major);
      then, if add_noise, standard_normal(n_all * p)               (by outputs).
    Returns the by-outputs vector (n * p,) for N=None, else (n * p, N), in the callers' order of points.  For fixed normals the path is
    ill-conditioned in the spacings where they are small against the lengthscale; its distribution is not."""
    f, x = fx.f, fx.x
    yc = _statespace_args(fx, np.broadcast_to(0.0, (x.n * x.out_dim,)) if y is None else y, "statespace_rand")
    if y is None and xs is not None:
        raise ValueError("statespace_rand: xs needs y; to sample the prior at other inputs, put them into fx.x")
    if N is not None and (int(N) != N or N < 1):
        raise ValueError("statespace_rand: N is None or a number of samples >= 1")
    if xs is not None:
        if not hasattr(xs, "shape"):
            xs = np.asarray(xs, dtype=np.float64)
        if len(xs.shape) != 1:
            raise ValueError("statespace_rand: xs is a (ns,) array of one-dimensional inputs")
        if int(xs.shape[0]) == 0:
            xs = None
    xa, ya, perm, n = _statespace_sorted(x.x.reshape(-1), None if y is None else yc, x.out_dim, xs)
    na, Ns = int(perm.shape[0]), 1 if N is None else int(N)
    L.ensure_init()
    _, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    dims = [_statespace_dim(g.kernel) for g in f.f.fs]
    z = _empty_for(rng, Ns, sum(dims) * na)
    xi = _empty_for(rng, Ns, m * na) if y is not None else None
    eps = _empty_for(rng, Ns, na * p) if add_noise else None
    for q in range(Ns):
        off = 0
        for D in dims:
            z[q, off:off + D * na] = rng.standard_normal(D * na)
            off += D * na
        if xi is not None:
            xi[q] = rng.standard_normal(m * na)
        if eps is not None:
            eps[q] = rng.standard_normal(na * p)
    out = _empty_for(rng, Ns, na * p)
    L.check(L.load().lmm_oilmm_rand_statespace(L.Arr(xa).ptr, na, None if y is None else L.Arr(ya).ptr, p, Ua.ptr, Sa.ptr, m,
                                               float(fx.sigma2), gps, 0, m, int(add_noise), Ns, L.Arr(z).ptr,
                                               None if xi is None else L.Arr(xi).ptr, None if eps is None else L.Arr(eps).ptr,
                                               L.Arr(out, True).ptr))
    if L._is_torch(out) and not L._is_torch(perm):        # the un-permuting happens where the result lives
        import torch
        perm = torch.as_tensor(perm, device=out.device)
    elif L._is_torch(perm) and not L._is_torch(out):
        perm = perm.cpu().numpy()
    cols = [_statespace_unsorted(out[q], perm, p, n, xs is not None) for q in range(Ns)]
    if N is None:
        return cols[0]
    if L._is_torch(out):
        import torch
        return torch.stack(cols, dim=1)
    return np.stack(cols, axis=1)


# Dense-H ILMM logpdf: allow the identical-kernel decoupled shortcut (exact).  Set False to force
# the reference's single (mn) x (mn) factorisation.  ILMM_LAST_PATH records which ran.
ILMM_ALLOW_DECOUPLED = True
ILMM_LAST_PATH = None


# ---- the AbstractGPs verbs ----------------------------------------------------------------------------
def logpdf(fx: FiniteGP, y, with_regulariser: bool = True) -> float:
    """logpdf(fx, y).  ILMM/OILMM: reference src/oilmm.jl:79-93, src/ilmm.jl:150-163; IndependentMOGP:
    src/independent_mogp.jl:74-80.  Returns this process's shard of the sum (the whole value when the model
    is not sharded)."""
    _refuse_sparse(fx, "logpdf")
    _refuse_sho_dims(fx, "logpdf")
    L.ensure_init()
    lib = L.load()
    if _has_nan(y):
        return _logpdf_missing(fx, y, with_regulariser)
    f, x, s2 = fx.f, fx.x, fx.sigma2
    if isinstance(x, MOInputIsotopicByFeatures):          # reference src/independent_mogp.jl:222-229
        if not isinstance(f, IndependentMOGP):
            raise TypeError("ILMM needs MOInputIsotopicByOutputs (reference src/ilmm.jl:45)")
        if fx.heteroscedastic:                            # reorder_by_outputs(Sigma_y, x): src/independent_mogp.jl:149-151
            s2 = _reorder(s2, x.n, x.out_dim, True)
        return logpdf(FiniteGP(f, x.by_outputs(), s2), _reorder(y, x.n, x.out_dim, True))
    if fx.heteroscedastic:
        if not isinstance(f, IndependentMOGP) or f._post is not None:
            raise TypeError("per-point Diagonal noise is supported for the prior IndependentMOGP logpdf only "
                            "(reference src/ilmm.jl:41 requires Diagonal{<:Real,<:Fill})")
        if x.out_dim != len(f.fs):
            raise RuntimeError("out dim of x != out dim of f.")
        ya, na = L.Arr(y), L.Arr(s2)
        if ya.size != x.n * x.out_dim or na.size != x.n * x.out_dim:
            raise ValueError("length(y), length(diag(Sigma_y)) != n * out_dim")
        out = C.c_double()
        L.check(lib.lmm_mogp_logpdf_diag(x.carr().ptr, x.dim, x.n, ya.ptr, len(f.fs), na.ptr, L.gps_array([g.desc() for g in f.fs]),
                                         0, len(f.fs), C.byref(out)))
        return out.value
    if hasattr(y, "shape") and len(y.shape) == 2:         # logpdf(fx, Y::AbstractMatrix): one value per column
        return _logpdf_matrix(fx, y, with_regulariser)
    out = C.c_double()
    xa, ya = x.carr(), L.Arr(y)
    if isinstance(f, IndependentMOGP):
        if x.out_dim != len(f.fs):
            raise RuntimeError("out dim of x != out dim of f.")
        if ya.size != x.n * x.out_dim:
            raise ValueError("length(y) != n * out_dim")
        if f._post is not None and f._post.dense:      # latent PosteriorGP of a dense-H posterior: generic Gaussian logpdf
            L.check(lib.lmm_ilmm_post_logpdf(f._post.latent_view().ptr, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr,
                                             L.jitters((0.0, s2, 0.0)), C.byref(out)))
            return out.value
        if f._post is not None:
            return _post_logpdf(f._post, [g.desc() for g in f.fs], np.eye(len(f.fs)), np.ones(len(f.fs)), x, s2, ya, False)
        gps = L.gps_array([g.desc() for g in f.fs])
        L.check(lib.lmm_mogp_logpdf(xa.ptr, x.dim, x.n, ya.ptr, len(f.fs), C.c_double(s2), gps, 0, len(f.fs), C.byref(out)))
        return out.value
    unpack(fx)
    if ya.size != x.n * x.out_dim:
        raise ValueError("length(y) != n * out_dim")
    descs, gps = _gps_arg(f.f)
    Ua, Sa, p, m = _H_args(f.H)
    l0, l1 = f.shard
    if f.f._post is not None:
        if not f.is_oilmm:         # dense-H posterior: reference test/ilmm.jl:25
            L.check(lib.lmm_ilmm_post_logpdf(f.f._post.ptr, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr, None, C.byref(out)))
            return out.value
        return _post_logpdf(f.f._post, descs, f.H.U, f.H.S, x, s2, ya, with_regulariser)
    if f.is_oilmm:
        L.check(lib.lmm_oilmm_logpdf(xa.ptr, x.dim, x.n, ya.ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(s2), gps, l0, l1,
                                     int(with_regulariser), C.byref(out)))
    else:
        if (l0, l1) != (0, m):
            raise NotImplementedError("dense-H ILMM does not shard (SURVEY.md 8e: replicas only)")
        path = C.c_int(0)
        L.check(lib.lmm_ilmm_logpdf_ex(xa.ptr, x.dim, x.n, ya.ptr, p, Ua.ptr, m, C.c_double(s2), gps, None,
                                       int(ILMM_ALLOW_DECOUPLED), C.byref(path), C.byref(out)))
        global ILMM_LAST_PATH
        ILMM_LAST_PATH = "decoupled" if path.value else "dense"
    return out.value


def _x_buf(x):
    """Output buffer of d logpdf / d x for the inputs x (d x n column-major, on the side of x.x)."""
    return _alloc_like(x.x, x.dim * x.n)


def _x_grad(g, xv):
    """d logpdf / d x (d x n column-major, as the library writes it) in the shape and type of the inputs xv: (n,) or (d, n)."""
    if len(xv.shape) == 1:
        return g
    n, d = int(xv.shape[-1]), int(xv.shape[0])
    return g.reshape(n, d).T.contiguous() if L._is_torch(g) else np.ascontiguousarray(g.reshape(n, d).T)


def _split_train_x(gx0, train, sizes):
    """d/dx of the merged conditioning points back to one array per conditioning batch (shaped like that batch's inputs); a single
    batch gets the array itself, in the type of its inputs (the rule of _split_train_grad)."""
    if len(sizes) == 1:
        return _x_grad(gx0, train[0][0].x)
    g = np.asarray(gx0.cpu() if L._is_torch(gx0) else gx0)
    d = g.size // sum(sizes)
    g = g.reshape(-1, d)
    out, o = [], 0
    for t, nb in zip(train, sizes):
        out.append(g[o:o + nb, 0].copy() if len(t[0].x.shape) == 1 else np.ascontiguousarray(g[o:o + nb].T)); o += nb
    return out


def _gps_grads(gg, ga, m: int, d: int) -> list:
    """The latents' kernel-parameter gradients: "lengthscale" is a float for an isotropic latent and, for a per-dimension (ARD) one,
    the length-d array d logpdf / d lengthscale_k (its tag's lmm_ard_grad: the array passes multiplier 1).  An RQ latent adds
    "alpha" (its tag's lmm_kernel_tag_alpha_grad), an SHO latent "quality" (lmm_kernel_tag_quality_grad; its "lengthscale" is d / d period).  A sum latent's "variance" and "lengthscale" are those of the whole sum, and its
    "terms" hold the per-term gradients (ArdTags.sum_grad)."""
    out = []
    for l in range(m):
        if ga.ard.terms[l] is not None:
            out.append({"variance": gg[l].variance, "lengthscale": gg[l].lengthscale, "mean": gg[l].mean,
                        "terms": ga.ard.sum_grad(l, d)})
            continue
        ls = ga.ard.grad(l, d) if ga.ard.has_ard[l] else gg[l].lengthscale
        out.append({"variance": gg[l].variance, "lengthscale": ls, "mean": gg[l].mean})
        if ga.ard.has_alpha[l]:
            out[-1]["alpha"] = ga.ard.alpha_grad(l)
        if ga.ard.has_rho[l]:
            out[-1]["r"] = ga.ard.rho_grad(l)
        if ga.ard.has_decay[l]:
            out[-1]["decay"] = ga.ard.decay_grad(l)
        if ga.ard.has_quality[l]:
            out[-1]["quality"] = ga.ard.quality_grad(l)
    return out


def _dense_post_gradient(symbol: str, post, H, fs, x, s2, y, latent: bool, inputs: bool) -> dict:
    """The predictive logpdf gradient of a dense-H posterior through `symbol` (`symbol + "_x"` with inputs): the ILMM itself (y has
    p columns) or, with `latent`, its latent view (m columns).  H is the p x m matrix the conditioning batches were observed through."""
    lib = L.load()
    Ha, _, p, m = _H_args(H)
    n = x.n
    x0, s2b, y0, sizes = _merged_train(post.train, p)
    bn, bs, gb = _batch_args(s2b, sizes)
    val, gs2 = C.c_double(), C.c_double()
    gy, gH = _alloc_like(y if L._is_torch(y) else x.x, n * (m if latent else p)), np.empty(p * m)
    gy0 = _alloc_like(y0 if L._is_torch(y0) else x0.x, x0.n * p)
    gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in fs])
    gx0, gxs = (_x_buf(x0), _x_buf(x)) if inputs else (None, None)
    fn = getattr(lib, symbol + "_x" if inputs else symbol)
    L.check(fn(x0.carr().ptr, x0.dim, x0.n, bn, bs, len(sizes), L.Arr(y0).ptr, x.carr().ptr, n,
               L.Arr(y).ptr, p, Ha.ptr, m, C.c_double(s2), ga,
               None, C.byref(val), L.Arr(gy0, True).ptr, L.Arr(gy, True).ptr, gb, C.byref(gs2),
               L.Arr(gH, True).ptr, gg, *((L.Arr(gx0, True).ptr, L.Arr(gxs, True).ptr) if inputs else ())))
    out = {"value": val.value, "y": gy, "y_train": _split_train_grad(gy0, sizes, p), "sigma2": gs2.value,
           "sigma2_train": _train_noise_grad(gb, s2b), "H": gH.reshape(m, p).T.copy(),
           "gps": _gps_grads(gg, ga, m, x.dim)}
    if inputs:
        out.update(x=_x_grad(gxs, x.x), x_train=_split_train_x(gx0, post.train, sizes))
    return out


def logpdf_and_gradient(fx: FiniteGP, y, with_regulariser: bool = True, inputs: bool = False) -> dict:
    """Value and gradient of logpdf(fx, y) -- what `Zygote.gradient(logpdf, fx, y)` differentiates in the reference's tests
    (test/oilmm.jl:31-32, test/ilmm.jl:31-32, test/independent_mogp.jl:65-66).

      prior OILMM / IndependentMOGP : {"value", "y", "sigma2", "S", "U", "gps": [{"variance","lengthscale","mean"}, ...]}
      prior dense-H ILMM            : {"value", "y", "sigma2", "H", "gps"}
      posterior dense-H ILMM        : as the posterior OILMM below with "H" in place of "S", "U" (test/ilmm.jl:32)
      posterior OILMM / MOGP        : fx = posterior(f(x, s2), y0)(xs, s2s); TOTAL derivatives of the predictive logpdf through the
                                      posterior: {"value", "y" (= d/d ys), "y_train", "sigma2" (= d/d s2s), "sigma2_train", "S", "U", "gps"}
                                      After sequential conditioning (equal noise variance per batch) "y_train" is a LIST with one
                                      by-outputs vector per conditioning batch, while "sigma2_train" stays ONE number: the derivative
                                      with respect to the variance the batches share (= the sum of the per-batch derivatives).
    inputs=True adds the gradient with respect to the input locations (reference: Zygote differentiates through fx.x), shaped and
    typed like the inputs ((n,) or (d, n); NumPy or torch): prior models gain "x"; posterior models gain "x" (d/d xs, the test inputs)
    and "x_train" (d/d the conditioning inputs: a list with one array per batch after sequential conditioning, as "y_train").  It
    costs one more read of each latent's K^-1; d <= 32.  With inputs=False the call and its keys are unchanged.
    A y with NaN (missing observations, prior OILMM only): {"value", "y" (0 at the missing entries), "sigma2", "gps"}; "S", "U" and
    inputs=True raise NotImplementedError.
    Partial sums over the latent shard."""
    _refuse_sparse(fx, "logpdf_and_gradient")
    _refuse_sho_dims(fx, "logpdf_and_gradient")
    if inputs:
        _refuse_sho(fx, "logpdf_and_gradient(inputs=True)")
    L.ensure_init()
    lib = L.load()
    if _has_nan(y):
        return _NoMixingGradient(_gradient_missing(fx, y, with_regulariser, inputs))
    f, x, s2 = fx.f, fx.x, fx.sigma2
    mogp = isinstance(f, IndependentMOGP)
    post = f._post if mogp else (f.f._post if isinstance(f, ILMM) else None)
    if not mogp and not isinstance(f, ILMM):
        raise TypeError("logpdf_and_gradient needs an ILMM / OILMM / IndependentMOGP FiniteGP")
    if mogp and post is not None and post.dense:
        # logpdf(get_latent_gp(posterior(ilmm(x, s2), y))(xs, s2s), zs): the coupled latent PosteriorGP of a dense-H posterior (reference
        # src/ilmm.jl:39 on the ILMM of :196-197).  Joint density of the conditioning batches (observed through H) and the latent test
        # block (observed through [I; 0]) minus the marginal of the batches: lmm_ilmm_post_latent_logpdf_grad_seq.
        if post.latent or post.mix is None:
            raise NotImplementedError("gradient of the latent view after conditioning ON latent observations is not built")
        m = len(f.fs)
        if x.out_dim != m:
            raise RuntimeError("out dim of x != out dim of f.")
        return _dense_post_gradient("lmm_ilmm_post_latent_logpdf_grad_seq", post, post.mix, f.fs, x, s2, y, True, inputs)
    if not mogp and not f.is_oilmm:
        unpack(fx)
        if post is not None:          # reference test/ilmm.jl:32: gradient(logpdf, pi, y_test) on the dense-H posterior
            return _dense_post_gradient("lmm_ilmm_post_logpdf_grad_seq", post, f.H, f.f.fs, x, s2, y, False, inputs)
        Ha, _, p, m = _H_args(f.H)
        n = x.n
        val, gs2 = C.c_double(), C.c_double()
        gy, gH = _alloc_like(y if L._is_torch(y) else x.x, n * p), np.empty(p * m)
        gg, ga = (L.GpGradT * m)(), L.gps_array([g.desc() for g in f.f.fs])
        gx = _x_buf(x) if inputs else None
        fn = lib.lmm_ilmm_logpdf_grad_x if inputs else lib.lmm_ilmm_logpdf_grad
        L.check(fn(x.carr().ptr, x.dim, n, L.Arr(y).ptr, p, Ha.ptr, m, C.c_double(s2),
                   ga, None, C.byref(val), L.Arr(gy, True).ptr,
                   C.byref(gs2), L.Arr(gH, True).ptr, gg, *((L.Arr(gx, True).ptr,) if inputs else ())))
        out = {"value": val.value, "y": gy, "sigma2": gs2.value, "H": gH.reshape(m, p).T.copy(),
               "gps": _gps_grads(gg, ga, m, x.dim)}
        if inputs:
            out["x"] = _x_grad(gx, x.x)
        return out
    if mogp:                      # gradient(logpdf, fx, y) on an IndependentMOGP (reference test/independent_mogp.jl:65-66):
        m = p = len(f.fs)         # the OILMM with U = I, S = 1 (regulariser identically 0, so it is skipped)
        if x.out_dim != m:
            raise RuntimeError("out dim of x != out dim of f.")
        Ua, Sa, descs, shard, with_regulariser = L.Arr(L.colmajor(np.eye(m))), L.Arr(np.ones(m)), [g.desc() for g in f.fs], (0, m), False
    else:
        unpack(fx)
        Ua, Sa, p, m = _H_args(f.H)
        descs, shard = [g.desc() for g in f.f.fs], f.shard
    n = x.n
    val, gs2 = C.c_double(), C.c_double()
    gy, gS, gU = _alloc_like(y if L._is_torch(y) else x.x, n * p), np.empty(m), np.empty(p * m)
    gg, ga = (L.GpGradT * m)(), L.gps_array(descs)
    out = {}
    gx = _x_buf(x) if inputs else None
    if post is None:
        fn = lib.lmm_oilmm_logpdf_grad_x if inputs else lib.lmm_oilmm_logpdf_grad
        L.check(fn(x.carr().ptr, x.dim, n, L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(s2),
                   ga, shard[0], shard[1], int(with_regulariser), C.byref(val),
                   L.Arr(gy, True).ptr, C.byref(gs2), L.Arr(gS, True).ptr, L.Arr(gU, True).ptr, gg,
                   *((L.Arr(gx, True).ptr,) if inputs else ())))
    else:
        x0, s2b, y0, sizes = _merged_train(post.train, p)
        bn, bs, gb = _batch_args(s2b, sizes)
        gy0 = _alloc_like(y0 if L._is_torch(y0) else x0.x, x0.n * p)
        gx0 = _x_buf(x0) if inputs else None
        fn = lib.lmm_oilmm_post_logpdf_grad_seq_x if inputs else lib.lmm_oilmm_post_logpdf_grad_seq
        L.check(fn(x0.carr().ptr, x0.dim, x0.n, bn, bs, len(sizes), L.Arr(y0).ptr, x.carr().ptr, n,
                   L.Arr(y).ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(s2), ga, shard[0],
                   shard[1], int(with_regulariser), C.byref(val), L.Arr(gy0, True).ptr,
                   L.Arr(gy, True).ptr, gb, C.byref(gs2), L.Arr(gS, True).ptr, L.Arr(gU, True).ptr, gg,
                   *((L.Arr(gx0, True).ptr, L.Arr(gx, True).ptr) if inputs else ())))
        out.update(y_train=_split_train_grad(gy0, sizes, p), sigma2_train=_train_noise_grad(gb, s2b))
        if inputs:
            out["x_train"] = _split_train_x(gx0, post.train, sizes)
    if inputs:
        out["x"] = _x_grad(gx, x.x)
    out.update({"value": val.value, "y": gy, "sigma2": gs2.value,
                "gps": _gps_grads(gg, ga, m, x.dim)})
    if not mogp:
        out["S"], out["U"] = gS, gU.reshape(m, p).T.copy()
    return out


def _logpdf_matrix(fx: FiniteGP, Y, with_regulariser: bool = True) -> np.ndarray:
    """logpdf(fx, Y) for Y of shape (n*p, ncol): ONE factorisation per latent, the columns ride as extra right-hand sides."""
    lib = L.load()
    f, x, s2 = fx.f, fx.x, fx.sigma2
    ncol = int(Y.shape[1])
    Yc = Y.T.contiguous() if L._is_torch(Y) else np.ascontiguousarray(np.asarray(Y, dtype=np.float64).T)   # column-major image
    fpost = f._post if isinstance(f, IndependentMOGP) else f.f._post
    if fpost is not None:          # posterior models (TestUtils on po(x*, s2): reference test/oilmm.jl:36, test/ilmm.jl:36): the columns
        return np.array([logpdf(fx, Yc[c], with_regulariser) for c in range(ncol)])      # are evaluated one by one on the handle
    if isinstance(f, IndependentMOGP):
        m = len(f.fs)
        descs, Ua, Sa, p, shard, post = [g.desc() for g in f.fs], L.Arr(L.colmajor(np.eye(m))), L.Arr(np.ones(m)), m, (0, m), f._post
        with_regulariser = False                   # U = I, S = 1, p == m: the regulariser is identically 0 only up to its
        s2_eff = s2                                # log S = 0 and (p-m) = 0 terms; skip it exactly
    else:
        unpack(fx)
        if not f.is_oilmm:                         # dense H: one (mn) x (mn) factorisation, the columns ride it
            Ha, _, p, m = _H_args(f.H)
            if x.out_dim != p:
                raise RuntimeError("out dim of x != out dim of f.")
            out = np.empty(ncol)
            L.check(lib.lmm_ilmm_logpdf_multi(x.carr().ptr, x.dim, x.n, L.Arr(Yc).ptr, p, ncol, Ha.ptr, m, C.c_double(s2),
                                              L.gps_array([g.desc() for g in f.f.fs]), None, L.Arr(out, True).ptr))
            return out
        descs, (Ua, Sa, p, m), shard, post, s2_eff = [g.desc() for g in f.f.fs], _H_args(f.H), f.shard, f.f._post, s2
    if x.out_dim != p:
        raise RuntimeError("out dim of x != out dim of f.")
    out = np.empty(ncol)
    L.check(lib.lmm_oilmm_logpdf_multi(x.carr().ptr, x.dim, x.n, L.Arr(Yc).ptr, p, ncol, Ua.ptr, Sa.ptr, m, C.c_double(s2_eff),
                                       L.gps_array(descs), shard[0], shard[1], int(with_regulariser), L.Arr(out, True).ptr))
    return out


def _post_logpdf(post: _PostHandle, descs, U, S, x, s2, ya, with_reg) -> float:
    lib = L.load()
    out = C.c_double()
    Ua, Sa = L.Arr(L.colmajor(U)), L.Arr(S)
    xa = x.carr()
    L.check(lib.lmm_oilmm_post_logpdf(post.ptr, Ua.ptr, Sa.ptr, U.shape[0], U.shape[1], C.c_double(s2), xa.ptr, x.dim,
                                      x.n, ya.ptr, int(with_reg), C.byref(out)))
    return out.value


def _more_train(post: "_PostHandle", x, s2, y):
    """Conditioning batches of posterior(po(x, s2), y): those of `po` plus this one (None if `po` does not know its own)."""
    return None if post.train is None else post.train + [(x, s2, y)]


def posterior(fx: FiniteGP, y):
    """posterior(fx, y): reference src/oilmm.jl:116-134 (returns ILMM(independent_mogp(posteriors), H) -- again
    an OILMM with the same H) and src/independent_mogp.jl:119-126."""
    _refuse_sparse(fx, "posterior (conditioning on further data)")
    _refuse_sho_dims(fx, "posterior (conditioning on further data)")
    L.ensure_init()
    lib = L.load()
    if _has_nan(y):
        return _posterior_missing(fx, y)
    f, x, s2 = fx.f, fx.x, fx.sigma2
    if isinstance(x, MOInputIsotopicByFeatures):
        return posterior(FiniteGP(f, x.by_outputs(), s2), _reorder(y, x.n, x.out_dim, True))
    xa, ya = x.carr(), L.Arr(y)
    handle = C.c_void_p()
    if isinstance(f, IndependentMOGP):
        m = len(f.fs)
        if f._post is not None and f._post.dense:      # posterior(f_latent(x2, s2), y2) on the coupled latent PosteriorGP
            L.check(lib.lmm_ilmm_post_condition(f._post.latent_view().ptr, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr,
                                                L.jitters((0.0, s2, 0.0)), C.byref(handle)))
            return IndependentMOGP(f.fs, _PostHandle(handle, 0, m, dense=True, latent=True))
        if f._post is not None:        # sequential conditioning: posterior(po(x2, s2), y2)
            Ui, Si = L.Arr(L.colmajor(np.eye(m))), L.Arr(np.ones(m))
            L.check(lib.lmm_post_condition(f._post.ptr, Ui.ptr, Si.ptr, m, m, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr,
                                           C.byref(handle)))
            return IndependentMOGP(f.fs, _PostHandle(handle, 0, m, train=_more_train(f._post, x, s2, y)))
        gps = L.gps_array([g.desc() for g in f.fs])
        L.check(lib.lmm_mogp_posterior_create(xa.ptr, x.dim, x.n, ya.ptr, m, C.c_double(s2), gps, 0, m, C.byref(handle)))
        return IndependentMOGP(f.fs, _PostHandle(handle, 0, m, train=(x, s2, y)))
    unpack(fx)
    Ua, Sa, p, m = _H_args(f.H)
    l0, l1 = f.shard
    if f.f._post is not None:          # sequential conditioning of a posterior OILMM (same H: reference src/oilmm.jl:133)
        if not f.is_oilmm:         # dense-H posterior: both projected data sets condition the prior (reference src/ilmm.jl:184-198)
            L.check(lib.lmm_ilmm_post_condition(f.f._post.ptr, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr, None, C.byref(handle)))
            return ILMM(IndependentMOGP(f.f.fs, _PostHandle(handle, l0, l1, dense=True, train=_more_train(f.f._post, x, s2, y), mix=f.H)), f.H,
                        shard=f.shard)
        L.check(lib.lmm_post_condition(f.f._post.ptr, Ua.ptr, Sa.ptr, p, m, C.c_double(s2), xa.ptr, x.dim, x.n, ya.ptr,
                                       C.byref(handle)))
        return ILMM(IndependentMOGP(f.f.fs, _PostHandle(handle, l0, l1, train=_more_train(f.f._post, x, s2, y))), f.H, shard=f.shard)
    gps = L.gps_array([g.desc() for g in f.f.fs])
    if f.is_oilmm:
        L.check(lib.lmm_oilmm_posterior_create(xa.ptr, x.dim, x.n, ya.ptr, p, Ua.ptr, Sa.ptr, m, C.c_double(s2), gps, l0,
                                               l1, C.byref(handle)))
    else:
        L.check(lib.lmm_ilmm_posterior_create(xa.ptr, x.dim, x.n, ya.ptr, p, Ua.ptr, m, C.c_double(s2), gps, None,
                                              C.byref(handle)))
    return ILMM(IndependentMOGP(f.f.fs, _PostHandle(handle, l0, l1, dense=not f.is_oilmm, train=(x, s2, y), mix=None if f.is_oilmm else f.H)),
                f.H, shard=f.shard)


def mean_and_var(fx: FiniteGP, add_noise: bool = True):
    """mean_and_var(fx): reference src/oilmm.jl:57-76 (OILMM) and src/independent_mogp.jl:50,55.  For a sharded
    model the outputs are this shard's partial sums (add_noise only on one rank)."""
    if _sparse_post(fx) is not None:
        return _sparse_mean_and_var(fx, add_noise, True)
    _refuse_sho_dims(fx, "mean_and_var")
    L.ensure_init()
    lib = L.load()
    f, x, s2 = fx.f, fx.x, fx.sigma2
    if isinstance(x, MOInputIsotopicByFeatures):          # reference src/independent_mogp.jl:169-215
        mo, vo = mean_and_var(FiniteGP(f, x.by_outputs(), s2), add_noise)
        return _reorder(mo, x.n, x.out_dim, False), _reorder(vo, x.n, x.out_dim, False)
    xa = x.carr()
    if isinstance(f, IndependentMOGP):
        m = len(f.fs)
        if x.out_dim != m:
            raise RuntimeError("out dim of x != out dim of f.")
        mean, var = _alloc_like(x.x, x.n * m), _alloc_like(x.x, x.n * m)
        ma, va = L.Arr(mean, True), L.Arr(var, True)
        if f._post is not None and f._post.dense:      # coupled latent PosteriorGP: diag of its joint covariance + sigma2
            L.check(lib.lmm_ilmm_post_mean_and_var(f._post.latent_view().ptr, C.c_double(s2), xa.ptr, x.dim, x.n,
                                                   L.jitters((0.0, s2, 0.0)), ma.ptr, va.ptr))
            return mean, var
        post = f._post.ptr if f._post is not None else None
        gps = L.gps_array([g.desc() for g in f.fs])
        L.check(lib.lmm_latent_marginals(post, gps, m, xa.ptr, x.dim, x.n, ma.ptr, va.ptr))
        return mean, var + s2                      # var(f, x) + Sigma_y diagonal
    unpack(fx)
    Ua, Sa, p, m = _H_args(f.H)
    if not f.is_oilmm and f.f._post is not None:
        # dense-H posterior: coupled latents (reference src/ilmm.jl:108-129 on the PosteriorGP of :196-197)
        mean, var = _alloc_like(x.x, x.n * p), _alloc_like(x.x, x.n * p)
        ma, va = L.Arr(mean, True), L.Arr(var, True)
        L.check(lib.lmm_ilmm_post_mean_and_var(f.f._post.ptr, C.c_double(s2), xa.ptr, x.dim, x.n, None, ma.ptr, va.ptr))
        return mean, var
    l0, l1 = f.shard
    mean, var = _alloc_like(x.x, x.n * p), _alloc_like(x.x, x.n * p)
    ma, va = L.Arr(mean, True), L.Arr(var, True)
    post = f.f._post.ptr if f.f._post is not None else None
    gps = L.gps_array([g.desc() for g in f.f.fs])
    # dense-H prior: latents are independent, so V = abs2.(H) * V_latent + s2 exactly as in the OILMM form (S == NULL)
    L.check(lib.lmm_oilmm_mean_and_var(post, gps, Ua.ptr, Sa.ptr if Sa is not None else None, p, m, l0, l1,
                                       C.c_double(s2), int(add_noise), xa.ptr, x.dim, x.n, None, ma.ptr, va.ptr))
    return mean, var


def mean_and_var_vjp(fx: FiniteGP, dmean=None, dvar=None, add_noise: bool = True) -> dict:
    """Pullback of mean_and_var(fx, add_noise) for the cotangents dmean, dvar (shaped like its outputs; None = zero):
    {"x": d/d fx.x.x (shaped and typed like it), "sigma2": d/d sigma2}.  dvar=None takes no triangular solve (the pullback of mean).
    OILMM and IndependentMOGP priors and posteriors (sequentially conditioned and sharded ones included: a shard's partial sum) and
    the dense-H prior, by lmm_oilmm_mean_and_var_grad_xs.  The dense-H posterior and the coupled latent view raise NotImplementedError."""
    _refuse_sparse(fx, "mean_and_var_vjp")
    _refuse_sho(fx, "mean_and_var_vjp")
    L.ensure_init()
    lib = L.load()
    f, x, s2 = fx.f, fx.x, fx.sigma2
    if isinstance(x, MOInputIsotopicByFeatures):          # mean_and_var permutes by-outputs results: permute the cotangents back
        n, p = x.n, x.out_dim
        dm = None if dmean is None else _reorder(dmean, n, p, True)
        dv = None if dvar is None else _reorder(dvar, n, p, True)
        return mean_and_var_vjp(FiniteGP(f, x.by_outputs(), s2), dm, dv, add_noise)
    if isinstance(f, IndependentMOGP):
        m = len(f.fs)
        if x.out_dim != m:
            raise RuntimeError("out dim of x != out dim of f.")
        if f._post is not None and f._post.dense:
            raise NotImplementedError("gradients of the predictive marginals of a coupled (dense-H) latent posterior are not served")
        Ua, Sa, p, post, mogp, (l0, l1), noise = L.Arr(L.colmajor(np.eye(m))), None, m, f._post, f, (0, m), True   # var + Sigma_y
    else:
        unpack(fx)
        if not f.is_oilmm and f.f._post is not None:
            raise NotImplementedError("gradients of the predictive marginals of a dense-H posterior (coupled latents) are not served")
        Ua, Sa, p, m = _H_args(f.H)
        post, mogp, (l0, l1), noise = f.f._post, f.f, f.shard, add_noise
    xa = x.carr()
    g = _x_buf(x)
    dm = L.Arr(dmean) if dmean is not None else None
    dv = L.Arr(dvar) if dvar is not None else None
    for a in (dm, dv):
        if a is not None and a.size != x.n * p:
            raise ValueError(f"cotangent has {a.size} entries, mean_and_var returns {x.n * p}")
    L.check(lib.lmm_oilmm_mean_and_var_grad_xs(post.ptr if post is not None else None, L.gps_array([g_.desc() for g_ in mogp.fs]),
                                               Ua.ptr, Sa.ptr if Sa is not None else None, p, m, l0, l1, xa.ptr, x.dim, x.n,
                                               dm.ptr if dm is not None else None, dv.ptr if dv is not None else None,
                                               L.Arr(g, True).ptr))
    gs2 = float(dvar.sum()) if (noise and dvar is not None) else 0.0
    return {"x": _x_grad(g, x.x), "sigma2": gs2}


def mean_and_cov(fx: FiniteGP):
    """mean_and_cov(fx): reference src/ilmm.jl:132-139 (ILMM/OILMM) and AbstractGPs' generic form over
    src/independent_mogp.jl:60-63 (IndependentMOGP).  Returns (mean, C) with C (p n) x (p n), by-outputs order."""
    _refuse_sparse(fx, "mean_and_cov")
    _refuse_sho_dims(fx, "mean_and_cov")
    L.ensure_init()
    lib = L.load()
    f, x, s2 = fx.f, fx.x, fx.sigma2
    xa = x.carr()
    if isinstance(f, IndependentMOGP):
        m = len(f.fs)
        if x.out_dim != m:
            raise RuntimeError("out dim of x != out dim of f.")
        if f._post is not None and f._post.dense:      # coupled latent PosteriorGP: its joint covariance + sigma2 I
            n = x.n
            mean, cov = np.empty(n * m), np.empty((n * m) * (n * m))
            L.check(lib.lmm_ilmm_post_mean_and_cov(f._post.latent_view().ptr, C.c_double(s2), xa.ptr, x.dim, n,
                                                   L.jitters((0.0, s2, 0.0)), L.Arr(mean, True).ptr, L.Arr(cov, True).ptr))
            return mean, cov.reshape(n * m, n * m).T
        Ua, Sa, p, post, descs, shard = L.Arr(L.colmajor(np.eye(m))), None, m, f._post, [g.desc() for g in f.fs], (0, m)
        jit = L.jitters((1e-9, 0.0, 0.0))          # cov(f, x) + Sigma_y: no latent jitter for a bare MOGP
    else:
        unpack(fx)
        if not f.is_oilmm and f.f._post is not None:      # coupled latents: reference src/ilmm.jl:132-139 on the PosteriorGP
            n, p = x.n, f.H.shape[0]
            mean, cov = np.empty(n * p), np.empty((n * p) * (n * p))
            L.check(lib.lmm_ilmm_post_mean_and_cov(f.f._post.ptr, C.c_double(s2), xa.ptr, x.dim, n, None, L.Arr(mean, True).ptr,
                                                   L.Arr(cov, True).ptr))
            return mean, cov.reshape(n * p, n * p).T
        Ua, Sa, p, m = _H_args(f.H)
        post, descs, shard, jit = f.f._post, [g.desc() for g in f.f.fs], f.shard, None
    n = x.n
    mean, cov = np.empty(n * p), np.empty((n * p) * (n * p))
    L.check(lib.lmm_lmm_mean_and_cov(post.ptr if post is not None else None, L.gps_array(descs), Ua.ptr,
                                     Sa.ptr if Sa is not None else None, p, m, shard[0], shard[1], C.c_double(s2), 1, xa.ptr,
                                     x.dim, n, jit, L.Arr(mean, True).ptr, L.Arr(cov, True).ptr))
    return mean, cov.reshape(n * p, n * p).T       # column-major -> (row, col); symmetric


def cov(fx, x=None, y=None):
    """cov(fx): reference src/ilmm.jl:147.
    cov(f::IndependentMOGP, x, y): the two-input cross-covariance, reference src/independent_mogp.jl:66-71 (both inputs by outputs)
    and :184-215 (either one MOInputIsotopicByFeatures); cov(f::IndependentMOGP, x) = cov(f, x, x) (:60-63, :176-181).  Prior or
    (independent) posterior latents; (m n) x (m n2), one lmm_mogp_cross_cov call."""
    _refuse_sparse(fx, "cov")
    _refuse_sho_dims(fx, "cov", *((getattr(fx, "x", None),) if x is None else (x, x if y is None else y)))
    if isinstance(fx, IndependentMOGP):
        if x is None:
            raise TypeError("cov(f::IndependentMOGP, x[, y]) needs the inputs")
        return _mogp_cross_cov(fx, x, x if y is None else y)
    if x is not None or y is not None:
        raise TypeError("cov(f, x, y) is defined for an IndependentMOGP (reference src/independent_mogp.jl:66-71)")
    return mean_and_cov(fx)[1]


def _mogp_cross_cov(f: IndependentMOGP, x, y) -> np.ndarray:
    if isinstance(f._post, _SparsePostHandle):      # its pointer is no lmm_post_t*: never hand it to an entry point that takes one
        raise NotImplementedError("cov is not served on an inducing-point posterior (approx_posterior): it answers mean_and_var, "
                                  "mean, var and marginals")
    L.ensure_init()
    m = len(f.fs)
    if x.out_dim != m or y.out_dim != m:
        raise RuntimeError("out dim of x != out dim of f.")
    if f._post is not None and f._post.dense:
        raise NotImplementedError("cov(f, x, y) of the coupled latent PosteriorGP of a dense-H posterior is not built")
    xb = x.by_outputs() if isinstance(x, MOInputIsotopicByFeatures) else x
    yb = y.by_outputs() if isinstance(y, MOInputIsotopicByFeatures) else y
    if xb.dim != yb.dim:
        raise ValueError("x and y have different input dimensions")
    n, n2 = xb.n, yb.n
    out = np.empty((m * n) * (m * n2))
    post = f._post.ptr if f._post is not None else None
    L.check(L.load().lmm_mogp_cross_cov(post, L.gps_array([g.desc() for g in f.fs]), m, 0, m, xb.carr().ptr, xb.dim, n,
                                        int(isinstance(x, MOInputIsotopicByFeatures)), yb.carr().ptr, n2,
                                        int(isinstance(y, MOInputIsotopicByFeatures)), L.Arr(out, True).ptr))
    return out.reshape(m * n2, m * n).T          # column-major (m n) x (m n2) -> (row, col)


def mean(fx: FiniteGP):
    """reference src/ilmm.jl:142 (mean_and_var(fx)[1]).  For an OILMM (prior or posterior, by-outputs inputs) the means alone
    are computed -- mu + K(x*, x) alpha per latent, no triangular solve for variances that would be discarded."""
    f, x = fx.f, fx.x
    if _sparse_post(fx) is not None:
        return _sparse_mean_and_var(fx, False, False)[0]
    _refuse_sho_dims(fx, "mean")
    if isinstance(f, ILMM) and isinstance(x, MOInputIsotopicByOutputs) and (f.is_oilmm or f.f._post is None):
        L.ensure_init()
        unpack(fx)
        Ua, Sa, p, m = _H_args(f.H)
        l0, l1 = f.shard
        out = _alloc_like(x.x, x.n * p)
        post = f.f._post.ptr if f.f._post is not None else None
        L.check(L.load().lmm_oilmm_mean_and_var(post, L.gps_array([g.desc() for g in f.f.fs]), Ua.ptr,
                                               Sa.ptr if Sa is not None else None, p, m, l0, l1, C.c_double(fx.sigma2), 0,
                                               x.carr().ptr, x.dim, x.n, None, L.Arr(out, True).ptr, None))
        return out
    return mean_and_var(fx)[0]


def var(fx: FiniteGP):
    """reference src/ilmm.jl:145."""
    return mean_and_var(fx)[1]


def marginals(fx: FiniteGP) -> Normal:
    """AbstractGPs.marginals(fx) = Normal.(mean, sqrt.(var)) (vectorised)."""
    m, v = mean_and_var(fx)
    return Normal(m, v ** 0.5)


class DeviceNormals:
    """Standard normals generated on the GPU (lmm_normals: Philox4x32-10 + Box-Muller, Float64).  Pass it to `rand` in place of
    a numpy Generator when the reference's host random stream is not needed: the draw ORDER of the reference is kept (latent
    normals, then noise normals), the buffers never leave the device, and the sample comes back as a device tensor."""

    def __init__(self, seed: int):
        self.seed, self.stream = int(seed), 0

    def standard_normal(self, count: int):
        import torch
        L.ensure_init()
        out = torch.empty(int(count), dtype=torch.float64, device="cuda")
        # through Arr, so that the library's stream waits for what torch has queued: the allocator may hand out memory that work still
        # in flight on torch's stream (the temporaries of a sort, say) was using
        L.check(L.load().lmm_normals(C.c_ulonglong(self.seed), C.c_ulonglong(self.stream), C.c_size_t(int(count)),
                                     L.Arr(out, True).ptr))
        self.stream += 1
        return out


def _empty_for(rng, *shape):
    """Result / staging buffer on the side the normals live on."""
    if isinstance(rng, DeviceNormals):
        import torch
        return torch.empty(*shape, dtype=torch.float64, device="cuda")
    return np.empty(shape)


def rand(rng, fx: FiniteGP, N: Optional[int] = None, jitters=None, add_noise: bool = True):
    """rand(rng, fx[, N]): reference src/oilmm.jl:40-54, src/ilmm.jl:78-92, src/independent_mogp.jl:83-96.
    `rng` is a numpy Generator; standard normals are drawn on the host in the reference's order (m blocks of n
    latent normals, then n*p noise normals) and handed to the device, as the Julia shim does with randn(rng, ...)."""
    _refuse_sparse(fx, "rand")
    _refuse_sho_dims(fx, "rand")
    f, x, s2 = fx.f, fx.x, fx.sigma2
    if isinstance(x, MOInputIsotopicByFeatures):          # reference src/independent_mogp.jl:217-220
        s = rand(rng, FiniteGP(f, x.by_outputs(), s2), N, jitters, add_noise)
        if N is None:
            return _reorder(s, x.n, x.out_dim, False)
        return np.stack([_reorder(np.ascontiguousarray(s[:, q]), x.n, x.out_dim, False) for q in range(N)], axis=1)
    L.ensure_init()
    lib = L.load()
    xa = x.carr()
    n = x.n
    if isinstance(f, IndependentMOGP) and f._post is not None and f._post.dense:
        # rand(rng, f_latent(x, s2)) on the coupled latent PosteriorGP of a dense-H posterior: AbstractGPs' generic
        # mean + chol(cov + s2 I).U' z, one draw of m n normals per sample (N samples = N repeats, as the reference does)
        m = len(f.fs)
        view = f._post.latent_view()

        def one():
            z = rng.standard_normal(m * n)
            o = _empty_for(rng, n * m)
            L.check(lib.lmm_ilmm_post_rand(view.ptr, C.c_double(s2), 0, xa.ptr, x.dim, n, L.Arr(z).ptr, None,
                                           L.jitters((0.0, s2, 0.0)), L.Arr(o, True).ptr))
            return o
        if N is None:
            return one()
        cols = [one() for _ in range(N)]
        import torch
        return torch.stack(cols, dim=1) if L._is_torch(cols[0]) else np.stack(cols, axis=1)
    if N is not None:
        # reference src/ilmm.jl:90-92 / src/independent_mogp.jl:92-96 repeat the whole call N times; here ONE factorisation
        # serves all N samples (lmm_lmm_rand_multi).  Normals are still drawn sample by sample in the reference's order.
        if isinstance(f, IndependentMOGP):
            m = p = len(f.fs)
            Ua, Sa, descs, post, shard, jit, noise = L.Arr(L.colmajor(np.eye(m))), None, [g.desc() for g in f.fs], f._post, (0, m), \
                L.jitters((1e-9, s2, s2)), 0
        else:
            unpack(fx)
            Ua, Sa, p, m = _H_args(f.H)
            descs, post, shard, jit, noise = [g.desc() for g in f.f.fs], f.f._post, f.shard, L.jitters(jitters), int(add_noise)
        z = _empty_for(rng, N, m * n); eps = _empty_for(rng, N, n * p)
        for q in range(N):
            z[q] = rng.standard_normal(m * n)
            if not isinstance(f, IndependentMOGP):
                eps[q] = rng.standard_normal(n * p)
        out = _empty_for(rng, N, n * p)
        L.check(lib.lmm_lmm_rand_multi(post.ptr if post is not None else None, L.gps_array(descs), Ua.ptr,
                                       Sa.ptr if Sa is not None else None, p, m, shard[0], shard[1], C.c_double(s2), noise, xa.ptr,
                                       x.dim, n, N, L.Arr(z).ptr, L.Arr(eps).ptr if noise else None, jit, L.Arr(out, True).ptr))
        return out.T
    if isinstance(f, IndependentMOGP):
        # vcat(rand(rng, f_l(x, s2))): latent jitter = s2, H = I, no extra noise term
        m = len(f.fs)
        z = rng.standard_normal(m * n)
        out = _empty_for(rng, n * m)
        gps = L.gps_array([g.desc() for g in f.fs])
        post = f._post.ptr if f._post is not None else None
        Ua = L.Arr(L.colmajor(np.eye(m)))
        jit = L.jitters((1e-9, s2, s2))
        L.check(lib.lmm_lmm_rand(post, gps, Ua.ptr, None, m, m, 0, m, C.c_double(s2), 0, xa.ptr, x.dim, n, L.Arr(z).ptr,
                                 None, jit, L.Arr(out, True).ptr))
        return out
    unpack(fx)
    Ua, Sa, p, m = _H_args(f.H)
    z = rng.standard_normal(m * n)
    eps = rng.standard_normal(n * p)
    out = _empty_for(rng, n * p)
    if not f.is_oilmm and f.f._post is not None:      # dense-H posterior: coupled latents, reference src/ilmm.jl:78-87
        L.check(lib.lmm_ilmm_post_rand(f.f._post.ptr, C.c_double(s2), int(add_noise), xa.ptr, x.dim, n, L.Arr(z).ptr,
                                       L.Arr(eps).ptr, L.jitters(jitters), L.Arr(out, True).ptr))
        return out
    gps = L.gps_array([g.desc() for g in f.f.fs])
    post = f.f._post.ptr if f.f._post is not None else None
    l0, l1 = f.shard
    L.check(lib.lmm_lmm_rand(post, gps, Ua.ptr, Sa.ptr if Sa is not None else None, p, m, l0, l1, C.c_double(s2),
                             int(add_noise), xa.ptr, x.dim, n, L.Arr(z).ptr, L.Arr(eps).ptr, L.jitters(jitters),
                             L.Arr(out, True).ptr))
    return out
