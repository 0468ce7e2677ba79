"""ctypes binding of liblmm_hip.so (include/lmm_hip.h).  No fallback: if the HIP library or a GPU is
missing every compute entry point raises -- the product path never routes through a CPU implementation."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LMM_HIP_LIB (the variable the Julia shim reads too): another build of the library, for same-box A/B runs of two kernel versions
LIB_PATH = os.environ.get("LMM_HIP_LIB") or os.path.join(_HERE, "liblmm_hip.so")

LMM_OK, LMM_ERR_DIM, LMM_ERR_NOT_ORTHOGONAL, LMM_ERR_NOT_PD, LMM_ERR_HIP, LMM_ERR_ARG, LMM_ERR_UNSUPPORTED, LMM_ERR_RCCL = range(8)
UNIQUE_ID_BYTES = 128
KERNEL_KINDS = {"se": 0, "matern32": 1, "matern52": 2, "matern12": 3, "rq": 4}
KERNEL_SUM = 5              # LMM_KERNEL_SUM: a sum latent (descriptor kind "sum"), not a base kind
SUM_MAX_TERMS = 4
KERNEL_PERIODIC = 7         # LMM_KERNEL_PERIODIC: a base kind outside lmm_kernel_kind (descriptor kind "periodic")
KERNEL_LOCALLY_PERIODIC = 10     # LMM_KERNEL_LOCALLY_PERIODIC: SE x Periodic as one base kind (descriptor kind "locally_periodic")
KERNEL_SHO = 12             # LMM_KERNEL_SHO: the damped oscillator, a base kind outside lmm_kernel_kind (descriptor kind "sho"; d = 1 only)

# Every symbol include/lmm_hip.h declares (tests/test_abi.py checks the library exports each one).
SYMBOLS = [
    "lmm_init", "lmm_shutdown", "lmm_last_error_string", "lmm_last_error_detail", "lmm_device_synchronize", "lmm_release_cached_memory",
    "lmm_stream_wait_caller", "lmm_ard_create", "lmm_ard_destroy", "lmm_ard_grad", "lmm_kernel_tag_create", "lmm_kernel_tag_alpha_grad", "lmm_kernel_tag_create_periodic", "lmm_kernel_tag_rho_grad", "lmm_kernel_tag_create_locally_periodic", "lmm_kernel_tag_decay_grad", "lmm_kernel_tag_create_sho", "lmm_kernel_tag_quality_grad", "lmm_kernel_sum_create", "lmm_kernel_sum_grad", "lmm_kernel_sum_create_statespace", "lmm_set_compute_dtype", "lmm_get_compute_dtype", "lmm_set_projection_dtype", "lmm_get_projection_dtype", "lmm_comm_get_unique_id", "lmm_comm_init_rank", "lmm_comm_info", "lmm_allreduce_sum_f64", "lmm_allreduce_max_f64",
    "lmm_comm_destroy",
    "lmm_set_strict_progress", "lmm_get_strict_progress", "lmm_dev_claim_scramble", "lmm_orthogonal_validate", "lmm_oilmm_logpdf", "lmm_oilmm_logpdf_grad", "lmm_oilmm_post_logpdf_grad", "lmm_oilmm_post_logpdf_grad_seq", "lmm_ilmm_logpdf_grad", "lmm_ilmm_post_logpdf_grad", "lmm_ilmm_post_logpdf_grad_seq", "lmm_ilmm_post_latent_logpdf_grad_seq", "lmm_oilmm_logpdf_grad_x", "lmm_oilmm_post_logpdf_grad_seq_x", "lmm_ilmm_logpdf_grad_x",
    "lmm_ilmm_post_logpdf_grad_seq_x", "lmm_ilmm_post_latent_logpdf_grad_seq_x", "lmm_oilmm_logpdf_multi", "lmm_reorder", "lmm_ilmm_logpdf", "lmm_ilmm_logpdf_ex", "lmm_ilmm_logpdf_multi", "lmm_mogp_logpdf", "lmm_mogp_logpdf_diag",
    "lmm_missing_patterns", "lmm_oilmm_project_missing", "lmm_oilmm_logpdf_missing", "lmm_oilmm_posterior_create_missing", "lmm_oilmm_logpdf_grad_missing",
    "lmm_oilmm_posterior_create", "lmm_mogp_posterior_create", "lmm_post_condition", "lmm_ilmm_posterior_create", "lmm_post_destroy", "lmm_ilmm_post_latent_view", "lmm_ilmm_post_mean_and_var", "lmm_ilmm_post_mean_and_cov", "lmm_ilmm_post_condition", "lmm_ilmm_post_logpdf", "lmm_ilmm_post_rand",
    "lmm_latent_marginals", "lmm_oilmm_mean_and_var", "lmm_oilmm_mean_and_var_grad_xs", "lmm_lmm_mean_and_cov", "lmm_mogp_cross_cov", "lmm_oilmm_post_logpdf", "lmm_lmm_rand", "lmm_lmm_rand_multi", "lmm_normals",
    "lmm_profile_begin", "lmm_profile_end",
    "lmm_oilmm_elbo", "lmm_oilmm_sparse_posterior_create", "lmm_sparse_post_destroy", "lmm_oilmm_sparse_mean_and_var", "lmm_dev_sparse_moments",
    "lmm_oilmm_elbo_grad", "lmm_dev_sparse_grad",
    "lmm_oilmm_logpdf_statespace", "lmm_oilmm_mean_and_var_statespace", "lmm_dev_statespace_filter", "lmm_dev_statespace_smooth",
    "lmm_oilmm_logpdf_grad_statespace", "lmm_dev_statespace_grad", "lmm_dev_statespace_grad_sho", "lmm_dev_statespace_grad_sum",
    "lmm_oilmm_logpdf_grad_statespace_x", "lmm_dev_statespace_grad_x", "lmm_oilmm_statespace_post_mean_and_var_grad_xs",
    "lmm_oilmm_rand_statespace", "lmm_dev_statespace_sample", "lmm_dev_statespace_sample_posterior",
    "lmm_oilmm_statespace_posterior_create", "lmm_statespace_post_destroy", "lmm_oilmm_statespace_post_mean_and_var",
    "lmm_dev_statespace_states", "lmm_dev_statespace_interp", "lmm_dev_statespace_interp_layout",
    "lmm_statespace_post_window", "lmm_oilmm_statespace_post_rand", "lmm_dev_statespace_post_sample",
    "lmm_oilmm_statespace_post_append", "lmm_statespace_post_smooth", "lmm_statespace_post_reserve", "lmm_statespace_post_size",
    "lmm_dev_statespace_filter_from",
    "lmm_oilmm_statespace_post_logpdf", "lmm_dev_statespace_post_logpdf",
    "lmm_dev_potrf", "lmm_dev_check_info", "lmm_dev_extent_check", "lmm_dev_region_plan", "lmm_dev_flag_epoch", "lmm_dev_gemm_nt_sub", "lmm_dev_gram", "lmm_dev_write_rate", "lmm_dev_mfma_f64_peak",
    "lmm_dev_set_f64_emul", "lmm_dev_syrk_emul", "lmm_dev_emul_host", "lmm_dev_emul_residues", "lmm_dev_set_emul_gemm_workgroups", "lmm_dev_emul_acc_residues",
    "lmm_dev_set_f64_emul_rule", "lmm_dev_set_emul_group", "lmm_dev_set_emul_amax_reuse", "lmm_dev_emul_plan", "lmm_dev_potrf_plan",
    "lmm_dev_set_emul_zero_skip", "lmm_dev_emul_stage_list", "lmm_dev_set_emul_scratch_poison", "lmm_dev_emul_block_live",
    "lmm_dev_set_emul_screen", "lmm_dev_emul_last_live_tiles", "lmm_dev_emul_negligible",
    "lmm_dev_set_f64_screen", "lmm_dev_set_deterministic", "lmm_dev_f64_screen_stats", "lmm_dev_f64_screen_flags",
    "lmm_dev_set_zero_extents", "lmm_dev_set_zero_extents_min_cols", "lmm_dev_zero_extent_stats", "lmm_dev_potrf_zext", "lmm_dev_train_gram",
    "lmm_dev_backsolve", "lmm_dev_factor_inverse",
]


# Argument types of the inducing-point entry points (include/lmm_hip.h, "inducing points"), set on the library by load().
_P, _I, _D = C.c_void_p, C.c_int, C.c_double
SPARSE_ARGTYPES = {
    "lmm_oilmm_elbo": [_P, _I, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _P, _I, _D, _I, _P, _P],
    "lmm_oilmm_sparse_posterior_create": [_P, _I, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _P, _I, _D, _P],
    "lmm_sparse_post_destroy": [_P],
    "lmm_oilmm_sparse_mean_and_var": [_P, _P, _P, _P, _I, _I, _D, _I, _P, _I, _I, _P, _P],
    "lmm_dev_sparse_moments": [_P, _I, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P],
    "lmm_oilmm_elbo_grad": [_P, _I, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _P, _I, _D, _I, _P, _P, _P, _P, _P, _P, _P],
    "lmm_dev_sparse_grad": [_P, _I, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P],
}


# Argument types of the state-space entry points (include/lmm_hip.h, "state space"), set on the library by load().
STATESPACE_ARGTYPES = {
    "lmm_oilmm_logpdf_statespace": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _I, _P],
    "lmm_oilmm_mean_and_var_statespace": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _I, _P, _P],
    "lmm_dev_statespace_filter": [_P, _I, _P, _P, _P, _I, _P, _P, _P],
    "lmm_dev_statespace_smooth": [_P, _I, _P, _P, _P, _I, _P, _P],
    "lmm_oilmm_logpdf_grad_statespace": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "lmm_dev_statespace_grad": [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P],
    "lmm_dev_statespace_grad_sho": [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P],
    "lmm_dev_statespace_grad_sum": [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P],
    "lmm_oilmm_logpdf_grad_statespace_x": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "lmm_dev_statespace_grad_x": [_P, _I, _P, _P, _P, _I, _P],
    "lmm_oilmm_statespace_post_mean_and_var_grad_xs": [_P, _P, _I, _P, _P, _P],
    "lmm_oilmm_rand_statespace": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "lmm_dev_statespace_sample": [_P, _I, _P, _P, _I, _I, _P],
    "lmm_dev_statespace_sample_posterior": [_P, _I, _P, _P, _P, _P, _P, _I, _I, _P],
    "lmm_oilmm_statespace_posterior_create": [_P, _I, _P, _I, _P, _P, _I, _D, _P, _I, _I, _P, _P],
    "lmm_statespace_post_destroy": [_P],
    "lmm_oilmm_statespace_post_mean_and_var": [_P, _P, _I, _I, _P, _P],
    "lmm_dev_statespace_states": [_P, _I, _P, _P, _P, _I, _P, _P],
    "lmm_dev_statespace_interp": [_P, _I, _P, _P, _P, _P, _I, _P, _P],
    "lmm_dev_statespace_interp_layout": [_P, _I, _P, _P, _P, _I, _P, _I, _P, _P],
    "lmm_statespace_post_window": [_P, _D, _D, _P, _P],
    "lmm_oilmm_statespace_post_rand": [_P, _P, _I, _P, _P, _I, _I, _P],
    "lmm_dev_statespace_post_sample": [_P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P],
    "lmm_oilmm_statespace_post_append": [_P, _P, _I, _P, _P],
    "lmm_statespace_post_smooth": [_P],
    "lmm_statespace_post_reserve": [_P, _I],
    "lmm_statespace_post_size": [_P, _P, _P, _P],
    "lmm_dev_statespace_filter_from": [_P, _D, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P],
    "lmm_oilmm_statespace_post_logpdf": [_P, _P, _I, _P, _D, _P],
    "lmm_dev_statespace_post_logpdf": [_P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P],
}

# Argument types of the solve-chain building blocks (include/lmm_hip.h, "building blocks"), set on the library by load().
_Z = C.c_size_t
SOLVE_CHAIN_ARGTYPES = {
    "lmm_dev_backsolve": [_P, _Z, _I, _P, _Z, _I, _P, _Z, _I],
    "lmm_dev_factor_inverse": [_P, _Z, _I, _I, _P, _Z, _P, _Z, _I],
}

# Argument types of the SHO tag entry points (include/lmm_hip.h, LMM_KERNEL_SHO), set on the library by load().
SHO_ARGTYPES = {
    "lmm_kernel_tag_create_sho": [_D, C.POINTER(C.c_int)],
    "lmm_kernel_tag_quality_grad": [_I, C.POINTER(C.c_double)],
}


class GpT(C.Structure):
    _fields_ = [("kind", C.c_int), ("variance", C.c_double), ("lengthscale", C.c_double), ("mean", C.c_double)]


class JittersT(C.Structure):
    _fields_ = [("project_jitter", C.c_double), ("ilmm_rand_jitter", C.c_double), ("default_jitter", C.c_double)]


class GpGradT(C.Structure):
    _fields_ = [("variance", C.c_double), ("lengthscale", C.c_double), ("mean", C.c_double)]


class ProfEntryT(C.Structure):
    _fields_ = [("launches", C.c_longlong), ("ms", C.c_double), ("work", C.c_double), ("bytes", C.c_double)]


PROF_CLASSES = ["gram", "update", "update_narrow", "trsm", "diag", "region", "update_short", "solve", "solve_leaf", "strip"]


class PosDefException(ArithmeticError):
    """Julia's LinearAlgebra.PosDefException(info)."""

    def __init__(self, msg: str, latent: int, info: int):
        super().__init__(msg)
        self.latent, self.info = latent, info


class LMMError(RuntimeError):
    pass


_lib = None
_initialised_device: Optional[int] = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LMMError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  A process must hold ONE HIP
        # runtime, so when torch is present load it first: the dynamic linker then binds liblmm_hip.so's
        # libamdhip64.so.7 dependency to the copy torch already mapped (device pointers, streams and RCCL of
        # both sides then live in the same runtime).  Without torch the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.lmm_last_error_string.restype = C.c_char_p
        for name, types in list(SPARSE_ARGTYPES.items()) + list(STATESPACE_ARGTYPES.items()) + list(SHO_ARGTYPES.items()) + list(SOLVE_CHAIN_ARGTYPES.items()):
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = types, C.c_int
    return _lib


def init(device: Optional[int] = None) -> int:
    """lmm_init: one process per GPU.  device defaults to LOCAL_RANK (torch.distributed launch) or 0."""
    global _initialised_device
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    lib = load()
    check(lib.lmm_init(C.c_int(device)))
    _initialised_device = device
    return device


def ensure_init() -> None:
    if _initialised_device is None:
        init()


def check(rc: int) -> None:
    if rc == LMM_OK:
        return
    lib = load()
    msg = lib.lmm_last_error_string().decode()
    if rc == LMM_ERR_DIM:
        raise RuntimeError(msg)                      # Julia: ErrorException("out dim of x != out dim of f.")
    if rc == LMM_ERR_NOT_ORTHOGONAL:
        raise ValueError(msg)                        # Julia: ArgumentError
    if rc == LMM_ERR_NOT_PD:
        lat, info = C.c_int(), C.c_int()
        lib.lmm_last_error_detail(C.byref(lat), C.byref(info))
        raise PosDefException(msg, lat.value, info.value)
    if rc == LMM_ERR_ARG:
        raise ValueError(msg)
    if rc == LMM_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise LMMError(msg)


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


class _OwnedPtr(C.c_void_p):
    """A void* that keeps the array it points into alive.  Call sites write `lib.f(Arr(a).ptr, ...)`: the temporary Arr dies as soon as
    `.ptr` has been read, and with it a converted copy it may own (a transposed (d, n) input, a non-contiguous or non-float64 array)
    -- the C call would then read freed memory.  (Found by tools/stress_alternate.py: gradients of d = 2 problems were occasionally
    evaluated on recycled memory; a plain c_void_p holds only the integer.)"""


def _ptr_of(addr, owner):
    p = _OwnedPtr(addr)
    p._owner = owner
    return p


# id(ndarray) -> (ndarray, pointer, size) of the last few SMALL read-only host arrays handed over (model matrices, inputs of the
# reference's regime): taking the address of a NumPy buffer through ctypes costs 2-4 us, several times per call, which shows at
# n = 200 (an evaluation is ~140 us).  The entry keeps the array alive, so an id cannot be reused by another object while it is
# cached; it is only trusted while the array still has the size it was cached with (an in-place ndarray.resize, the one way a live
# array's buffer moves, changes it).  Outputs, temporaries of conversions and anything above _PTRS_MAX_ELEMS are never inserted, so
# the cache cannot pin large buffers the caller has dropped.
_PTRS: dict = {}
_PTRS_MAX_ELEMS = 1 << 16


class Arr:
    """A Float64 array handed to the C ABI: a NumPy array (host pointer) or a CUDA/HIP torch tensor
    (device pointer).  Keeps the owner alive for the duration of the call."""

    def __init__(self, a, writable: bool = False):
        if _is_torch(a):
            import torch
            if a.dtype != torch.float64:
                raise TypeError("expected a float64 tensor")
            if not a.is_contiguous():
                if writable:
                    raise ValueError("output tensor must be contiguous")
                a = a.contiguous()
            self.owner = a
            self.ptr = _ptr_of(a.data_ptr(), a)
            self.size = a.numel()
            if a.is_cuda:
                order_after_torch()
        else:
            hit = None if writable else _PTRS.get(id(a))
            if hit is not None and hit[0] is a and a.size == hit[2]:      # the same, un-resized ndarray object as before
                self.owner, self.ptr, self.size = hit
                return
            ok = type(a) is np.ndarray and a.dtype == np.float64 and a.flags.c_contiguous
            if writable:
                if not ok:
                    raise ValueError("output array must be a C-contiguous float64 ndarray")
            elif not ok:
                a = np.ascontiguousarray(a, dtype=np.float64)
            self.owner = a
            self.ptr = _ptr_of(a.ctypes.data, a)
            self.size = a.size
            if ok and not writable and a.size <= _PTRS_MAX_ELEMS:
                if len(_PTRS) >= 64:
                    _PTRS.clear()
                _PTRS[id(a)] = (a, self.ptr, self.size)


def set_compute_dtype(dtype: str) -> None:
    """"f64" (default, parity mode) or "f32": Float32 matrices on v_mfma_f32 for the per-latent paths (include/lmm_hip.h)."""
    check(load().lmm_set_compute_dtype(C.c_int({"f64": 0, "f32": 1}[dtype])))


def get_compute_dtype() -> str:
    return "f32" if load().lmm_get_compute_dtype() == 1 else "f64"


def set_strict_progress(on: bool) -> None:
    """True (the default): the dataflow kernel's workgroups take their task index in turn from a counter, so its deadlock-freedom
    argument holds in any dispatch order; False: task = blockIdx.x, which relies on in-order dispatch (include/lmm_hip.h,
    conventions).  Same values either way."""
    check(load().lmm_set_strict_progress(C.c_int(1 if on else 0)))


def get_strict_progress() -> bool:
    return load().lmm_get_strict_progress() == 1


_PROJ = {"f64": 0, "native": 0, "bf16": 1, "bf16x2": 2}


def set_projection_dtype(dtype: str) -> None:
    """Dtype of the H unprojection of predictive marginals (reference src/oilmm.jl:69-72): "native" (Float64, default), "bf16"
    (v_mfma_f32_16x16x32_bf16, BASELINE configs[3]; tolerance 2^-7 * sum_l |H||M_lat|, include/lmm_hip.h) or "bf16x2"."""
    check(load().lmm_set_projection_dtype(C.c_int(_PROJ[dtype])))


def get_projection_dtype() -> str:
    return ["native", "bf16", "bf16x2"][load().lmm_get_projection_dtype()]


def wait_stream(stream) -> None:
    """Order the library's streams behind everything queued so far on `stream` (a torch.cuda.Stream, or any object with a
    `cuda_stream` handle; None = the legacy default stream): lmm_stream_wait_caller.  Call it before handing over a device tensor
    that was produced on a stream OTHER than torch's current one -- order_after_torch() below only looks at the current stream."""
    ensure_init()
    h = None if stream is None else getattr(stream, "cuda_stream", stream)
    check(load().lmm_stream_wait_caller(C.c_void_p(h)))


def order_after_torch() -> None:
    """The library runs on its own non-blocking HIP streams; torch produces (and recycles) device tensors asynchronously on ITS
    current stream.  Before a device pointer crosses the ABI, make the library's streams wait for everything torch has queued
    (lmm_stream_wait_caller: one event record + one stream wait, no host stall).  Skipped when torch's CURRENT stream is already
    idle; a tensor produced on another stream (torch.cuda.stream(s) blocks, side streams of a data loader) must be named by
    the caller: lmm_amd.wait_stream(s)."""
    import torch
    st = torch.cuda.current_stream()
    if st.query():
        return
    ensure_init()
    check(load().lmm_stream_wait_caller(C.c_void_p(st.cuda_stream)))


# ---- RCCL communicator of the C ABI (one process per GPU) ---------------------------------------------------------
def comm_world() -> int:
    """World size of the ABI's RCCL communicator (0: none)."""
    if _lib is None or _initialised_device is None:
        return 0
    r, w = C.c_int(), C.c_int()
    check(_lib.lmm_comm_info(C.byref(r), C.byref(w)))
    return w.value


def comm_get_unique_id() -> bytes:
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    check(load().lmm_comm_get_unique_id(buf))
    return buf.raw


def comm_init_rank(uid: bytes, rank: int, world: int) -> None:
    ensure_init()
    if len(uid) != UNIQUE_ID_BYTES:
        raise ValueError("unique id must be %d bytes" % UNIQUE_ID_BYTES)
    check(load().lmm_comm_init_rank(C.create_string_buffer(uid, UNIQUE_ID_BYTES), C.c_int(rank), C.c_int(world)))


def comm_init_from_torch() -> None:
    """Create the ABI's RCCL communicator for the ranks of torch.distributed's default group.  Rank 0 draws the unique id and
    ships it through the group's rendezvous STORE (a TCP key-value store: the out-of-band step a Julia caller does with
    MPI.bcast) -- no torch collective is involved, so torch's own NCCL communicator need not exist yet and the two RCCL
    initialisations never interleave.  Falls back to the object broadcast when the process group exposes no store."""
    import torch.distributed as dist
    global _comm_generation
    rank, world = dist.get_rank(), dist.get_world_size()
    _comm_generation += 1
    store = None
    try:
        store = dist.distributed_c10d._get_default_store()
    except Exception:
        store = None
    if store is not None:
        key = f"lmm_rccl_unique_id/{_comm_generation}"
        if rank == 0:
            store.set(key, comm_get_unique_id())
        uid = bytes(store.get(key))          # blocks until rank 0 has set it
    else:
        box = [comm_get_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        uid = box[0]
    comm_init_rank(uid, rank, world)


_comm_generation = 0


def comm_destroy() -> None:
    if _lib is not None:
        check(_lib.lmm_comm_destroy())


def allreduce_sum(a, op: str = "sum"):
    """In-place sum (or max) all-reduce of a float64 NumPy array or CUDA tensor over the ABI communicator."""
    arr = Arr(a, True)
    fn = load().lmm_allreduce_sum_f64 if op == "sum" else load().lmm_allreduce_max_f64
    check(fn(arr.ptr, C.c_size_t(arr.size)))
    return a


KERNEL_BASE_MASK = 0xFF


class ArdTags:
    """Owner of the kernel tags (lmm_ard_create / lmm_kernel_tag_create) of one lmm_gp_t array: destroyed with the array (gps_array
    attaches it as `.ard`).  tags[l] is latent l's tag, 0 for an isotropic latent without an RQ shape; has_ard[l] tells whether the
    tag holds per-dimension factors, has_alpha[l] whether it holds an RQ shape, has_rho[l] whether it holds a periodic or locally periodic latent's r, has_decay[l] whether it holds a locally periodic latent's decay.  A sum latent's tag is its lmm_kernel_sum_create tag,
    and terms[l] is the ArdTags of its terms (None for other latents); close() destroys the sum tag before the term tags."""

    def __init__(self, m: int):
        self.tags = [0] * m
        self.has_ard = [False] * m
        self.has_alpha = [False] * m
        self.has_rho = [False] * m
        self.has_decay = [False] * m
        self.has_quality = [False] * m
        self.terms = [None] * m
        self._lib = None

    def create_sum(self, l: int, terms: Sequence[dict], statespace: bool = False) -> int:
        """latent l's sum tag over the term descriptors `terms` (their own factor / alpha tags are created first).  statespace (the
        state-space functions' arrays, statespace_gps_array): a sum with an SHO term is registered with
        lmm_kernel_sum_create_statespace, which admits it; every other sum, and every sum of another caller, with
        lmm_kernel_sum_create, which the dense entry points serve too."""
        n = len(terms)
        if not 1 <= n <= SUM_MAX_TERMS:
            raise ValueError(f"a sum kernel has 1..{SUM_MAX_TERMS} terms, got {n}")
        sho = [c for c, t in enumerate(terms) if t["kind"] == "sho"]
        if sho and not statespace:
            raise NotImplementedError(f"latent {l}: an SHO term inside a sum kernel is not served (term {sho[0]})")
        self._lib = self._lib or load()
        tarr = gps_array(terms)
        self.terms[l] = tarr.ard
        t = C.c_int()
        check((self._lib.lmm_kernel_sum_create_statespace if sho else self._lib.lmm_kernel_sum_create)(n, tarr, C.byref(t)))
        self.tags[l] = t.value
        return t.value

    def sum_grad(self, l: int, d: int) -> list:
        """Per-term gradients of sum latent l after a gradient call: [{"variance", "lengthscale" (float, or the length-d array
        d logpdf / d lengthscale_k of a term with per-dimension lengthscales), "alpha" (RQ terms), "r" (periodic and locally periodic terms), "decay" (locally periodic terms),
        "quality" (SHO terms of a state-space sum whose descriptor has one; "lengthscale" is then d / d period)}, ...]."""
        ta = self.terms[l]
        n = len(ta.tags)
        out = (GpGradT * n)()
        check(self._lib.lmm_kernel_sum_grad(self.tags[l], out))
        res = []
        for c in range(n):
            e = {"variance": out[c].variance, "lengthscale": ta.grad(c, d) if ta.has_ard[c] else out[c].lengthscale}
            if ta.has_alpha[c]:
                e["alpha"] = ta.alpha_grad(c)
            if ta.has_rho[c]:
                e["r"] = ta.rho_grad(c)
            if ta.has_decay[c]:
                e["decay"] = ta.decay_grad(c)
            if ta.has_quality[c]:
                e["quality"] = ta.quality_grad(c)
            res.append(e)
        return res

    def create(self, l: int, ls: Optional[np.ndarray], alpha: Optional[float] = None, rho: Optional[float] = None,
               decay: Optional[float] = None) -> int:
        """One tag for latent l: the factors `ls` (None: none) and / or the RQ shape `alpha` (None: none), or a periodic latent's
        `rho` (None: none), or a locally periodic latent's `rho` and `decay` (both given)."""
        self._lib = self._lib or load()
        t = C.c_int()
        if decay is not None:
            d, p = (0, None) if ls is None else (int(ls.size), ls.ctypes.data_as(C.POINTER(C.c_double)))
            check(self._lib.lmm_kernel_tag_create_locally_periodic(d, p, C.c_double(rho), C.c_double(decay), C.byref(t)))
        elif rho is not None:
            d, p = (0, None) if ls is None else (int(ls.size), ls.ctypes.data_as(C.POINTER(C.c_double)))
            check(self._lib.lmm_kernel_tag_create_periodic(d, p, C.c_double(rho), C.byref(t)))
        elif alpha is None:
            check(self._lib.lmm_ard_create(int(ls.size), ls.ctypes.data_as(C.POINTER(C.c_double)), C.byref(t)))
        else:
            d, p = (0, None) if ls is None else (int(ls.size), ls.ctypes.data_as(C.POINTER(C.c_double)))
            check(self._lib.lmm_kernel_tag_create(d, p, C.c_double(alpha), C.byref(t)))
        self.tags[l] = t.value
        self.has_ard[l] = ls is not None
        self.has_alpha[l] = alpha is not None
        self.has_rho[l] = rho is not None
        self.has_decay[l] = decay is not None
        return t.value

    def create_sho(self, l: int, quality: float) -> int:
        """latent l's tag carrying an SHO latent's quality factor (lmm_kernel_tag_create_sho)."""
        self._lib = self._lib or load()
        t = C.c_int()
        check(self._lib.lmm_kernel_tag_create_sho(C.c_double(quality), C.byref(t)))
        self.tags[l] = t.value
        self.has_quality[l] = True
        return t.value

    def quality_grad(self, l: int) -> float:
        """d logpdf / d quality of latent l's tag after a gradient call."""
        out = C.c_double(0.0)
        check(self._lib.lmm_kernel_tag_quality_grad(self.tags[l], C.byref(out)))
        return out.value

    def alpha_grad(self, l: int) -> float:
        """d logpdf / d alpha of latent l's tag after a gradient call."""
        out = C.c_double(0.0)
        check(self._lib.lmm_kernel_tag_alpha_grad(self.tags[l], C.byref(out)))
        return out.value

    def rho_grad(self, l: int) -> float:
        """d logpdf / d r of latent l's tag after a gradient call."""
        out = C.c_double(0.0)
        check(self._lib.lmm_kernel_tag_rho_grad(self.tags[l], C.byref(out)))
        return out.value

    def decay_grad(self, l: int) -> float:
        """d logpdf / d decay of latent l's tag after a gradient call."""
        out = C.c_double(0.0)
        check(self._lib.lmm_kernel_tag_decay_grad(self.tags[l], C.byref(out)))
        return out.value

    def grad(self, l: int, d: int) -> np.ndarray:
        """d logpdf / d ard of latent l's tag after a gradient call (its own tag: d / d lengthscale_k, the multiplier being 1)."""
        out = np.zeros(d)
        check(self._lib.lmm_ard_grad(self.tags[l], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def close(self) -> None:
        if self._lib is not None:
            for t in self.tags:
                if t:
                    self._lib.lmm_ard_destroy(t)
        for ta in self.terms:
            if ta is not None:
                ta.close()
        self.terms = [None] * len(self.tags)
        self.tags = [0] * len(self.tags)
        self.has_ard = [False] * len(self.tags)
        self.has_alpha = [False] * len(self.tags)
        self.has_rho = [False] * len(self.tags)
        self.has_decay = [False] * len(self.tags)
        self.has_quality = [False] * len(self.tags)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sho_quality(q) -> float:
    """An SHO latent's quality factor, validated: one finite scalar > 1 / 2 (the underdamped oscillator)."""
    if np.ndim(q) != 0:
        raise ValueError("an SHO kernel's quality is one scalar")
    q = float(q)
    if not (q > 0.5 and np.isfinite(q)):
        raise ValueError("quality must be finite and > 0.5 (the underdamped oscillator; Q <= 1/2 is not served)")
    return q


def gps_array(gps: Sequence[dict], statespace: bool = False):
    """lmm_gp_t array of latent descriptors.  A vector "lengthscale" (length d) becomes an ARD latent: a tag holding the vector, kind
    = base | tag << 8 and lengthscale (the common multiplier) 1.  An "rq" latent's "alpha" (default 2.0) goes into its tag too (one
    tag holds both).  A "periodic" latent's "lengthscale" is its period and its "r" (default 1.0) goes into a tag
    (lmm_kernel_tag_create_periodic) with the vector, if any; a descriptor without "r" and with a scalar period needs no tag.  A "locally_periodic" latent is a
    periodic one with a scalar "decay" (default 1.0) next to "r": both go into one tag (lmm_kernel_tag_create_locally_periodic), needed
    when the descriptor has "r", "decay" or a vector period.  A "sum" latent's "terms" (descriptors as above, mean 0) get their own tags and then one sum tag
    (lmm_kernel_sum_create); its "variance" and scalar "lengthscale" scale the whole sum.  An "sho" latent's "lengthscale" is its period
    (a scalar: the kernel is defined for d = 1) and its "quality" (default 1.0) goes into a tag (lmm_kernel_tag_create_sho) when the
    descriptor has one.  An "sho" term of a sum raises NotImplementedError naming the latent, before any library call -- unless
    `statespace` (statespace_gps_array below).  The tags live as long as the returned array (its `.ard`)."""
    arr = (GpT * max(len(gps), 1))()
    arr.ard = ArdTags(len(gps))
    for l, g in enumerate(gps):
        a = arr[l]
        a.variance = float(g.get("variance", 1.0))
        if g["kind"] == "sum":
            a.kind = KERNEL_SUM
            ls = g.get("lengthscale", 1.0)
            if np.ndim(ls) != 0:
                raise ValueError("per-dimension lengthscales around a whole sum kernel are not supported")
            a.lengthscale = float(ls)
            a.kind |= arr.ard.create_sum(l, g["terms"], statespace) << 8
            a.mean = float(g.get("mean", 0.0))
            continue
        if g["kind"] == "sho":
            ls = g.get("lengthscale", 1.0)
            if np.ndim(ls) != 0:
                raise ValueError("an SHO kernel's period is one scalar (the kernel is defined for one-dimensional inputs)")
            a.kind = KERNEL_SHO
            a.lengthscale = float(ls)
            if "quality" in g:
                a.kind |= arr.ard.create_sho(l, sho_quality(g["quality"])) << 8
            a.mean = float(g.get("mean", 0.0))
            continue
        special = {"periodic": KERNEL_PERIODIC, "locally_periodic": KERNEL_LOCALLY_PERIODIC}
        a.kind = special[g["kind"]] if g["kind"] in special else KERNEL_KINDS[g["kind"]]
        ls = g.get("lengthscale", 1.0)
        alpha = float(g.get("alpha", 2.0)) if g["kind"] == "rq" else None
        rho = decay = None
        if g["kind"] in ("periodic", "locally_periodic"):
            r = g.get("r", 1.0)
            if np.ndim(r) != 0:
                r = np.asarray(r, dtype=np.float64).reshape(-1)
                if r.size == 0 or not np.all(r == r[0]):
                    raise ValueError("a periodic kernel's r must be one scalar for all dimensions (a vector with equal entries is accepted)")
                r = r[0]
            r = float(r)
            if not (r > 0.0 and np.isfinite(r)):
                raise ValueError("r must be finite and > 0")
            if "r" in g or "decay" in g or np.ndim(ls) != 0:      # a descriptor without "r" and with a scalar period needs no tag (and reports no r gradient)
                rho = r
        if g["kind"] == "locally_periodic":
            dc = g.get("decay", 1.0)
            if np.ndim(dc) != 0:
                raise ValueError("a locally periodic kernel's decay is one scalar (a per-dimension decay is not supported)")
            dc = float(dc)
            if not (dc > 0.0 and np.isfinite(dc)):
                raise ValueError("decay must be finite and > 0")
            if rho is not None:
                decay = dc
        elif "decay" in g:
            raise ValueError(f"a {g['kind']!r} kernel takes no decay")
        vec = None
        if np.ndim(ls) == 0:
            a.lengthscale = float(ls)
        else:
            vec = np.ascontiguousarray(ls, dtype=np.float64).reshape(-1)
            a.lengthscale = 1.0
        if vec is not None or alpha is not None or rho is not None:
            a.kind |= arr.ard.create(l, vec, alpha, rho, decay) << 8
        a.mean = float(g.get("mean", 0.0))
    return arr


def statespace_gps_array(gps: Sequence[dict]):
    """gps_array for the state-space functions: a "sum" latent with an "sho" term gets its tag from lmm_kernel_sum_create_statespace (the
    term's "quality" in a tag of its own, as an "sho" latent's), which only the state-space entry points take; every other latent is
    built as gps_array builds it, so a Matern-only sum runs on the dense verbs with the same array."""
    return gps_array(gps, statespace=True)


def jitters(j: Optional[Tuple[float, float, float]]):
    if j is None:
        return None
    return C.byref(JittersT(*map(float, j)))


def colmajor(a: np.ndarray) -> np.ndarray:
    """Column-major (Julia Array) image of a 2-D host matrix as a flat float64 vector (a view when `a` already is one)."""
    return np.ravel(np.asarray(a, dtype=np.float64), order="F")
