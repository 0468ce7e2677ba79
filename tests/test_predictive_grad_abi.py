"""Host-only checks of the predictive-marginal input gradient (include/lmm_hip.h lmm_oilmm_mean_and_var_grad_xs): the symbol is exported,
declared with its signature and listed; the Python mirror has mean_and_var_vjp; the Julia shim calls the entry point and defines
rrules for mean_and_var, mean and var (static parse, as in tests/test_shim_signatures.py)."""
import inspect
import os
import re

import lmm_amd
from lmm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "linearmixingmodels.jl_amd", "julia", "LinearMixingModelsHIP.jl")
HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
SYM = "lmm_oilmm_mean_and_var_grad_xs"


def _header_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert mt, name
    return [" ".join(a.split()) for a in mt.group(1).split(",")]


def test_symbol_exported_declared_listed():
    assert hasattr(lmm_amd.load(), SYM)
    assert SYM in L.SYMBOLS
    assert _header_params(SYM) == [
        "const lmm_post_t* post", "const lmm_gp_t* gps", "const double* U", "const double* S", "int p", "int m", "int latent_begin",
        "int latent_end", "const double* xs", "int d", "int ns", "const double* dmean", "const double* dvar", "double* grad_xs"]


def test_python_vjp_signature():
    assert "mean_and_var_vjp" in lmm_amd.__all__
    sig = inspect.signature(lmm_amd.mean_and_var_vjp)
    assert list(sig.parameters) == ["fx", "dmean", "dvar", "add_noise"]
    assert sig.parameters["dmean"].default is None and sig.parameters["dvar"].default is None
    assert sig.parameters["add_noise"].default is True


def test_shim_calls_symbol_and_defines_rrules():
    src = re.sub(r"#[^\n]*", "", open(SHIM).read())
    assert SYM in set(re.findall(r"ccall\(\(:(lmm_[a-z0-9_]+),\s*liblmm\),", src))
    for verb in ["mean_and_var", "mean", "var"]:
        assert re.search(r"function ChainRulesCore\.rrule\(::typeof\(AbstractGPs\.%s\), fx::_MVFinite\)" % verb, src), verb
    mt = re.search(r"const _MVFinite = Union\{([^\n]*)\}\n", src)
    assert mt
    for t in ["ByOutputsFill{HIPOILMM}", "ByOutputsFill{HIPMOGP}", "ByFeaturesFill{HIPMOGP}", "ByOutputsFill{HIPDenseILMM}"]:
        assert t in mt.group(1), t
    assert "@not_implemented" in src and "_noise_tangent(fx, Δv === nothing ? 0.0 : sum(Δv))" in src
