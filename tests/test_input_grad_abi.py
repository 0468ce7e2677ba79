"""Host-only checks of the input-location gradients (include/lmm_hip.h lmm_*_grad_x): the five entry points are exported, declared and
listed; the Julia shim calls each of them and its three logpdf rrules put an `x` field into the FiniteGP tangent (static parse, as in
tests/test_shim_signatures.py); the Python mirror's logpdf_and_gradient takes `inputs`, off by default."""
import inspect
import os
import re

import lmm_amd
from lmm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "linearmixingmodels.jl_amd", "julia", "LinearMixingModelsHIP.jl")
HEADER = os.path.join(ROOT, "include", "lmm_hip.h")
X_SYMBOLS = ["lmm_oilmm_logpdf_grad_x", "lmm_oilmm_post_logpdf_grad_seq_x", "lmm_ilmm_logpdf_grad_x", "lmm_ilmm_post_logpdf_grad_seq_x",
             "lmm_ilmm_post_latent_logpdf_grad_seq_x"]


def _header_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert mt, name
    return [" ".join(a.split()) for a in mt.group(1).split(",")]


def test_x_symbols_exported_declared_listed():
    lib = lmm_amd.load()
    for s in X_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in L.SYMBOLS, s
        _header_params(s)


def test_x_entry_points_extend_the_old_signatures():
    for s in X_SYMBOLS:
        old, new = _header_params(s[:-2]), _header_params(s)
        extra = 2 if "post" in s else 1
        assert new[:-extra] == old, s
        assert new[-extra:] == (["double* grad_x", "double* grad_xs"] if extra == 2 else ["double* grad_x"]), s


def _rrules(src):
    out = []
    for mt in re.finditer(r"function ChainRulesCore\.rrule\(::typeof\(AbstractGPs\.logpdf\)", src):
        end = src.find("\nend\n", mt.start())
        out.append(src[mt.start():end])
    return out


def test_shim_calls_x_symbols_and_rrules_carry_x():
    src = re.sub(r"#[^\n]*", "", open(SHIM).read())
    called = set(re.findall(r"ccall\(\(:(lmm_[a-z0-9_]+),\s*liblmm\),", src))
    for s in X_SYMBOLS:
        assert s in called, s
    rr = _rrules(src)
    assert len(rr) == 3
    for body in rr:
        assert re.search(r"Tangent\{typeof\((fx|ft)\)\}\(;[^\n]*\bx=", body), body[:120]


def test_python_inputs_keyword_defaults_off():
    sig = inspect.signature(lmm_amd.logpdf_and_gradient)
    assert "inputs" in sig.parameters and sig.parameters["inputs"].default is False
