# LinearMixingModelsHIP.jl -- the Julia-side binding a LinearMixingModels.jl maintainer would add to route the
# ILMM/OILMM inference hot path through liblmm_hip.so (include/lmm_hip.h).
#
# NOT EXECUTED IN THIS REPOSITORY: Julia is absent from the build image and from the GPU box (SURVEY.md section 8c).
# The file is argument marshalling only -- every method body is one `ccall`, so there is no arithmetic here to get
# wrong; parity is proven through the same C ABI from Python (tests/test_gpu_parity*.py).
#
# Design: NO method of LinearMixingModels is overwritten (overwriting another module's methods breaks precompilation on
# Julia >= 1.10).  The reference's types `ILMM` and `Orthogonal` are kept; the opt-in is the latent container: `hip(f)`
# swaps the `IndependentMOGP` inside an ILMM for a `HIPMOGP` (same `fs` field, plus a device handle once conditioned), and
# every method below dispatches on `FiniteGP{<:ILMM{<:HIPMOGP, ...}}` -- strictly more specific than the reference's
# `FiniteGP{<:ILMM}` / `FiniteGP{<:OILMM}` signatures, so Julia picks it without ambiguity:
#
#     f  = hip(ILMM(independent_mogp(fs), Orthogonal(U, S)))     # or ILMM(hip(independent_mogp(fs)), H)
#     fx = f(MOInputIsotopicByOutputs(x, p), σ²)
#     logpdf(fx, y); po = posterior(fx, y); marginals(po(xs, σ²)); rand(rng, fx); Zygote.gradient(logpdf, fx, y)
module LinearMixingModelsHIP

using AbstractGPs, KernelFunctions, LinearAlgebra, Random, FillArrays, ChainRulesCore, Distributions
using LinearMixingModels
using LinearMixingModels: ILMM, IndependentMOGP, Orthogonal, unpack, noise_var

export hip, HIPMOGP, SHOKernel, statespace_logpdf, statespace_mean_and_var, statespace_rand

const liblmm = get(ENV, "LMM_HIP_LIB", "liblmm_hip.so")

# ---- C structs (include/lmm_hip.h) -------------------------------------------------------------------------
struct LmmGp            # lmm_gp_t
    kind::Cint
    variance::Cdouble
    lengthscale::Cdouble
    mean::Cdouble
end
struct LmmGpGrad        # lmm_gp_grad_t
    variance::Cdouble
    lengthscale::Cdouble
    mean::Cdouble
end
struct LmmJitters       # lmm_jitters_t
    project_jitter::Cdouble
    ilmm_rand_jitter::Cdouble
    default_jitter::Cdouble
end

function check(rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:lmm_last_error_string, liblmm), Cstring, ()))
    if rc == 1                                   # LMM_ERR_DIM            -> reference src/ilmm.jl:52
        throw(ErrorException("out dim of x != out dim of f."))
    elseif rc == 2                               # LMM_ERR_NOT_ORTHOGONAL -> reference src/orthogonal_matrix.jl:22
        throw(ArgumentError("`U` is not an orthogonal matrix"))
    elseif rc == 3                               # LMM_ERR_NOT_PD         -> LinearAlgebra.PosDefException(info)
        lat = Ref{Cint}(0); info = Ref{Cint}(0)
        ccall((:lmm_last_error_detail, liblmm), Cint, (Ref{Cint}, Ref{Cint}), lat, info)
        throw(PosDefException(info[]))
    else                                         # LMM_ERR_HIP / _ARG / _UNSUPPORTED / _RCCL
        error(msg)
    end
end

__init__() = check(ccall((:lmm_init, liblmm), Cint, (Cint,), parse(Cint, get(ENV, "LOCAL_RANK", "0"))))

# ---- the opt-in latent container ----------------------------------------------------------------------------------
# Prior: handle == C_NULL.  Posterior: lmm_post_t* (device-resident factors, alpha, x) + the data it was built from
# (train: needed for TOTAL derivatives of the predictive logpdf; one entry per conditioning batch, in conditioning order).
mutable struct HIPMOGP{Tfs<:Vector{<:AbstractGP}} <: AbstractGPs.AbstractGP
    fs::Tfs
    handle::Ptr{Cvoid}
    train::Any               # nothing | Vector of (X::Matrix{Float64}, σ²::Float64, y::Vector{Float64}), one per batch
    # filled by the posterior logpdf rrule: the total-derivative cotangents of the predictive logpdf w.r.t. the training data and
    # training noise, (y_train = ..., sigma2_train = ...), which the pullback itself cannot route anywhere (see the rrule)
    last_train_cotangents::Base.RefValue{Any}
    mix::Any                 # latent view of a dense-H posterior only: the H (p x m) its conditioning batches were observed through
    function HIPMOGP(fs::Tfs, h::Ptr{Cvoid}=C_NULL, train=nothing, mix=nothing) where {Tfs<:Vector{<:AbstractGP}}
        obj = new{Tfs}(fs, h, train, Ref{Any}(nothing), mix)
        h == C_NULL || finalizer(o -> ccall((:lmm_post_destroy, liblmm), Cint, (Ptr{Cvoid},), o.handle), obj)
        return obj
    end
end
hip(f::IndependentMOGP) = HIPMOGP(f.fs)
hip(f::ILMM) = ILMM(hip(f.f), f.H)
LinearMixingModels.get_latent_gp(f::ILMM{<:HIPMOGP}) = f.f

const HIPOILMM = ILMM{<:HIPMOGP,<:Orthogonal}
const HIPDenseILMM = ILMM{<:HIPMOGP,<:Matrix}
const ByOutputsFill{F} = FiniteGP{<:F,<:MOInputIsotopicByOutputs,<:Diagonal{<:Real,<:Fill}}
isposterior(f::HIPMOGP) = f.handle != C_NULL

# ---- latent descriptors: kernel -> (kind, variance, lengthscale) ---------------------------------------------
_kind(::SEKernel) = Cint(0)
_kind(::Matern32Kernel) = Cint(1)
_kind(::Matern52Kernel) = Cint(2)
# Matern12Kernel is an alias of ExponentialKernel.  Only the Euclidean metric is served (the library computes |x - x'| itself).
_euclidean(k) = nameof(typeof(k.metric)) === :Euclidean ||
    error("LinearMixingModelsHIP: $(nameof(typeof(k))) with metric $(k.metric) is not served (Euclidean only)")
_kind(k::ExponentialKernel) = (_euclidean(k); Cint(3))
_kind(k::RationalQuadraticKernel) = (_euclidean(k); Cint(4))
# PeriodicKernel(; r): v exp(-sum_k sin^2(pi (x_k - x'_k)) / (2 r^2)) under a ScaleTransform(1 / P) or ARDTransform(1 ./ P): the
# lengthscale slot (and the ARD factors) carry the period(s).  The library takes ONE rho for all dimensions: r = fill(rho, d).
_kind(k::PeriodicKernel) = Cint(7)
# SHOKernel(; quality): the stochastically driven damped harmonic oscillator (the celerite "SHO" kernel; kind 12, LMM_KERNEL_SHO),
#     kappa(r) = exp(-pi r / Q) (cos(2 pi eta r) + sin(2 pi eta r) / (2 eta Q)),  eta = sqrt(1 - 1 / (4 Q^2)),  r = |x - x'| / P,
# under a ScaleTransform(1 / P) (the lengthscale slot carries the undamped period P) and a ScaledKernel.  A SimpleKernel with its own
# kappa, so the reference's CPU methods work on it too.  Underdamped only (Q > 1/2); one-dimensional inputs only (the radial form is
# not positive definite for d > 1).  Q travels in the latent's tag (lmm_kernel_tag_create_sho).  The library serves it on the state-space
# path (statespace_logpdf, statespace_mean_and_var, statespace_rand and the rrule of statespace_logpdf) and refuses it everywhere else.
const LMM_KERNEL_SHO = 12
struct SHOKernel{T<:Real} <: KernelFunctions.SimpleKernel
    quality::Vector{T}
    function SHOKernel(; quality::Real=1.0)
        (isfinite(quality) && quality > 0.5) || throw(ArgumentError("SHOKernel: quality must be finite and > 1/2 (underdamped)"))
        return new{typeof(quality)}([quality])
    end
end
function KernelFunctions.kappa(k::SHOKernel, r::Real)
    Q = only(k.quality); η = sqrt((2Q - 1) * (2Q + 1)) / (2Q)
    return exp(-π * r / Q) * (cos(2π * η * r) + sin(2π * η * r) / (2η * Q))
end
KernelFunctions.metric(::SHOKernel) = KernelFunctions.Euclidean()
Base.show(io::IO, k::SHOKernel) = print(io, "SHO Kernel (quality = ", only(k.quality), ")")
_kind(k::SHOKernel) = Cint(LMM_KERNEL_SHO)
_desc(k::Kernel) = (_kind(k), 1.0, 1.0)
_desc(k::ScaledKernel) = ((kd, v, l) = _desc(k.kernel); (kd, v * only(k.σ²), l))
_desc(k::TransformedKernel{<:Kernel,<:ScaleTransform}) = ((kd, v, l) = _desc(k.kernel); (kd, v, l / only(k.transform.s)))
# per-dimension lengthscales (KernelFunctions' with_lengthscale(k, ℓ::AbstractVector) = k ∘ ARDTransform(1 ./ ℓ)): the common
# multiplier stays in `lengthscale`, the factors ard[k] (effective ℓ_k = lengthscale * ard[k]) travel as a tag (lmm_ard_create)
_desc(k::TransformedKernel{<:Kernel,<:ARDTransform}) = _desc(k.kernel)
_ard(k::Kernel) = nothing                                       # isotropic
_ard(k::ScaledKernel) = _ard(k.kernel)
_ard(k::TransformedKernel{<:Kernel,<:ScaleTransform}) = _ard(k.kernel)
function _ard(k::TransformedKernel{<:Kernel,<:ARDTransform})   # the inner kernel sees v .* x: its lengthscales divide by v
    a = _ard(k.kernel); v = Vector{Float64}(k.transform.v)
    return a === nothing ? 1.0 ./ v : a ./ v
end
# the RQ shape alpha (it travels in the latent's tag, lmm_kernel_tag_create); nothing for the other kernels
_alpha(k::Kernel) = nothing
_alpha(k::RationalQuadraticKernel) = Float64(only(k.α))
_alpha(k::ScaledKernel) = _alpha(k.kernel)
_alpha(k::TransformedKernel) = _alpha(k.kernel)
# a periodic kernel's rho (it travels in the latent's tag, lmm_kernel_tag_create_periodic); nothing for the other kernels
_rho(k::Kernel) = nothing
function _rho(k::PeriodicKernel)
    r = k.r
    all(==(first(r)), r) || error("LinearMixingModelsHIP: PeriodicKernel with unequal entries of r is not served (r = fill(rho, d) only)")
    return Float64(first(r))
end
_rho(k::ScaledKernel) = _rho(k.kernel)
_rho(k::TransformedKernel) = _rho(k.kernel)
# an SHO kernel's quality (it travels in the latent's tag, lmm_kernel_tag_create_sho); nothing for the other kernels.  An SHO kernel
# takes a ScaleTransform and a ScaledKernel only.
_quality(k::Kernel) = nothing
_quality(k::SHOKernel) = Float64(only(k.quality))
_quality(k::ScaledKernel) = _quality(k.kernel)
_quality(k::TransformedKernel{<:Kernel,<:ScaleTransform}) = _quality(k.kernel)
_desc(k::TransformedKernel{<:SHOKernel,<:ARDTransform}) =
    error("LinearMixingModelsHIP: an SHOKernel under an ARDTransform is not served (the kernel is defined for one-dimensional inputs)")
# Locally periodic kernels: the ONE KernelProduct that is served, SqExponentialKernel * PeriodicKernel in either order (kind 10,
# LMM_KERNEL_LOCALLY_PERIODIC).  The SE factor may sit under a ScaleTransform (1 / decay), the periodic factor under a ScaleTransform or
# ARDTransform (1 / period); the product itself may sit under ScaledKernel / ScaleTransform (which then scales the period AND the decay)
# and inside a KernelSum.  rho and the decay travel in one tag (lmm_kernel_tag_create_locally_periodic).  Everything else is refused.
const _SEFactor = Union{SqExponentialKernel,TransformedKernel{<:SqExponentialKernel,<:ScaleTransform}}
const _PerFactor = Union{PeriodicKernel,TransformedKernel{<:PeriodicKernel,<:ScaleTransform},TransformedKernel{<:PeriodicKernel,<:ARDTransform}}
_product_refused(k) = error("LinearMixingModelsHIP: this KernelProduct is not served (only SqExponentialKernel * PeriodicKernel, " *
                            "each optionally under a ScaleTransform, the periodic factor also under an ARDTransform): $(k)")
function _lpfactors(k::KernelProduct)      # (SE factor, periodic factor)
    ks = k.kernels
    length(ks) == 2 || _product_refused(k)
    (a, b) = (ks[1], ks[2])
    a isa _SEFactor && b isa _PerFactor && return (a, b)
    b isa _SEFactor && a isa _PerFactor && return (b, a)
    _product_refused(k)
end
_desc(k::KernelProduct) = ((_, per) = _lpfactors(k); (Cint(10), 1.0, _desc(per)[3]))
_desc(k::TransformedKernel{<:KernelProduct,<:ARDTransform}) =
    error("LinearMixingModelsHIP: an ARDTransform around a whole KernelProduct is not served (a per-dimension decay; put it on the periodic factor)")
_ard(k::KernelProduct) = _ard(_lpfactors(k)[2])
_rho(k::KernelProduct) = _rho(_lpfactors(k)[2])
# the decay (the SE factor's lengthscale) of a locally periodic product; nothing for the other kernels
_decay(k::Kernel) = nothing
_decay(k::KernelProduct) = Float64(_desc(_lpfactors(k)[1])[3])
_decay(k::ScaledKernel) = _decay(k.kernel)
_decay(k::TransformedKernel{<:Kernel,<:ScaleTransform}) = (δ = _decay(k.kernel); δ === nothing ? nothing : δ / only(k.transform.s))
# Sum kernels (KernelFunctions' KernelSum, k1 + k2): kind 5 with a sum tag (lmm_kernel_sum_create).  `_desc` of the sum is (5, 1, 1), so
# a ScaledKernel / ScaleTransform around it gives the latent's outer variance v0 and lengthscale s0; each term is read with the
# single-kernel methods above.  A nested sum with unit outer variance and lengthscale is flattened; any other is rejected, as is an
# ARDTransform around a whole sum.
_desc(k::KernelSum) = (Cint(5), 1.0, 1.0)
_desc(k::TransformedKernel{<:KernelSum,<:ARDTransform}) =
    error("LinearMixingModelsHIP: an ARDTransform around a whole KernelSum is not served (put it on the terms)")
_terms(k::Kernel) = nothing
_terms(k::ScaledKernel) = _terms(k.kernel)
_terms(k::TransformedKernel) = _terms(k.kernel)
function _terms(k::KernelSum)
    out = Kernel[]
    for t in k.kernels
        tt = _terms(t)
        if tt === nothing
            push!(out, t)
        else
            (_, v, l) = _desc(t)
            (v == 1.0 && l == 1.0) || error("LinearMixingModelsHIP: a scaled KernelSum cannot be a term of another sum")
            append!(out, tt)
        end
    end
    length(out) <= 4 || error("LinearMixingModelsHIP: a KernelSum has at most 4 terms (got $(length(out)))")
    return out
end
_mean(::AbstractGPs.ZeroMean) = 0.0
_mean(m::AbstractGPs.ConstMean) = Float64(m.c)
# `_gps(fs) do gps, tags ... end`: the lmm_gp_t array of the latents fs (nothing: none, for calls on a posterior handle) for the
# duration of ONE library call.  Each ARD latent's factors and each RQ latent's alpha are registered as one tag (kind = base | tag << 8)
# before the body runs and destroyed after it, whatever happens; tags[l] is latent l's tag (id 0 for an isotropic latent without
# alpha; a handle keeps its own copy of the lengthscales and alpha, so destroying the tags after a posterior call is safe).
struct KTag
    id::Cint
    ard::Bool      # the tag holds per-dimension factors
    alpha::Bool    # the tag holds an RQ shape
    rho::Bool      # the tag holds a periodic kernel's rho (its gradient travels in the `alpha` field of the gradient tuples)
    decay::Bool    # the tag holds a locally periodic kernel's rho and decay (the `alpha` field is then the tuple (rho = , decay = ))
    terms::Vector{KTag}   # a sum tag: its terms' tags (empty otherwise)
    quality::Bool  # the tag holds an SHO kernel's quality (its gradient travels in the `alpha` field of the gradient tuples)
end
KTag(id, ard, alpha, rho::Bool=false, decay::Bool=false; terms::Vector{KTag}=KTag[], quality::Bool=false) =
    KTag(id, ard, alpha, rho, decay, terms, quality)
# the factor / alpha tag of one kernel (a latent's or a sum term's); 0: none needed
function _ktag(a, α, ρ=nothing, δ=nothing, q=nothing)
    tr = Ref{Cint}(0)
    if q !== nothing
        check(ccall((:lmm_kernel_tag_create_sho, liblmm), Cint, (Cdouble, Ref{Cint}), q, tr))
    elseif δ !== nothing
        av = a === nothing ? Float64[] : a
        GC.@preserve av check(ccall((:lmm_kernel_tag_create_locally_periodic, liblmm), Cint, (Cint, Ptr{Cdouble}, Cdouble, Cdouble, Ref{Cint}),
                                    length(av), a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(av), ρ, δ, tr))
    elseif ρ !== nothing
        av = a === nothing ? Float64[] : a
        GC.@preserve av check(ccall((:lmm_kernel_tag_create_periodic, liblmm), Cint, (Cint, Ptr{Cdouble}, Cdouble, Ref{Cint}),
                                    length(av), a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(av), ρ, tr))
    elseif a !== nothing && α === nothing
        GC.@preserve a check(ccall((:lmm_ard_create, liblmm), Cint, (Cint, Ptr{Cdouble}, Ref{Cint}), length(a), a, tr))
    elseif α !== nothing
        av = a === nothing ? Float64[] : a
        GC.@preserve av check(ccall((:lmm_kernel_tag_create, liblmm), Cint, (Cint, Ptr{Cdouble}, Cdouble, Ref{Cint}),
                                    length(av), a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(av), α, tr))
    end
    return tr[]
end
function _destroy(t::KTag)
    t.id == 0 || ccall((:lmm_ard_destroy, liblmm), Cint, (Cint,), t.id)      # a sum tag before its terms' tags
    foreach(_destroy, t.terms)
end
function _gps(body, fs)
    gps = LmmGp[]; tags = KTag[]
    try
        for f in (fs === nothing ? () : fs)
            (kd, v, l) = _desc(f.kernel)
            if kd == 5
                tts = KTag[]; tgps = LmmGp[]
                push!(tags, KTag(Cint(0), false, false; terms=tts))    # registered first, so that the finally destroys the term tags on error
                for k in _terms(f.kernel)
                    (tk, tv, tl) = _desc(k); a = _ard(k); α = _alpha(k); ρ = _rho(k); δ = _decay(k)
                    t = _ktag(a, α, ρ, δ)
                    push!(tts, KTag(t, a !== nothing, α !== nothing, ρ !== nothing, δ !== nothing))
                    push!(tgps, LmmGp(t == 0 ? tk : tk | (t << 8), tv, tl, 0.0))
                end
                tr = Ref{Cint}(0)
                GC.@preserve tgps check(ccall((:lmm_kernel_sum_create, liblmm), Cint, (Cint, Ptr{LmmGp}, Ref{Cint}),
                                              length(tgps), pointer(tgps), tr))
                tags[end] = KTag(tr[], false, false; terms=tts)
                push!(gps, LmmGp(kd | (tr[] << 8), v, l, _mean(f.mean)))
                continue
            end
            q = _quality(f.kernel)
            if q !== nothing                                   # an SHO latent: its tag carries the quality alone
                t = _ktag(nothing, nothing, nothing, nothing, q)
                push!(tags, KTag(t, false, false; quality=true))
                push!(gps, LmmGp(kd | (t << 8), v, l, _mean(f.mean)))
                continue
            end
            a = _ard(f.kernel); α = _alpha(f.kernel); ρ = _rho(f.kernel); δ = _decay(f.kernel)
            t = _ktag(a, α, ρ, δ)
            push!(tags, KTag(t, a !== nothing, α !== nothing, ρ !== nothing, δ !== nothing))
            push!(gps, LmmGp(t == 0 ? kd : kd | (t << 8), v, l, _mean(f.mean)))
        end
        return body(gps, tags)
    finally
        foreach(_destroy, tags)
    end
end
# after a gradient call inside _gps, per latent: nothing (no tag) or (ard = d logpdf / d ard[k] (lmm_ard_grad) or nothing,
# alpha = d logpdf / d alpha (lmm_kernel_tag_alpha_grad), of a periodic latent d logpdf / d rho (lmm_kernel_tag_rho_grad), of a locally
# periodic one (rho = that, decay = d logpdf / d decay (lmm_kernel_tag_decay_grad)), or nothing)
# A sum latent: (ard = nothing, alpha = nothing, terms = per term (variance, lengthscale, ard, alpha) from lmm_kernel_sum_grad and
# the terms' own tags).
function _rho_decay_grads(id)
    ρ = Ref{Cdouble}(0.0); δ = Ref{Cdouble}(0.0)
    check(ccall((:lmm_kernel_tag_rho_grad, liblmm), Cint, (Cint, Ref{Cdouble}), id, ρ))
    check(ccall((:lmm_kernel_tag_decay_grad, liblmm), Cint, (Cint, Ref{Cdouble}), id, δ))
    return (rho = ρ[], decay = δ[])
end
function _tag_grads(t::KTag, d::Integer)
    t.id == 0 && return nothing
    terms = nothing
    if !isempty(t.terms)
        g = Vector{LmmGpGrad}(undef, length(t.terms))
        GC.@preserve g check(ccall((:lmm_kernel_sum_grad, liblmm), Cint, (Cint, Ptr{LmmGpGrad}), t.id, pointer(g)))
        terms = map(eachindex(t.terms)) do c
            tg = _tag_grads(t.terms[c], d)          # the term's own tag: once per term
            (variance = g[c].variance, lengthscale = g[c].lengthscale,
             ard = tg === nothing ? nothing : tg.ard, alpha = tg === nothing ? nothing : tg.alpha)
        end
    end
    return (ard = t.ard ? (g = Vector{Float64}(undef, d);
                           GC.@preserve g check(ccall((:lmm_ard_grad, liblmm), Cint, (Cint, Ptr{Cdouble}), t.id, g)); g) : nothing,
            alpha = t.alpha ? (r = Ref{Cdouble}(0.0);
                               check(ccall((:lmm_kernel_tag_alpha_grad, liblmm), Cint, (Cint, Ref{Cdouble}), t.id, r)); r[]) :
                    t.decay ? _rho_decay_grads(t.id) :
                    t.quality ? (r = Ref{Cdouble}(0.0);
                                 check(ccall((:lmm_kernel_tag_quality_grad, liblmm), Cint, (Cint, Ref{Cdouble}), t.id, r)); r[]) :
                    t.rho ? (r = Ref{Cdouble}(0.0);
                             check(ccall((:lmm_kernel_tag_rho_grad, liblmm), Cint, (Cint, Ref{Cdouble}), t.id, r)); r[]) : nothing,
            terms = terms)
end
_ard_grads(tags::Vector{KTag}, d::Integer) = [_tag_grads(t, d) for t in tags]

# x as a d x n column-major matrix: Vector{Float64} => 1 x n; ColVecs => its X; RowVecs => transposed copy.
_xmat(x::AbstractVector{<:Real}) = reshape(collect(Float64, x), 1, :)
_xmat(x::ColVecs) = Matrix{Float64}(x.X)
_xmat(x::RowVecs) = Matrix{Float64}(x.X')

# (U, S-or-NULL, p, m) of the mixing matrix: Orthogonal passes U and diag(S) -- never collect(H), whose getindex
# materialises U sqrt(S) per element (reference src/orthogonal_matrix.jl:27-30)
_hargs(H::Orthogonal) = (Matrix{Float64}(H.U), Vector{Float64}(H.S.diag), size(H.U)...)
_hargs(H::AbstractMatrix) = (Matrix{Float64}(H), nothing, size(H)...)
_ptr(::Nothing) = Ptr{Cdouble}(C_NULL)
_ptr(a::Array{Float64}) = pointer(a)

# ---- logpdf -------------------------------------------------------------------------------------------------------
# reference src/oilmm.jl:79-93 (prior) and test/oilmm.jl:25 (posterior: the posterior is again an OILMM, src/oilmm.jl:133)
function AbstractGPs.logpdf(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real})
    fs, H, σ², x = unpack(fx)                       # keeps the reference's out-dim check (src/ilmm.jl:45-54)
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); yv = Vector{Float64}(y)
    out = Ref{Cdouble}(0.0)
    if isposterior(fs)
        GC.@preserve X U S yv check(ccall((:lmm_oilmm_post_logpdf, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ref{Cdouble}),
            fs.handle, U, S, p, m, σ², X, d, n, yv, 1, out))
    else
        _gps(fs.fs) do gps, tags
            GC.@preserve X yv U S gps check(ccall((:lmm_oilmm_logpdf, liblmm), Cint,
                (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}),
                X, d, n, yv, p, U, S, m, σ², gps, 0, m, 1, out))
        end
    end
    return out[]
end

# logpdf(fx, Y::AbstractMatrix): one value per column from ONE factorisation per latent (AbstractGPs.TestUtils calls it)
function AbstractGPs.logpdf(fx::ByOutputsFill{HIPOILMM}, Y::AbstractMatrix{<:Real})
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && return [logpdf(fx, Y[:, c]) for c in axes(Y, 2)]
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); Ym = Matrix{Float64}(Y)
    out = Vector{Float64}(undef, size(Ym, 2))
    _gps(fs.fs) do gps, tags
        GC.@preserve X Ym U S gps out check(ccall((:lmm_oilmm_logpdf_multi, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ptr{Cdouble}),
            X, d, n, Ym, p, size(Ym, 2), U, S, m, σ², gps, 0, m, 1, out))
    end
    return out
end

# the same for the dense-H ILMM (lmm_ilmm_logpdf_multi: the columns ride the one (mn) x (mn) factorisation) and the IndependentMOGP
# (the OILMM with U = I, S = 1, no regulariser); on posterior models the columns are evaluated one by one on the handle
function AbstractGPs.logpdf(fx::ByOutputsFill{HIPDenseILMM}, Y::AbstractMatrix{<:Real})
    f, H, σ², x = unpack(fx)
    isposterior(f) && return [logpdf(fx, Y[:, c]) for c in axes(Y, 2)]
    X = _xmat(x); d, n = size(X); p, m = size(H); Ym = Matrix{Float64}(Y); Hm = Matrix{Float64}(H)
    out = Vector{Float64}(undef, size(Ym, 2))
    _gps(f.fs) do gps, tags
        GC.@preserve X Ym Hm gps out check(ccall((:lmm_ilmm_logpdf_multi, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ptr{Cdouble}),
            X, d, n, Ym, p, size(Ym, 2), Hm, m, σ², gps, C_NULL, out))
    end
    return out
end
function AbstractGPs.logpdf(ft::ByOutputsFill{HIPMOGP}, Y::AbstractMatrix{<:Real})
    isposterior(ft.f) && return [logpdf(ft, Y[:, c]) for c in axes(Y, 2)]
    X = _xmat(ft.x.x); d, n = size(X); m = length(ft.f.fs); σ² = noise_var(ft.Σy)
    ft.x.out_dim == m || throw(ErrorException("out dim of x != out dim of f."))
    U = Matrix{Float64}(I, m, m); S = ones(m); Ym = Matrix{Float64}(Y)
    out = Vector{Float64}(undef, size(Ym, 2))
    _gps(ft.f.fs) do gps, tags
        GC.@preserve X Ym U S gps out check(ccall((:lmm_oilmm_logpdf_multi, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ptr{Cdouble}),
            X, d, n, Ym, m, size(Ym, 2), U, S, m, σ², gps, 0, m, 0, out))
    end
    return out
end

# reference src/ilmm.jl:150-163 (prior) and test/ilmm.jl:25 (posterior), dense H
function AbstractGPs.logpdf(fx::ByOutputsFill{HIPDenseILMM}, y::AbstractVector{<:Real})
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); p, m = size(H); yv = Vector{Float64}(y)
    out = Ref{Cdouble}(0.0)
    if isposterior(f)
        GC.@preserve X yv check(ccall((:lmm_ilmm_post_logpdf, liblmm), Cint,
            (Ptr{Cvoid}, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{LmmJitters}, Ref{Cdouble}),
            f.handle, σ², X, d, n, yv, C_NULL, out))
    else
        Hm = Matrix{Float64}(H)
        _gps(f.fs) do gps, tags
            GC.@preserve X yv Hm gps check(ccall((:lmm_ilmm_logpdf, liblmm), Cint,
                (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}),
                X, d, n, yv, p, Hm, m, σ², gps, C_NULL, out))
        end
    end
    return out[]
end

# reference src/independent_mogp.jl:74-80 (by-outputs, scalar noise); posterior MOGP == posterior OILMM with U = I, S = 1
function AbstractGPs.logpdf(ft::ByOutputsFill{HIPMOGP}, y::AbstractVector{<:Real})
    X = _xmat(ft.x.x); d, n = size(X); m = length(ft.f.fs); yv = Vector{Float64}(y); σ² = noise_var(ft.Σy)
    ft.x.out_dim == m || throw(ErrorException("out dim of x != out dim of f."))
    out = Ref{Cdouble}(0.0)
    if isposterior(ft.f)
        U = Matrix{Float64}(I, m, m); S = ones(m)
        GC.@preserve X U S yv check(ccall((:lmm_oilmm_post_logpdf, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ref{Cdouble}),
            ft.f.handle, U, S, m, m, σ², X, d, n, yv, 0, out))
    else
        _gps(ft.f.fs) do gps, tags
            GC.@preserve X yv gps check(ccall((:lmm_mogp_logpdf, liblmm), Cint,
                (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Ref{Cdouble}),
                X, d, n, yv, m, σ², gps, 0, m, out))
        end
    end
    return out[]
end

# general Diagonal noise on a by-outputs IndependentMOGP (what reference src/independent_mogp.jl:222-229 reaches after
# reorder_by_outputs, :149-159): per-point noise variances ride the Gram diagonal
function AbstractGPs.logpdf(ft::FiniteGP{<:HIPMOGP,<:MOInputIsotopicByOutputs,<:Diagonal{<:Real,<:Vector}}, y::AbstractVector{<:Real})
    isposterior(ft.f) && error("logpdf with a general Diagonal noise is served for the prior IndependentMOGP only")
    X = _xmat(ft.x.x); d, n = size(X); m = length(ft.f.fs)
    ft.x.out_dim == m || throw(ErrorException("out dim of x != out dim of f."))
    yv = Vector{Float64}(y); nv = Vector{Float64}(ft.Σy.diag)
    out = Ref{Cdouble}(0.0)
    _gps(ft.f.fs) do gps, tags
        GC.@preserve X yv nv gps check(ccall((:lmm_mogp_logpdf_diag, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{LmmGp}, Cint, Cint, Ref{Cdouble}),
            X, d, n, yv, m, nv, gps, 0, m, out))
    end
    return out[]
end

# ---- posterior ----------------------------------------------------------------------------------------------------
# the conditioning batches a posterior was built from (nothing: unknown, e.g. the latent view of a dense-H posterior)
_push_train(train, X, σ², yv) = train === nothing ? nothing : vcat(train, [(X, Float64(σ²), yv)])
# ... as ONE set of points for the *_post_logpdf_grad_seq entries: X (d x n), sizes, variances, y by outputs over the n points
function _merged_train(train, p::Integer)
    length(train) <= 7 || error("gradient of the predictive logpdf after more than 7 conditioning batches is not built")
    X0 = reduce(hcat, [t[1] for t in train])
    y0 = vec(reduce(vcat, [reshape(t[3], :, p) for t in train]))            # (n_b x p) blocks stacked per output
    return X0, Cint[size(t[1], 2) for t in train], Cdouble[t[2] for t in train], y0
end
# d/dy of the merged points back to one by-outputs vector per batch; d/dσ² per batch (a scalar for a single batch)
# gx0: d/dx of the merged points (d x n, nothing when not computed) -> x_train, one d x n_b block per batch when there are several
function _split_train(gy0, gb, bn, p::Integer, gx0=nothing)
    length(bn) == 1 && return (y_train=gy0, sigma2_train=gb[1], x_train=gx0)
    G = reshape(gy0, :, p); o = cumsum(vcat(0, bn))
    return (y_train=[vec(G[o[b]+1:o[b+1], :]) for b in eachindex(bn)], sigma2_train=copy(gb),
            x_train=(gx0 === nothing ? nothing : [gx0[:, o[b]+1:o[b+1]] for b in eachindex(bn)]))
end
# reference src/oilmm.jl:116-134; on a posterior: sequential conditioning (TestUtils on `po`, test/oilmm.jl:34-37)
function AbstractGPs.posterior(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real})
    fs, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); yv = Vector{Float64}(y)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if isposterior(fs)
        GC.@preserve X yv U S check(ccall((:lmm_post_condition, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
            fs.handle, U, S, p, m, σ², X, d, n, yv, h))
        return ILMM(HIPMOGP(fs.fs, h[], _push_train(fs.train, X, σ², yv)), H)
    end
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S gps check(ccall((:lmm_oilmm_posterior_create, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Ref{Ptr{Cvoid}}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, h))
    end
    return ILMM(HIPMOGP(fs.fs, h[], [(X, Float64(σ²), yv)]), H)    # again an ILMM with the same H (src/oilmm.jl:133)
end

# ---- inducing points: AbstractGPs' VFE(f(z, ε)) on the latents of an OILMM -----------------------------------------------------------
# elbo(VFE(f(z, ε)), fx, y) and dtc(...) (AbstractGPs src/sparse_approximations.jl) through lmm_oilmm_elbo (include/lmm_hip.h,
# "inducing points"): Titsias' collapsed bound per latent after the OILMM projection, plus the regulariser of src/oilmm.jl:101-113.
# z = vfe.fz.x.x (by outputs, shared by all latents), ε = the Fill noise of vfe.fz.  Prior OILMM only.  posterior(::VFE, fx, y) is
# served by the C ABI and the Python mirror (lmm_oilmm_sparse_posterior_create, approx_posterior) and not yet by this shim.  The rrule of
# elbo (lmm_oilmm_elbo_grad) is with the other rrules below.
function _elbo_dtc(vfe::VFE{<:ByOutputsFill{HIPOILMM}}, fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real})
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("inducing-point inference is served on a prior OILMM only")
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); yv = Vector{Float64}(y)
    Z = _xmat(vfe.fz.x.x); ε = Float64(noise_var(vfe.fz.Σy))
    size(Z, 1) == d || error("the inducing inputs have d = $(size(Z, 1)), the inputs d = $d")
    e = Ref{Cdouble}(0.0); t = Ref{Cdouble}(0.0)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S Z gps check(ccall((:lmm_oilmm_elbo, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint,
             Ptr{Cdouble}, Cint, Cdouble, Cint, Ref{Cdouble}, Ref{Cdouble}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, Z, size(Z, 2), ε, 1, e, t))
    end
    return e[], t[]
end
AbstractGPs.elbo(vfe::VFE{<:ByOutputsFill{HIPOILMM}}, fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real}) = _elbo_dtc(vfe, fx, y)[1]
AbstractGPs.dtc(vfe::VFE{<:ByOutputsFill{HIPOILMM}}, fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real}) = _elbo_dtc(vfe, fx, y)[2]

# ---- state space: Matern12 / 32 / 52 latents over a one-dimensional input -------------------------------------------------------------
# statespace_logpdf(fx, y) and statespace_mean_and_var(fx, y; add_noise, xs) through lmm_oilmm_logpdf_statespace and
# lmm_oilmm_mean_and_var_statespace (include/lmm_hip.h, "state space"): a Kalman filter / RTS smoother per latent, O(n) and exact.
# The library takes sorted inputs: the points are sorted here (stably) and the results put back in the caller's order.  `missing` or
# NaN entries of y are missing observations; new inputs xs are merged in as points without observations.  Prior OILMM only.
# The reusable posterior (lmm_oilmm_statespace_posterior_create, lmm_oilmm_statespace_post_mean_and_var; Python:
# statespace_posterior) is served by the C ABI and the Python mirror and not yet by this shim: its handle type, lmm_ss_post_t, has
# no Julia mapping in the static check of this file's ccalls (tests/test_shim_signatures.py), as lmm_sparse_post_t above.
function _statespace_sorted(x, y::AbstractVector, p::Integer, xs)
    X = _xmat(x)
    size(X, 1) == 1 || error("state-space inference is served for one-dimensional inputs (d = $(size(X, 1)))")
    xv = vec(X); n = length(xv)
    Y = reshape(Float64[ismissing(v) ? NaN : Float64(v) for v in y], n, p)
    if xs !== nothing
        xn = vec(_xmat(xs))
        xv = vcat(xv, xn); Y = vcat(Y, fill(NaN, length(xn), p))
    end
    perm = sortperm(xv; alg=MergeSort)
    return xv[perm], vec(Y[perm, :]), perm, n
end
function statespace_logpdf(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector; with_regulariser::Bool=true)
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("state-space inference is served on a prior OILMM only")
    U, S, p, m = _hargs(H)
    xv, yv, _, _ = _statespace_sorted(x, y, p, nothing)
    out = Ref{Cdouble}(0.0)
    _gps(fs.fs) do gps, tags
        GC.@preserve xv yv U S gps check(ccall((:lmm_oilmm_logpdf_statespace, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}),
            xv, length(xv), yv, p, U, S, m, σ², gps, 0, m, Cint(with_regulariser), out))
    end
    return out[]
end
function statespace_mean_and_var(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector; add_noise::Bool=true, xs=nothing)
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("state-space inference is served on a prior OILMM only")
    U, S, p, m = _hargs(H)
    xv, yv, perm, n = _statespace_sorted(x, y, p, xs)
    N = length(xv)
    mean = Vector{Float64}(undef, N * p); var = Vector{Float64}(undef, N * p)
    _gps(fs.fs) do gps, tags
        GC.@preserve xv yv U S gps mean var check(ccall((:lmm_oilmm_mean_and_var_statespace, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
             Ptr{Cdouble}, Ptr{Cdouble}),
            xv, N, yv, p, U, S, m, σ², gps, 0, m, Cint(add_noise), mean, var))
    end
    rows = xs === nothing ? (1:n) : (n+1:N)
    back(v) = (B = similar(reshape(v, N, p)); B[perm, :] = reshape(v, N, p); vec(B[rows, :]))
    return back(mean), back(var)
end

# statespace_rand(rng, fx[, N]; y, xs, add_noise) through lmm_oilmm_rand_statespace: joint samples in O(n), exact -- of the prior fx
# (y === nothing), or of the posterior given y at the training inputs or at new inputs xs (only their rows are returned).  The normals
# are drawn with randn(rng, ...) per sample in the library's order, all indexed by SORTED point (N_all points, new inputs included):
# for each latent l in order D_l * N_all (D = 1 / 2 / 3 for Matern12 / 32 / 52; component i of sorted point t at i * N_all + t), then,
# with y only, m * N_all, then, if add_noise, N_all * p.  Returns a vector (no N) or an (n p) x N matrix, by outputs.
_statespace_dim(kd) = kd == 3 ? 1 : kd == 1 ? 2 : kd == 2 ? 3 : kd == LMM_KERNEL_SHO ? 2 : error("state-space inference is served for Matern12, Matern32 and Matern52 latents")
function _statespace_rand(rng::AbstractRNG, fx::ByOutputsFill{HIPOILMM}, N::Integer, y, xs, add_noise::Bool)
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("state-space inference is served on a prior OILMM only")
    y === nothing && xs !== nothing && throw(ArgumentError("statespace_rand: xs needs y; to sample the prior at other inputs, put them into fx.x"))
    N >= 1 || throw(ArgumentError("statespace_rand: N must be >= 1"))
    U, S, p, m = _hargs(H)
    if y === nothing
        X = _xmat(x)
        size(X, 1) == 1 || error("state-space inference is served for one-dimensional inputs (d = $(size(X, 1)))")
        xv = vec(X); n = length(xv); perm = sortperm(xv; alg=MergeSort); xv = xv[perm]; yv = Float64[]
    else
        xv, yv, perm, n = _statespace_sorted(x, y, p, xs)
    end
    Na = length(xv)
    dims = [_statespace_dim(_desc(f.kernel)[1]) for f in fs.fs]
    z = Matrix{Float64}(undef, sum(dims) * Na, N)
    ξ = Matrix{Float64}(undef, y === nothing ? 0 : m * Na, N)
    ε = Matrix{Float64}(undef, add_noise ? Na * p : 0, N)
    for q in 1:N
        off = 0
        for D in dims
            z[off+1:off+D*Na, q] = randn(rng, D * Na); off += D * Na
        end
        y === nothing || (ξ[:, q] = randn(rng, m * Na))
        add_noise && (ε[:, q] = randn(rng, Na * p))
    end
    out = Matrix{Float64}(undef, Na * p, N)
    _gps(fs.fs) do gps, tags
        GC.@preserve xv yv U S gps z ξ ε out check(ccall((:lmm_oilmm_rand_statespace, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Cint,
             Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
            xv, Na, y === nothing ? Ptr{Cdouble}(C_NULL) : pointer(yv), p, U, S, m, σ², gps, 0, m, Cint(add_noise), N,
            z, y === nothing ? Ptr{Cdouble}(C_NULL) : pointer(ξ), add_noise ? pointer(ε) : Ptr{Cdouble}(C_NULL), out))
    end
    rows = xs === nothing ? (1:n) : (n+1:Na)
    back(v) = (B = similar(reshape(v, Na, p)); B[perm, :] = reshape(v, Na, p); vec(B[rows, :]))
    return reduce(hcat, [back(out[:, q]) for q in 1:N])
end
statespace_rand(rng::AbstractRNG, fx::ByOutputsFill{HIPOILMM}; y=nothing, xs=nothing, add_noise::Bool=true) =
    vec(_statespace_rand(rng, fx, 1, y, xs, add_noise))
statespace_rand(rng::AbstractRNG, fx::ByOutputsFill{HIPOILMM}, N::Integer; y=nothing, xs=nothing, add_noise::Bool=true) =
    _statespace_rand(rng, fx, N, y, xs, add_noise)

# ---- missing observations: y::AbstractVector{Union{Missing,Float64}} ----------------------------------------------------------------
# The reference's notebook: "Heterotopic and missing data ... are not supported yet ... using the missing data techniques identified in
# the paper".  `missing` becomes NaN and the prior OILMM goes through the library's *_missing entry points (include/lmm_hip.h, "missing
# observations": the diagonal approximation of the OILMM paper).  Points without any observation are dropped first (they carry no
# information; the C ABI refuses them).  Posterior models, dense-H ILMM, IndependentMOGP, matrix Y and rand do not take missing data.
const MissingVec = AbstractVector{Union{Missing,Float64}}
_nan(y::MissingVec) = Float64[ismissing(v) ? NaN : v for v in y]
function _drop_unobserved(X::Matrix{Float64}, yv::Vector{Float64}, p::Integer)
    Y = reshape(yv, :, p)                           # n x p, by outputs
    keep = [!all(isnan, view(Y, t, :)) for t in 1:size(Y, 1)]
    all(keep) && return X, yv, keep
    return X[:, keep], vec(Y[keep, :]), keep
end
_no_missing(fs) = isposterior(fs) && error("posterior models do not take missing data (lmm_post_condition and the predictive logpdf are not served with NaN)")

function AbstractGPs.logpdf(fx::ByOutputsFill{HIPOILMM}, y::MissingVec)
    fs, H, σ², x = unpack(fx); _no_missing(fs)
    U, S, p, m = _hargs(H); X, yv, _ = _drop_unobserved(_xmat(x), _nan(y), p); d, n = size(X)
    out = Ref{Cdouble}(0.0)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S gps check(ccall((:lmm_oilmm_logpdf_missing, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, 1, out))
    end
    return out[]
end

function AbstractGPs.posterior(fx::ByOutputsFill{HIPOILMM}, y::MissingVec)
    fs, H, σ², x = unpack(fx); _no_missing(fs)
    U, S, p, m = _hargs(H); X, yv, _ = _drop_unobserved(_xmat(x), _nan(y), p); d, n = size(X)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S gps check(ccall((:lmm_oilmm_posterior_create_missing, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Ref{Ptr{Cvoid}}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, h))
    end
    return ILMM(HIPMOGP(fs.fs, h[], nothing), H)    # no training record: predictive gradients through NaN-carrying data are not built
end

# reference src/independent_mogp.jl:119-126; on a posterior: sequential conditioning (test/independent_mogp.jl:68-76)
function AbstractGPs.posterior(ft::ByOutputsFill{HIPMOGP}, y::AbstractVector{<:Real})
    X = _xmat(ft.x.x); d, n = size(X); m = length(ft.f.fs); yv = Vector{Float64}(y); σ² = noise_var(ft.Σy)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if isposterior(ft.f)
        U = Matrix{Float64}(I, m, m); S = ones(m)
        GC.@preserve X yv U S check(ccall((:lmm_post_condition, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
            ft.f.handle, U, S, m, m, σ², X, d, n, yv, h))
        return HIPMOGP(ft.f.fs, h[], _push_train(ft.f.train, X, σ², yv))
    end
    _gps(ft.f.fs) do gps, tags
        GC.@preserve X yv gps check(ccall((:lmm_mogp_posterior_create, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Ref{Ptr{Cvoid}}),
            X, d, n, yv, m, σ², gps, 0, m, h))
    end
    return HIPMOGP(ft.f.fs, h[], [(X, Float64(σ²), yv)])
end

# reference src/ilmm.jl:184-198 (one coupled (mn) x (mn) factorisation); on a posterior: TestUtils on `pi` (test/ilmm.jl:34-37)
function AbstractGPs.posterior(fx::ByOutputsFill{HIPDenseILMM}, y::AbstractVector{<:Real})
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); p, m = size(H); yv = Vector{Float64}(y)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if isposterior(f)
        GC.@preserve X yv check(ccall((:lmm_ilmm_post_condition, liblmm), Cint,
            (Ptr{Cvoid}, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{LmmJitters}, Ref{Ptr{Cvoid}}),
            f.handle, σ², X, d, n, yv, C_NULL, h))
        # (a latent view conditioned ON latent observations keeps no training record: its batches were observed through different H's)
        return ILMM(HIPMOGP(f.fs, h[], f.mix === nothing ? _push_train(f.train, X, σ², yv) : nothing), H)
    end
    Hm = Matrix{Float64}(H)
    _gps(f.fs) do gps, tags
        GC.@preserve X yv Hm gps check(ccall((:lmm_ilmm_posterior_create, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Ptr{Cvoid}}),
            X, d, n, yv, p, Hm, m, σ², gps, C_NULL, h))
    end
    return ILMM(HIPMOGP(f.fs, h[], [(X, Float64(σ²), yv)]), H)
end

# ---- mean_and_var / marginals / mean / var / mean_and_cov / cov --------------------------------------------------------
# Independent latents (OILMM prior or posterior, dense-H prior): reference src/oilmm.jl:57-76, src/ilmm.jl:108-145.
# want_var = false: means only -- mu + K(x*, x) alpha per latent, no triangular solve (the reference computes and discards
# the variances, src/ilmm.jl:142).
function _mean_var(fx, want_var::Bool)
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, ns = size(X); U, S, p, m = _hargs(H)
    M = Vector{Float64}(undef, ns * p); V = want_var ? similar(M) : Float64[]
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X U S gps M V check(ccall((:lmm_oilmm_mean_and_var, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint,
             Ptr{LmmJitters}, Ptr{Cdouble}, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, _ptr(S), p, m, 0, m, σ², 1, X, d, ns, C_NULL,
            M, want_var ? pointer(V) : Ptr{Cdouble}(C_NULL)))
    end
    return M, V
end
AbstractGPs.mean_and_var(fx::ByOutputsFill{HIPOILMM}) = _mean_var(fx, true)
AbstractGPs.mean(fx::ByOutputsFill{HIPOILMM}) = _mean_var(fx, false)[1]
AbstractGPs.var(fx::ByOutputsFill{HIPOILMM}) = _mean_var(fx, true)[2]

function AbstractGPs.mean_and_var(fx::ByOutputsFill{HIPDenseILMM})
    f = fx.f.f
    isposterior(f) || return _mean_var(fx, true)             # prior latents are independent: same mixing as the OILMM form
    unpack(fx)
    X = _xmat(fx.x.x); d, ns = size(X); p = size(fx.f.H, 1)
    M = Vector{Float64}(undef, ns * p); V = similar(M)
    GC.@preserve X M V check(ccall((:lmm_ilmm_post_mean_and_var, liblmm), Cint,
        (Ptr{Cvoid}, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{LmmJitters}, Ptr{Cdouble}, Ptr{Cdouble}),
        f.handle, noise_var(fx.Σy), X, d, ns, C_NULL, M, V))
    return M, V
end
AbstractGPs.mean(fx::ByOutputsFill{HIPDenseILMM}) = isposterior(fx.f.f) ? mean_and_var(fx)[1] : _mean_var(fx, false)[1]
AbstractGPs.var(fx::ByOutputsFill{HIPDenseILMM}) = mean_and_var(fx)[2]

# reference src/independent_mogp.jl:50,55: vcat of the latent marginals (+ Σy on the variances)
function AbstractGPs.mean_and_var(ft::ByOutputsFill{HIPMOGP})
    X = _xmat(ft.x.x); d, ns = size(X); m = length(ft.f.fs)
    M = Vector{Float64}(undef, ns * m); V = similar(M)
    _gps(isposterior(ft.f) ? nothing : ft.f.fs) do gps, tags
        GC.@preserve X gps M V check(ccall((:lmm_latent_marginals, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
            ft.f.handle, isposterior(ft.f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), m, X, d, ns, M, V))
    end
    return M, V .+ noise_var(ft.Σy)
end
AbstractGPs.mean(ft::ByOutputsFill{HIPMOGP}) = mean_and_var(ft)[1]
AbstractGPs.var(ft::ByOutputsFill{HIPMOGP}) = mean_and_var(ft)[2]

# reference src/ilmm.jl:132-147: full (p n*) x (p n*) covariance, small n* only (as in the reference)
function AbstractGPs.mean_and_cov(fx::Union{ByOutputsFill{HIPOILMM},ByOutputsFill{HIPDenseILMM}})
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, ns = size(X); U, S, p, m = _hargs(H)
    M = Vector{Float64}(undef, ns * p); Cm = Matrix{Float64}(undef, ns * p, ns * p)
    if isposterior(f) && S === nothing                         # coupled latents of the dense-H posterior
        GC.@preserve X M Cm check(ccall((:lmm_ilmm_post_mean_and_cov, liblmm), Cint,
            (Ptr{Cvoid}, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{LmmJitters}, Ptr{Cdouble}, Ptr{Cdouble}),
            f.handle, σ², X, d, ns, C_NULL, M, Cm))
        return M, Cm
    end
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X U S gps M Cm check(ccall((:lmm_lmm_mean_and_cov, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint,
             Ptr{LmmJitters}, Ptr{Cdouble}, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, _ptr(S), p, m, 0, m, σ², 1, X, d, ns, C_NULL, M, Cm))
    end
    return M, Cm
end
AbstractGPs.cov(fx::Union{ByOutputsFill{HIPOILMM},ByOutputsFill{HIPDenseILMM}}) = mean_and_cov(fx)[2]

# ---- rand: the normals are drawn HERE, in the reference's order (src/oilmm.jl:47,53: m blocks of n latent draws, then
# n*p noise draws; N samples = N repeats, src/ilmm.jl:90-92), so the same `rng` gives the same samples as the reference;
# ONE factorisation per latent serves all N samples (lmm_lmm_rand_multi) --------------------------------------------------
function _rand(rng::AbstractRNG, fx, N::Int)
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, ns = size(X); U, S, p, m = _hargs(H)
    z = Matrix{Float64}(undef, ns * m, N); ε = Matrix{Float64}(undef, ns * p, N)
    for q in 1:N
        z[:, q] = randn(rng, ns * m); ε[:, q] = randn(rng, ns * p)
    end
    out = Matrix{Float64}(undef, ns * p, N)
    if isposterior(f) && S === nothing                         # dense-H posterior: coupled latents, reference src/ilmm.jl:78-87
        for q in 1:N
            zq = z[:, q]; εq = ε[:, q]; oq = Vector{Float64}(undef, ns * p)
            GC.@preserve X zq εq oq check(ccall((:lmm_ilmm_post_rand, liblmm), Cint,
                (Ptr{Cvoid}, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmJitters}, Ptr{Cdouble}),
                f.handle, σ², 1, X, d, ns, zq, εq, C_NULL, oq))
            out[:, q] = oq
        end
        return out
    end
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X U S gps z ε out check(ccall((:lmm_lmm_rand_multi, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint, Cint,
             Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmJitters}, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, _ptr(S), p, m, 0, m, σ², 1, X, d, ns, N, z, ε, C_NULL, out))
    end
    return out
end
const HIPLMMFinite = Union{ByOutputsFill{HIPOILMM},ByOutputsFill{HIPDenseILMM}}
AbstractGPs.rand(rng::AbstractRNG, fx::HIPLMMFinite) = vec(_rand(rng, fx, 1))          # src/oilmm.jl:40-54, src/ilmm.jl:78-87
AbstractGPs.rand(rng::AbstractRNG, fx::HIPLMMFinite, N::Int) = _rand(rng, fx, N)       # src/ilmm.jl:90-92

# reference src/independent_mogp.jl:83-96: vcat(rand(rng, f_l(x, σ²))): latent jitter = σ², H = I, no extra noise term
function _rand_mogp(rng::AbstractRNG, ft, N::Int)
    X = _xmat(ft.x.x); d, ns = size(X); m = length(ft.f.fs); σ² = noise_var(ft.Σy)
    U = Matrix{Float64}(I, m, m)
    z = Matrix{Float64}(undef, ns * m, N)
    for q in 1:N
        z[:, q] = randn(rng, ns * m)
    end
    out = Matrix{Float64}(undef, ns * m, N)
    jit = Ref(LmmJitters(1e-9, σ², σ²))
    _gps(isposterior(ft.f) ? nothing : ft.f.fs) do gps, tags
        GC.@preserve X U gps z out check(ccall((:lmm_lmm_rand_multi, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint, Cint,
             Ptr{Cdouble}, Ptr{Cdouble}, Ref{LmmJitters}, Ptr{Cdouble}),
            ft.f.handle, isposterior(ft.f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, C_NULL, m, m, 0, m, σ², 0, X, d, ns, N, z, C_NULL, jit, out))
    end
    return out
end
AbstractGPs.rand(rng::AbstractRNG, ft::ByOutputsFill{HIPMOGP}) = vec(_rand_mogp(rng, ft, 1))
AbstractGPs.rand(rng::AbstractRNG, ft::ByOutputsFill{HIPMOGP}, N::Int) = _rand_mogp(rng, ft, N)

# reference src/ilmm.jl:95-106 and src/independent_mogp.jl:102-113: `rand!(rng, fx, y)` (what AbstractGPs.TestUtils reaches through
# Distributions) fills y with one sample (vector, or one column) or N samples (N columns) -- the draws come from the methods above, so the
# normals are consumed in the reference's order
function Distributions._rand!(rng::AbstractRNG, fx::Union{HIPLMMFinite,ByOutputsFill{HIPMOGP}}, y::AbstractVecOrMat{<:Real})
    N = size(y, 2)
    if N == 1
        y .= AbstractGPs.rand(rng, fx)
    else
        y .= AbstractGPs.rand(rng, fx, N)
    end
end

# ---- MOInputIsotopicByFeatures (reference src/independent_mogp.jl:128-229) --------------------------------------------------------
# The reference serves by-features inputs of an IndependentMOGP by re-ordering to by-outputs, calling the by-outputs method and
# permuting the result back (indices_which_reorder_*, :135-147).  Same here: the by-outputs methods above do the work, the
# permutation of the length-(n p) vectors is the library's (lmm_reorder: to_outputs = 1 is `v[indices_which_reorder_features_to_outputs]`,
# 0 the inverse), and the (n p) x (n p) covariance is permuted on the host with the reference's own index vectors.
const ByFeatures{F} = FiniteGP{<:F,<:MOInputIsotopicByFeatures,<:Diagonal{<:Real}}
const ByFeaturesFill{F} = FiniteGP{<:F,<:MOInputIsotopicByFeatures,<:Diagonal{<:Real,<:Fill}}
function _reorder(v::AbstractVector{<:Real}, n::Integer, p::Integer, to_outputs::Bool)
    vin = Vector{Float64}(v); out = Vector{Float64}(undef, n * p)
    GC.@preserve vin out check(ccall((:lmm_reorder, liblmm), Cint, (Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}),
        vin, n, p, to_outputs ? 1 : 0, out))
    return out
end
_nx(x::MOInputIsotopicByFeatures) = length(x.x)
_by_outputs(x::MOInputIsotopicByFeatures) = MOInputIsotopicByOutputs(x.x, x.out_dim)                      # src/independent_mogp.jl:149
_by_outputs(Σy::Diagonal{<:Real,<:Fill}, x::MOInputIsotopicByFeatures) = Σy                                # :155
_by_outputs(Σy::Diagonal{<:Real}, x::MOInputIsotopicByFeatures) = Diagonal(_reorder(Σy.diag, _nx(x), x.out_dim, true))   # :151-153
_by_outputs(ft::ByFeatures{HIPMOGP}) = FiniteGP(ft.f, _by_outputs(ft.x), _by_outputs(ft.Σy, ft.x))        # :157-159
_to_features(v::AbstractVector{<:Real}, x::MOInputIsotopicByFeatures) = _reorder(v, _nx(x), x.out_dim, false)

# src/independent_mogp.jl:222-229 (any Diagonal noise: a Fill stays a Fill and reaches the ByOutputsFill method; a general diagonal is
# permuted with the data into a Diagonal{Float64,Vector{Float64}} and reaches the per-point-noise method above, lmm_mogp_logpdf_diag)
AbstractGPs.logpdf(ft::ByFeatures{HIPMOGP}, y::AbstractVector{<:Real}) =
    logpdf(_by_outputs(ft), _reorder(y, _nx(ft.x), ft.x.out_dim, true))
# src/independent_mogp.jl:217-220: the by-outputs sample, permuted (the normals are drawn latent by latent, as in the reference)
AbstractGPs.rand(rng::AbstractRNG, ft::ByFeaturesFill{HIPMOGP}) = _to_features(rand(rng, _by_outputs(ft)), ft.x)
function AbstractGPs.rand(rng::AbstractRNG, ft::ByFeaturesFill{HIPMOGP}, N::Int)
    return reduce(hcat, [rand(rng, ft) for _ in 1:N])
end
# src/independent_mogp.jl:165-175 (mean, var) on the finite GP: by-outputs marginals, permuted
function AbstractGPs.mean_and_var(ft::ByFeaturesFill{HIPMOGP})
    M, V = mean_and_var(_by_outputs(ft))
    return _to_features(M, ft.x), _to_features(V, ft.x)
end
AbstractGPs.mean(ft::ByFeaturesFill{HIPMOGP}) = mean_and_var(ft)[1]
AbstractGPs.var(ft::ByFeaturesFill{HIPMOGP}) = mean_and_var(ft)[2]
# src/independent_mogp.jl:177-182: C_by_outputs[idx, idx] (block-diagonal latent covariances + Σy, lmm_lmm_mean_and_cov with U = I)
function AbstractGPs.mean_and_cov(ft::ByOutputsFill{HIPMOGP})
    X = _xmat(ft.x.x); d, ns = size(X); m = length(ft.f.fs); σ² = noise_var(ft.Σy)
    U = Matrix{Float64}(I, m, m)
    M = Vector{Float64}(undef, ns * m); Cm = Matrix{Float64}(undef, ns * m, ns * m)
    jit = Ref(LmmJitters(1e-9, 0.0, 0.0))                   # cov(f, x) + Σy of a bare MOGP: no latent jitter (src/independent_mogp.jl:60-63)
    _gps(isposterior(ft.f) ? nothing : ft.f.fs) do gps, tags
        GC.@preserve X U gps M Cm check(ccall((:lmm_lmm_mean_and_cov, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Cdouble, Cint, Ptr{Cdouble}, Cint, Cint,
             Ref{LmmJitters}, Ptr{Cdouble}, Ptr{Cdouble}),
            ft.f.handle, isposterior(ft.f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, Ptr{Cdouble}(C_NULL), m, m, 0, m, σ², 1, X, d, ns, jit, M, Cm))
    end
    return M, Cm
end
AbstractGPs.cov(ft::ByOutputsFill{HIPMOGP}) = mean_and_cov(ft)[2]
function AbstractGPs.mean_and_cov(ft::ByFeaturesFill{HIPMOGP})
    M, Cm = mean_and_cov(_by_outputs(ft))
    idx = LinearMixingModels.indices_which_reorder_outputs_to_features(_by_outputs(ft.x))
    return _to_features(M, ft.x), Cm[idx, idx]
end
AbstractGPs.cov(ft::ByFeaturesFill{HIPMOGP}) = mean_and_cov(ft)[2]
# conditioning on by-features data: reorder, then the by-outputs posterior (the reference reaches the same through reorder_by_outputs)
AbstractGPs.posterior(ft::ByFeaturesFill{HIPMOGP}, y::AbstractVector{<:Real}) =
    posterior(_by_outputs(ft), _reorder(y, _nx(ft.x), ft.x.out_dim, true))
function Distributions._rand!(rng::AbstractRNG, ft::ByFeaturesFill{HIPMOGP}, y::AbstractVecOrMat{<:Real})
    N = size(y, 2)
    if N == 1
        y .= AbstractGPs.rand(rng, ft)
    else
        y .= AbstractGPs.rand(rng, ft, N)
    end
end

# ---- cov(f, x, y), mean(f, x), var(f, x) on the GP itself (AbstractGPs' internal interface) --------------------------------------
# reference src/independent_mogp.jl:66-71 (x, y by outputs: Matrix(BlockDiagonal(cov(f_l, x.x, y.x)))) and :184-215 (either input by
# features: the same blocks at rows / columns permuted with indices_which_reorder_outputs_to_features) -- the library writes every
# block at its final place (lmm_mogp_cross_cov); cov(f, x) = cov(f, x, x) (:60-63, :177-182).  Reference tests:
# test/independent_mogp.jl:136-141.
const MOIsotopic = Union{MOInputIsotopicByOutputs,MOInputIsotopicByFeatures}
_byfeat(::MOInputIsotopicByOutputs) = Cint(0)
_byfeat(::MOInputIsotopicByFeatures) = Cint(1)
function AbstractGPs.cov(f::HIPMOGP, x::MOIsotopic, y::MOIsotopic)
    m = length(f.fs)
    (x.out_dim == m && y.out_dim == m) || throw(ErrorException("out dim of x != out dim of f."))
    X = _xmat(x.x); Y = _xmat(y.x); d, n = size(X); n2 = size(Y, 2)
    Cm = Matrix{Float64}(undef, m * n, m * n2)
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X Y gps Cm check(ccall((:lmm_mogp_cross_cov, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), m, 0, m, X, d, n, _byfeat(x), Y, n2, _byfeat(y), Cm))
    end
    return Cm
end
AbstractGPs.cov(f::HIPMOGP, x::MOIsotopic) = cov(f, x, x)
# reference src/independent_mogp.jl:50,55 (by outputs: vcat of the latent marginals) and :169-175 (by features: permuted)
function _mean_var(f::HIPMOGP, x::MOIsotopic)
    m = length(f.fs)
    x.out_dim == m || throw(ErrorException("out dim of x != out dim of f."))
    X = _xmat(x.x); d, ns = size(X)
    M = Vector{Float64}(undef, ns * m); V = similar(M)
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X gps M V check(ccall((:lmm_latent_marginals, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), m, X, d, ns, M, V))
    end
    x isa MOInputIsotopicByFeatures && return _to_features(M, x), _to_features(V, x)
    return M, V
end
AbstractGPs.mean(f::HIPMOGP, x::MOIsotopic) = _mean_var(f, x)[1]
AbstractGPs.var(f::HIPMOGP, x::MOIsotopic) = _mean_var(f, x)[2]

# ---- gradients: ChainRulesCore.rrule around the ccall --------------------------------------------------------------------
# The reference's tests take Zygote.gradient(logpdf, fx, y) on prior and posterior models (test/oilmm.jl:31-32,
# test/ilmm.jl:31-32, test/independent_mogp.jl:65-66).  A ccall is opaque to Zygote, so the pullbacks come from the library
# (lmm_oilmm_logpdf_grad, lmm_ilmm_logpdf_grad, lmm_oilmm_post_logpdf_grad_seq, lmm_ilmm_post_logpdf_grad_seq, and their _x forms, which
# add d logpdf / d x) and are mapped onto the reference's structs.

# kernel cotangent: the library differentiates w.r.t. the EFFECTIVE (variance, lengthscale); the chain rule through the
# kernel's construction: ScaledKernel: v = v_inner σ² -> d/dσ² = gv v_inner; ScaleTransform: ℓ = ℓ_inner / s -> d/ds = -gl ℓ_inner / s².
# ga: d/d ard[k] of an ARD latent (lmm_ard_grad; gl is then d/d the common multiplier).  ARDTransform(v): ard = ard_inner ./ v
# -> d/dv_k = -ga_k ard_inner_k / v_k^2 (with no inner factors, ℓ_k = multiplier / v_k: d/dv_k = -ℓ_k^2 d/dℓ_k), d/d ard_inner = ga ./ v.
# gα: d/d alpha of an RQ latent (lmm_kernel_tag_alpha_grad), d/d rho of a periodic one (lmm_kernel_tag_rho_grad), the tuple
# (rho = d/d rho, decay = d/d decay) of a locally periodic one (lmm_kernel_tag_decay_grad), nothing otherwise
# gt: the per-term gradients of a sum latent (_tag_grads(...).terms), nothing otherwise.
_ktangent(k::Kernel, gv, gl, ga=nothing, gα=nothing, gt=nothing) = NoTangent()            # SEKernel() etc. carry no parameters
_ktangent(k::RationalQuadraticKernel, gv, gl, ga=nothing, gα=nothing, gt=nothing) =
    gα === nothing ? NoTangent() : Tangent{typeof(k)}(; α=[gα], metric=NoTangent())
# PeriodicKernel: gα carries d/d rho, the derivative along r = fill(rho, d); it is spread evenly over the d entries of r (their sum is
# d/d rho, which is all the library's one-rho kernel defines; exact for d = 1).
_ktangent(k::PeriodicKernel, gv, gl, ga=nothing, gα=nothing, gt=nothing) =
    gα === nothing ? NoTangent() : Tangent{typeof(k)}(; r=fill(gα / length(k.r), length(k.r)))
# SHOKernel: gα carries d/d quality (lmm_kernel_tag_quality_grad)
_ktangent(k::SHOKernel, gv, gl, ga=nothing, gα=nothing, gt=nothing) =
    gα === nothing ? NoTangent() : Tangent{typeof(k)}(; quality=[gα])
function _ktangent(k::ScaledKernel, gv, gl, ga=nothing, gα=nothing, gt=nothing)
    (_, vin, _) = _desc(k.kernel)
    return Tangent{typeof(k)}(; kernel=_ktangent(k.kernel, gv * only(k.σ²), gl, ga, gα, gt), σ²=[gv * vin])
end
function _ktangent(k::TransformedKernel{<:Kernel,<:ScaleTransform}, gv, gl, ga=nothing, gα=nothing, gt=nothing)
    (_, _, lin) = _desc(k.kernel); s = only(k.transform.s)
    gs = -gl * lin / s^2
    if gα isa NamedTuple          # a locally periodic product inside: the transform scales its decay too (decay = decay_inner / s)
        gs -= gα.decay * _decay(k.kernel) / s^2
        gα = (rho = gα.rho, decay = gα.decay / s)
    end
    return Tangent{typeof(k)}(; kernel=_ktangent(k.kernel, gv, gl / s, ga, gα, gt), transform=Tangent{typeof(k.transform)}(; s=[gs]))
end
# The locally periodic product: gα = (rho, decay).  The periodic factor takes (gl, ga, rho) as a periodic latent would, the SE factor the
# decay cotangent as the lengthscale gradient of its ScaleTransform (a bare SqExponentialKernel carries no parameter); gv belongs to the
# ScaledKernel around the product.
function _ktangent(k::KernelProduct, gv, gl, ga=nothing, gα=nothing, gt=nothing)
    (se, per) = _lpfactors(k)
    tper = _ktangent(per, 0.0, gl, ga, gα === nothing ? nothing : gα.rho)
    tse = _ktangent(se, 0.0, gα === nothing ? 0.0 : gα.decay)
    return Tangent{typeof(k)}(; kernels=Tuple(t === se ? tse : tper for t in k.kernels))
end
# A sum: the outer (gv, gl) went to the ScaledKernel / ScaleTransform around it; each term gets its own tangent from gt, in the
# flattened order of _terms.  A nested sum (flattened because its wrappers have unit scale) takes the next entries; its wrappers see
# gv = sum_c v_c d/dv_c and gl = sum_c l_c d/dl_c, the derivatives with respect to a scale of 1 on its variance and lengthscale.
function _ktangent(k::KernelSum, gv, gl, ga=nothing, gα=nothing, gt=nothing)
    gt === nothing && return NoTangent()
    i = Ref(0)
    function term(t)
        tt = _terms(t)
        if tt !== nothing
            n = length(tt); sub = gt[i[] + 1:i[] + n]; i[] += n
            gv = sum(_desc(tk)[2] * g.variance for (tk, g) in zip(tt, sub))
            gl = sum(_desc(tk)[3] * g.lengthscale for (tk, g) in zip(tt, sub))
            return _ktangent(t, gv, gl, nothing, nothing, sub)
        end
        g = gt[i[] += 1]
        return _ktangent(t, g.variance, g.lengthscale, g.ard, g.alpha)
    end
    return Tangent{typeof(k)}(; kernels=Tuple(term(t) for t in k.kernels))
end
function _ktangent(k::TransformedKernel{<:Kernel,<:ARDTransform}, gv, gl, ga=nothing, gα=nothing, gt=nothing)
    v = Vector{Float64}(k.transform.v); ain = _ard(k.kernel)
    ga === nothing && return Tangent{typeof(k)}(; kernel=_ktangent(k.kernel, gv, gl, nothing, gα, gt), transform=NoTangent())
    a0 = ain === nothing ? ones(length(v)) : ain
    return Tangent{typeof(k)}(; kernel=_ktangent(k.kernel, gv, gl, ain === nothing ? nothing : ga ./ v, gα, gt),
                              transform=Tangent{typeof(k.transform)}(; v=-ga .* a0 ./ v .^ 2))
end
_mtangent(::AbstractGPs.ZeroMean, g) = NoTangent()
_mtangent(m::AbstractGPs.ConstMean, g) = Tangent{typeof(m)}(; c=g)
# gard: nothing, or per latent the tag gradients of _ard_grads (nothing for an untagged latent)
_tagfield(gard, l, s) = (gard === nothing || gard[l] === nothing) ? nothing : getfield(gard[l], s)
_scaleα(Δ, ::Nothing) = nothing
_scaleα(Δ, g::Real) = Δ * g
_scaleα(Δ, g::NamedTuple) = map(x -> Δ * x, g)          # (rho, decay) of a locally periodic latent
_fstangent(fs::Vector{<:AbstractGP}, gg::Vector{LmmGpGrad}, Δ, gard=nothing) =
    [Tangent{typeof(f)}(; mean=_mtangent(f.mean, Δ * g.mean),
                          kernel=_ktangent(f.kernel, Δ * g.variance, Δ * g.lengthscale,
                                           (ga = _tagfield(gard, l, :ard); ga === nothing ? nothing : Δ .* ga),
                                           _scaleα(Δ, _tagfield(gard, l, :alpha)),
                                           (gt = _tagfield(gard, l, :terms); gt === nothing ? nothing :
                                            [(variance = Δ * t.variance, lengthscale = Δ * t.lengthscale,
                                              ard = t.ard === nothing ? nothing : Δ .* t.ard, alpha = _scaleα(Δ, t.alpha))
                                             for t in gt])))
     for (l, (f, g)) in enumerate(zip(fs, gg))]
_noise_tangent(fx, g) = Tangent{typeof(fx.Σy)}(; diag=Tangent{typeof(fx.Σy.diag)}(; value=g))     # Fill(σ², n p): one parameter
# Input locations: the library's d logpdf / d x (G, d x n) as the cotangent of the FiniteGP's x = MOInputIsotopicByOutputs(inner, p):
# a Vector input gets a vector, ColVecs its X (d x n), RowVecs its X transposed (n x d).  INPUT_GRADIENTS[] = false skips the input
# gradient (the lmm_*_grad entry points without _x; one read of each latent's K^-1 less) and leaves x without a cotangent.
const INPUT_GRADIENTS = Ref(true)
_xtangent(x::AbstractVector{<:Real}, G) = vec(G)
_xtangent(x::ColVecs, G) = Tangent{typeof(x)}(; X=G)
_xtangent(x::RowVecs, G) = Tangent{typeof(x)}(; X=permutedims(G))
_xtangent(x, G) = NoTangent()
_motangent(x::MOInputIsotopicByOutputs, G) = G === nothing ? NoTangent() : Tangent{typeof(x)}(; x=_xtangent(x.x, G), out_dim=NoTangent())
_htangent(H::Orthogonal, gU, gS) = Tangent{typeof(H)}(; U=gU, S=Tangent{typeof(H.S)}(; diag=gS))

function ChainRulesCore.rrule(::typeof(AbstractGPs.logpdf), fx::ByOutputsFill{HIPOILMM}, y::Union{AbstractVector{<:Real},MissingVec})
    y isa MissingVec && return _logpdf_missing_rrule(fx, y)       # missing observations: below
    fs, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); gard = nothing; yv = Vector{Float64}(y)
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * p); gS = Vector{Float64}(undef, m); gU = Matrix{Float64}(undef, p, m)
    gg = Vector{LmmGpGrad}(undef, m)
    wantx = INPUT_GRADIENTS[]; gx = wantx ? Matrix{Float64}(undef, d, n) : nothing
    if isposterior(fs)
        fs.train === nothing && error("this posterior does not carry its training data")
        X0, bn, bs, y0 = _merged_train(fs.train, p); n0 = size(X0, 2); gy0 = Vector{Float64}(undef, n0 * p); gb = similar(bs)
        gx0 = wantx ? Matrix{Float64}(undef, d, n0) : nothing
        _gps(fs.fs) do gps, tags
            if wantx
                GC.@preserve X0 bn bs y0 X yv U S gps gy0 gy gb gS gU gg gx0 gx check(ccall((:lmm_oilmm_post_logpdf_grad_seq_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}, Ptr{Cdouble}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, p, U, S, m, σ², gps, 0, m, 1, val, gy0, gy, gb, gσ, gS, gU, gg, gx0, gx))
            else
                GC.@preserve X0 bn bs y0 X yv U S gps gy0 gy gb gS gU gg check(ccall((:lmm_oilmm_post_logpdf_grad_seq, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, p, U, S, m, σ², gps, 0, m, 1, val, gy0, gy, gb, gσ, gS, gU, gg))
            end
            gard = _ard_grads(tags, d)
        end
        # The library returns TOTAL derivatives through the posterior, including those w.r.t. the training data (gy0) and the
        # training noise (gb, one per conditioning batch).  The posterior model object has no differentiable slot for (x, σ², y) -- they entered through
        # `posterior`, whose own rrule would be the place to receive them -- so THIS pullback propagates the cotangents of the
        # latent GPs, H, the predictive noise and y* only; gy0 / gb are NOT propagated by it.  Callers who differentiate
        # θ -> logpdf(posterior(f_θ(x, σ²), y)(x*, σ²*), y*) end to end use `predictive_logpdf_and_gradient` below, which returns them.
        fs.last_train_cotangents[] = _split_train(gy0, gb, bn, p, gx0)      # one entry per conditioning batch when there are several
    else
        _gps(fs.fs) do gps, tags
            if wantx
                GC.@preserve X yv U S gps gy gS gU gg gx check(ccall((:lmm_oilmm_logpdf_grad_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
                     Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}),
                    X, d, n, yv, p, U, S, m, σ², gps, 0, m, 1, val, gy, gσ, gS, gU, gg, gx))
            else
                GC.@preserve X yv U S gps gy gS gU gg check(ccall((:lmm_oilmm_logpdf_grad, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
                     Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X, d, n, yv, p, U, S, m, σ², gps, 0, m, 1, val, gy, gσ, gS, gU, gg))
            end
            gard = _ard_grads(tags, d)
        end
    end
    function logpdf_pullback(Δ)
        dlat = Tangent{typeof(fs)}(; fs=_fstangent(fs.fs, gg, Δ, gard))
        dx = _motangent(fx.x, gx === nothing ? nothing : Δ .* gx)
        dfx = Tangent{typeof(fx)}(; x=dx, f=Tangent{typeof(fx.f)}(; f=dlat, H=_htangent(H, Δ .* gU, Δ .* gS)), Σy=_noise_tangent(fx, Δ * gσ[]))
        return NoTangent(), dfx, Δ .* gy
    end
    return val[], logpdf_pullback
end

# elbo(VFE(f(z, ε)), fx, y) (lmm_oilmm_elbo_grad; include/lmm_hip.h "inducing points"): cotangents for the latent GPs' kernel parameters
# and means, H = (U, S), σ², y and the inducing inputs z, in the way the logpdf rrule above is written.  The model's cotangent is
# attached to fx.f: vfe.fz.f is the same model, and its slot in the VFE's tangent carries only z (a model given twice would otherwise
# receive its cotangent twice).  The jitter ε gets no cotangent.  There is no rrule for dtc.
function ChainRulesCore.rrule(::typeof(AbstractGPs.elbo), vfe::VFE{<:ByOutputsFill{HIPOILMM}}, fx::ByOutputsFill{HIPOILMM},
                              y::AbstractVector{<:Real})
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("inducing-point inference is served on a prior OILMM only")
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); gard = nothing; yv = Vector{Float64}(y)
    Z = _xmat(vfe.fz.x.x); ε = Float64(noise_var(vfe.fz.Σy)); nz = size(Z, 2)
    size(Z, 1) == d || error("the inducing inputs have d = $(size(Z, 1)), the inputs d = $d")
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * p); gS = Vector{Float64}(undef, m); gU = Matrix{Float64}(undef, p, m)
    gg = Vector{LmmGpGrad}(undef, m); gz = Matrix{Float64}(undef, d, nz)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S Z gps gy gS gU gg gz check(ccall((:lmm_oilmm_elbo_grad, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint,
             Ptr{Cdouble}, Cint, Cdouble, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad},
             Ptr{Cdouble}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, Z, nz, ε, 1, val, gy, gσ, gS, gU, gg, gz))
        gard = _ard_grads(tags, d)
    end
    function elbo_pullback(Δ)
        dlat = Tangent{typeof(fs)}(; fs=_fstangent(fs.fs, gg, Δ, gard))
        dfx = Tangent{typeof(fx)}(; x=NoTangent(), f=Tangent{typeof(fx.f)}(; f=dlat, H=_htangent(H, Δ .* gU, Δ .* gS)),
                                  Σy=_noise_tangent(fx, Δ * gσ[]))
        dvfe = Tangent{typeof(vfe)}(; fz=Tangent{typeof(vfe.fz)}(; x=_motangent(vfe.fz.x, Δ .* gz), f=NoTangent(), Σy=NoTangent()))
        return NoTangent(), dvfe, dfx, Δ .* gy
    end
    return val[], elbo_pullback
end

# statespace_logpdf(fx, y) (lmm_oilmm_logpdf_grad_statespace_x; include/lmm_hip.h "state space"): cotangents for the latent GPs' variances,
# lengthscales and means, σ², y (0 at missing entries, in the caller's order of points) and, for complete data, H = (U, S), in the way
# the logpdf rrules above are written and in O(n).  With `missing` or NaN in y the library builds no derivative through the per-point
# projection, so H gets ZeroTangent, as in _logpdf_missing_rrule.  The inputs fx.x get the library's d logpdf / d x (O(n) as well, in
# the caller's order of points, 0 at points without observations; NaN in y is served), unless INPUT_GRADIENTS[] = false.
function ChainRulesCore.rrule(::typeof(statespace_logpdf), fx::ByOutputsFill{HIPOILMM}, y::AbstractVector; with_regulariser::Bool=true)
    fs, H, σ², x = unpack(fx)
    isposterior(fs) && error("state-space inference is served on a prior OILMM only")
    U, S, p, m = _hargs(H)
    xv, yv, perm, n = _statespace_sorted(x, y, p, nothing)
    complete = !any(isnan, yv)
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * p); gS = Vector{Float64}(undef, m); gU = Matrix{Float64}(undef, p, m)
    gg = Vector{LmmGpGrad}(undef, m); gard = nothing
    gx = INPUT_GRADIENTS[] ? Vector{Float64}(undef, n) : nothing
    _gps(fs.fs) do gps, tags
        GC.@preserve xv yv U S gps gy gS gU gg gx check(ccall((:lmm_oilmm_logpdf_grad_statespace_x, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
             Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}),
            xv, n, yv, p, U, S, m, σ², gps, 0, m, Cint(with_regulariser), val, gy, gσ,
            complete ? pointer(gS) : Ptr{Cdouble}(C_NULL), complete ? pointer(gU) : Ptr{Cdouble}(C_NULL), gg,
            gx === nothing ? Ptr{Cdouble}(C_NULL) : pointer(gx)))
        gard = _ard_grads(tags, 1)
    end
    gfull = similar(reshape(gy, n, p)); gfull[perm, :] = reshape(gy, n, p)      # back in the caller's order
    gxfull = gx === nothing ? nothing : (g = similar(gx); g[perm] = gx; g)
    function statespace_logpdf_pullback(Δ)
        dlat = Tangent{typeof(fs)}(; fs=_fstangent(fs.fs, gg, Δ, gard))
        dH = complete ? _htangent(H, Δ .* gU, Δ .* gS) : ZeroTangent()
        dx = _motangent(fx.x, gxfull === nothing ? nothing : Δ .* gxfull)
        dfx = Tangent{typeof(fx)}(; x=dx, f=Tangent{typeof(fx.f)}(; f=dlat, H=dH), Σy=_noise_tangent(fx, Δ * gσ[]))
        return NoTangent(), dfx, Δ .* vec(gfull)
    end
    return val[], statespace_logpdf_pullback
end

# logpdf with missing observations (lmm_oilmm_logpdf_grad_missing): cotangents for the latent GPs, the noise and the observed entries
# of y (0 at the missing ones); the library builds no derivative through the per-point projection, so H gets ZeroTangent.  Reached
# from the OILMM logpdf rrule above, whose signature admits a y with `missing`.
function _logpdf_missing_rrule(fx::ByOutputsFill{HIPOILMM}, y::MissingVec)
    fs, H, σ², x = unpack(fx); _no_missing(fs)
    U, S, p, m = _hargs(H); X, yv, keep = _drop_unobserved(_xmat(x), _nan(y), p); d, n = size(X); gard = nothing
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * p); gg = Vector{LmmGpGrad}(undef, m)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S gps gy gg check(ccall((:lmm_oilmm_logpdf_grad_missing, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
             Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{LmmGpGrad}),
            X, d, n, yv, p, U, S, m, σ², gps, 0, m, 1, val, gy, gσ, gg))
        gard = _ard_grads(tags, d)
    end
    gfull = zeros(length(keep), p); gfull[keep, :] = reshape(gy, :, p)
    function logpdf_missing_pullback(Δ)
        dlat = Tangent{typeof(fs)}(; fs=_fstangent(fs.fs, gg, Δ, gard))
        dfx = Tangent{typeof(fx)}(; x=NoTangent(), f=Tangent{typeof(fx.f)}(; f=dlat, H=ZeroTangent()), Σy=_noise_tangent(fx, Δ * gσ[]))
        return NoTangent(), dfx, Δ .* vec(gfull)
    end
    return val[], logpdf_missing_pullback
end

# Value, pullback-at-1 and the training cotangents of the predictive logpdf in one call: what an end-to-end differentiation of
# θ -> logpdf(posterior(f_θ(x, σ²), y)(x*, σ²*), y*) needs beyond the rrule above (whose pullback cannot return d/dy_train, d/dσ²_train).
function predictive_logpdf_and_gradient(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real})
    val, back = ChainRulesCore.rrule(AbstractGPs.logpdf, fx, y)
    _, dfx, dy = back(1.0)
    tr = unpack(fx)[1].last_train_cotangents[]
    return (value=val, fx=dfx, y=dy, y_train=(tr === nothing ? nothing : tr.y_train), sigma2_train=(tr === nothing ? nothing : tr.sigma2_train),
            x_train=(tr === nothing ? nothing : tr.x_train))
end

# IndependentMOGP (reference test/independent_mogp.jl:65-66): the OILMM with U = I, S = 1 and no regulariser
function ChainRulesCore.rrule(::typeof(AbstractGPs.logpdf), ft::ByOutputsFill{HIPMOGP}, y::AbstractVector{<:Real})
    f = ft.f; X = _xmat(ft.x.x); d, n = size(X); m = length(f.fs); σ² = noise_var(ft.Σy)
    U = Matrix{Float64}(I, m, m); S = ones(m); gard = nothing; yv = Vector{Float64}(y)
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * m); gg = Vector{LmmGpGrad}(undef, m)
    wantx = INPUT_GRADIENTS[]; gx = wantx ? Matrix{Float64}(undef, d, n) : nothing
    if isposterior(f)
        f.train === nothing && error("this posterior does not carry its training data")
        X0, bn, bs, y0 = _merged_train(f.train, m); n0 = size(X0, 2)
        _gps(f.fs) do gps, tags
            if wantx        # (d/dx of the training points is not kept: this pullback does not return the training cotangents)
                GC.@preserve X0 bn bs y0 X yv U S gps gy gg gx check(ccall((:lmm_oilmm_post_logpdf_grad_seq_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}, Ptr{Cdouble}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, m, U, S, m, σ², gps, 0, m, 0, val, C_NULL, gy, C_NULL, gσ, C_NULL, C_NULL, gg,
                    C_NULL, gx))
            else
                GC.@preserve X0 bn bs y0 X yv U S gps gy gg check(ccall((:lmm_oilmm_post_logpdf_grad_seq, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, m, U, S, m, σ², gps, 0, m, 0, val, C_NULL, gy, C_NULL, gσ, C_NULL, C_NULL, gg))
            end
            gard = _ard_grads(tags, d)
        end
    else
        _gps(f.fs) do gps, tags
            if wantx
                GC.@preserve X yv U S gps gy gg gx check(ccall((:lmm_oilmm_logpdf_grad_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
                     Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}),
                    X, d, n, yv, m, U, S, m, σ², gps, 0, m, 0, val, gy, gσ, C_NULL, C_NULL, gg, gx))
            else
                GC.@preserve X yv U S gps gy gg check(ccall((:lmm_oilmm_logpdf_grad, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint,
                     Ref{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X, d, n, yv, m, U, S, m, σ², gps, 0, m, 0, val, gy, gσ, C_NULL, C_NULL, gg))
            end
            gard = _ard_grads(tags, d)
        end
    end
    function logpdf_pullback(Δ)
        dx = _motangent(ft.x, gx === nothing ? nothing : Δ .* gx)
        dft = Tangent{typeof(ft)}(; x=dx, f=Tangent{typeof(f)}(; fs=_fstangent(f.fs, gg, Δ, gard)), Σy=_noise_tangent(ft, Δ * gσ[]))
        return NoTangent(), dft, Δ .* gy
    end
    return val[], logpdf_pullback
end

# dense-H ILMM, prior and posterior (reference test/ilmm.jl:31-32): the reference's (mn) x (mn) operation + its explicit inverse;
# the posterior's predictive logpdf as the joint density of (y, y*) under two-block noise minus the density of y
function ChainRulesCore.rrule(::typeof(AbstractGPs.logpdf), fx::ByOutputsFill{HIPDenseILMM}, y::AbstractVector{<:Real})
    f, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); p, m = size(H); gard = nothing; Hm = Matrix{Float64}(H); yv = Vector{Float64}(y)
    val = Ref{Cdouble}(0.0); gσ = Ref{Cdouble}(0.0)
    gy = Vector{Float64}(undef, n * p); gH = Matrix{Float64}(undef, p, m); gg = Vector{LmmGpGrad}(undef, m)
    wantx = INPUT_GRADIENTS[]; gx = wantx ? Matrix{Float64}(undef, d, n) : nothing
    if isposterior(f) && f.mix !== nothing
        # the latent view of a dense-H posterior (latent_view; reference src/ilmm.jl:39 on :196-197): here H = I_m, p = m, y = latent
        # observations; the conditioning batches were observed through f.mix.  d/d(mix) and the training cotangents have no slot in
        # this model's tangent (its H is the constant I): they are left in last_train_cotangents.
        f.train === nothing && error("gradient of the latent view after conditioning ON latent observations is not built")
        Hp = f.mix::Matrix{Float64}; pp = size(Hp, 1)
        X0, bn, bs, y0 = _merged_train(f.train, pp); n0 = size(X0, 2); gy0 = Vector{Float64}(undef, n0 * pp); gb = similar(bs)
        gHp = Matrix{Float64}(undef, pp, m); gx0 = wantx ? Matrix{Float64}(undef, d, n0) : nothing
        _gps(f.fs) do gps, tags
            if wantx
                GC.@preserve X0 bn bs y0 X yv Hp gps gy0 gy gb gHp gg gx0 gx check(ccall((:lmm_ilmm_post_latent_logpdf_grad_seq_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint,
                     Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, pp, Hp, m, σ², gps, C_NULL, val, gy0, gy, gb, gσ, gHp, gg, gx0, gx))
            else
                GC.@preserve X0 bn bs y0 X yv Hp gps gy0 gy gb gHp gg check(ccall((:lmm_ilmm_post_latent_logpdf_grad_seq, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint,
                     Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, pp, Hp, m, σ², gps, C_NULL, val, gy0, gy, gb, gσ, gHp, gg))
            end
            gard = _ard_grads(tags, d)
        end
        f.last_train_cotangents[] = merge(_split_train(gy0, gb, bn, pp, gx0), (H_train=gHp,))
        fill!(gH, 0.0)
    elseif isposterior(f)
        f.train === nothing && error("this posterior does not carry its training data")
        X0, bn, bs, y0 = _merged_train(f.train, p); n0 = size(X0, 2); gy0 = Vector{Float64}(undef, n0 * p); gb = similar(bs)
        gx0 = wantx ? Matrix{Float64}(undef, d, n0) : nothing
        _gps(f.fs) do gps, tags
            if wantx
                GC.@preserve X0 bn bs y0 X yv Hm gps gy0 gy gb gH gg gx0 gx check(ccall((:lmm_ilmm_post_logpdf_grad_seq_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint,
                     Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, p, Hm, m, σ², gps, C_NULL, val, gy0, gy, gb, gσ, gH, gg, gx0, gx))
            else
                GC.@preserve X0 bn bs y0 X yv Hm gps gy0 gy gb gH gg check(ccall((:lmm_ilmm_post_logpdf_grad_seq, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint,
                     Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X0, d, n0, bn, bs, length(bn), y0, X, n, yv, p, Hm, m, σ², gps, C_NULL, val, gy0, gy, gb, gσ, gH, gg))
            end
            gard = _ard_grads(tags, d)
        end
        f.last_train_cotangents[] = _split_train(gy0, gb, bn, p, gx0)
    else
        _gps(f.fs) do gps, tags
            if wantx
                GC.@preserve X yv Hm gps gy gH gg gx check(ccall((:lmm_ilmm_logpdf_grad_x, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble},
                     Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}, Ptr{Cdouble}),
                    X, d, n, yv, p, Hm, m, σ², gps, C_NULL, val, gy, gσ, gH, gg, gx))
            else
                GC.@preserve X yv Hm gps gy gH gg check(ccall((:lmm_ilmm_logpdf_grad, liblmm), Cint,
                    (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Ptr{LmmJitters}, Ref{Cdouble}, Ptr{Cdouble},
                     Ref{Cdouble}, Ptr{Cdouble}, Ptr{LmmGpGrad}),
                    X, d, n, yv, p, Hm, m, σ², gps, C_NULL, val, gy, gσ, gH, gg))
            end
            gard = _ard_grads(tags, d)
        end
    end
    function logpdf_pullback(Δ)
        dx = _motangent(fx.x, gx === nothing ? nothing : Δ .* gx)
        dfx = Tangent{typeof(fx)}(; x=dx, f=Tangent{typeof(fx.f)}(; f=Tangent{typeof(f)}(; fs=_fstangent(f.fs, gg, Δ, gard)), H=Δ .* gH),
                                  Σy=_noise_tangent(fx, Δ * gσ[]))
        return NoTangent(), dfx, Δ .* gy
    end
    return val[], logpdf_pullback
end

# ---- gradients of the predictive marginals w.r.t. the test inputs ---------------------------------------------------------------
# mean_and_var / mean / var of independent latents (OILMM prior or posterior, dense-H prior, IndependentMOGP through U = I, S = NULL):
# lmm_oilmm_mean_and_var_grad_xs returns d/dx* of sum(Δm .* mean) + sum(Δv .* var).  An AbstractZero cotangent goes in as C_NULL, so
# mean's rule takes no triangular solve.  The parameter cotangents of the predictive marginals are not built (@not_implemented).
# marginals(fx) goes through mean_and_var in AbstractGPs, so it needs no rule of its own.
const _MVFinite = Union{ByOutputsFill{HIPOILMM},ByOutputsFill{HIPMOGP},ByFeaturesFill{HIPMOGP},ByOutputsFill{HIPDenseILMM}}
_cot(Δ) = Δ isa AbstractZero ? nothing : Vector{Float64}(unthunk(Δ))
_motangent(x::MOInputIsotopicByFeatures, G) = G === nothing ? NoTangent() : Tangent{typeof(x)}(; x=_xtangent(x.x, G), out_dim=NoTangent())
function _mean_var_grad_xs(f::HIPMOGP, U, S, p, m, X, Δm, Δv)
    d, ns = size(X); G = Matrix{Float64}(undef, d, ns)
    pm = Δm === nothing ? Ptr{Cdouble}(C_NULL) : pointer(Δm); pv = Δv === nothing ? Ptr{Cdouble}(C_NULL) : pointer(Δv)
    _gps(isposterior(f) ? nothing : f.fs) do gps, tags
        GC.@preserve X U S gps Δm Δv G check(ccall((:lmm_oilmm_mean_and_var_grad_xs, liblmm), Cint,
            (Ptr{Cvoid}, Ptr{LmmGp}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble},
             Ptr{Cdouble}, Ptr{Cdouble}),
            f.handle, isposterior(f) ? Ptr{LmmGp}(C_NULL) : pointer(gps), U, _ptr(S), p, m, 0, m, X, d, ns, pm, pv, G))
    end
    return G
end
function _grad_xs(fx::Union{ByOutputsFill{HIPOILMM},ByOutputsFill{HIPDenseILMM}}, Δm, Δv)
    f, H, σ², x = unpack(fx)
    U, S, p, m = _hargs(H)
    return _mean_var_grad_xs(f, U, S, p, m, _xmat(x), Δm, Δv)
end
function _grad_xs(ft::ByOutputsFill{HIPMOGP}, Δm, Δv)
    m = length(ft.f.fs)
    return _mean_var_grad_xs(ft.f, Matrix{Float64}(I, m, m), nothing, m, m, _xmat(ft.x.x), Δm, Δv)
end
function _grad_xs(ft::ByFeaturesFill{HIPMOGP}, Δm, Δv)      # the marginals are permuted by-outputs ones: permute the cotangents back
    n, p = _nx(ft.x), ft.x.out_dim
    return _grad_xs(_by_outputs(ft), Δm === nothing ? nothing : _reorder(Δm, n, p, true),
                    Δv === nothing ? nothing : _reorder(Δv, n, p, true))
end
function _mv_check(fx)
    fx isa ByOutputsFill{HIPDenseILMM} && isposterior(fx.f.f) &&
        error("gradients of the predictive marginals of a dense-H ILMM posterior (coupled latents) are not built")
end
function _mv_tangent(fx, Δm, Δv)
    G = _grad_xs(fx, Δm, Δv)
    return Tangent{typeof(fx)}(; x=_motangent(fx.x, G),
                               f=@not_implemented("parameter gradients of the predictive marginals (kernels, means, H, training data) are not built"),
                               Σy=_noise_tangent(fx, Δv === nothing ? 0.0 : sum(Δv)))
end
function ChainRulesCore.rrule(::typeof(AbstractGPs.mean_and_var), fx::_MVFinite)
    _mv_check(fx)
    MV = mean_and_var(fx)
    function mean_and_var_pullback(Δ)
        Δ = unthunk(Δ)
        Δ isa AbstractZero && return NoTangent(), _mv_tangent(fx, nothing, nothing)
        return NoTangent(), _mv_tangent(fx, _cot(Δ[1]), _cot(Δ[2]))
    end
    return MV, mean_and_var_pullback
end
function ChainRulesCore.rrule(::typeof(AbstractGPs.mean), fx::_MVFinite)
    _mv_check(fx)
    mean_pullback(Δ) = (NoTangent(), _mv_tangent(fx, _cot(Δ), nothing))
    return mean(fx), mean_pullback
end
function ChainRulesCore.rrule(::typeof(AbstractGPs.var), fx::_MVFinite)
    _mv_check(fx)
    var_pullback(Δ) = (NoTangent(), _mv_tangent(fx, nothing, _cot(Δ)))
    return var(fx), var_pullback
end

# ---- modes -------------------------------------------------------------------------------------------------------------
# compute dtype of the per-latent matrices: :f64 (parity mode) | :f32 (BASELINE configs[4])
set_compute_dtype(d::Symbol) = check(ccall((:lmm_set_compute_dtype, liblmm), Cint, (Cint,), d === :f32 ? 1 : 0))
# the region kernel's task hand-out: true (default) = in turn to started workgroups (no reliance on dispatch order), false = task = blockIdx.x
set_strict_progress(on::Bool) = check(ccall((:lmm_set_strict_progress, liblmm), Cint, (Cint,), on ? 1 : 0))
# dtype of the H unprojection of predictive marginals (reference src/oilmm.jl:69-72): :native | :bf16 (BASELINE configs[3]:
# v_mfma_f32_16x16x32_bf16, tolerance 2^-7 Σ_l |H||M_lat|) | :bf16x2 (hi + lo split, <= 2^-15 Σ_l |H||M_lat|, include/lmm_hip.h)
set_projection_dtype(d::Symbol) =
    check(ccall((:lmm_set_projection_dtype, liblmm), Cint, (Cint,), d === :bf16 ? 1 : (d === :bf16x2 ? 2 : 0)))

# get_latent_gp(posterior(fx::FiniteGP{<:ILMM}, y)) for a dense H (reference src/ilmm.jl:39 on the ILMM of :196-197): the coupled
# latent PosteriorGP{IndependentMOGP} as a handle that shares the posterior's device state with H = I_m; the lmm_ilmm_post_*
# entry points then answer for the m latent outputs (jitters {0, σ², 0}: see include/lmm_hip.h).
function latent_view(f::ILMM{<:HIPMOGP,<:Matrix})
    isposterior(f.f) || return f.f
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lmm_ilmm_post_latent_view, liblmm), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), f.f.handle, h))
    # (train and mix ride along for the gradient of the view's logpdf: lmm_ilmm_post_latent_logpdf_grad_seq)
    return ILMM(HIPMOGP(f.f.fs, h[], f.f.train, Matrix{Float64}(f.H)), Matrix{Float64}(I, length(f.f.fs), length(f.f.fs)))
end

# ---- multi-GPU: one Julia process per GPU; the collective lives in the library (RCCL over xGMI) ----------------------------
# rank 0: id = unique_id(); ship the 128 bytes to the other ranks (MPI.bcast!(id, 0, comm)); all: comm_init_rank(id, rank, world).
unique_id() = (id = Vector{UInt8}(undef, 128); check(ccall((:lmm_comm_get_unique_id, liblmm), Cint, (Ptr{UInt8},), id)); id)
comm_init_rank(id::Vector{UInt8}, rank::Integer, world::Integer) =
    check(ccall((:lmm_comm_init_rank, liblmm), Cint, (Ptr{UInt8}, Cint, Cint), id, rank, world))
allreduce_sum!(buf::Vector{Float64}) = (check(ccall((:lmm_allreduce_sum_f64, liblmm), Cint, (Ptr{Cdouble}, Csize_t), buf, length(buf))); buf)
comm_destroy() = check(ccall((:lmm_comm_destroy, liblmm), Cint, ()))

# contiguous block partition of m latents over `world` ranks (the first m % world ranks get one extra)
function latent_shard(m::Integer, rank::Integer, world::Integer)
    base, extra = divrem(m, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (rank < extra ? 1 : 0)
end

# logpdf of an OILMM with the latents sharded over the ranks: each rank evaluates its block (no data-path collective), rank 0
# adds the regulariser, ONE 8-byte all-reduce finishes it (SURVEY.md section 8e)
function sharded_logpdf(fx::ByOutputsFill{HIPOILMM}, y::AbstractVector{<:Real}, rank::Integer, world::Integer)
    fs, H, σ², x = unpack(fx)
    X = _xmat(x); d, n = size(X); U, S, p, m = _hargs(H); yv = Vector{Float64}(y)
    l0, l1 = latent_shard(m, rank, world)
    out = Ref{Cdouble}(0.0)
    _gps(fs.fs) do gps, tags
        GC.@preserve X yv U S gps check(ccall((:lmm_oilmm_logpdf, liblmm), Cint,
            (Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{LmmGp}, Cint, Cint, Cint, Ref{Cdouble}),
            X, d, n, yv, p, U, S, m, σ², gps, l0, l1, rank == 0 ? 1 : 0, out))
    end
    return allreduce_sum!([out[]])[1]
end

end # module
