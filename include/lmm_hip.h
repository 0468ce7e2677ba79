/*
 * lmm_hip.h -- C ABI of liblmm_hip.so: MI355X (gfx950) ILMM / OILMM inference hot path.
 *
 * The reference (LinearMixingModels.jl 0.1.11) has no FFI; its boundary is Julia multiple dispatch
 * on AbstractGPs' generic functions.  Each entry point below is what ONE reference method body
 * becomes after `ccall`; the method it replaces is cited as  file:line  relative to the reference
 * repository.  INTEGRATION.md shows the Julia-side stubs.
 *
 * Conventions (all entry points)
 *   - Float64, column-major, dense, contiguous (Julia `Array` layout).
 *   - x   : d x n input locations (`Vector{Float64}` => d = 1; `ColVecs(X)` => X).
 *   - y   : length n*p "by-outputs" vector == n x p column-major (MOInputIsotopicByOutputs order,
 *           reference src/ilmm.jl:43 `reshape_y`).
 *   - x, y, xs, z, eps and every OUTPUT array may be HOST or DEVICE (HIP) pointers; the library
 *     detects which (hipPointerGetAttributes).  Small model arrays (U, S, H, gps) are host.
 *   - latents are described by lmm_gp_t (ConstMean + variance * kernel(|x-x'| / lengthscale)), or with per-dimension lengthscales
 *     (kernel(|(x-x') ./ l|), l = lengthscale * ard) through an ARD tag in the kind word (lmm_ard_create below).
 *   - `latent_begin, latent_end` select the shard [begin, end) of latent processes this process
 *     (one process per GPU) evaluates; partial results are summed by the caller (RCCL all-reduce
 *     in the Python/Julia host layer).  Use 0, m for the whole model.
 *   - return value: LMM_OK or an lmm_status code; lmm_last_error_string() gives the message,
 *     lmm_last_error_detail() the failing latent and LAPACK-style pivot `info`
 *     (-> Julia `PosDefException(info)`).  Nothing is ever NaN-and-continue.
 *   - calls are blocking; the library never keeps a caller pointer after returning.  Scalar results (log-likelihoods, the
 *     regulariser's residual, pivot info) are written by the kernels straight into a pinned host arena that is mapped into the
 *     device and read after one stream synchronisation (LMM_DIRECT_RESULTS=0 in the environment: device buffers + hipMemcpy).
 *   - reproducibility: by default the last partial scheduling round of a trailing update is split along K and combined with f64
 *     atomics, so results are reproducible to ~1e-13 relative, NOT bitwise; LMM_DETERMINISTIC=1 (environment) disables the split
 *     and makes every result bitwise reproducible (slower tail of the large updates).
 *   - threading: one context per process (= one GPU).  Every entry point takes the context lock, so calls from several
 *     threads are safe but execute one at a time (the context owns ONE set of HIP streams, one device-memory pool and one
 *     pinned staging arena, which concurrent calls would have to share).  Concurrency across GPUs = one process per GPU.
 *   - device pointers produced by another stream (e.g. a PyTorch tensor still being written by torch's stream): call
 *     lmm_stream_wait_caller(that stream) first; the library's streams then order themselves behind it.
 *   - process-global modes: the compute dtype (lmm_set_compute_dtype) and the projection dtype (lmm_set_projection_dtype) are state
 *     of the process's one context, NOT call arguments: they apply to every later call of every thread until changed (a posterior
 *     handle remembers the dtype it was built in and refuses the other one).
 *   - forward progress of the dataflow kernels: potrf_region_kernel runs cooperating workgroups that wait on flags written by other
 *     workgroups of the SAME launch; its deadlock-freedom argument needs "a task waits only for tasks with LOWER indices, which are
 *     running or finished" (one exception: the walker of a matrix waits for the helper of its current row -- a higher index -- only
 *     after it has published everything the lower-indexed helpers need to finish and free their slots).  HIP does not promise that
 *     workgroups start in index order, so by DEFAULT (round 5) a workgroup does not take its task index from blockIdx.x: it takes its
 *     TURN -- a per-matrix counter hands the indices out in order to workgroups that have started; a workgroup whose turn does not
 *     come within 200 us (a lower-indexed workgroup has not started: the device did not dispatch in order) takes the next free index
 *     instead.  The argument then holds in ANY dispatch order, and while the device does dispatch in order every workgroup runs exactly
 *     the task it would have had (values identical; cost 0.1-0.7 % of an evaluation).
 *     lmm_set_strict_progress(0) (LMM_STRICT_PROGRESS=0 at lmm_init) restores the round-4 behaviour: task = blockIdx.x, and the fused
 *     update launches (NODE_FUSE, off by default anyway) allowed -- correct under in-order dispatch, which every AMD GPU to date does.
 *     In both modes every wait is bounded (4 s of the 100-MHz wall clock, or another workgroup's epoch-tagged abort word): should a
 *     launch ever stall, the grid drains and the call returns LMM_ERR_HIP -- no hang, no wrong value.
 */
#ifndef LMM_HIP_H
#define LMM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  LMM_OK = 0,
  LMM_ERR_DIM = 1,             /* "out dim of x != out dim of f."   (reference src/ilmm.jl:52)          */
  LMM_ERR_NOT_ORTHOGONAL = 2,  /* "`U` is not an orthogonal matrix" (reference src/orthogonal_matrix.jl:22) */
  LMM_ERR_NOT_PD = 3,          /* PosDefException from cholesky                                         */
  LMM_ERR_HIP = 4,
  LMM_ERR_ARG = 5,
  LMM_ERR_UNSUPPORTED = 6,
  LMM_ERR_RCCL = 7             /* a collective failed (lmm_last_error_string carries ncclGetErrorString)             */
} lmm_status;

/* kappa(r), r = |x - x'| / lengthscale:  SE v e^{-r^2/2};  Matern32 v (1 + sqrt3 r) e^{-sqrt3 r};  Matern52 v (1 + sqrt5 r + 5 r^2/3)
 * e^{-sqrt5 r};  Matern12 (= KernelFunctions' ExponentialKernel) v e^{-r};  RQ (RationalQuadraticKernel) v (1 + r^2 / (2 alpha))^{-alpha},
 * alpha from the latent's tag (lmm_kernel_tag_create below), 2 without one. */
typedef enum {
  LMM_KERNEL_SE = 0, LMM_KERNEL_MATERN32 = 1, LMM_KERNEL_MATERN52 = 2, LMM_KERNEL_MATERN12 = 3, LMM_KERNEL_RQ = 4
} lmm_kernel_kind;
/* Not a base kind: a sum of up to LMM_SUM_MAX_TERMS base kernels (lmm_kernel_sum_create below); never a term itself. */
#define LMM_KERNEL_SUM 5
#define LMM_SUM_MAX_TERMS 4
/* A base kind outside the enum (code 6 stays refused): KernelFunctions' PeriodicKernel(; r) o ScaleTransform(1 / P) (or ARDTransform),
 *     k(x, x') = v exp( -(1 / (2 rho^2)) sum_k sin^2( pi (x_k - x'_k) / P_k ) ),
 * v = variance; the period P_k = lengthscale (times the tag's ard[k] if it has factors), so `lengthscale` and its gradient slot keep
 * their meaning, "the ScaleTransform"; rho = KernelFunctions' r, one scalar for all dimensions, from the latent's tag
 * (lmm_kernel_tag_create_periodic below), 1 without one.  kappa(0) = v, and the kernel is smooth at coincident points. */
#define LMM_KERNEL_PERIODIC 7
/* A base kind outside the enum (codes 6, 8 and 9 stay refused): the locally periodic kernel, KernelFunctions'
 * (SEKernel o ScaleTransform(1 / l)) * (PeriodicKernel(; r) o ScaleTransform(1 / P)) (or ARDTransform for a vector period),
 *     k(x, x') = v exp( -|x - x'|^2 / (2 l^2) - (1 / (2 rho^2)) sum_k sin^2( pi (x_k - x'_k) / P_k ) ).
 * v, the period P_k (the `lengthscale` slot, times the tag's ard[k]) and rho are those of LMM_KERNEL_PERIODIC; l is the `decay`, one
 * scalar SE lengthscale.  rho and decay come from the latent's tag (lmm_kernel_tag_create_locally_periodic below), 1 and 1 without
 * one.  kappa(0) = v, smooth at coincident points.  It is the one product the library represents: a base kind, so it may be a sum term. */
#define LMM_KERNEL_LOCALLY_PERIODIC 10
/* A base kind outside the enum (codes 6, 8, 9 and 11 stay refused): the stochastically driven damped harmonic oscillator ("SHO", the
 * celerite kernel of Foreman-Mackey et al. 2017), underdamped, over a ONE-dimensional input:
 *     k(tau) = v exp(-a tau) ( cos(eta tau) + (a / eta) sin(eta tau) ),   tau = |x - x'|,
 *     w0 = 2 pi / P,   a = w0 / (2 Q),   eta = w0 sqrt(1 - 1 / (4 Q^2)).
 * v = variance; P = lengthscale, the undamped period (so `lengthscale` and its gradient slot keep their meaning); Q > 1 / 2 is the
 * quality factor, from the latent's tag (lmm_kernel_tag_create_sho below), 1 without one.  kappa(0) = v; paths are once differentiable;
 * the spectrum peaks near 1 / P with a width set by Q.  Q -> 1 / 2 is LMM_KERNEL_MATERN32 with sqrt3 / lengthscale = 2 pi / P; Q <= 1 / 2
 * (critically and overdamped) is not served.  The kernel is exactly the two-dimensional SDE
 *     F = [0 1; -w0^2 -w0 / Q],  Pinf = diag(v, w0^2 v),  A(dt) = exp(-a dt) (cos(eta dt) I + sin(eta dt) / eta (F + a I)),
 * observed in its first component, which the state-space entry points run ("state space" below).  The dense entry points evaluate it
 * as a function of r = tau / P with Q in the descriptor's alpha slot, as RQ its shape:
 *     kappa(r) = v exp(-pi r / Q) ( cos(2 pi h r) + sin(2 pi h r) / (2 h Q) ),   h = sqrt(1 - 1 / (4 Q^2)),
 * one exp and one sincospi per element; they serve it for d = 1 wherever a plain latent is served: logpdf, the posteriors and what is
 * asked of them (marginals, covariances, samples, predictive logpdf), the gradient entry points (variance, period, quality through
 * lmm_kernel_tag_quality_grad, mean, y, sigma2, S, U, H), missing data, OILMM, IndependentMOGP and dense-H, latent shards, the fp32
 * compute mode and lmm_dev_gram.  Refused with LMM_ERR_UNSUPPORTED, naming the latent, before any device work: d > 1 (the radial form
 * is not positive definite there) in every entry point; gradients with respect to the inputs (a non-NULL grad_x / grad_xs, and
 * lmm_oilmm_mean_and_var_grad_xs); the inducing-point entry points (lmm_oilmm_elbo and its kin, lmm_dev_sparse_moments / _grad); and a
 * kind-12 term of lmm_kernel_sum_create.  No entry point evaluates another kernel in its place. */
#define LMM_KERNEL_SHO 12

/* One latent GP: GP(mean, variance * Kernel o ScaleTransform(1/lengthscale)).
 * kind = base | (tag << 8): the low byte is the lmm_kernel_kind; a non-zero tag (lmm_ard_create) gives the latent per-dimension
 * lengthscales (KernelFunctions' Kernel o ARDTransform(1 ./ l)): the effective lengthscale of input dimension k is then
 * lengthscale * ard[k], so `lengthscale` becomes a common multiplier.  A tag may be shared by several latents (tied parameters).
 * A tag may also (or instead) carry the shape alpha of an RQ latent (lmm_kernel_tag_create). */
typedef struct {
  int kind;            /* lmm_kernel_kind | (tag << 8) */
  double variance;
  double lengthscale;
  double mean;         /* ConstMean / ZeroMean */
} lmm_gp_t;
/* Gradient of a scalar with respect to one latent's parameters (the gradient entry points below). */
typedef struct { double variance; double lengthscale; double mean; } lmm_gp_grad_t;

/* The reference's hard-coded numerics constants, passed explicitly so that fp32 callers can
 * widen them (SURVEY.md section 7 "jitter hazards"); pass NULL for the reference values. */
typedef struct {
  double project_jitter;   /* 1e-9  : reference src/ilmm.jl:63                                 */
  double ilmm_rand_jitter; /* 1e-12 : reference src/ilmm.jl:84                                 */
  double default_jitter;   /* 1e-18 : AbstractGPs f(x) default, reference src/oilmm.jl:47,61   */
} lmm_jitters_t;

typedef struct lmm_post lmm_post_t;   /* opaque posterior state (device resident) */

/* ---- per-dimension (ARD) lengthscales -------------------------------------------------------
 * Host-only registry: no device or lmm_init needed, safe from any thread (own mutex, never the context lock).
 *   lmm_ard_create : registers d > 0 positive finite factors ard[0..d-1]; *tag > 0.  At most 4096 live tags
 *                    (LMM_ERR_UNSUPPORTED beyond).  Use kind = base_kind | (tag << 8) in lmm_gp_t.
 *   lmm_ard_destroy: unknown or destroyed tag -> LMM_ERR_ARG.  Posterior handles keep their own copy of the effective
 *                    lengthscales, so destroying a tag never affects a handle built with it.
 *   lmm_ard_grad   : d values d logpdf / d ard[k] = lengthscale * d logpdf / d l_k from the most recent gradient entry point that
 *                    named the tag: summed over that call's latents carrying the tag, partial over its latent shard like grad_gps,
 *                    zeros if its grad_gps was NULL.  (grad_gps[l].lengthscale of such a latent is the derivative with respect to
 *                    the multiplier lengthscale.)
 *   lmm_kernel_tag_create : the general form of lmm_ard_create.  d > 0 with ard != NULL: per-dimension factors as above; d = 0 with
 *                    ard = NULL: none.  alpha > 0 and finite: the shape of an RQ latent; alpha = 0: none.  Anything else, or a tag
 *                    with neither, is LMM_ERR_ARG.  lmm_ard_create(d, ard, tag) == lmm_kernel_tag_create(d, ard, 0, tag).
 *   lmm_kernel_tag_alpha_grad : d logpdf / d alpha from the most recent gradient entry point that named the tag, with the semantics
 *                    of lmm_ard_grad (summed over that call's RQ latents carrying the tag, partial over its shard, 0 if grad_gps
 *                    was NULL).
 *   lmm_kernel_tag_create_periodic : a tag for a periodic latent (LMM_KERNEL_PERIODIC): d, ard as in lmm_kernel_tag_create (d = 0,
 *                    ard = NULL: none); rho finite and > 0, otherwise LMM_ERR_ARG.  Same registry, mutex and 4096 limit; freed by
 *                    lmm_ard_destroy.
 *   lmm_kernel_tag_rho_grad : d logpdf / d rho, with the semantics of lmm_kernel_tag_alpha_grad (the most recent gradient entry
 *                    point that named the tag; summed over that call's latents carrying it, partial over its shard, 0 if grad_gps
 *                    was NULL).  LMM_ERR_ARG on a tag without a rho; lmm_kernel_tag_alpha_grad on a tag with a rho is LMM_ERR_ARG.
 *   lmm_kernel_tag_create_locally_periodic : a tag for a locally periodic latent (LMM_KERNEL_LOCALLY_PERIODIC): d, ard as in
 *                    lmm_kernel_tag_create_periodic (factors of the period); rho and decay finite and > 0, otherwise LMM_ERR_ARG.
 *                    Same registry, mutex and 4096 limit; freed by lmm_ard_destroy.  lmm_kernel_tag_rho_grad serves its rho.
 *   lmm_kernel_tag_decay_grad : d logpdf / d decay, with the semantics of lmm_kernel_tag_rho_grad.  LMM_ERR_ARG on a tag without a
 *                    decay.
 *   lmm_kernel_tag_create_sho : a tag for an SHO latent (LMM_KERNEL_SHO) carrying its quality factor: finite and > 1 / 2, otherwise
 *                    LMM_ERR_ARG.  No factors (the kernel is defined for d = 1).  Same registry, mutex and 4096 limit; freed by
 *                    lmm_ard_destroy.  A kind-12 latent without a tag has quality 1 and reports no quality gradient.
 *   lmm_kernel_tag_quality_grad : d logpdf / d quality, with the semantics of lmm_kernel_tag_alpha_grad (the most recent gradient
 *                    entry point that named the tag: the dense ones and lmm_oilmm_logpdf_grad_statespace).  LMM_ERR_ARG on a tag without a quality;
 *                    lmm_kernel_tag_alpha_grad, _rho_grad and _decay_grad on a tag with a quality are LMM_ERR_ARG.
 *                    A tag with a quality on a latent whose base kind is not LMM_KERNEL_SHO is LMM_ERR_ARG, and so is a tag with
 *                    an alpha, a rho, a decay or factors on a kind-12 latent.
 * Validation in every entry point: the base kind must be 0..4, 7, 10 or (LMM_KERNEL_SHO above, d = 1 only) 12 (LMM_ERR_UNSUPPORTED
 * otherwise) and the tag live (LMM_ERR_ARG
 * otherwise); a tag with an alpha on a latent whose base kind is not LMM_KERNEL_RQ is LMM_ERR_ARG, and so is a tag with a rho (and no
 * decay) on a latent whose base kind is not LMM_KERNEL_PERIODIC, and a tag with a decay on one whose base kind is not
 * LMM_KERNEL_LOCALLY_PERIODIC; a tag with factors must have the
 * call's d (LMM_ERR_DIM, naming the latent).  With d == 1, or when all ard[k] are equal, the latent is folded into the isotropic
 * descriptor (lengthscale * ard[0]) before anything runs: its values are then exactly those of the isotropic latent, and it keeps
 * its alpha or rho.  An RQ latent without a tag, or whose tag has no alpha, uses alpha = 2 (KernelFunctions' default) and reports no alpha
 * gradient.  lmm_ard_destroy frees any tag; lmm_ard_grad on a tag without factors writes nothing.  The 4096-tag limit counts every
 * tag.  Posterior handles keep their own copy of alpha, rho and decay, as of the lengthscales.  The gradient entry points serve d <= 32 for
 * latents with d > 1 factors (LMM_ERR_UNSUPPORTED beyond). */
#define LMM_KERNEL_BASE_MASK 0xff
int lmm_ard_create(int d, const double* lengthscale, int* tag);
int lmm_ard_destroy(int tag);
int lmm_ard_grad(int tag, double* out);
int lmm_kernel_tag_create(int d, const double* ard, double alpha, int* tag);
int lmm_kernel_tag_alpha_grad(int tag, double* out);
int lmm_kernel_tag_create_periodic(int d, const double* ard, double rho, int* tag);
int lmm_kernel_tag_rho_grad(int tag, double* out);
int lmm_kernel_tag_create_locally_periodic(int d, const double* ard, double rho, double decay, int* tag);
int lmm_kernel_tag_decay_grad(int tag, double* out);
int lmm_kernel_tag_create_sho(double quality, int* tag);
int lmm_kernel_tag_quality_grad(int tag, double* out);

/* ---- sum kernels (KernelFunctions' KernelSum) ------------------------------------------------
 * A sum latent has kind = LMM_KERNEL_SUM | (tag << 8) with a tag from lmm_kernel_sum_create, and the kernel
 *     k(x, x') = v0 * sum_c v_c * kappa_{kind_c}( |x - x'|_c / (s0 * l_c) )
 * where v0 and s0 are the latent's own `variance` and `lengthscale` (the ScaledKernel and ScaleTransform around the whole sum) and
 * term c has base kind kind_c, variance v_c and lengthscale l_c.  A term's kind may carry a tag of its own (lmm_kernel_tag_create):
 * its per-dimension lengthscales are then s0 * l_c * ard_c[k], and an RQ term takes its alpha from it and a periodic term (whose l_c is its
 * period) its rho; a locally periodic term its rho and decay, and the outer ScaleTransform acts on both of its factors: its period is
 * s0 * l_c and its decay s0 * decay (d/ds0 collects both).  The latent's `mean` applies to the whole sum.  Sums do not nest; general
 * products and an ARD transform around a whole sum are not represented.
 *   lmm_kernel_sum_create : registers nterms (1..LMM_SUM_MAX_TERMS) terms in the tag registry above (same mutex, no lmm_init needed,
 *                    counted against its 4096-tag limit, freed by lmm_ard_destroy).  Each term: kind = base | (ktag << 8) with base
 *                    0..4, 7 (LMM_KERNEL_PERIODIC) or 10 (LMM_KERNEL_LOCALLY_PERIODIC), variance > 0, lengthscale > 0, mean == 0.  nterms out of range or a bad term value -> LMM_ERR_ARG; a term
 *                    of kind LMM_KERNEL_SUM, 6, 8, 9 or a base kind > 10 -> LMM_ERR_UNSUPPORTED; a term tag that is unknown, is itself a sum
 *                    tag, carries an alpha while the term's base kind is not LMM_KERNEL_RQ, or a rho while it is not
 *                    LMM_KERNEL_PERIODIC, or a decay while it is not LMM_KERNEL_LOCALLY_PERIODIC -> LMM_ERR_ARG.
 *   lmm_kernel_sum_grad : nterms entries (d/dv_c, d/dl_c, 0) from the most recent gradient entry point that named the tag, with the
 *                    semantics of lmm_ard_grad (summed over that call's latents carrying the tag, partial over its shard, zeros if
 *                    grad_gps was NULL).  A term's ARD, alpha, rho and decay gradients are published to the term's own tag (lmm_ard_grad,
 *                    lmm_kernel_tag_alpha_grad, lmm_kernel_tag_rho_grad, lmm_kernel_tag_decay_grad) with s0 * l_c as the multiplier of its factors.  grad_gps[l].variance and
 *                    .lengthscale of a sum latent are d/dv0 and d/ds0.
 * Term tags are looked up when an entry point resolves its latents: a destroyed term tag is LMM_ERR_ARG and a term tag with factors
 * of another d than the call's LMM_ERR_DIM, both naming the latent.  Posterior handles keep their own copy of the resolved terms.
 * Sum latents are served by every entry point that takes gps: OILMM / IndependentMOGP (logpdf, _multi, posteriors, marginals,
 * mean_and_var, rand, cov, cross-covariance and all their gradients, latent shards and the fp32 mode) and dense-H (lmm_ilmm_*, with
 * their gradients; the decoupled shortcut requires equal term lists). */
int lmm_kernel_sum_create(int nterms, const lmm_gp_t* terms, int* tag);
int lmm_kernel_sum_grad(int tag, lmm_gp_grad_t* out);
/* State space: sum latents.  The state-space entry points ("state space" below) serve a latent of kind LMM_KERNEL_SUM | (tag << 8)
 * whose sum has exactly two terms, each a plain Matern12 / 32 / 52 with a scalar lengthscale (no tag) or an SHO (kind 12; its tag, if
 * any, carries its quality), with state dimensions (1 / 2 / 3, SHO 2) adding up to at most 4: Matern12 + Matern12 / Matern32 / SHO /
 * Matern52, Matern32 + Matern32 / SHO, SHO + SHO, in either order of the terms.  The sum's own variance v0 and lengthscale s0 fold
 * into the terms: v = v0 v_c, l = s0 l_c, and an SHO term's period is s0 P.  Every other sum (three or more terms, Matern32 +
 * Matern52 and other state dimensions above 4, another term kind, a term with per-dimension lengthscales) is refused there with
 * LMM_ERR_UNSUPPORTED naming the latent, as before.  The tag comes from either creator:
 *   lmm_kernel_sum_create            : Matern-only sums; the same gps run on every other entry point too.
 *   lmm_kernel_sum_create_statespace : as above, and admits kind-12 terms (with a quality tag of lmm_kernel_tag_create_sho, or none:
 *                    Q = 1).  nterms < 1 or a NULL -> LMM_ERR_ARG; nterms != 2, a term of another kind, a tag on a Matern term, or
 *                    state dimensions adding up to more than 4 -> LMM_ERR_UNSUPPORTED; a bad term value, or an SHO term's tag that is
 *                    not a live quality tag -> LMM_ERR_ARG.  Every entry point that is not a state-space one refuses a latent with such a
 *                    tag with LMM_ERR_UNSUPPORTED naming the latent, before any device work.
 * Per-term gradients come back through lmm_kernel_sum_grad, an SHO term's d/d quality through lmm_kernel_tag_quality_grad on the
 * term's tag, and grad_gps[l].variance / .lengthscale are d/dv0 and d/ds0, as on the dense path.  The gradients with respect to
 * locations (lmm_oilmm_logpdf_grad_statespace_x, lmm_dev_statespace_grad_x, lmm_oilmm_statespace_post_mean_and_var_grad_xs) refuse a
 * sum latent with LMM_ERR_UNSUPPORTED naming it: the second component of its state is not f'. */
int lmm_kernel_sum_create_statespace(int nterms, const lmm_gp_t* terms, int* tag);

/* ---- lifetime -------------------------------------------------------------------------- */
int lmm_init(int device);                 /* bind this process to HIP device `device`, create streams */
int lmm_shutdown(void);
const char* lmm_last_error_string(void);
int lmm_last_error_detail(int* latent, int* info);
int lmm_device_synchronize(void);
int lmm_release_cached_memory(void);      /* return the caching device-memory pool (factor-matrix slots) to HIP */
/* Compute dtype of the per-latent hot path (SURVEY.md section 8b "dtype selected by symbol suffix or enum"; BASELINE configs[4]).
 * LMM_F64 (default): everything Float64 -- the parity mode (rtol 1e-6 against the reference's CPU path).
 * LMM_F32: the MATRICES -- latent Grams, Cholesky factors, inverse diagonal blocks, cross-solve blocks -- are Float32 and the
 *   trailing updates / TRSMs run on v_mfma_f32_32x32x2_f32 (2x the FP64 matrix rate, half the factor memory); vectors at the
 *   boundary (x, y, normals, outputs), the kernel evaluation, the 64x64 diagonal-block factorisation and all reductions stay
 *   Float64.  Served: OILMM / IndependentMOGP logpdf, posterior, marginals, rand, posterior logpdf, sequential conditioning, the
 *   decoupled dense-H logpdf and (round 3) the OILMM / IndependentMOGP logpdf gradients, prior and predictive
 *   (lmm_oilmm_logpdf_grad, lmm_oilmm_post_logpdf_grad: Float32 factor, triangular inverse and K^-1 on v_mfma_f32, every reduction
 *   Float64; tolerance at sigma2 = 0.1, n ~ 10^3: d/dy, d/dU within 1e-4 of their largest component, d/dsigma2 rtol 1e-4, d/dS and
 *   kernel parameters rtol 2e-3 + 1e-2 absolute -- tests/test_gpu_f32.py) and the dense (mn)x(mn) ILMM logpdf (lmm_ilmm_logpdf[_ex],
 *   lmm_ilmm_logpdf_multi: Float32 (mn)x(mn) matrix, rtol 2e-4 on the value) and (round 4) the dense-H POSTERIOR (reference
 *   src/ilmm.jl:184-198: lmm_ilmm_posterior_create, lmm_ilmm_post_condition, _post_mean_and_var, _post_mean_and_cov, _post_logpdf,
 *   _post_rand, the latent view): Float32 (mn)x(mn) factor, cross-solve block and posterior covariance; means in the rider form
 *   mu + R (L^-1 delta); rtol 2e-4 on means, 1e-3 on variances / covariances / logpdf at sigma2 = 0.1), the full covariance of
 *   independent latents (lmm_lmm_mean_and_cov: Float32 latent covariances, Float64 mixing; entries within 5e-5 of the largest) and the
 *   dense-H GRADIENTS (lmm_ilmm_logpdf_grad, lmm_ilmm_post_logpdf_grad: Float32 (mn)x(mn) factor and explicit inverse; value rtol
 *   2e-5, d/dy within 1e-4, d/dy_train and d/dH within 5e-4 of their largest component, d/dsigma2 rtol 1e-4, kernel parameters
 *   rtol 2e-3 + 1e-2 absolute at sigma2 = 0.1, mn ~ 10^3 -- tests/test_gpu_f32.py).  No entry point refuses the fp32 mode any more.
 *   Jitters stay explicit arguments: the reference's 1e-18 / 1e-12 defaults are below Float32 resolution, so prior sampling
 *   needs a caller-chosen jitter (>= ~1e-5 x kernel variance).  A posterior handle remembers the dtype it was built in. */
typedef enum { LMM_F64 = 0, LMM_F32 = 1 } lmm_dtype;
int lmm_set_compute_dtype(int dtype);
int lmm_get_compute_dtype(void);
/* Strict forward progress of the dataflow kernels (conventions above): 1 (default) = task indices handed out in turn to workgroups
 * that have started, 0 = task = blockIdx.x (relies on in-order dispatch).  Process-global like the dtype modes. */
int lmm_set_strict_progress(int on);
int lmm_get_strict_progress(void);

/* Dtype of the H unprojection of predictive marginals,  M = H M_latent,  V = abs2.(H) V_latent .+ sigma2  (reference
 * src/oilmm.jl:69-72; lmm_oilmm_mean_and_var) -- BASELINE configs[3] "bf16 MFMA covariance projection".
 *   LMM_PROJ_NATIVE (default): Float64 FMAs (the parity mode).
 *   LMM_PROJ_BF16: H (or abs2.(H)) and the latent marginals are rounded to bfloat16 (round-to-nearest-even) and multiplied on
 *     v_mfma_f32_16x16x32_bf16 with Float32 accumulation; sigma2 is added in Float64.  STATED TOLERANCE: each operand carries a
 *     relative rounding error <= 2^-8 (bfloat16 keeps 8 significant bits), so |M - M_f64| <= 2^-7 * sum_l |H[o,l]| |M_latent[l,s]| (plus Float32 accumulation,
 *     ~m 2^-24) and likewise for V; the latent marginals themselves (Gram, Cholesky, triangular solves) stay in the compute dtype.
 *   LMM_PROJ_BF16X2: the same pipe with each operand split into two bfloat16 terms (hi + lo), three MFMA products: error <= 2^-15 * sum_l |H||M_lat| (the dropped lo*lo term and the rounding of the lo parts are ~2^-16; Float32 accumulation on top). */
typedef enum { LMM_PROJ_NATIVE = 0, LMM_PROJ_BF16 = 1, LMM_PROJ_BF16X2 = 2 } lmm_proj_dtype;
int lmm_set_projection_dtype(int dtype);
int lmm_get_projection_dtype(void);

/* Order the library's streams behind everything queued so far on `hip_stream` (a hipStream_t; NULL = the legacy default
 * stream): the NEXT entry point may then be handed device pointers that stream is still producing, or output buffers it is
 * still reading.  Entry points are blocking, so no ordering is needed in the other direction. */
int lmm_stream_wait_caller(void* hip_stream);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -----------------------------------------
 * The reference has no parallelism; latents shard over ranks (latent_begin/latent_end above) with NO data-path collective,
 * and ONE sum all-reduce finishes logpdf (8 bytes), marginals (2 p n* doubles) or a sample (n p doubles).
 *   rank 0:  lmm_comm_get_unique_id(id)  -> ship the LMM_UNIQUE_ID_BYTES bytes to the other ranks out of band
 *            (MPI.bcast in Julia, a file, torch.distributed's store, ...)
 *   all   :  lmm_comm_init_rank(id, rank, world)   after lmm_init(device); world == 1 is valid (all-reduce = identity)
 *   all   :  lmm_allreduce_sum_f64(buf, count)     in place; buf host or device; blocking                                  */
#define LMM_UNIQUE_ID_BYTES 128
int lmm_comm_get_unique_id(void* id_out);
int lmm_comm_init_rank(const void* id, int rank, int world);
int lmm_comm_info(int* rank, int* world);              /* world = 0 when no communicator exists */
int lmm_allreduce_sum_f64(double* buf, size_t count);
int lmm_allreduce_max_f64(double* buf, size_t count);  /* e.g. max-over-ranks timing */
int lmm_comm_destroy(void);

/* ---- Orthogonal(U, S) validation: reference src/orthogonal_matrix.jl:21-23 -------------- */
int lmm_orthogonal_validate(const double* U, int p, int m);

/* ---- logpdf ------------------------------------------------------------------------------ */
/* logpdf(fx::FiniteGP{<:OILMM}, y): reference src/oilmm.jl:79-93 (+ project :20-30, regulariser
 * :101-113, per-latent generic logpdf).  *out = sum_{l in shard} lml_l + (with_regulariser ? reg : 0). */
int lmm_oilmm_logpdf(const double* x, int d, int n, const double* y, int p,
                     const double* U, const double* S, int m, double sigma2,
                     const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                     double* out);

/* Value and gradient of logpdf(fx::FiniteGP{<:OILMM}, y) -- what `Zygote.gradient(logpdf, fx, y)` differentiates in the
 * reference's tests (test/oilmm.jl:31-32), to be wrapped in a ChainRulesCore.rrule by the
 * Julia shim.  Gradients w.r.t. y (n*p, by-outputs), sigma2, S (m), U (p x m, treated as an unconstrained matrix as Zygote
 * treats the field) and each latent's (variance, lengthscale, mean).  Any grad pointer may be NULL.  Outputs are partial
 * sums over the latent shard; entries of grad_gps outside the shard are 0. */
int lmm_oilmm_logpdf_grad(const double* x, int d, int n, const double* y, int p,
                          const double* U, const double* S, int m, double sigma2,
                          const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                          double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                          lmm_gp_grad_t* grad_gps);

/* Value and TOTAL gradient of the predictive logpdf  logpdf(posterior(f(x, sigma2), y)(xs, sigma2_s), ys)  of an OILMM or (U = I,
 * S = 1, with_regulariser = 0) an IndependentMOGP: what the reference differentiates with Zygote.gradient(logpdf, po_x, y*) on its
 * posterior models (test/oilmm.jl:32, test/independent_mogp.jl:66), with the derivatives carried through the posterior
 * (alpha, the factor, the Schur complement).  Gradients w.r.t. y (n*p), ys (ns*p), sigma2 (training noise), sigma2_s (predictive
 * noise), S, U and each latent's (variance, lengthscale, mean).  Any grad pointer may be NULL; partial sums over the shard. */
int lmm_oilmm_post_logpdf_grad(const double* x, int d, int n, const double* y, const double* xs, int ns, const double* ys, int p,
                               const double* U, const double* S, int m, double sigma2, double sigma2_s, const lmm_gp_t* gps,
                               int latent_begin, int latent_end, int with_regulariser, double* out_logpdf, double* grad_y,
                               double* grad_ys, double* grad_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                               lmm_gp_grad_t* grad_gps);

/* The same after SEQUENTIAL conditioning, posterior(posterior(f(x1, s1), y1)(x2, s2), y2) ... (reference src/oilmm.jl:116-134
 * applied to its own result; nbatch <= 7 batches, each with its OWN noise variance).  x (d x n) and y (n x p, by outputs over the
 * n points) hold the batches' points in conditioning order, n = sum batch_n; grad_batch_sigma2 receives one derivative per batch.
 * Exact conditioning makes this the posterior given all batches at once under per-batch noise, so value and total derivatives are
 * again joint minus marginal.  lmm_oilmm_post_logpdf_grad is this entry with nbatch = 1. */
int lmm_oilmm_post_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                   const double* y, const double* xs, int ns, const double* ys, int p, const double* U,
                                   const double* S, int m, double sigma2_s, const lmm_gp_t* gps, int latent_begin, int latent_end,
                                   int with_regulariser, double* out_logpdf, double* grad_y, double* grad_ys,
                                   double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                                   lmm_gp_grad_t* grad_gps);

/* Value and gradient of logpdf(fx::FiniteGP{<:ILMM}, y) for a dense H (reference src/ilmm.jl:150-181; Zygote.gradient(logpdf,
 * ilmmx, y) in test/ilmm.jl:31) w.r.t. y, sigma2, H (p x m, column-major) and each latent's (variance, lengthscale, mean).
 * The reference's dense operation plus the explicit (mn) x (mn) inverse; m*n <= 46000.  Does not shard. */
int lmm_ilmm_logpdf_grad(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                         const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y, double* grad_sigma2,
                         double* grad_H, lmm_gp_grad_t* grad_gps);

/* Value and TOTAL derivatives of logpdf(posterior(f(x, sigma2), y)(xs, sigma2_s), ys) for a dense H -- what
 * Zygote.gradient(logpdf, pi, y_test) differentiates in reference test/ilmm.jl:32 (posterior: src/ilmm.jl:184-198): the joint
 * prior density of (y, ys) under two-block observation noise minus the prior density of y (T y is sufficient for the latents, so
 * the reference's projected posterior is the exact conditional).  Gradients w.r.t. y (n*p), ys (ns*p), sigma2 (training noise),
 * sigma2_s (predictive noise), H (p x m) and each latent's (variance, lengthscale, mean); any grad pointer may be NULL.
 * m*(n + ns) <= 46000.  Does not shard. */
int lmm_ilmm_post_logpdf_grad(const double* x, int d, int n, const double* y, const double* xs, int ns, const double* ys, int p,
                              const double* H, int m, double sigma2, double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit,
                              double* out_logpdf, double* grad_y, double* grad_ys, double* grad_sigma2, double* grad_sigma2_s,
                              double* grad_H, lmm_gp_grad_t* grad_gps);

/* The same after sequential conditioning (src/ilmm.jl:184-198 applied to its own result): arguments as in
 * lmm_oilmm_post_logpdf_grad_seq; lmm_ilmm_post_logpdf_grad is this entry with nbatch = 1. */
int lmm_ilmm_post_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                  const double* y, const double* xs, int ns, const double* ys, int p, const double* H, int m,
                                  double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                                  double* grad_ys, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                                  lmm_gp_grad_t* grad_gps);

/* The same for the LATENT view of a dense-H posterior: logpdf(get_latent_gp(posterior(...))(xs, sigma2_s), zs), zs = ns x m by outputs over
 * the m latent processes (reference src/ilmm.jl:39 on the posterior ILMM of :196-197: the coupled PosteriorGP of the IndependentMOGP,
 * whose logpdf Zygote differentiates like any other).  Joint density of the conditioning batches (observed through H) and the latent
 * test block (observed through [I_m; 0], noise sigma2_s I) minus the marginal of the batches.  grad_zs: ns x m; grad_H: through the
 * conditioning batches.  m <= p.  Posteriors conditioned ON latent observations are not served. */
int lmm_ilmm_post_latent_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                         const double* y, const double* xs, int ns, const double* zs, int p, const double* H, int m,
                                         double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf,
                                         double* grad_y, double* grad_zs, double* grad_batch_sigma2, double* grad_sigma2_s,
                                         double* grad_H, lmm_gp_grad_t* grad_gps);

/* Gradients with respect to the INPUT LOCATIONS (what the reference's Zygote.gradient(logpdf, fx, y) carries through fx.x): each _x
 * entry point is the entry point of the same name without the suffix, plus trailing outputs; the entry without it is the _x entry with
 * NULL there.  For every latent, with K its Gram (noise on the diagonal), alpha = K^-1 (T y - mean), w = alpha alpha' - K^-1, its
 * effective per-dimension lengthscales l_k (isotropic: all equal), t_k = (x_ik - x_jk) / l_k and r^2 = sum_k t_k^2,
 *     d logpdf / d x_ik = -(1 / l_k^2) sum_{j != i} w_ij h(r_ij) (x_ik - x_jk),
 *     h(r) = v e^{-r^2/2} (SE), 3 v e^{-sqrt3 r} (Matern32), (5/3) v (1 + sqrt5 r) e^{-sqrt5 r} (Matern52), v e^{-r} / r (Matern12),
 *            v (1 + r^2 / (2 alpha))^{-alpha-1} (RQ);  a periodic latent, not a function of r, contributes
 *     d kappa / d x_ik = -kappa pi sin(2 pi t_k) / (2 rho^2 P_k), t_k = (x_ik - x_jk) / P_k, in place of -h t_k / l_k
 *     (a locally periodic latent: that plus -kappa (x_ik - x_jk) / decay^2),
 * summed over the latents (the noise, the mean, the projection and the regulariser do not depend on x).  Matern12 has a cusp at
 * coincident points: a pair at r = 0 contributes 0 there (the convention of the lengthscale gradient).  Predictive forms: the joint
 * over [x; xs] minus the marginal over x, as for every other derivative there.
 *   grad_x : d x n, column-major (the layout of x); for the _seq forms all batches' points in conditioning order.
 *   grad_xs: d x ns, column-major.
 * OILMM / IndependentMOGP: partial sums over the latent shard, like every other gradient output.  Any output may be NULL (no extra
 * work is done for a NULL output); requesting one with d > 32 returns LMM_ERR_UNSUPPORTED.  fp32 compute mode: K^-1 is Float32, the
 * reduction Float64. */
int lmm_oilmm_logpdf_grad_x(const double* x, int d, int n, const double* y, int p,
                            const double* U, const double* S, int m, double sigma2,
                            const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                            double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                            lmm_gp_grad_t* grad_gps, double* grad_x);
int lmm_oilmm_post_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                     const double* y, const double* xs, int ns, const double* ys, int p, const double* U,
                                     const double* S, int m, double sigma2_s, const lmm_gp_t* gps, int latent_begin, int latent_end,
                                     int with_regulariser, double* out_logpdf, double* grad_y, double* grad_ys,
                                     double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                                     lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs);
int lmm_ilmm_logpdf_grad_x(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                           const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y, double* grad_sigma2,
                           double* grad_H, lmm_gp_grad_t* grad_gps, double* grad_x);
int lmm_ilmm_post_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                    const double* y, const double* xs, int ns, const double* ys, int p, const double* H, int m,
                                    double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                                    double* grad_ys, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                                    lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs);
int lmm_ilmm_post_latent_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                           const double* y, const double* xs, int ns, const double* zs, int p, const double* H, int m,
                                           double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf,
                                           double* grad_y, double* grad_zs, double* grad_batch_sigma2, double* grad_sigma2_s,
                                           double* grad_H, lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs);

/* logpdf(fx, Y::AbstractMatrix): one value per column of Y ((n p) x ncol, column-major) from ONE factorisation per latent
 * (the extra columns ride the factorisation as rider rows).  The reference does not overload this (it falls to AbstractGPs'
 * dense generic path); AbstractGPs.TestUtils calls it.  out: ncol values. */
int lmm_oilmm_logpdf_multi(const double* x, int d, int n, const double* Y, int p, int ncol,
                           const double* U, const double* S, int m, double sigma2,
                           const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                           double* out);

/* MOInputIsotopicByFeatures <-> MOInputIsotopicByOutputs reordering of an n*p vector (reference
 * src/independent_mogp.jl:135-159 reorder_by_outputs / its inverse).  to_outputs != 0: out[o n + i] = in[i p + o]. */
int lmm_reorder(const double* in, int n, int p, int to_outputs, double* out);

/* logpdf(fx::FiniteGP{<:ILMM}, y), dense H (p x m): reference src/ilmm.jl:150-163 (+ project :61-68,
 * regulariser :171-181; cov(::IndependentMOGP) src/independent_mogp.jl:60-63): ONE (mn) x (mn)
 * factorisation.  Does not shard (replicas only). */
int lmm_ilmm_logpdf(const double* x, int d, int n, const double* y, int p,
                    const double* H, int m, double sigma2, const lmm_gp_t* gps,
                    const lmm_jitters_t* jit, double* out);

/* Same, with control over the decoupled shortcut: when every latent has the SAME kernel (kind, variance, lengthscale)
 * the latent covariance I (x) K + SigmaT (x) I block-diagonalises under the m x m eigen-rotation of SigmaT (SURVEY.md
 * section 3.2), and the value is obtained from m independent n x n factorisations instead of one (mn) x (mn).
 * allow_decoupled = 0 forces the reference's dense operation; *path_used (may be NULL) = 1 if the shortcut ran.
 * lmm_ilmm_logpdf == allow_decoupled 1. */
int lmm_ilmm_logpdf_ex(const double* x, int d, int n, const double* y, int p,
                       const double* H, int m, double sigma2, const lmm_gp_t* gps,
                       const lmm_jitters_t* jit, int allow_decoupled, int* path_used, double* out);

/* logpdf(fx::FiniteGP{<:ILMM}, Y::AbstractMatrix), dense H: one value per column of Y ((n p) x ncol, column-major) from ONE
 * (mn) x (mn) factorisation (TestUtils on ilmmx, reference test/ilmm.jl:34-37).  out: ncol values. */
int lmm_ilmm_logpdf_multi(const double* x, int d, int n, const double* Y, int p, int ncol, const double* H, int m, double sigma2,
                          const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out);

/* logpdf(ft::FiniteGP{<:IndependentMOGP,<:MOInputIsotopicByOutputs,<:Diagonal{<:Real,<:Fill}}, y):
 * reference src/independent_mogp.jl:74-80.  y is n x m. */
int lmm_mogp_logpdf(const double* x, int d, int n, const double* y, int m, double sigma2,
                    const lmm_gp_t* gps, int latent_begin, int latent_end, double* out);
/* logpdf(ft::FiniteGP{<:IndependentMOGP,<:MOInputIsotopicByFeatures,<:Diagonal{<:Real}}, y) after the reference's
 * reorder_by_outputs (src/independent_mogp.jl:149-159, 222-229): per-point (heteroscedastic) noise variances
 * noise_diag[i + l*n] (by-outputs order, n x m), y n x m by-outputs. */
int lmm_mogp_logpdf_diag(const double* x, int d, int n, const double* y, int m, const double* noise_diag,
                         const lmm_gp_t* gps, int latent_begin, int latent_end, double* out);

/* ---- posterior ---------------------------------------------------------------------------- */
/* posterior(fx::FiniteGP{<:OILMM}, y): reference src/oilmm.jl:116-134.  Keeps, per latent of the
 * shard, the Cholesky factor C_l, alpha_l = C_l \ delta_l and x on the device. */
int lmm_oilmm_posterior_create(const double* x, int d, int n, const double* y, int p,
                               const double* U, const double* S, int m, double sigma2,
                               const lmm_gp_t* gps, int latent_begin, int latent_end,
                               lmm_post_t** out);
/* posterior(ft::IsotropicByOutputsFiniteIndependentMOGP, y): reference src/independent_mogp.jl:119-126. */
int lmm_mogp_posterior_create(const double* x, int d, int n, const double* y, int m, double sigma2,
                              const lmm_gp_t* gps, int latent_begin, int latent_end, lmm_post_t** out);
/* posterior(po(x2, sigma2), y2): condition a posterior OILMM / IndependentMOGP (U = I, S = 1) on further observations
 * (AbstractGPs.TestUtils exercises `posterior` on `po`: reference test/oilmm.jl:34-37, test/independent_mogp.jl:68-76).
 * Returns a NEW handle (the old one stays valid). */
int lmm_post_condition(const lmm_post_t* post, const double* U, const double* S, int p, int m, double sigma2,
                       const double* x2, int d, int n2, const double* y2, lmm_post_t** out);
/* posterior(fx::FiniteGP{<:ILMM}, y), dense H: reference src/ilmm.jl:184-198. */
int lmm_ilmm_posterior_create(const double* x, int d, int n, const double* y, int p,
                              const double* H, int m, double sigma2, const lmm_gp_t* gps,
                              const lmm_jitters_t* jit, lmm_post_t** out);
int lmm_post_destroy(lmm_post_t* post);
/* get_latent_gp(posterior(fx::FiniteGP{<:ILMM}, y)) for a dense H: reference src/ilmm.jl:39 applied to the ILMM of :196-197 -- the
 * latent PosteriorGP{IndependentMOGP}.  Returns a handle that SHARES the device state of `post` and has H = I_m (p = m): the
 * lmm_ilmm_post_* entry points below then answer mean / var / cov / logpdf / rand / posterior for the m latent outputs at
 * MOInputIsotopicByOutputs(xs, m).  Pass jitters {0, sigma2, 0}: with project_jitter = 0 the projection is the identity and the
 * regulariser vanishes (logpdf = the generic Gaussian of the latent posterior + sigma2 I); rand with ilmm_rand_jitter = sigma2 and
 * add_noise = 0 is AbstractGPs' mean + chol(cov + sigma2 I).U' z.  Either handle may be destroyed first. */
int lmm_ilmm_post_latent_view(const lmm_post_t* post, lmm_post_t** out);
/* logpdf(pi(xs, sigma2), ys) on the dense-H posterior ILMM: reference test/ilmm.jl:25 (src/ilmm.jl:150-163 applied to the
 * PosteriorGP latent of :196-197).  One (m ns) x (m ns) factorisation. */
int lmm_ilmm_post_logpdf(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns, const double* ys,
                         const lmm_jitters_t* jit, double* out);
/* rand(rng, pi(xs, sigma2)) on the dense-H posterior ILMM: reference src/ilmm.jl:78-87.  z_lat: m*ns normals (by latents),
 * eps: ns*p normals (by outputs), in the reference's draw order. */
int lmm_ilmm_post_rand(const lmm_post_t* post, double sigma2, int add_noise, const double* xs, int d, int ns,
                       const double* z_lat, const double* eps, const lmm_jitters_t* jit, double* out);
/* mean_and_var / marginals of the dense-H posterior ILMM at xs: reference src/ilmm.jl:108-129,142-145 applied to the
 * PosteriorGP latent of src/ilmm.jl:196-197.  Outputs length ns*p, by-outputs; sigma2 included. */
int lmm_ilmm_post_mean_and_var(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns,
                               const lmm_jitters_t* jit, double* mean_out, double* var_out);
/* mean_and_cov / cov of the dense-H posterior ILMM at xs: reference src/ilmm.jl:132-147 on the PosteriorGP latent
 * (AbstractGPs.TestUtils secondary interface on `pi`, test/ilmm.jl:34-37).  cov_out is (p ns) x (p ns) column-major,
 * by-outputs order, sigma2 on the diagonal; small ns only ((p ns)^2 <= 4e8). */
int lmm_ilmm_post_mean_and_cov(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns,
                               const lmm_jitters_t* jit, double* mean_out, double* cov_out);
/* posterior(pi(x2, sigma2), y2): condition the dense-H posterior ILMM on further observations (reference src/ilmm.jl:184-198
 * applied to the PosteriorGP latent; TestUtils on `pi`, test/ilmm.jl:34-37).  Returns a NEW handle (the old one stays
 * valid); the two batches may carry different sigma2. */
int lmm_ilmm_post_condition(const lmm_post_t* post, double sigma2, const double* x2, int d, int n2, const double* y2,
                            const lmm_jitters_t* jit, lmm_post_t** out);

/* Latent marginals of the (prior if post == NULL, else posterior) latent processes of the shard at xs:
 * mean_lat, var_lat are (m_shard x ns) row-per-latent, i.e. ns x m_shard column-major.  No jitter, no
 * mixing.  AbstractGPs PosteriorGP mean/var reached from reference
 * src/oilmm.jl:61 and src/independent_mogp.jl:50,55. */
int lmm_latent_marginals(const lmm_post_t* post, const lmm_gp_t* gps, int m_shard,
                         const double* xs, int d, int ns, double* mean_lat, double* var_lat);

/* mean_and_var(fx::FiniteGP{<:OILMM}) => marginals / mean / var: reference src/oilmm.jl:57-76.
 * H = U sqrt(S) (pass S == NULL to give a dense H in U: the diagonal-covariance mixing of an ILMM whose
 * latents are independent).  Outputs are the shard's PARTIAL sums over its latents, length ns*p,
 * by-outputs; sigma2 (+ default jitter per latent) is added iff add_noise != 0.
 * post == NULL => prior latents `gps` (m_shard of them, starting at latent_begin).
 * var_out == NULL => means only (AbstractGPs.mean(fx), src/ilmm.jl:142): mu + K(x*, x) alpha per latent, no triangular solve. */
int lmm_oilmm_mean_and_var(const lmm_post_t* post, const lmm_gp_t* gps,
                           const double* U, const double* S, int p, int m,
                           int latent_begin, int latent_end, double sigma2, int add_noise,
                           const double* xs, int d, int ns, const lmm_jitters_t* jit,
                           double* mean_out, double* var_out);

/* d/d xs of  sum(dmean .* mean) + sum(dvar .* var)  for the outputs of lmm_oilmm_mean_and_var (same post / gps / U / S / shard
 * conventions; sigma2, add_noise and jitters are constants here).  dmean, dvar: ns*p by-outputs, either may be NULL (zero
 * cotangent; dvar == NULL takes no triangular solve).  grad_xs: d x ns, the layout of xs.  Host or device pointers.  Partial sum
 * over the shard.  post == NULL (prior): zeros.  d <= 32.  Dense-H posterior handles and the fp32 compute mode: LMM_ERR_UNSUPPORTED.
 * Per latent l, with mbar_l = H' dmean, vbar_l = (H .* H)' dvar, alpha_l = K_l^-1 delta_l and W_l = K_l(xs, x) K_l^-1:
 *     grad_xs[:, s] = sum_l sum_i (mbar_l[s] alpha_li - 2 vbar_l[s] W_l[s, i]) d kappa_l(xs_s, x_i) / d xs_s
 * (DESIGN.md 4.11).  W_l = R_l L_l^-1 from the forward path's R_l = K_l(xs, x) L_l^-T by a right solve; Matern12 pairs at coincident
 * points contribute 0.  IndependentMOGP posteriors use this entry point with U = I_m, S = NULL and p = m. */
int lmm_oilmm_mean_and_var_grad_xs(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                                   int latent_begin, int latent_end, const double* xs, int d, int ns,
                                   const double* dmean, const double* dvar, double* grad_xs);

/* mean_and_cov(fx) / cov(fx): reference src/ilmm.jl:132-139,147 (+ src/independent_mogp.jl:60-63 through H = I) for
 * independent latents (OILMM prior or posterior, dense-H prior with S == NULL):
 *   C[(o,i),(o',j)] = sum_l H[o,l] H[o',l] (Cov_l[i,j] + jitter [i==j]) + sigma2 [o==o', i==j],
 * (p ns) x (p ns) column-major, by-outputs ordering.  Same numbers as the reference's Xt_A_X(cholesky(latent_cov), H_full')
 * + sigma2 I without its Cholesky of a 1e-18-jittered covariance.  Partial sums over the shard as in lmm_oilmm_mean_and_var. */
int lmm_lmm_mean_and_cov(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                         int latent_begin, int latent_end, double sigma2, int add_noise,
                         const double* xs, int d, int ns, const lmm_jitters_t* jit,
                         double* mean_out, double* cov_out);

/* cov(f::IndependentMOGP, x, y) -- the two-input cross-covariance: reference src/independent_mogp.jl:66-71 (x, y both
 * MOInputIsotopicByOutputs: Matrix(BlockDiagonal(cov(f_l, x.x, y.x)))) and :184-215 (either input MOInputIsotopicByFeatures: the same
 * blocks with rows / columns permuted by indices_which_reorder_outputs_to_features); tested by the reference at
 * test/independent_mogp.jl:136-141.  post == NULL: prior latents `gps` (block l = kernelmatrix(k_l, x, y)); post != NULL (a handle
 * of lmm_mogp_posterior_create / lmm_oilmm_posterior_create / lmm_post_condition): PosteriorGP latents, block l =
 * K_l(x, y) - A_x' A_y with A_z = C_l.U' \ K_l(x_train, z).  x is d x n, y is d x n2.  cov_out: (m n) x (m n2) column-major; entry
 * ((l, i), (l', j)) sits at row  l n + i  (x by outputs)  or  i m + l  (x_by_features != 0), column  l' n2 + j  or  j m + l'.  Only the
 * blocks of the shard [latent_begin, latent_end) are filled, everything else is zero (shards sum to the whole).  (m n)(m n2) <= 4e8. */
int lmm_mogp_cross_cov(const lmm_post_t* post, const lmm_gp_t* gps, int m, int latent_begin, int latent_end,
                       const double* x, int d, int n, int x_by_features, const double* y, int n2, int y_by_features,
                       double* cov_out);

/* logpdf(po(xs, sigma2), ys) where po is the posterior OILMM (reference test/oilmm.jl:25; the posterior
 * is again an OILMM with the same H, reference src/oilmm.jl:133): per-latent posterior covariance at
 * xs (Schur complement) + the reference src/oilmm.jl:79-93 algorithm. */
int lmm_oilmm_post_logpdf(const lmm_post_t* post, const double* U, const double* S, int p, int m,
                          double sigma2, const double* xs, int d, int ns, const double* ys,
                          int with_regulariser, double* out);

/* ---- missing observations (NaN in y) ----------------------------------------------------------
 * The reference's notebook (examples/oilmm_and_ilmm.ipynb) says: "Heterotopic and missing data (semi-heterotopic) are not supported
 * yet ... using the missing data techniques identified in the paper".  These entry points are that technique, the diagonal approximation of Bruinsma et al.
 * 2020 (the OILMM paper) for missing data.  An entry of y is missing iff it is NaN (+-Inf is data).  With H = U sqrt(S) and, for point
 * t, O_t its observed outputs, p_t = |O_t|, H_t = H[O_t, :], G_t = H_t' H_t (m x m):
 *     z_t = G_t^-1 H_t' y_t[O_t];   latent l sees the pseudo-observation z_t[l] at x_t with noise variance sigma2 (G_t^-1)_ll;
 *     r_t = -1/2 [(p_t - m) log(2 pi sigma2) + log det G_t + |y_t[O_t] - H_t z_t|^2 / sigma2];
 *     logpdf = sum_l log N(z_{.,l}; mean_l, K_l + diag_t(sigma2 (G_t^-1)_ll)) + sum_t r_t      (with_regulariser switches sum_t r_t).
 * N(y_t | H_t x, sigma2 I) = N(z_t | x, sigma2 G_t^-1) exp(r_t) is exact; the one approximation is dropping the off-diagonal of
 * G_t^-1, so the value is exact whenever every G_t is diagonal.  Without NaN, G_t = S and every formula is that of lmm_oilmm_logpdf
 * (reference src/oilmm.jl:20-30, 101-113), evaluated by other arithmetic (agreement to rounding, not bitwise).
 * Points with equal O_t share one pattern: a device kernel writes one ceil(p / 64)-word mask per point, only those words reach the
 * host (y may be a device pointer and is never downloaded), and the m x m work is done once per pattern.
 * Refusals: a point with p_t < m (p_t = 0 included: drop such points before the call) -> LMM_ERR_UNSUPPORTED; a G_t that is not
 * positive definite although p_t >= m -> LMM_ERR_NOT_PD; both report the 0-based index of the first such point in
 * lmm_last_error_detail's `info` (latent = -1).  m > 128 -> LMM_ERR_UNSUPPORTED.  This stage is Float64 in both compute dtypes.
 * Not served with NaN: lmm_post_condition, the predictive logpdf (NaN ys), matrix Y (_multi), dense-H ILMM, IndependentMOGP, rand.
 *   lmm_missing_patterns : host-only (no lmm_init): groups the n points of y_host (n x p) by their mask, numbering the patterns by
 *                    first appearance: pattern_of_point[t] (n ints), *npatterns, *n_observed = sum_t p_t; any output may be NULL.
 *                    Gives the p_t < m refusal above.
 *   lmm_oilmm_project_missing : the front end alone: z_out[t + l n] = z_t[l] - means[l] (means NULL: 0), noise_out[t + l n] =
 *                    sigma2 (G_t^-1)_ll (both n x m, host or device, may be NULL), *reg_out = sum_t r_t, *npatterns_out.
 *                    y, z_out and noise_out may be host or device pointers; U, S and means are host arrays (as everywhere).
 *   All four device entry points return LMM_ERR_ARG for an S[l] that is not finite and > 0.
 *   lmm_oilmm_logpdf_missing, lmm_oilmm_posterior_create_missing : the arguments and shard semantics of lmm_oilmm_logpdf and
 *                    lmm_oilmm_posterior_create; the handle is an ordinary one (every prediction entry point, and sequential
 *                    conditioning on complete further data, work on it).
 *   lmm_oilmm_logpdf_grad_missing : value and gradients with respect to the observed entries of y (grad_y: n*p, exactly 0 at the
 *                    missing entries), sigma2 and each latent's parameters (tags, sums, ARD, alpha, rho and decay exactly as in
 *                    lmm_oilmm_logpdf_grad).  It has NO grad_S, grad_U or grad_x arguments: derivatives through the per-point
 *                    projection with respect to the mixing matrix and the inputs are not built.  Any grad pointer may be NULL. */
int lmm_missing_patterns(const double* y_host, int n, int p, int m, int* pattern_of_point, int* npatterns, int* n_observed);
int lmm_oilmm_project_missing(const double* y, int n, int p, const double* U, const double* S, int m, double sigma2,
                              const double* means, double* z_out, double* noise_out, double* reg_out, int* npatterns_out);
int lmm_oilmm_logpdf_missing(const double* x, int d, int n, const double* y, int p,
                             const double* U, const double* S, int m, double sigma2,
                             const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                             double* out);
int lmm_oilmm_posterior_create_missing(const double* x, int d, int n, const double* y, int p,
                                       const double* U, const double* S, int m, double sigma2,
                                       const lmm_gp_t* gps, int latent_begin, int latent_end,
                                       lmm_post_t** out);
int lmm_oilmm_logpdf_grad_missing(const double* x, int d, int n, const double* y, int p,
                                  const double* U, const double* S, int m, double sigma2,
                                  const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                  double* out_logpdf, double* grad_y, double* grad_sigma2, lmm_gp_grad_t* grad_gps);

/* ---- inducing points (VFE) --------------------------------------------------------------------
 * Titsias' collapsed bound on the independent latents of an OILMM, as AbstractGPs states it for VFE(f(z, jitter))
 * (src/sparse_approximations.jl): linear cost in n.  z: d x nz inducing inputs shared by all latents (host or device), nz <= 1024
 * (LMM_ERR_UNSUPPORTED beyond, before any launch), d <= 32, jitter > 0 is added to the diagonal of K_uu.  Per latent l of the shard,
 * with r = (T y)_l - mean_l and w = sigma2 / S_l (the projection of reference src/oilmm.jl:20-30):
 *     Phi = sum_t k_u(x_t) k_u(x_t)' / w,  b = sum_t k_u(x_t) r_t / w,  s = sum_t r_t^2 / w,  kappa = sum_t k(x_t, x_t) / w,
 *     lambda = sum_t log w_t (= n log w here),  L_u = chol(K_uu + jitter I),  B = I + L_u^-1 Phi L_u^-T,  L_B = chol(B),  c = L_B^-1 L_u^-1 b,
 *     dtc_l = -(n log 2pi + lambda + log det B + s - c'c) / 2,   elbo_l = dtc_l - (kappa - tr(L_u^-1 Phi L_u^-T)) / 2.
 * Only Phi, b, s, kappa, lambda touch the n points: one pass that generates K_uf tiles on the fly and never stores K_uf
 * (DESIGN.md 4.16); no atomics, so these moments are bitwise reproducible whatever LMM_DETERMINISTIC says (the two M x M
 * factorisations follow the library's rule: split-K atomics only in large trailing updates).  Float64 only: the fp32
 * compute mode is refused (LMM_ERR_UNSUPPORTED).  A failed pivot of K_uu + jitter I or of B is LMM_ERR_NOT_PD with the latent and the
 * pivot in lmm_last_error_detail.  Not built: NaN in y, dense H, gradients of dtc.
 *   lmm_oilmm_elbo : elbo(VFE(f(z, jitter)), fx, y) and dtc(VFE(f(z, jitter)), fx, y) of AbstractGPs for fx::FiniteGP{<:OILMM}.
 *                    Arguments as lmm_oilmm_logpdf; *elbo = sum_{l in shard} elbo_l + (with_regulariser ? the regulariser of
 *                    reference src/oilmm.jl:101-113 : 0), *dtc likewise; either output may be NULL.
 *   lmm_oilmm_sparse_posterior_create : posterior(VFE(f(z, jitter)), fx, y) of AbstractGPs (ApproxPosteriorGP), per latent of the
 *                    shard: the handle keeps z, L_u, L_B and c.
 *   lmm_sparse_post_destroy : releases such a handle.
 *   lmm_oilmm_sparse_mean_and_var : mean_and_var(fx) (reference src/oilmm.jl:57-76) on the posterior OILMM whose latents are those
 *                    ApproxPosteriorGPs: with a = L_u^-1 k_u(x*), latent mean = mean_l + a' L_B^-T c and latent variance
 *                    k** - |a|^2 + |L_B^-1 a|^2, mixed through H = U sqrt(S) and sigma2 exactly as lmm_oilmm_mean_and_var does;
 *                    output layout as there (partial sums over the handle's shard; var may be NULL).  gps is not read (the handle
 *                    keeps its latents) and may be NULL.
 *   lmm_dev_sparse_moments : building block exported for tests (DEVICE pointers x, z, w, r, Phi, b, scalars; gp on the host): one
 *                    latent's Phi (nz x nz column-major, ld >= nz; only the lower triangle is written), b (nz) and scalars = (s,
 *                    kappa, lambda) for per-point noise w (n) and data r (n).  chunk: points per partial sum (0: the library's
 *                    default); partials are added in chunk order, so equal arguments give bitwise equal results.
 *   lmm_oilmm_elbo_grad : value and gradient of the bound of lmm_oilmm_elbo: *out_elbo is bitwise that call's *elbo;
 *                    grad_y (n x p, the layout of y), grad_sigma2, grad_S (m), grad_U (p x m), grad_gps (m; per-dimension lengthscales,
 *                    alpha, rho, decay and sum terms through the tag registry) exactly as lmm_oilmm_logpdf_grad returns them, and
 *                    grad_z (d x nz, the layout of z).  Any output may be NULL; grad_y and grad_z may be host or device pointers.
 *                    Partial sums over the shard.  A second pass over the n points forms G = PhiBar K_uf on the FP64 MFMA from K_uf
 *                    tiles generated on the fly and contracts (2 G + beta r') / w with the kernel derivatives; no atomics.  Refusals
 *                    are those of lmm_oilmm_elbo.  There is no gradient of dtc.
 *   lmm_dev_sparse_grad : building block exported for tests (DEVICE pointers x, z, w, r, PhiBar, beta and outputs; gp on the host):
 *                    that second pass for one latent with per-point noise w, a symmetric PhiBar (nz x nz column-major, ld >= nz,
 *                    both triangles read) and beta (nz).  term_records: LMM_SUM_MAX_TERMS records of 10 + d raw sums over (i, t) of
 *                    g_it d k_c(z_i, x_t) -- [0] d / d (the term's lengthscale multiplier), [7] sum g k_c, [8] d / d alpha (RQ) or rho
 *                    (periodic kinds), [9] d / d decay, [10 + k] d / d (the term's k-th per-dimension lengthscale); zeros elsewhere
 *                    and in the records of terms the latent does not have.  grad_z (d x nz, may be NULL): sum_t g_it d k / d z_i.
 *                    grad_r (n, may be NULL): (beta' k_u(x_t) - r_t) / w_t.  chunk as in lmm_dev_sparse_moments; equal arguments give
 *                    bitwise equal results. */
typedef struct lmm_sparse_post lmm_sparse_post_t;
int lmm_oilmm_elbo(const double* x, int d, int n, const double* y, int p,
                   const double* U, const double* S, int m, double sigma2,
                   const lmm_gp_t* gps, int latent_begin, int latent_end,
                   const double* z, int nz, double jitter, int with_regulariser, double* elbo, double* dtc);
int lmm_oilmm_sparse_posterior_create(const double* x, int d, int n, const double* y, int p,
                                      const double* U, const double* S, int m, double sigma2,
                                      const lmm_gp_t* gps, int latent_begin, int latent_end,
                                      const double* z, int nz, double jitter, lmm_sparse_post_t** out);
int lmm_sparse_post_destroy(lmm_sparse_post_t* post);
int lmm_oilmm_sparse_mean_and_var(const lmm_sparse_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                                  double sigma2, int add_noise, const double* xs, int d, int ns, double* mean, double* var);
int lmm_dev_sparse_moments(const double* x, int d, int n, const double* z, int nz, const lmm_gp_t* gp, const double* w,
                           const double* r, int chunk, double* Phi, int ld, double* b, double* scalars);
int lmm_oilmm_elbo_grad(const double* x, int d, int n, const double* y, int p,
                        const double* U, const double* S, int m, double sigma2,
                        const lmm_gp_t* gps, int latent_begin, int latent_end,
                        const double* z, int nz, double jitter, int with_regulariser, double* out_elbo, double* grad_y,
                        double* grad_sigma2, double* grad_S, double* grad_U, lmm_gp_grad_t* grad_gps, double* grad_z);
int lmm_dev_sparse_grad(const double* x, int d, int n, const double* z, int nz, const lmm_gp_t* gp, const double* w,
                        const double* r, const double* PhiBar, int ld, const double* beta, int chunk, double* term_records,
                        double* grad_z, double* grad_r);

/* ---- state space (Matern latents over a one-dimensional input) --------------------------------------
 * Matern12, Matern32 and Matern52 over a one-dimensional input are exactly a 1-, 2- or 3-dimensional linear SDE, so once the OILMM
 * projection has decoupled the latents a Kalman filter gives the value of lmm_oilmm_logpdf and a Rauch-Tung-Striebel smoother the
 * posterior marginals, both in O(n) and without approximation (the OILMM paper names state-space methods next to
 * inducing points as the two ways to linear cost).  Both recursions run as parallel scans over the points (Sarkka & Garcia-Fernandez,
 * "Temporal parallelization of Bayesian smoothers"): each thread folds `chunk` consecutive points, the aggregates are scanned, each
 * thread restarts the ordinary recursion from its prefix.  No atomics: results depend only on (arguments, chunk) and are bitwise
 * reproducible.  x: n inputs (d = 1 is part of the signature), NON-DECREASING (equal points are legal); anything else is LMM_ERR_ARG
 * with the index of the first x[t] that is not >= x[t - 1] in lmm_last_error_detail's `info` (the Python mirror sorts).
 * Per latent l, with lam = 1 / l, sqrt(3) / l or sqrt(5) / l: the state is (f, f', f''), F the companion matrix of (s + lam)^D,
 * A(dt) = exp(-lam dt) (I + N dt + N^2 dt^2 / 2) with N = F + lam I, Q(dt) = Pinf - A Pinf A', prior N(0, Pinf); the observation is the
 * first component plus N(0, w_t).
 * An SHO latent (LMM_KERNEL_SHO, above; its tag carries the quality Q, 1 without one) is the two-dimensional SDE of a damped
 * oscillator: state (f, f'), a = w0 / (2 Q), eta = w0 sqrt(1 - 1 / (4 Q^2)), N = F + a I with N^2 = -eta^2 I, A(dt) = exp(-a dt)
 * (cos(eta dt) I + sin(eta dt) / eta N), Pinf = diag(v, w0^2 v), Q(dt) and the observation as above; everything downstream of A(dt) is
 * the text the Matern latents run.  Matern and SHO latents mix freely in one call, in any order: launches group latents by MODEL
 * (Matern32 and SHO share D = 2 but not a launch).  Its z takes 2 n doubles per sample, like a Matern32 latent's.  grad_gps[l] of an
 * SHO latent holds d/d variance, d/d period (the `lengthscale` slot) and d/d mean; d/d quality goes to the latent's tag
 * (lmm_kernel_tag_quality_grad), seeded as a third parameter of the forward-mode pass.
 * Data: y as for lmm_oilmm_logpdf, NaN = missing.  The front end is that of the missing-data entry points (the diagonal approximation,
 * exact without NaN and whenever every G_t is diagonal; m <= 128): per point the pseudo-observation z_t[l] - mean_l with noise variance
 * sigma2 (G_t^-1)_ll, and the same regulariser.  Additionally a point with NO observed output is kept, as a predict-only step that
 * contributes no term: that is how marginals at new inputs are asked for (merge them into x with all-NaN rows of y).
 * Refusals, all before any kernel of the scan is launched: a latent that is not a plain Matern12 / 32 / 52 or an SHO latent (SE, RQ,
 * the periodic kinds, sums, Matern latents with a tag) -> LMM_ERR_UNSUPPORTED with the latent in the error detail; the fp32 compute mode ->
 * LMM_ERR_UNSUPPORTED; a point with 0 < p_t < m -> LMM_ERR_UNSUPPORTED with the point in `info`; S not finite and > 0, sigma2 <= 0 ->
 * LMM_ERR_ARG.  Not built: gradients with respect to x, gradients of the marginals, sums of Matern terms.
 *   lmm_oilmm_logpdf_statespace : the value of lmm_oilmm_logpdf (no NaN) or lmm_oilmm_logpdf_missing (NaN) by the filter: agreement
 *                    to rounding, not bitwise.  Shard semantics and with_regulariser as there.
 *   lmm_oilmm_mean_and_var_statespace : the smoothed latent marginals at the n inputs, mixed through H = U sqrt(S) exactly as
 *                    lmm_oilmm_mean_and_var mixes (+ sigma2 when add_noise): mean_and_var(posterior(fx, y)(x, sigma2)) at the
 *                    training inputs.  mean, var: n x p in the layout of y, host or device; var may be NULL.  Partial sums over the
 *                    shard.  The filtered states it keeps are D + D (D + 1) / 2 doubles per point and latent; latents run in groups
 *                    that keep them within 1 GiB.
 *   lmm_dev_statespace_filter, lmm_dev_statespace_smooth : building blocks exported for tests (DEVICE pointers x, w, r and outputs; gp
 *                    on the host, its mean is not read): one latent with per-point noise w (n; +Inf = unobserved) and data r (n).
 *                    fmean, fvar: the filtered first-component mean and variance (the predicted ones at an unobserved point);
 *                    *lml: sum_t -1/2 (log 2 pi S_t + e_t^2 / S_t) over the observed points; smean, svar: the smoothed ones.
 *                    chunk: points per thread (0: the library's plan, a function of n alone); chunk >= n is one sequential thread.
 *   lmm_oilmm_logpdf_grad_statespace : value and gradient of lmm_oilmm_logpdf_statespace in O(n), with respect to y (grad_y: n x p in
 *                    the layout of y, host or device; exactly 0 at NaN entries and in the rows of points without observations), sigma2,
 *                    S (m), U (p x m, column-major) and every latent's (variance, lengthscale, mean) (grad_gps: m records, zeros
 *                    outside the shard).  Any output may be NULL.  *out_logpdf is bitwise the value of lmm_oilmm_logpdf_statespace.
 *                    Per latent, with C = K + diag(w) over the observed points: d/d r_t = -alpha_t, alpha = C^-1 r, and d/d w_t =
 *                    (alpha_t^2 - (C^-1)_tt) / 2, both read off the smoothed marginals (alpha_t = (r_t - mu_t) / w_t, (C^-1)_tt =
 *                    (w_t - P_t) / w_t^2); d/d variance and d/d lengthscale by forward-mode differentiation of the filter scan (the same
 *                    fold, scan and filter on (value, tangent) pairs, one launch serving both parameters).  No atomics: the result
 *                    depends on the arguments only.  y, sigma2, S and U follow by the chain rule of lmm_oilmm_logpdf_grad (complete
 *                    data) or lmm_oilmm_logpdf_grad_missing (NaN in y, all-NaN points included: then grad_S or grad_U non-NULL is
 *                    LMM_ERR_UNSUPPORTED).  Every refusal of lmm_oilmm_logpdf_statespace applies, in its order.  Partial sums over
 *                    the shard; with_regulariser as there.
 *   lmm_dev_statespace_grad : the building block beside lmm_dev_statespace_filter (DEVICE pointers throughout): *lml as there (bitwise),
 *                    grad_r and grad_w (n each; 0 at unobserved points), grad_theta = {d lml / d variance, d lml / d lengthscale}.
 *   lmm_dev_statespace_grad_sho : the same block with grad_theta = {d lml / d variance, d lml / d lengthscale, d lml / d quality} (3
 *                    values; the third is 0 for a Matern latent): lmm_dev_statespace_grad keeps its two-value output, which cannot
 *                    carry an SHO latent's quality.
 *   lmm_dev_statespace_grad_sum : the same block for a sum latent ("State space: sum latents" above; a plain latent is served too):
 *                    grad_theta holds 6 values, the seeds of the sum's first term in the library's order of the terms (Matern12,
 *                    Matern32, SHO, Matern52; two terms of one kind keep the caller's order), then those of its second: d lml / d V_c, d lml / d E_c and, for an SHO term,
 *                    d lml / d quality, with V_c = v0 v_c and E_c = s0 l_c the term's own variance and lengthscale (period); the
 *                    slots behind the last seed are 0.  lmm_dev_statespace_grad and lmm_dev_statespace_grad_sho refuse a sum latent with
 *                    LMM_ERR_UNSUPPORTED naming it (latent 0): their two or three values cannot carry its seeds.
 *   lmm_oilmm_logpdf_grad_statespace_x : lmm_oilmm_logpdf_grad_statespace with one more output, grad_x (n values in the order of the
 *                    sorted x, host or device; may be NULL): d logpdf / d x_t, in O(n).  The value depends on x through the spacings
 *                    dt_t = x_t - x_{t-1} alone, and spacing t through the predicted state (mp, Pp) of point t alone: with the
 *                    smoothed state (ms, Ps) of point t, delta = ms - mp and F the drift of the latent's SDE (dA / dt = F A),
 *                      g_t = (Pp^-1 delta)' F mp + tr(Pp^-1 (delta delta' + Ps - Pp) Pp^-1 F (Pp - Pinf)),   g_0 = g_n = 0,
 *                    is d lml_l / d dt_t, and d lml_l / d x_t = g_t - g_{t+1}.  The smoother evaluates g_t when it steps from point t
 *                    to point t - 1 (nothing is stored but the n values per latent); the latents are added in their order, no
 *                    atomics.  grad_x is exactly 0 at a point without any observation.  Every other output is bitwise that of
 *                    lmm_oilmm_logpdf_grad_statespace, whose refusals apply in their order; NaN in y is served (x does not enter
 *                    the projection, so unlike grad_S and grad_U nothing is refused).  Partial sums over the shard.
 *   lmm_dev_statespace_grad_x : the building block beside lmm_dev_statespace_grad (DEVICE pointers throughout; gp on the host, its mean
 *                    not read; a Matern or an SHO latent, whose tag carries its quality): grad_x (n) = d lml / d x_t of one latent
 *                    with noise w (+Inf: unobserved, where grad_x is exactly 0) and data r.  chunk as for lmm_dev_statespace_filter.
 *   lmm_oilmm_rand_statespace : rand in O(n), exact: joint samples of the prior (y == NULL) or of the posterior given y, at the n inputs,
 *                    from caller-supplied standard normals.  The prior path of a latent is the recursion s_0 = chol(Pinf) zeta_0,
 *                    s_t = A(dt_t) s_{t-1} + chol(Q(dt_t)) zeta_t, f_t = (s_t)_1 (chol: the lower factor with non-negative diagonal;
 *                    a pivot that is not > 0 gives a zero column, so equal points repeat the state), run as a scan over affine maps.
 *                    A posterior path is mean_l + f + the smoothed mean of the data r_t - f_t - sqrt(w_t) xi_t (pathwise conditioning,
 *                    Matheron's rule), through the filter and smoother above: an exact joint sample at observed and unobserved points
 *                    alike.  With y given every rule of lmm_oilmm_mean_and_var_statespace holds (NaN = missing; a point whose outputs
 *                    are all NaN is predict-only, which is how samples at new inputs are asked for; 0 < p_t < m is refused); with
 *                    y == NULL there is no front end and xi is not read.  Layouts, points in the order of x, every buffer host or
 *                    device: z per sample the latents 0 .. m - 1 one after the other, latent l taking D_l n doubles with component i
 *                    of point t at i n + t (one sample: n sum_l D_l doubles; a shard reads only its own); xi [sample][m][n] (posterior
 *                    only; ignored where a point is unobserved); eps and out [sample][p][n], the layout of lmm_lmm_rand_multi.  out =
 *                    H (latent paths) + sqrt(sigma2) eps (iff add_noise), H = U sqrt(S): the partial sum over the shard's latents.
 *                    Every refusal of lmm_oilmm_logpdf_statespace applies, in its order; then nsamples < 1, z == NULL, xi == NULL
 *                    with y given and eps == NULL with add_noise are LMM_ERR_ARG.  Bitwise reproducible, and sample q of an
 *                    nsamples-call is bitwise the single-sample call with the same normals.  As a function of FIXED normals the path
 *                    is ill-conditioned where dt / lengthscale is small (Q's small pivots come out of a cancellation); its law is not
 *                    (DESIGN.md 4.18 "Sampling").
 *   lmm_dev_statespace_sample, lmm_dev_statespace_sample_posterior : building blocks exported for tests (DEVICE pointers; gp on the
 *                    host, its mean is not read; chunk as for lmm_dev_statespace_filter): f [sample][n], the zero-mean latent path of
 *                    one latent from z [sample][D n] (and, posterior, w, r and xi [sample][n]).  With z = xi = 0 the posterior block
 *                    returns bitwise the smean of lmm_dev_statespace_smooth at the same chunk. */
int lmm_oilmm_logpdf_statespace(const double* x, int n, const double* y, int p,
                                const double* U, const double* S, int m, double sigma2,
                                const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser, double* out);
int lmm_oilmm_mean_and_var_statespace(const double* x, int n, const double* y, int p,
                                      const double* U, const double* S, int m, double sigma2,
                                      const lmm_gp_t* gps, int latent_begin, int latent_end, int add_noise,
                                      double* mean, double* var);
int lmm_dev_statespace_filter(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                              double* fmean, double* fvar, double* lml);
int lmm_dev_statespace_smooth(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                              double* smean, double* svar);
int lmm_oilmm_logpdf_grad_statespace(const double* x, int n, const double* y, int p,
                                     const double* U, const double* S, int m, double sigma2,
                                     const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                     double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                                     lmm_gp_grad_t* grad_gps);
int lmm_dev_statespace_grad(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                            double* lml, double* grad_r, double* grad_w, double* grad_theta);
int lmm_dev_statespace_grad_sho(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                                double* lml, double* grad_r, double* grad_w, double* grad_theta);
int lmm_dev_statespace_grad_sum(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                                double* lml, double* grad_r, double* grad_w, double* grad_theta);
int lmm_oilmm_logpdf_grad_statespace_x(const double* x, int n, const double* y, int p,
                                       const double* U, const double* S, int m, double sigma2,
                                       const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                       double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                                       lmm_gp_grad_t* grad_gps, double* grad_x);
int lmm_dev_statespace_grad_x(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                              double* grad_x);
int lmm_oilmm_rand_statespace(const double* x, int n, const double* y /* NULL: prior sample */, int p,
                              const double* U, const double* S, int m, double sigma2,
                              const lmm_gp_t* gps, int latent_begin, int latent_end, int add_noise, int nsamples,
                              const double* z, const double* xi /* posterior only */, const double* eps /* iff add_noise */,
                              double* out);
int lmm_dev_statespace_sample(const double* x, int n, const lmm_gp_t* gp, const double* z, int nsamples, int chunk, double* f);
int lmm_dev_statespace_sample_posterior(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r,
                                        const double* z, const double* xi, int nsamples, int chunk, double* f);

/* ---- state space: the posterior object ---------------------------------------------------------------
 * What posterior(fx, y) followed by mean_and_var(post(x*, sigma2)) is on the dense path (lmm_oilmm_posterior_create, then
 * lmm_oilmm_mean_and_var), in O(n) once and O(log n) per query and latent (DESIGN.md 4.18 "Posterior object").  One conditioning pass
 * (the front end, the filter and the smoother of lmm_oilmm_mean_and_var_statespace) keeps the filtered states (m^f_t, P^f_t) and the
 * FULL smoothed states (m^s_t, P^s_t) of every latent of the shard.  By the Markov property the posterior at a new input s needs the
 * filtered state of the training point just before it and the smoothed state of the one just after it, and nothing else: with
 * k = #{t : x_t <= s} (a query equal to a training input comes behind every copy of it),
 *   predict  (m, P) = (A(d1) m^f_{k-1}, A(d1) P^f_{k-1} A(d1)' + Q(d1)), d1 = s - x_{k-1}; k = 0: (0, Pinf);
 *   smooth   k < n, d2 = x_k - s, A = A(d2): E = P A' (A P A' + Q(d2))^-1, m <- E m^s_k + (m - E A m), P <- E P^s_k E' + (P - E A P);
 *            k = n (a forecast behind the last point): the prediction is the answer;
 * and the latent marginal is (m[0] + mean_l, P[0][0]).  One thread per (query, latent) finds k by binary search over the sorted x;
 * queries come in any order and a query's result depends on no other query (bitwise).
 *   lmm_oilmm_statespace_posterior_create : conditions on (x, y).  Arguments, data rules (NaN = missing) and every refusal of
 *                    lmm_oilmm_logpdf_statespace, in its order.  *out_logpdf (may be NULL) is bitwise the value of
 *                    lmm_oilmm_logpdf_statespace with the regulariser (the filter runs anyway).  The handle owns, on the device, the
 *                    sorted x, the states and H = U sqrt(S) of the shard, and on the host the latents' descriptors and means and sigma2
 *                    (they travel as kernel arguments) and copies of U and S (lmm_oilmm_statespace_post_append projects with them): 2 (D_l + D_l (D_l + 1) / 2) n doubles per latent l of the shard (2 n, 10 n, 18 n
 *                    for Matern12, Matern32 and SHO, Matern52) + n doubles for x + p (l1 - l0) for H.  States are stored
 *                    point-major, [latent][n][component] (a query reads one or two lines per state; measured against
 *                    component-major in DESIGN.md 4.18), the D means first and then the upper triangle of the covariance by rows;
 *                    while it is built, the filter's own component-major states of one launch's latents exist beside them.  A failed
 *                    allocation returns LMM_ERR_HIP, frees what the handle held and sets *out to NULL.
 *   lmm_statespace_post_destroy : frees the handle; NULL is accepted.
 *   lmm_oilmm_statespace_post_mean_and_var : mean_and_var(post(xs, sigma2)): the latent marginals at xs (ns values in any order, host or
 *                    device) mixed through H exactly as lmm_oilmm_mean_and_var_statespace mixes (+ sigma2 when add_noise).  mean, var:
 *                    ns x p by outputs, host or device; var may be NULL.  Partial sums over the handle's shard.  post, xs or mean NULL
 *                    or ns < 1 -> LMM_ERR_ARG; a NaN or +-Inf in xs -> LMM_ERR_ARG with the first such index in lmm_last_error_detail's
 *                    `info`, before the search runs; the fp32 compute mode -> LMM_ERR_UNSUPPORTED.
 *   lmm_oilmm_statespace_post_mean_and_var_grad_xs : the pullback of lmm_oilmm_statespace_post_mean_and_var to the queries: grad_xs[q]
 *                    (ns values, host or device) = d / d xs_q of sum(dmean * mean) + sum(dvar * var) for cotangents dmean, dvar (ns x p
 *                    by outputs, host or device; either may be NULL, both NULL -> LMM_ERR_ARG).  A Matern32, Matern52 or SHO latent
 *                    carries f' as its second state component, so d mean_l / d s = m[1] and d var_l / d s = 2 P[0][1] of the state
 *                    the query computes anyway; Matern12 differentiates its predict-then-smooth step in closed form (at a query
 *                    equal to a training input its mean has a kink: the derivative is that of the side the search sorts the query
 *                    to, behind every copy).  grad_xs[q] = sum_l (sum_o dmean[o, q] H[o, l]) d mean_l + (sum_o dvar[o, q] H[o, l]^2)
 *                    d var_l, latents in order; a query's entry depends on no other query (bitwise).  The added sigma2 does not
 *                    depend on xs.  post, xs or grad_xs NULL or ns < 1 -> LMM_ERR_ARG; xs checked as there.
 *   lmm_dev_statespace_states, lmm_dev_statespace_interp : building blocks exported for tests (DEVICE pointers; one latent, gp on the
 *                    host, its mean is not read; chunk as for lmm_dev_statespace_filter).  states: fstate, sstate, each
 *                    n x (D + D (D + 1) / 2) in the layout above, from per-point noise w and data r.  interp: mean, var (ns each), the
 *                    zero-mean latent marginals at xs from given states in that layout.  lmm_dev_statespace_interp_layout: the same
 *                    with point_major == 0 reading states stored (D + D (D + 1) / 2) x n, component-major, instead (the layout
 *                    experiment of DESIGN.md 4.18; point_major != 0 is lmm_dev_statespace_interp). */
typedef struct lmm_ss_post lmm_ss_post_t;
int lmm_oilmm_statespace_posterior_create(const double* x, int n, const double* y, int p,
                                          const double* U, const double* S, int m, double sigma2,
                                          const lmm_gp_t* gps, int latent_begin, int latent_end,
                                          lmm_ss_post_t** out, double* out_logpdf);
int lmm_statespace_post_destroy(lmm_ss_post_t* post);
int lmm_oilmm_statespace_post_mean_and_var(const lmm_ss_post_t* post, const double* xs, int ns, int add_noise,
                                           double* mean, double* var);
int lmm_oilmm_statespace_post_mean_and_var_grad_xs(const lmm_ss_post_t* post, const double* xs, int ns,
                                                   const double* dmean, const double* dvar, double* grad_xs);
int lmm_dev_statespace_states(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk,
                              double* fstate, double* sstate);
int lmm_dev_statespace_interp(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate,
                              const double* xs, int ns, double* mean, double* var);
int lmm_dev_statespace_interp_layout(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate,
                                     int point_major, const double* xs, int ns, double* mean, double* var);

/* ---- state space: sampling from the posterior object ------------------------------------------------
 * Joint samples of post(xs, sigma2) from the handle, without touching the data again (DESIGN.md 4.18 "Sampling from the posterior
 * object"): what lmm_oilmm_rand_statespace with y draws at new inputs, in O(ns + training points between the smallest and the largest
 * query) per latent and sample.  Given the data the states are a Markov chain that runs backwards, s_j | s_{j+1}, y = N(g_j + E_j
 * s_{j+1}, L_j) with (E_j, g_j, L_j) the smoother's element of the FILTERED state of point j, so a path is an affine scan from the right
 * over the WINDOW of the sorted queries q_0 <= ... <= q_{ns-1}: the queries and the training points first .. first + count - 1, first =
 * #{t : x_t <= q_0}, count = #{t : x_t <= q_{ns-1}} - first, ordered by input (a training point before an equal query, equal queries in
 * their order); W = ns + count.  The last window point is q_{ns-1} and starts the chain at its posterior state (the state
 * lmm_oilmm_statespace_post_mean_and_var reads its marginal from).  Factors are upper triangular (the highest derivative is eliminated
 * first), which keeps the law exact where queries lie 1e-12 lengthscales from a training input.  No atomics: results are bitwise
 * reproducible, and sample q of a call is bitwise the one-sample call on its normals.
 *   lmm_statespace_post_window : *first and *count for q_0 = lo and q_{ns-1} = hi (host scalars), so that a caller can size z.  lo > hi,
 *                    a NaN or +-Inf, or a NULL pointer -> LMM_ERR_ARG.
 *   lmm_oilmm_statespace_post_rand : nsamples joint samples at xs (ns values, NON-DECREASING and finite, host or device; otherwise
 *                    LMM_ERR_ARG with the first offending index in lmm_last_error_detail's `info`).  z: per sample, for each latent l
 *                    of the handle's shard in order, D_l W standard normals, component-major over window positions (component i of
 *                    window point j at i W + j).  eps: per sample ns p standard normals by outputs, read only when add_noise (and then
 *                    required).  out: per sample ns x p by outputs, H f + sqrt(sigma2) eps, mixed exactly as lmm_oilmm_rand_statespace
 *                    mixes; partial sums over the handle's shard.  z, eps, out: host or device.  post, xs, z or out NULL, ns < 1 or
 *                    nsamples < 1 -> LMM_ERR_ARG; the fp32 compute mode -> LMM_ERR_UNSUPPORTED ("Float64 only").
 *   lmm_dev_statespace_post_sample : building block exported for tests (DEVICE pointers; one latent, gp on the host, its mean is not
 *                    read): the zero-mean paths f ([sample][ns], in the order of the sorted xs) from given states in the layout of
 *                    lmm_dev_statespace_states and z ([sample][D W]); chunk: window points per thread, 0 = the library's default. */
int lmm_statespace_post_window(const lmm_ss_post_t* post, double lo, double hi, int* first, int* count);
int lmm_oilmm_statespace_post_rand(const lmm_ss_post_t* post, const double* xs, int ns, const double* z, const double* eps,
                                   int nsamples, int add_noise, double* out);
int lmm_dev_statespace_post_sample(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate,
                                   const double* xs, int ns, const double* z, int nsamples, int chunk, double* f);

/* ---- state space: appending observations --------------------------------------------------------------
 * Conditioning a live handle on LATER observations without starting over (DESIGN.md 4.18 "Appending observations").  The filtered state
 * of the last training point is a sufficient statistic for everything in front of it, so k new points at or behind the last input cost
 * one front end and one filter over those k points, started from that state: O(k), whatever n is.  The RTS recursion consumes filtered
 * states and inputs only, never the data, so the smoothed states are rebuilt from the handle alone, in O(n), when they are needed.
 * LAZINESS.  An append leaves the smoothed states behind (smoothed_n < n).  A query reads a smoothed state only when it lies in FRONT
 * of the last input, so lmm_oilmm_statespace_post_mean_and_var, ..._grad_xs and ..._post_rand first decide on the device whether any of
 * their queries does (one small kernel, a 4-byte download) and run the O(n) pass only then; lmm_statespace_post_window does when lo
 * does.  A batch of pure forecasts (every query >= the last input; a query equal to it is a forecast) never triggers the pass, and
 * its results are bitwise those of the same call after lmm_statespace_post_smooth.  The query entry points keep their const handle.
 * CAPACITY.  The handle's buffers (x, and the filtered and smoothed states of every latent of the shard) have room for cap >= n points;
 * a latent's block is cap x (D_l + D_l (D_l + 1) / 2), so the memory of lmm_oilmm_statespace_posterior_create reads with cap for n.
 * Create leaves cap = n (its memory is what it was).  An append that needs more grows to max(2 cap, n + k) with one device-to-device
 * copy of the filled rows; lmm_statespace_post_reserve grows once to a known size.  Results do not depend on cap (bitwise).
 *   lmm_oilmm_statespace_post_append : x_new: k values, finite and non-decreasing, host or device, with x_new[0] >= the handle's last
 *                    input (ties are served: a spacing of 0 is exact).  y_new: k x p by outputs (y_new[o k + t]), host or device, NaN =
 *                    missing, with create's rules.  Projects the k points (create's front end, with the U, S and sigma2 the handle
 *                    keeps), filters them from the stored last state and appends x and the filtered states: n += k, smoothed_n stays.
 *                    *out_increment (may be NULL) = log p(y_new | all earlier data) with the regulariser terms of the new points, so
 *                    that create's *out_logpdf plus the increments is the log density of all the data.  Refusals, all before the handle
 *                    is touched (after a failed call it answers exactly as before): post NULL or k < 0 -> LMM_ERR_ARG; the fp32 compute
 *                    mode -> LMM_ERR_UNSUPPORTED; a NaN or +-Inf in x_new, or x_new[t] < x_new[t - 1] -> LMM_ERR_ARG with the index in
 *                    lmm_last_error_detail's `info`; x_new[0] in front of the last input -> LMM_ERR_ARG, `info` = 0 (appended points lie
 *                    at or behind the last input); a point observing 0 < p_t < m outputs -> LMM_ERR_UNSUPPORTED naming it by its index
 *                    in the handle's numbering, n + t (`info`); n + k > INT_MAX -> LMM_ERR_ARG.  k = 0 is LMM_OK and changes nothing.
 *   lmm_statespace_post_smooth : runs the smoother over all n kept filtered states when smoothed_n < n (then smoothed_n = n); else nothing.
 *   lmm_statespace_post_reserve : cap = n_total when that is larger than cap; else nothing.
 *   lmm_statespace_post_size : *n, *smoothed_n, *cap (each may be NULL).
 *   lmm_dev_statespace_filter_from : building block exported for tests beside lmm_dev_statespace_filter (DEVICE pointers; one latent, gp
 *                    on the host, its mean is not read): the filter over the k points (x, w, r) whose predecessor is the packed state
 *                    state0 (D + D (D + 1) / 2 values in the handle's layout) at the input x0 <= x[0] (a host scalar).  *lml = log p(r |
 *                    state0), fmean, fvar (k each) the filtered first-component marginals, fstate (k x (D + D (D + 1) / 2),
 *                    point-major) the filtered states.  chunk: points per thread, 0 = the library's default; one chunk (k <= chunk)
 *                    is a single launch that runs the sequential filter. */
int lmm_oilmm_statespace_post_append(lmm_ss_post_t* post, const double* x_new, int k, const double* y_new, double* out_increment);
int lmm_statespace_post_smooth(lmm_ss_post_t* post);
int lmm_statespace_post_reserve(lmm_ss_post_t* post, int n_total);
int lmm_statespace_post_size(const lmm_ss_post_t* post, int* n, int* smoothed_n, int* cap);
int lmm_dev_statespace_filter_from(const double* state0, double x0, const double* x, int k, const lmm_gp_t* gp, const double* w,
                                   const double* r, int chunk, double* fmean, double* fvar, double* fstate, double* lml);

/* ---- state space: predictive log density -----------------------------------------------------------------
 * logpdf(post(xs, sigma2), ys): the joint log density of held-out observations given the training data, from the handle alone
 * (DESIGN.md 4.18 "Predictive log density from the posterior object").  Given the data the states over the window of the sorted queries
 * ("sampling from the posterior object" above: the same window, the same backward chain s_j | s_{j+1}, y = N(g_j + E_j s_{j+1}, L_j))
 * are Markov, so observing ys at the queries is a Kalman filter over the window with affine transitions, run from the largest query
 * down to the smallest; its marginal likelihood is log p(ys | y) per latent, exactly.  Cost O(ns + count) per latent; a held-out
 * block behind the data touches no training point.  Training points inside the window are unobserved steps.  No atomics: the value
 * depends only on the handle and the queries, bitwise.  The handle is const and answers exactly as before after any call, refused or
 * not.  Served by the C ABI and the Python mirror (StateSpacePosterior.predictive_logpdf); the Julia shim has no state-space posterior
 * yet, hence no method there.
 *   lmm_oilmm_statespace_post_logpdf : xs: ns values, finite and NON-DECREASING, host or device (otherwise LMM_ERR_ARG with the first
 *                    offending index in lmm_last_error_detail's `info`); ties among the queries and with training inputs are served.
 *                    ys: ns x p by outputs (ys[o ns + t]), host or device, NaN = missing, with create's rules: a row without any
 *                    observed output is an unobserved query and contributes 0; a row observing 0 < p_t < m outputs ->
 *                    LMM_ERR_UNSUPPORTED naming the query by its index t (`info`); a singular G_t -> LMM_ERR_NOT_PD.  sigma2: the noise
 *                    at the queries, finite and > 0; exactly 0 means the handle's own; anything else -> LMM_ERR_ARG.  *out = the sum
 *                    over the shard's latents of the window filter's value plus the regulariser terms of the queries, i.e. what
 *                    lmm_oilmm_logpdf_statespace gives on all n + ns points minus what it gives on the n training points, and for
 *                    queries at or behind the last input what lmm_oilmm_statespace_post_append would return.  LAZINESS as for the
 *                    other query entry points: the O(n) pass runs only when a query lies in front of the last input.  ns = 0 ->
 *                    *out = 0.  post or out NULL, ns < 0, or xs or ys NULL with ns > 0 -> LMM_ERR_ARG; the fp32 compute mode ->
 *                    LMM_ERR_UNSUPPORTED ("Float64 only").
 *   lmm_dev_statespace_post_logpdf : building block exported for tests beside lmm_dev_statespace_post_sample (DEVICE pointers; one
 *                    latent, gp on the host, its mean is not read): *out (device) = the window filter's value from given states in the
 *                    layout of lmm_dev_statespace_states, with noise w and data r of the ns sorted queries (w = +Inf: unobserved).
 *                    chunk: window points per thread, 0 = the library's default; one chunk (W <= chunk) is a single launch that runs
 *                    the sequential filter. */
int lmm_oilmm_statespace_post_logpdf(const lmm_ss_post_t* post, const double* xs, int ns, const double* ys, double sigma2, double* out);
int lmm_dev_statespace_post_logpdf(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate,
                                   const double* xs, int ns, const double* w, const double* r, int chunk, double* out);

/* ---- rand ----------------------------------------------------------------------------------- */
/* rand(rng, fx::FiniteGP{<:OILMM}): reference src/oilmm.jl:40-54.  The caller supplies the standard
 * normals in the reference's draw order: z_lat = m blocks of ns (latent order), eps = ns*p (by-outputs),
 * so a Julia shim passing randn(rng, ...) reproduces the reference sample-for-sample.
 * H = U sqrt(S), or dense H in U with S == NULL and latent jitter `ilmm_rand_jitter`
 * (rand(rng, fx::FiniteGP{<:ILMM}): reference src/ilmm.jl:78-87 + src/independent_mogp.jl:83-86).
 * post == NULL => prior latents.  Output: PARTIAL sum over the shard's latents (length ns*p); the
 * noise term sqrt(sigma2)*eps is added iff add_noise != 0. */
int lmm_lmm_rand(const lmm_post_t* post, const lmm_gp_t* gps,
                 const double* U, const double* S, int p, int m,
                 int latent_begin, int latent_end, double sigma2, int add_noise,
                 const double* xs, int d, int ns, const double* z_lat, const double* eps,
                 const lmm_jitters_t* jit, double* out);

/* rand(rng, fx, N): N samples from ONE factorisation per latent (the reference repeats the whole call N times,
 * src/ilmm.jl:90-92, src/independent_mogp.jl:92-96).  z_lat: [sample][m][ns], eps / out: [sample][p][ns]; per sample the
 * draw order is the reference's (m blocks of ns latent normals, then ns*p noise normals). */
int lmm_lmm_rand_multi(const lmm_post_t* post, const lmm_gp_t* gps,
                       const double* U, const double* S, int p, int m,
                       int latent_begin, int latent_end, double sigma2, int add_noise,
                       const double* xs, int d, int ns, int nsamples, const double* z_lat, const double* eps,
                       const lmm_jitters_t* jit, double* out);

/* ---- building blocks exported for tests / profiling (device pointers only) ------------------ */
/* In-place lower Cholesky of the leading ncols columns of an nrows x ncols column-major matrix (ld),
 * rows >= ncols ride along (become A21 * L11^-T).  nrows, ncols multiples of 64.  Winv: ncols/64 dense
 * 64x64 inverse diagonal blocks (scratch / output).  info: device int (0 = ok, k = pivot k failed). */
int lmm_dev_potrf(double* A, int nrows, int ncols, int ld, double* Winv, int n_real, int* info_dev);
/* The back substitution behind every dense gradient and posterior, on its own: z_j <- L_j^-T z_j (64 nblk values each) for the nb <= 32
 * matrices of a batch, from the factors and inverse diagonal blocks lmm_dev_potrf leaves.  Matrix j is at L + j l_stride, its inverse
 * blocks at W + j w_stride, its vector at z + j z_stride (strides in Float64 elements; l_stride = w_stride = 0 lets all the solves
 * share one factor).  Words of z from 64 nblk on are not touched. */
int lmm_dev_backsolve(const double* L, size_t l_stride, int ld, const double* W, size_t w_stride, int nblk,
                      double* z, size_t z_stride, int nb);
/* The inverse behind every dense gradient, on its own, for a batch of nb <= 32 factored NC x NC matrices (ld; matrix j at
 * A + j a_stride, inverse blocks at W + j w_stride): R_j (NC columns of ld, at R + j r_stride) becomes L_j^-T -- upper triangular, its
 * strict lower triangle exactly 0 -- and the lower triangle of A_j, diagonal included, becomes (L_j L_j')^-1. */
int lmm_dev_factor_inverse(double* A, size_t a_stride, int ld, int NC, const double* W, size_t w_stride,
                           double* R, size_t r_stride, int nb);
/* Host-only (no GPU needed): the status the library derives from `count` pivot-info words of a batch -- LMM_OK; LMM_ERR_NOT_PD for
 * the first non-zero word (lmm_last_error_detail: latent_begin + index, pivot; reference: `cholesky` throwing PosDefException inside
 * src/oilmm.jl:90 / AbstractGPs logpdf); LMM_ERR_HIP when ANY word carries -7777, the marker potrf_region_kernel leaves when one of
 * its bounded dependency waits timed out (never expected; results are then undefined and must not be read as a PosDefException). */
int lmm_dev_check_info(const int* info, int count, int latent_begin);
/* Test hook of the allocation-extent guard (lmm_api.hip guard_extent: every Gram / triangular-solve / Schur-complement / factorisation
 * launch site checks the rows x cols (ld) block it touches against the pooled allocation the pointer lies in and returns LMM_ERR_ARG
 * instead of launching): applies it to a fresh pooled block of alloc_bytes, a block of Float64 elements. */
int lmm_dev_extent_check(size_t alloc_bytes, size_t rows, size_t ld, size_t cols);
/* Test hook of the region kernel's row-task plan (host arithmetic only, no device needed): for a block column of P 128-column panels of
 * nb matrices with rows_below rows under the square (rows_real of them holding data) on a device of `cus` CUs, with `assistants`
 * assistant workgroups available per matrix: out[0] = row tiles that stay 128 rows high, out[1] = row tasks per matrix (128-row tiles
 * + 64-row tiles), out[2] = assistants used.  The tiles cover the rows: 128 out[0] + 64 (out[1] - out[0]) >= rows_below. */
int lmm_dev_region_plan(int P, int nb, int rows_below, int rows_real, int cus, int assistants, int out[3]);
/* Test hook of the dataflow kernels' dependency flags: they carry a 26-bit launch epoch and are never reset; when the epoch wraps,
 * every persistent flag word is cleared.  *old_epoch (may be NULL) = the current epoch; set_to >= 0 replaces it (-1: read only). */
int lmm_dev_flag_epoch(int set_to, int* old_epoch);
/* Test hook of the strict-progress region kernel: on != 0 makes every workgroup ask for the task index a REVERSED dispatch order would
 * give it (the stand-in for a device that does not start workgroups in index order): small launches then run with all roles on the
 * "wrong" workgroups, launches larger than the device go through the 200-us time-out and take the next free index.  Values must not
 * change (tests/test_gpu_r5.py). */
int lmm_dev_claim_scramble(int on);
/* C[MxN] -= A[MxK] * B[NxK]^T (column-major, device). lower != 0: only tiles on/below the diagonal. */
int lmm_dev_gemm_nt_sub(double* C, int ldc, const double* A, int lda, const double* B, int ldb,
                        int M, int N, int K, int lower);
/* Exact int8 modular emulation of the large Float64 trailing updates (switches LMM_F64_EMUL, LMM_F64_EMUL_MINK, read
 * once).  Test hook of the switches: on = 0 / 1, min_k >= 128 (updates with K >= min_k are emulated), 8 <= nmod <= 16 moduli;
 * on < 0 goes back to the env defaults. */
int lmm_dev_set_f64_emul(int on, int min_k, int nmod);
/* Test hook of the shape rule that decides which updates are emulated while no explicit threshold is set (neither LMM_F64_EMUL_MINK nor
 * lmm_dev_set_f64_emul): K >= min_k_always always, min_k_shape <= K < min_k_always when (matrices of the batch) x (outputs of the update's
 * lower trapezoid) >= min_outputs, smaller K never.  min_k_always < 0 goes back to the defaults (4096, 2048 and the measured crossover). */
int lmm_dev_set_f64_emul_rule(int min_k_always, int min_k_shape, double min_outputs);
/* Test hook: an emulated update walks its batch in groups of as many matrices as its scratch block holds; g >= 1 caps the group size,
 * 0 goes back to the default.  Results do not depend on it. */
int lmm_dev_set_emul_group(int g);
/* Test hook: an emulated update of a factorisation takes the row maxima of the part of its panel that earlier emulated updates of the
 * same factorisation scanned from the arrays those kept, and scans only the rest; on = 0 makes every update scan its whole panel,
 * on != 0 goes back to the default.  Results do not depend on it. */
int lmm_dev_set_emul_amax_reuse(int on);
/* Host-only (no GPU, no lmm_init needed): the emulation plan of a factorisation of nb matrices with NR rows and NC columns, by the code
 * the factorisation itself runs.  out[0] = bytes of the scratch block it asks for (0: nothing is emulated), out[1] = matrices per group
 * that block is sized for; then 6 words per trailing update with at least 128 columns, in launch order: M, N, K, emulated (0 / 1),
 * matrices per group, scratch bytes needed at that group size.  out holds 2 + 6 cap words.  Returns the number of updates (those beyond
 * cap are counted, not written), or -LMM_ERR_ARG.  Updates inside a block column that one dataflow launch factors are listed too; they
 * never run on their own. */
int lmm_dev_emul_plan(int NR, int NC, int nb, long long* out, int cap);
/* Host-only (no GPU, no lmm_init needed): what the batched Cholesky launches for nb matrices of NR rows and NC columns (multiples of 64;
 * rows_real of the rows hold data, NC <= rows_real <= NR, or -1: all) while in_flight batches run side by side on a device of cus CUs, in Float32 (f32 != 0) or
 * Float64, with strict progress on or off, under the current switches (the decision table and the step kinds).
 * out holds LMM_POTRF_PLAN_HEADER + LMM_POTRF_PLAN_STEP cap words.
 *   header: [0] 1 = 128-column panel path, 0 = 64-column recursion; [1] widest block column that is one region launch (0: none);
 *           per matrix: [2] doubles of the W2 scratch, [3] ints of the fused-bulk flags (0: no launch fuses), [4] doubles of the region
 *           assistants' scratch; [5] bytes and [6] matrices-per-group G of the emulation block, [7] moduli.
 *   step:   [0] kind -- 0 diag64, 1 64-column solve by inverse, 2 plain update, 3 leaf128, 4 panel bulk, 5 update + leaf, 6 emulated
 *           update + leaf, 7 region; [1] j0 (first column); [2] h (depth K of an update's product; the block's width otherwise);
 *           [3] N (columns); [4] M (rows; of an update: from row j0 + h); [5] profile class (lmm_prof_class); [6] 1 when the profile
 *           names the step's (M, N, K) = ([4], [3], [2]); [7] work and [8] bytes booked for the class, as the bits of a double;
 *           [9] first_done (region: its first diagonal block is already factored); [10] fused_bulk (update + leaf: the next panel's
 *           bulk rows ride in the launch); [11] a ragged last 64 rows: 0 none, 1 as items of the launch, 2 as a launch of their own;
 *           [12] matrices per group and [13] scratch bytes of an emulated update; of an update + leaf (kind 5), [12] is 1 when the
 *           step is screened (lmm_dev_set_f64_screen): its panel's row maxima are scanned and kept, and its launch leaves out the
 *           128 x 128 tiles, from tile column 1 on, whose update cannot change a bit of C.
 * Returns the number of steps (those beyond cap are counted, not written), or -LMM_ERR_ARG. */
#define LMM_POTRF_PLAN_HEADER 8
#define LMM_POTRF_PLAN_STEP 14
int lmm_dev_potrf_plan(int NR, int NC, int nb, int rows_real, int in_flight, int cus, int f32, int strict, long long* out, int cap);
/* Test hook: the emulation's GEMM is a persistent kernel of min(work items, CUs) workgroups; wgs >= 1 caps that grid (a small shape
 * then makes one workgroup walk several tiles), 0 goes back to the default.  Results do not depend on it. */
int lmm_dev_set_emul_gemm_workgroups(int wgs);
/* Switch of the emulation GEMM's zero skip.  A pass before the convert records, per 256 rows of a panel, which 128-wide K blocks hold
 * a non-zero truncated integer (from the block maxima the row scan keeps); on != 0 (the default; the environment's LMM_EMUL_ZERO_SKIP=0 turns it off) the GEMM's tiles walk only the
 * blocks that are live in both operands, on = 0 walks every block with the same kernel, on < 0 goes back to the environment's
 * default.  A skipped block multiplies exact zeros: results do not depend on it. */
int lmm_dev_set_emul_zero_skip(int on);
/* Test hook, default 0, never set outside tests: on != 0 makes every emulated update fill the residue scratch of a group with a
 * non-zero byte before its convert.  With the zero skip on the convert stores nothing into a dead K block (block 0 excepted), so the
 * fill stands in for whatever an earlier update left there.  Results do not depend on it. */
int lmm_dev_set_emul_scratch_poison(int on);
/* Host-only (no GPU, no lmm_init needed): the K blocks a GEMM tile of the emulation walks when its two operands have the live masks
 * (a0, a1) and (b0, b1) (bit k / 128 of a0 for k < 8192, of a1 above) and K = 128 nk, 1 <= nk <= 128, by the helpers the kernel
 * uses: out[0 .. min(cap, length)) = the blocks in walk order, *count (may be NULL) = the number of K steps the kernel's MFMA loop
 * runs.  An empty intersection walks block 0 alone.  Returns the length of the walk, or -LMM_ERR_ARG. */
int lmm_dev_emul_stage_list(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1, int nk, int* out,
                            int cap, int* count);
/* C[MxN] -= A[MxK] * A[0:N, :]^T for i >= j only (column-major, device pointers, one matrix) through the emulation kernels.
 * M >= N, K a multiple of 128, K <= 16384.  |error_ij| <= 4 K 2^-b amax_i amax_j + rounding of C, b = the bit budget for K. */
int lmm_dev_syrk_emul(double* C, int ldc, const double* A, int lda, int M, int N, int K, int nmod);
/* Host-only (no GPU, no lmm_init needed): out[MxN] (ldo) = the emulated product A[MxK] * B[NxK]^T (column-major host pointers, K <=
 * 4096) -- row scaling, residues, products modulo each modulus and the CRT combine in plain C++ with the constants and scalar steps of
 * the kernels; the bit budget b is the one of depth k_bound >= K.  consts (may be NULL, 68 doubles): [0..15] moduli, [16..31],
 * [32..47], [48..63] the three chunks of the CRT weights, [64..66] the chunks of the moduli's product, [67] b. */
int lmm_dev_emul_host(const double* A, int lda, const double* B, int ldb, int M, int N, int K, int nmod, int k_bound, double* out,
                      int ldo, double* consts);
/* Host-only (no GPU, no lmm_init needed): the residue step of the emulation's convert kernel on `count` integers |v| <= 2^58:
 * out[i * nmod + t] = v[i] modulo the t-th modulus as an int8 (congruent, inside the symmetric range).  exhaustive (may be NULL, 2
 * words): the reduction behind it run on every input it can see, every odd modulus, both signs: [0] cases, [1] failures. */
int lmm_dev_emul_residues(const long long* v, int count, int nmod, signed char* out, long long* exhaustive);
/* Host-only (no GPU, no lmm_init needed): the liveness decision of the emulation's convert, which reads a 16-row piece of a 128-wide
 * K block only when the block maxima kept by the row scan say it holds a non-zero truncated integer.  For `count` (row, K block)
 * pairs at the bit budget 1 <= bits <= 58: out[i] = 1 when trunc(|blockmax[i]| 2^(bits - e)) != 0, e = ceil(log2 |rowmax[i]|), for a
 * finite non-zero rowmax[i]; 0 otherwise (a row of zeros, or one with a NaN or an infinity, is all zeros to the GEMM). */
int lmm_dev_emul_block_live(const double* rowmax, const double* blockmax, int count, int bits, int* out);
/* Switch of the emulation's screen.  Once the row maxima of a panel exist, a pass over C marks the 256 x 256 tiles of the update in
 * which every output is negligible (lmm_dev_emul_negligible); on != 0 (the default; the environment's LMM_EMUL_SCREEN=0 turns it off)
 * the GEMM and the combine leave those tiles out, on = 0 treats every tile as live with the same kernels, on < 0 goes back to the
 * environment's default.  A skipped tile's update would not have changed a bit of C: results do not depend on it. */
int lmm_dev_set_emul_screen(int on);
/* Test hook: the number of tiles of the last lmm_dev_syrk_emul call that were not skipped by the screen (all of the lower
 * trapezoid's 256 x 256 tiles with the screen off), -1 before the first call. */
int lmm_dev_emul_last_live_tiles(void);
/* Host-only (no GPU, no lmm_init needed): the screen's predicate.  For `count` outputs of an update of depth 1 <= K <= 16384:
 * out[i] = 1 when c[i] is finite and not zero, rowmax_i[i] and rowmax_j[i] (the largest |entry| of the output's two panel rows) are
 * finite, and one of them is zero or ceil(log2 K) + e_i + e_j + 56 <= ilogb(c[i]) with e = ceil(log2 |rowmax|); 0 otherwise.  Then
 * the update the emulation would subtract is below a quarter of the spacing of the doubles under |c[i]|, and c[i] keeps its bits. */
int lmm_dev_emul_negligible(int K, const double* rowmax_i, const double* rowmax_j, const double* c, int count, int* out);
/* The same screen in front of the f64 update launches (switches LMM_F64_SCREEN, LMM_F64_SCREEN_MINK, LMM_F64_SCREEN_VOTE,
 * LMM_F64_SCREEN_ROUNDS, read once).  By default an update on the f64 kernel is screened when K >= 512, it has more than one tile
 * column and its launch has more work items than one round of two workgroups per CU.  Test hook: on = 0 / 1; EVERY update on the f64
 * kernel with K >= min_k >= 128 and more than one tile column is screened, whatever its size; on < 0 goes back to the defaults.  A
 * skipped tile's update would not have changed a bit of C: results do not depend on it. */
int lmm_dev_set_f64_screen(int on, int min_k);
/* Test hook: LMM_DETERMINISTIC (read once) -- on != 0: no split-K atomics in the update launches, so sums are bitwise reproducible. */
int lmm_dev_set_deterministic(int on);
/* Test hook: on != 0 makes every later factorisation copy its screened updates' counters to the host (this synchronises its stream).
 * out (cap records of 5 ints; may be NULL with cap = 0): for every screened update of the last factorisation of the process, in
 * launch order: M, N, K, the dead tiles its screen counted, 1 when the screen did its work (0: the first screened update found no
 * dead tile and this one returned at entry).  Returns the number of records (those beyond cap are counted, not written), or -LMM_ERR_ARG. */
int lmm_dev_f64_screen_stats(int on, int* out, int cap);
/* The scan and the screen of ONE f64 update C[MxN] -= A[MxK] A[0:N, :]^T (column-major, device pointers; M >= N > 128, M >= 256, K a
 * multiple of 128), as a screened step of a factorisation runs them.  flags (host, ceil(M / 128) x ceil(N / 128) bytes, row-major over
 * (tile row, tile column)): for 1 <= tile column <= tile row, 1 when some entry i >= j of the tile is not negligible
 * (lmm_dev_emul_negligible), 0 when the tile is dead; 0xFF elsewhere (never written).  *dead = the dead tiles the screen counted. */
int lmm_dev_f64_screen_flags(const double* C, int ldc, const double* A, int lda, int M, int N, int K, unsigned char* flags, int* dead);
/* Zero extents (DESIGN.md 4.17 "rows whose panel is exactly zero"; switch LMM_ZERO_EXTENTS, read once, default 1).  The Gram launch of
 * a Float64 per-latent logpdf keeps, per block of 64 rows of each factor matrix, the number of leading columns (whole 64-column blocks
 * of the lower triangle) in which every entry of those rows was stored as +0; a row block that is all zeros keeps 0x7F7F7F7F.  The
 * factorisation leaves out the region row tasks, the f64 update items and the emulated update tiles whose rows are zero across the
 * whole panel: for a finite factor they would only rewrite the zeros that are there, so results do not depend on the switch, bit
 * for bit.  LMM_ZERO_EXTENTS=0: no extents are kept.  None are kept either for matrices of at most LMM_REGION (1024) columns, which one
 * region launch factors whole: no item of theirs can be void.  With LMM_REGION_OCC=2 the region launches leave nothing out (the
 * two-per-CU build has no void test; its counters stay 0) -- updates and screens still do.  Test hook: on = 0 / 1, on < 0 goes
 * back to the default. */
int lmm_dev_set_zero_extents(int on);
/* The size gate of the zero extents (LMM_ZERO_EXTENTS_MINCOLS, read once; default 2048): a per-latent logpdf keeps them only for
 * matrices of more than this many columns -- at 2048 columns they cost more than the little that is void there gains.  Test hook:
 * cols >= 0 sets the gate, cols < 0 goes back to the default. */
int lmm_dev_set_zero_extents_min_cols(int cols);
/* Test hook: on != 0 makes every later factorisation that has zero extents count the work items it leaves out and copy the counters to
 * the host (this synchronises its stream).  out (cap records of 7 ints; may be NULL with cap = 0): for every region, update + leaf
 * and emulated update + leaf step of the last factorisation of the process, in launch order: the step kind (as in
 * lmm_dev_potrf_plan), j0, h, N, M, the count over all matrices of the batch, and a shape word (a region launch: how many of its
 * row tasks are 128 rows high, the rest 64; an update: 1 when the bulk rows ride along + 2 x the strip mode of the plan).  The count: row tasks of a region launch that returned at
 * entry; rest and column-0 items of an f64 update launch that did (a split tile counts once); 256 x 256 tiles the emulation's
 * screen marked dead without reading C.  No records when that factorisation had no extents.  Returns the number of records (those
 * beyond cap are counted, not written), or -LMM_ERR_ARG. */
int lmm_dev_zero_extent_stats(int on, int* out, int cap);
/* lmm_dev_potrf with the caller's zero extents: zext (device, nrows / 64 ints) holds, per block of 64 rows, a number of leading
 * columns in which all entries of those rows are +0 -- the true extents or any smaller values.  NULL: exactly lmm_dev_potrf. */
int lmm_dev_potrf_zext(double* A, int nrows, int ncols, int ld, double* Winv, int n_real, int* info_dev, const int* zext);
/* The training Gram launch of the per-latent logpdf for nb latents on device memory: matrix j (nrows x ncols, leading dimension ld,
 * nrows and ncols multiples of 64, ncols >= n) at A + j * ld * ncols = K_j(x, x) + noise[j] I (or + diag(noisevec[j][.]), device,
 * when noisevec is given), the identity on the padding, rows ncols .. ncols + nrider - 1 = rider[j][r][.] (device).  zext (host,
 * nb x nrows / 64 ints): the zero extents the launch kept, -1 everywhere when none are kept (switch off, Float32). */
int lmm_dev_train_gram(double* A, int ld, int nrows, int ncols, const double* x, int d, int n, const lmm_gp_t* gp, int nb,
                       const double* noise, const double* noisevec, const double* rider, int nrider, int* zext);
/* Host-only (no GPU, no lmm_init needed): the reduction of the emulation's GEMM epilogue on `count` int32 accumulators |x| <= 2^28:
 * out[i * nmod + t] = x[i] modulo the t-th modulus as an int8 (congruent, inside the symmetric range).  exhaustive (may be NULL, 2
 * words): its float step run on every folded value it can see, every modulus: [0] cases, [1] failures. */
int lmm_dev_emul_acc_residues(const int* x, int count, int nmod, signed char* out, long long* exhaustive);
/* Gram assembly of one latent into a padded factor matrix (lower triangle + pad identity). */
int lmm_dev_gram(double* A, int ld, int nrows, int ncols, const double* x, int d, int n,
                 const lmm_gp_t* gp, double diag_add);
/* Standard normals generated on the device (Philox4x32-10 counter RNG + Box-Muller, Float64): out[j] for j < count is a
 * function of (seed, stream, j) only.  Optional companion of lmm_lmm_rand*: the reference draws its normals on the host with
 * the caller's rng (src/oilmm.jl:47,53), and the shim keeps doing so when the reference's random stream matters. */
int lmm_normals(unsigned long long seed, unsigned long long stream, size_t count, double* out);
/* ---- measurement hooks (bench.py roofline leg) ------------------------------------------------ */
/* Between lmm_profile_begin and lmm_profile_end every launch of the classes below is bracketed by HIP events
 * on the stream it is launched on.  serial != 0 forces all latents onto ONE stream, so an event pair times its
 * kernel alone (the production path runs latents on concurrent streams, where durations overlap).
 * work = algorithmic flops (MFMA classes) or algorithmic HBM bytes (Gram assembly) summed over launches. */
typedef enum {
  LMM_PROF_GRAM = 0,          /* gram_batch_kernel: lower-triangular f64 write, bytes                                          */
  LMM_PROF_UPDATE = 1,        /* potrf_node_kernel<2, .> (round 3: SYRK/GEMM trailing update with K >= 1024 + the next panel's leaf128 in
                                 one launch -- at K = 1024, 2048 also that panel's bulk rows --, + gemm16h_kernel<true> for a ragged
                                 last 64 rows; LMM_PANEL128=0 / fp32: every wide
                                 update: gemm16p_kernel / gemm16h_kernel / gemm32_kernel), flops                                */
  LMM_PROF_UPDATE_NARROW = 2, /* gemm44_kernel<64,false>: 64-column update (round-2 path; trailing 64 columns), flops           */
  LMM_PROF_TRSM = 3,          /* potrf_node_kernel<1> in bulk mode (the panels whose bulk rows do not ride in an update launch): panel
                                 rows x 128 x 128 inverse (round-2 path:
                                 gemm44_kernel<64,true>, TRSM by the 64 x 64 inverse block), flops                              */
  LMM_PROF_DIAG = 4,          /* leaf128_kernel (first panel) / diag64m_kernel: diagonal-block factor + inverse, flops          */
  LMM_PROF_REGION = 5,        /* potrf_region_kernel: a block column of <= 8 panels (leaves, bulk products, inner updates) in one
                                 dataflow launch, flops                                                                         */
  LMM_PROF_UPDATE_SHORT = 6,  /* potrf_node_kernel<1>: the same fused update + leaf for K < 1024 (latency- and epilogue-bound levels)  */
  LMM_PROF_SOLVE = 7,         /* gemm16p_kernel inside the triangular solves R <- R L^-T against a stored factor (cross-Gram rows of the
                                 predictive paths, L^-T of the gradient paths): the K = 64 .. n/2 block updates, flops 2 rows cols K;
                                 the dominant class of BASELINE configs[3] (n* n^2 of its n^3/3 + n* n^2 flops per latent)            */
  LMM_PROF_SOLVE_LEAF = 8,    /* gemm44_kernel<64,true>: the 64-column solves by the stored inverse diagonal blocks, flops rows 64^2    */
  LMM_PROF_STRIP = 9,         /* strip_reduce_kernel + strip_finish_kernel: posterior marginals from one read of R (HBM read), bytes   */
  LMM_PROF_COUNT = 10
} lmm_prof_class;
typedef struct { long long launches; double ms; double work; double bytes; /* algorithmic HBM bytes */ } lmm_prof_entry_t;
int lmm_profile_begin(int serial);
int lmm_profile_end(lmm_prof_entry_t* out /* LMM_PROF_COUNT entries */);

/* Write-only yardstick next to the Gram assembly's HBM roofline (bench.py roofline_gram.achievable_write_gbs): GB/s of `reps`
 * hipMemsetAsync fills of a pooled device block of `bytes` (>= 1 MiB), timed with HIP events on the library's main stream. */
int lmm_dev_write_rate(size_t bytes, int reps, double* gbs);

/* f64 MFMA issue-rate microbenchmark: measured TFLOP/s of v_mfma_f64_16x16x4_f64 in the form the update kernels issue it (16
 * accumulator blocks in architectural VGPRs, 4 + 4 operand fragments per k-step; tools/mfma_probe4: 77.7 = 98.9 % of the 78.6
 * datasheet peak -- the same instruction with AccVGPR accumulators issues at 36). */
int lmm_dev_mfma_f64_peak(double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* LMM_HIP_H */
