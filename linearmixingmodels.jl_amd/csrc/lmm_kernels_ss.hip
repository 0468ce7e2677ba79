// lmm_kernels_ss.hip -- linear-time state-space inference for Matern12 / 32 / 52 and SHO latents over a one-dimensional input:
// the Kalman filter and the Rauch-Tung-Striebel smoother as parallel scans over the n points.  Float64 only; built WITHOUT
// -amdgpu-mfma-vgpr-form=1 (no MFMA here).  Three phases per direction, no atomics, results depend only on (arguments, chunk):
//   1. ss_fold_kernel / ss_bfold_kernel: each thread folds the scan elements of its `chunk` consecutive points into one aggregate;
//   2. ss_scan_kernel (+ ss_addprefix_kernel): the aggregates are scanned, 128 per workgroup through LDS (Hillis-Steele); with more
//      aggregates than one workgroup takes, the workgroups' totals are scanned by the same kernel (recursion on the host) and applied;
//   3. ss_filter_kernel / ss_rts_kernel: each thread restarts the ordinary recursion from its prefix (suffix) state over its run and
//      writes the marginals; the filter's log-density partials are added in thread order by ss_finish_kernel.
// A(dt) and Q(dt) are evaluated on the fly from x_t - x_{t-1}; blockIdx.z is the latent.  Every latent of a launch has the same MODEL
// (the template arguments D and MOD: Matern12 / 32 / 52, or the damped oscillator of an SHO latent, which shares D = 2 with Matern32
// but not its A(dt), or the sum of two of them inside one latent, SSSum, with D = D_a + D_b <= 4 and no kernel text of its own); the
// scans see elements only and are shared between models of equal D.
// Gradients (launch_ss_grad): d lml / d variance and d lml / d lengthscale (and an SHO latent's d lml / d quality) are the forward-mode
// derivative of phases 1 - 3 of the filter, the same text instantiated with SSDual (lmm_statespace.h): ss_fold_kernel<D, MOD, SSDual>,
// the scan over SSFwd<D, SSDual> and ss_filter_kernel<D, MOD, SSDual>, with blockIdx.y the seeded parameter (2 per Matern latent, 3 per
// SHO latent), so a thread carries one tangent.  d lml / d r_t and d lml / d w_t come from the smoothed
// marginals (ss_point_kernel), with fixed-order sums of what the OILMM chain rule needs.
// Sampling (launch_ss_path): the prior path is an affine recursion in the caller's normals, so phases 1 - 3 run on SSAff<D> elements
// (ss_sfold_kernel, the scan with AffOp, ss_path_kernel); a posterior path is the prior path plus the smoothed mean of the residual
// data r - f - sqrt(w) xi (ss_pathwise_kernel, then the filter and smoother above, then ss_addpath_kernel).
// The posterior object (launch_ss_interp): ss_rts_kernel<D, MOD, SS_RTS_FULL> keeps the full smoothed and the filtered states point-major, and
// ss_interp_kernel answers a query at a new input from the two stored states that bracket it, one thread per (query, latent): a binary
// search over x, one predict step, one RTS step (ss_interp); no LDS, no atomics, a query's result depends on no other query.
// Sampling from the posterior object (launch_ss_post_path): given the data the states at the sorted queries and the training points
// between them are a Markov chain that runs backwards, an affine recursion in the caller's normals again, so phases 1 - 3 run from the
// right on SSAff<D> elements built from the stored states (ss_window_kernel, ss_pfold_kernel, the suffix scan with AffRevOp,
// ss_ppath_kernel); nothing outside the queries' span is read.
// Predictive log density from the posterior object (launch_ss_post_logpdf): held-out data at the queries are observations of that same
// backward chain, so its marginal likelihood is a Kalman filter over the window from the right with affine transitions: phases 1 - 3
// on SSFwd<D> elements (ss_lfold_kernel, the suffix scan with FwdRevOp, ss_lfilter_kernel, ss_finish_kernel).
// Gradients with respect to locations: d lml / d x_t = g_t - g_{t+1} with g_t = d lml / d (x_t - x_{t-1}) local to one
// transition (ss_input_grad); ss_rts_kernel<D, MOD, SS_RTS_GX> writes g while it steps through the points, ss_grad_x_kernel adds the
// latents in order.  For the posterior object ss_interp_dx_kernel writes d mean / d s and d var / d s per (query, latent) and
// ss_contract_dx_kernel contracts them with H and the cotangents, one thread per query, latents in order.  No atomics, no LDS.
// Appending observations (launch_ss_filter_from, launch_ss_smooth_kept) adds no kernel: ss_fold_kernel / ss_filter_kernel on SSFromArgs
// start from a stored state instead of the prior, and ss_bfold_kernel<.., true> / ss_rts_kernel<.., SS_RTS_KEPT> smooth over kept states.
// Shared by the kernels (lmm_statespace.h): ss_chunk_range (a thread's run), ss_count_le / ss_count_lt (the binary searches) and
// ss_load_state / ss_store_state (a stored state in either layout); ss_lat_model makes the model of any *Lat struct.  On the host, Models::dispatch hands a
// launch's model to a generic lambda as compile-time (D, MOD), and ss_phases is the fold - scan - restart sequence of every direction
// (ss_scored_phases: with the log-density finish, and the single launch when there is one chunk).
// Two translation units: the templated kernels and the launch sequences are in lmm_kernels_ss.h; this file instantiates them for the
// one-term models (SSOneTermModels) and holds the kernels that take no model; lmm_kernels_ss_sum.hip instantiates them for the seven
// sums of two terms (SSPairModels), and the launch_ss_* below hand a sum's model to its launch_ss_*_pair.
#include "lmm_kernels_ss.h"

namespace {

constexpr int SS_POINT_PER = 8;      // points per thread of ss_point_kernel

// Per point, from the smoothed first-component mean mu and variance Ps (without the latent's mean): alpha_t = (r_t - mu_t) / w_t and
// c_t = (w_t - Ps_t) / w_t^2, the t-th entry of C^-1 r and of diag C^-1 for C = K + diag(w) over the observed points: d lml / d r_t =
// -alpha_t and d lml / d w_t = grad_w = (alpha^2 - c) / 2.  Both outputs are 0 at an unobserved point.  ppart[((z 4 + q) nblk) + block]: this block's sums of alpha,
// w alpha^2, w c and grad_w, added in a fixed order (a thread its points in order, then a tree over the threads).
__global__ __launch_bounds__(SS_THREADS) void ss_point_kernel(SSArgs a, double* __restrict__ alpha, double* __restrict__ grad_w,
                                                              double* __restrict__ ppart) {
  __shared__ double sh[4][SS_THREADS];
  const int z = blockIdx.z, nblk = gridDim.x;
  const SSLat& L = a.lat[z];
  const double* sm = a.smean + (size_t)z * a.n;
  const double* sv = a.svar + (size_t)z * a.n;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < SS_POINT_PER; ++k) {
    const long long t = ((long long)blockIdx.x * SS_POINT_PER + k) * SS_THREADS + threadIdx.x;
    if (t >= a.n) break;
    const double w = L.w[t];
    double al = 0.0, gw = 0.0;
    if (w < INFINITY) {
      al = (L.r[t] - sm[t]) / w;
      const double c = (w - sv[t]) / (w * w);
      gw = 0.5 * (al * al - c);
      s[0] += al; s[1] += w * al * al; s[2] += w * c; s[3] += gw;
    }
    alpha[(size_t)z * a.n + t] = al;
    grad_w[(size_t)z * a.n + t] = gw;
  }
  for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int off = SS_THREADS / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 4) ppart[((size_t)z * 4 + threadIdx.x) * nblk + blockIdx.x] = sh[threadIdx.x][0];
}

// *flag = 1 when some xs_t < bound, else 0: one workgroup strides over the queries, an OR through LDS, thread 0 writes (no atomics)
__global__ __launch_bounds__(SS_THREADS) void ss_any_below_kernel(const double* __restrict__ xs, int ns, double bound, int* __restrict__ flag) {
  __shared__ int sh[SS_THREADS];
  int any = 0;
  for (int t = threadIdx.x; t < ns; t += SS_THREADS) any |= xs[t] < bound ? 1 : 0;
  sh[threadIdx.x] = any;
  __syncthreads();
  for (int off = SS_THREADS / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] |= sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *flag = sh[0];
}

// one thread per query: the latents' derivatives contracted with H and the cotangents, latents in order (launch_ss_contract_dx)
__global__ __launch_bounds__(256) void ss_contract_dx_kernel(const double* __restrict__ dmean, const double* __restrict__ dvar,
                                                             const double* __restrict__ H, int p, int ms, const double* __restrict__ dmu,
                                                             const double* __restrict__ dv, int ns, double* __restrict__ grad_xs) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= ns) return;
  double acc = 0.0;
  for (int l = 0; l < ms; ++l) {
    double cm = 0.0, cv = 0.0;
    for (int o = 0; o < p; ++o) {
      const double h = H[o + (size_t)l * p];
      if (dmean) cm += dmean[q + (size_t)o * ns] * h;
      if (dvar) cv += dvar[q + (size_t)o * ns] * (h * h);
    }
    acc += cm * dmu[(size_t)l * ns + q] + cv * dv[(size_t)l * ns + q];
  }
  grad_xs[q] = acc;
}

// one thread per point: d lml / d x_t from the spacings' derivatives, latents in order (launch_ss_grad_x)
__global__ __launch_bounds__(256) void ss_grad_x_kernel(const double* __restrict__ g, const double* __restrict__ w, int n, int ms,
                                                        double* __restrict__ grad_x) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= n) return;
  double acc = 0.0;
  for (int l = 0; l < ms; ++l) {
    const double* gl = g + (size_t)l * n;
    if (w[(size_t)l * n + t] < INFINITY) acc += gl[t] - (t + 1 < n ? gl[t + 1] : 0.0);
  }
  grad_x[t] = acc;
}

// *flag = the smallest t with xs_t NaN or +-Inf, left at its initial value (INT_MAX) when every query is finite (ss_sorted_kernel's way)
__global__ __launch_bounds__(256) void ss_finite_kernel(const double* __restrict__ xs, int ns, int* flag) {
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < ns; t += (long long)gridDim.x * 256)
    if (!(fabs(xs[t]) < INFINITY)) atomicMin(flag, (int)t);
}

// *flag = the smallest t >= 1 with !(x_t >= x_{t-1}) (a NaN counts), left at its initial value (INT_MAX) when x is non-decreasing.
// atomicMin on an index: the result does not depend on the order of arrival.
__global__ __launch_bounds__(256) void ss_sorted_kernel(const double* __restrict__ x, int n, int* flag) {
  for (long long t = 1 + blockIdx.x * 256ll + threadIdx.x; t < n; t += (long long)gridDim.x * 256)
    if (!(x[t] >= x[t - 1])) atomicMin(flag, (int)t);
}

// out[j + o nsel] = in[idx[j] + o n]: the selected rows of an n x p column-major matrix
__global__ __launch_bounds__(256) void ss_gather_rows_kernel(const double* __restrict__ in, int n, const int* __restrict__ idx, int nsel,
                                                             double* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (j < nsel) out[j + (size_t)o * nsel] = in[idx[j] + (size_t)o * n];
}

// out[idx[j] + o n] = in[j + o nsel]
__global__ __launch_bounds__(256) void ss_scatter_rows_kernel(const double* __restrict__ in, int n, const int* __restrict__ idx, int nsel,
                                                              double* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (j < nsel) out[idx[j] + (size_t)o * n] = in[j + (size_t)o * nsel];
}

// Pathwise conditioning, entry (latent k, sample q) = blockIdx.z, blockIdx.y: rp = r - f - sqrt(w) xi at an observed point; an
// unobserved one (w = +Inf) keeps its r, and xi is not read there.  r, w: [latent][n]; f: [sample][latent][n]; xi: sample q's values of
// latent k at q xi_stride + k n; rp: [latent][sample][n], the entry order of the filter and smoother that follow.
__global__ __launch_bounds__(256) void ss_pathwise_kernel(const double* __restrict__ r, const double* __restrict__ w,
                                                          const double* __restrict__ f, const double* __restrict__ xi, size_t xi_stride,
                                                          int n, double* __restrict__ rp) {
  const int t = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, k = blockIdx.z, ms = gridDim.z, N = gridDim.y;
  if (t >= n) return;
  const double wt = w[(size_t)k * n + t];
  double v = r[(size_t)k * n + t];
  if (wt < INFINITY) v = v - f[((size_t)q * ms + k) * n + t] - sqrt(wt) * xi[(size_t)q * xi_stride + (size_t)k * n + t];
  rp[((size_t)k * N + q) * n + t] = v;
}

// f[sample][latent][n] += sm[latent][sample][n]: the posterior path, prior path + smoothed mean of the residual (+ the latent's mean)
__global__ __launch_bounds__(256) void ss_addpath_kernel(double* __restrict__ f, const double* __restrict__ sm, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, k = blockIdx.z, ms = gridDim.z, N = gridDim.y;
  if (t >= n) return;
  const size_t i = ((size_t)q * ms + k) * n + t;
  f[i] = f[i] + sm[((size_t)k * N + q) * n + t];
}

// out[0] = #{t : x_t <= lo}, out[1] = #{t : x_t <= hi}; xs != nullptr: (lo, hi) = (xs[0], xs[ns - 1])
__global__ void ss_window_bounds_kernel(const double* __restrict__ x, int n, const double* __restrict__ xs, int ns, double lo, double hi,
                                        int* __restrict__ out) {
  if (threadIdx.x > 1 || blockIdx.x > 0) return;
  const double s = xs ? (threadIdx.x ? xs[ns - 1] : xs[0]) : (threadIdx.x ? hi : lo);
  out[threadIdx.x] = ss_count_le(x, 0, n, s);
}

// One thread per window point.  Thread u < count is training point t = first + u, at (t - first) + #{i : q_i < x_t}; thread count + i
// is query i, at i + #{t : x_t <= q_i} - first.  Both counts are binary searches; the positions are a permutation of 0 .. W - 1 (a
// stable merge with training points in front of equal queries), so every entry of src is written once.
__global__ __launch_bounds__(256) void ss_window_kernel(const double* __restrict__ x, int n, const double* __restrict__ xs, int ns,
                                                        int first, int count, int* __restrict__ src) {
  const long long u = blockIdx.x * 256ll + threadIdx.x;
  if (u >= (long long)count + ns) return;
  if (u < count) {
    const int t = first + (int)u;
    const double xt = x[t];
    src[(long long)u + ss_count_lt(xs, 0, ns, xt)] = t;
  } else {
    const int i = (int)(u - count);
    const double s = xs[i];
    // first <= #{t : x_t <= q_i} <= first + count: q_0 <= q_i <= q_{ns-1}
    src[(long long)i + (ss_count_le(x, first, first + count, s) - first)] = -1 - i;
  }
}

// ss_interp_kernel's threads, writing the derivatives of its two outputs with respect to the query instead (ss_interp_dx_state; Matern12:
// ss_interp_dx_ou on ss_interp's inputs).  At a query equal to a training input they are those of the side the search sorts it to
// (behind every copy), which matters for Matern12 alone: its posterior mean has a kink there.
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_interp_dx_kernel(SSInterpArgs a) {
  const int q = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (q >= a.ns) return;
  const SSInterpLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
  const double s = a.xs[q];
  const int k = ss_count_le(a.x, 0, a.n, s);
  double m[D], P[D][D], ms[D], Ps[D][D];
  for (int i = 0; i < D; ++i) {
    m[i] = 0.0; ms[i] = 0.0;
    for (int j = 0; j < D; ++j) { P[i][j] = 0.0; Ps[i][j] = 0.0; }
  }
  double d1 = 0.0, d2 = 0.0;
  if (k > 0) {
    ss_load_state<D>(a.fstate + (size_t)z * a.state_stride, a.comp_stride, a.point_stride, k - 1, m, P);
    d1 = s - a.x[k - 1];
  }
  if (k < a.n) {
    ss_load_state<D>(a.sstate + (size_t)z * a.state_stride, a.comp_stride, a.point_stride, k, ms, Ps);
    d2 = a.x[k] - s;
  }
  double dmu, dv;
  if constexpr (D == 1) ss_interp_dx_ou(M, k > 0, d1, k < a.n, d2, m[0], P[0][0], ms[0], Ps[0][0], dmu, dv);
  else {
    ss_interp<D>(M, k > 0, d1, k < a.n, d2, m, P, ms, Ps);
    ss_interp_dx_state<D>(m, P, dmu, dv);
  }
  a.dmean[(size_t)z * a.ns + q] = dmu;
  a.dvar[(size_t)z * a.ns + q] = dv;
}

size_t scan_items(int nch, int W = SS_SCAN) {         // items of every level below the first
  size_t tot = 0;
  int N = nch;
  while (N > W) { N = (N + W - 1) / W; tot += N; }
  return tot;
}

// doubles of one item's aggregates of type E and of its share of the scan's levels
template <typename E>
size_t agg_elems(int nch) { return ((size_t)nch + scan_items(nch, ss_scan_width<E>())) * (sizeof(E) / sizeof(double)); }

// f(std::integral_constant<int, D>()) for a state dimension 1 .. 4: the scan elements' sizes depend on D alone
template <typename F>
auto ss_dispatch_dim(int D, F&& f) {
  if (D == 1) return f(std::integral_constant<int, 1>());
  if (D == 2) return f(std::integral_constant<int, 2>());
  if (D == 3) return f(std::integral_constant<int, 3>());
  return f(std::integral_constant<int, 4>());
}

// The one-term models of a launch: 1 / 2 / 3 is the Matern model of that state dimension, SS_MODEL_SHO the oscillator (D = 2).
static_assert(SS_MODEL_SHO > 3, "a state dimension 1 / 2 / 3 is the number of its Matern model: none may be the oscillator's number");
struct SSOneTermModels {
  template <typename F>
  static auto dispatch(int model, F&& f) {
    if (model == SS_MODEL_SHO) return f(SSModelTag<2, true>());
    if (model == 1) return f(SSModelTag<1, false>());
    if (model == 2) return f(SSModelTag<2, false>());
    return f(SSModelTag<3, false>());
  }
};
inline bool ss_is_pair(int model) { return model >= SS_PAIR(1, 1); }      // a sum of two terms: lmm_kernels_ss_sum.hip has its kernels

}  // namespace

int ss_model_of(int kind) {
  return kind == LMM_KERNEL_MATERN12 ? 1 : kind == LMM_KERNEL_MATERN32 ? 2 : kind == LMM_KERNEL_MATERN52 ? 3 : kind == LMM_KERNEL_SHO ? SS_MODEL_SHO : 0;
}
// The one order of a sum's terms: Matern12, Matern32, SHO, Matern52 (by state dimension, the oscillator behind Matern32)
int ss_pair_model(int a, int b, int* swapped) {
  const auto rank = [](int t) { return t == 1 ? 0 : t == 2 ? 1 : t == SS_MODEL_SHO ? 2 : t == 3 ? 3 : -1; };
  if (rank(a) < 0 || rank(b) < 0 || ss_term_dim(a) + ss_term_dim(b) > 4) return 0;
  const bool sw = rank(b) < rank(a);
  if (swapped) *swapped = sw;
  return sw ? SS_PAIR(b, a) : SS_PAIR(a, b);
}
int ss_model_dim(int model) {
  return model >= SS_PAIR(1, 1) ? ss_term_dim(model / SS_PAIR(1, 0)) + ss_term_dim(model % SS_PAIR(1, 0)) : ss_term_dim(model);
}
int ss_model_seeds(int model) {
  return model >= SS_PAIR(1, 1) ? ss_term_seeds(model / SS_PAIR(1, 0)) + ss_term_seeds(model % SS_PAIR(1, 0)) : ss_term_seeds(model);
}
int ss_state_dim(int kind) { return ss_model_dim(ss_model_of(kind)); }
int ss_state_comps(int D) { return D + D * (D + 1) / 2; }
int ss_default_chunk(int n) { return n <= 4096 ? 16 : 64; }
size_t ss_fwd_agg_elems(int D, int nch) { return ss_dispatch_dim(D, [&](auto t) { return agg_elems<SSFwd<decltype(t)::value>>(nch); }); }
size_t ss_bwd_agg_elems(int D, int nch) { return ss_dispatch_dim(D, [&](auto t) { return agg_elems<SSBwd<decltype(t)::value>>(nch); }); }
size_t ss_aff_agg_elems(int D, int nch) { return ss_dispatch_dim(D, [&](auto t) { return agg_elems<SSAff<decltype(t)::value>>(nch); }); }
size_t ss_dual_agg_elems(int D, int nch, int nseeds) {
  return nseeds * ss_dispatch_dim(D, [&](auto t) { return agg_elems<SSFwd<decltype(t)::value, SSDual>>(nch); });
}
int ss_point_blocks(int n) { return (n + SS_THREADS * SS_POINT_PER - 1) / (SS_THREADS * SS_POINT_PER); }

void launch_ss_filter(const SSArgs& a, int model, int nb, double* lml, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_filter_pair(a, model, nb, lml, st);
  else ss_launch_filter<SSOneTermModels>(a, model, nb, lml, st);
}

void launch_ss_smooth(const SSArgs& a, int model, int nb, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_smooth_pair(a, model, nb, st);
  else ss_launch_smooth<SSOneTermModels>(a, model, nb, st);
}

void launch_ss_filter_from(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_filter_from_pair(a, model, nb, lml, st);
  else ss_launch_filter_from<SSOneTermModels>(a, model, nb, lml, st);
}

void launch_ss_smooth_kept(const SSArgs& a, int model, int nb, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_smooth_kept_pair(a, model, nb, st);
  else ss_launch_smooth_kept<SSOneTermModels>(a, model, nb, st);
}

void launch_ss_any_below(const double* xs, int ns, double bound, int* flag, hipStream_t st) {
  hipLaunchKernelGGL(ss_any_below_kernel, dim3(1), dim3(SS_THREADS), 0, st, xs, ns, bound, flag);
}

void launch_ss_grad(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_grad_pair(a, model, nb, gtheta, st);
  else ss_launch_grad<SSOneTermModels>(a, model, nb, gtheta, st);
}

void launch_ss_point(const SSArgs& a, int nb, double* alpha, double* grad_w, double* ppart, double* sums, hipStream_t st) {
  const int nblk = ss_point_blocks(a.n);
  hipLaunchKernelGGL(ss_point_kernel, dim3(nblk, 1, nb), dim3(SS_THREADS), 0, st, a, alpha, grad_w, ppart);
  hipLaunchKernelGGL(ss_finish_kernel, dim3(4 * nb), dim3(SS_THREADS), 0, st, (const double*)ppart, nblk, sums);
}

void launch_ss_path(const SSPathArgs& a, int model, int nb, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_path_pair(a, model, nb, st);
  else ss_launch_path<SSOneTermModels>(a, model, nb, st);
}

void launch_ss_post_path(const SSPostArgs& a, int model, int nb, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_post_path_pair(a, model, nb, st);
  else ss_launch_post_path<SSOneTermModels>(a, model, nb, st);
}

void launch_ss_post_logpdf(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_post_logpdf_pair(a, model, nb, lml, st);
  else ss_launch_post_logpdf<SSOneTermModels>(a, model, nb, lml, st);
}

void launch_ss_interp(const SSInterpArgs& a, int model, int nb, hipStream_t st) {
  if (ss_is_pair(model)) launch_ss_interp_pair(a, model, nb, st);
  else ss_launch_interp<SSOneTermModels>(a, model, nb, st);
}

void launch_ss_interp_dx(const SSInterpArgs& a, int model, int nb, hipStream_t st) {
  // (one-term models only: component 2 of a sum's state is not f', and the entry points refuse it before they come here)
  SSOneTermModels::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((ss_interp_dx_kernel<T::D, T::MOD>), dim3((a.ns + SS_THREADS - 1) / SS_THREADS, 1, nb), dim3(SS_THREADS), 0, st, a);
  });
}

void launch_ss_contract_dx(const double* dmean, const double* dvar, const double* H, int p, int ms, const double* dmu, const double* dv,
                           int ns, double* grad_xs, hipStream_t st) {
  hipLaunchKernelGGL(ss_contract_dx_kernel, dim3((ns + 255) / 256), dim3(256), 0, st, dmean, dvar, H, p, ms, dmu, dv, ns, grad_xs);
}

void launch_ss_grad_x(const double* g, const double* w, int n, int ms, double* grad_x, hipStream_t st) {
  hipLaunchKernelGGL(ss_grad_x_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g, w, n, ms, grad_x);
}

void launch_ss_pathwise(const double* r, const double* w, const double* f, const double* xi, size_t xi_stride, int n, int ms, int N,
                        double* rp, hipStream_t st) {
  hipLaunchKernelGGL(ss_pathwise_kernel, dim3((n + 255) / 256, N, ms), dim3(256), 0, st, r, w, f, xi, xi_stride, n, rp);
}

void launch_ss_addpath(double* f, const double* sm, int n, int ms, int N, hipStream_t st) {
  hipLaunchKernelGGL(ss_addpath_kernel, dim3((n + 255) / 256, N, ms), dim3(256), 0, st, f, sm, n);
}

void launch_ss_sorted(const double* x, int n, int* flag, hipStream_t st) {
  const int blocks = (int)std::min<long long>(2048, ((long long)n + 255) / 256);
  hipLaunchKernelGGL(ss_sorted_kernel, dim3(blocks), dim3(256), 0, st, x, n, flag);
}

void launch_ss_finite(const double* xs, int ns, int* flag, hipStream_t st) {
  const int blocks = (int)std::min<long long>(2048, ((long long)ns + 255) / 256);
  hipLaunchKernelGGL(ss_finite_kernel, dim3(blocks), dim3(256), 0, st, xs, ns, flag);
}

void launch_ss_window_bounds(const double* x, int n, const double* xs, int ns, double lo, double hi, int* out, hipStream_t st) {
  hipLaunchKernelGGL(ss_window_bounds_kernel, dim3(1), dim3(64), 0, st, x, n, xs, ns, lo, hi, out);
}

void launch_ss_window(const double* x, int n, const double* xs, int ns, int first, int count, int* src, hipStream_t st) {
  const long long W = (long long)ns + count;
  hipLaunchKernelGGL(ss_window_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, x, n, xs, ns, first, count, src);
}

void launch_ss_gather_rows(const double* in, int n, int p, const int* idx, int nsel, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ss_gather_rows_kernel, dim3((nsel + 255) / 256, p), dim3(256), 0, st, in, n, idx, nsel, out);
}

void launch_ss_scatter_rows(const double* in, int n, int p, const int* idx, int nsel, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ss_scatter_rows_kernel, dim3((nsel + 255) / 256, p), dim3(256), 0, st, in, n, idx, nsel, out);
}
