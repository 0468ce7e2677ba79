// lmm_kernels_ss.hip -- linear-time state-space inference for Matern12 / 32 / 52 and SHO latents over a one-dimensional input:
// the Kalman filter and the Rauch-Tung-Striebel smoother as parallel scans over the n points.  Float64 only; built WITHOUT
// -amdgpu-mfma-vgpr-form=1 (no MFMA here).  Three phases per direction, no atomics, results depend only on (arguments, chunk):
//   1. ss_fold_kernel / ss_bfold_kernel: each thread folds the scan elements of its `chunk` consecutive points into one aggregate;
//   2. ss_scan_kernel (+ ss_addprefix_kernel): the aggregates are scanned, 128 per workgroup through LDS (Hillis-Steele); with more
//      aggregates than one workgroup takes, the workgroups' totals are scanned by the same kernel (recursion on the host) and applied;
//   3. ss_filter_kernel / ss_rts_kernel: each thread restarts the ordinary recursion from its prefix (suffix) state over its run and
//      writes the marginals; the filter's log-density partials are added in thread order by ss_finish_kernel.
// A(dt) and Q(dt) are evaluated on the fly from x_t - x_{t-1}; blockIdx.z is the latent.  Every latent of a launch has the same MODEL
// (the template arguments D and OSC: Matern12 / 32 / 52, or the damped oscillator of an SHO latent, which shares D = 2 with Matern32
// but not its A(dt)); the scans see elements only and are shared between models of equal D.
// Gradients (launch_ss_grad): d lml / d variance and d lml / d lengthscale (and an SHO latent's d lml / d quality) are the forward-mode
// derivative of phases 1 - 3 of the filter, the same text instantiated with SSDual (lmm_statespace.h): ss_fold_kernel<D, OSC, SSDual>,
// the scan over SSFwd<D, SSDual> and ss_filter_kernel<D, OSC, SSDual>, with blockIdx.y the seeded parameter (2 per Matern latent, 3 per
// SHO latent), so a thread carries one tangent.  d lml / d r_t and d lml / d w_t come from the smoothed
// marginals (ss_point_kernel), with fixed-order sums of what the OILMM chain rule needs.
// Sampling (launch_ss_path): the prior path is an affine recursion in the caller's normals, so phases 1 - 3 run on SSAff<D> elements
// (ss_sfold_kernel, the scan with AffOp, ss_path_kernel); a posterior path is the prior path plus the smoothed mean of the residual
// data r - f - sqrt(w) xi (ss_pathwise_kernel, then the filter and smoother above, then ss_addpath_kernel).
// The posterior object (launch_ss_interp): ss_rts_kernel<D, OSC, SS_RTS_FULL> keeps the full smoothed and the filtered states point-major, and
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
// transition (ss_input_grad); ss_rts_kernel<D, OSC, SS_RTS_GX> writes g while it steps through the points, ss_grad_x_kernel adds the
// latents in order.  For the posterior object ss_interp_dx_kernel writes d mean / d s and d var / d s per (query, latent) and
// ss_contract_dx_kernel contracts them with H and the cotangents, one thread per query, latents in order.  No atomics, no LDS.
// Appending observations (launch_ss_filter_from, launch_ss_smooth_kept) adds no kernel: ss_fold_kernel / ss_filter_kernel on SSFromArgs
// start from a stored state instead of the prior, and ss_bfold_kernel<.., true> / ss_rts_kernel<.., SS_RTS_KEPT> smooth over kept states.
// Shared by the kernels (lmm_statespace.h): ss_chunk_range (a thread's run), ss_count_le / ss_count_lt (the binary searches) and
// ss_load_state / ss_store_state (a stored state in either layout); ss_lat_model makes the model of any *Lat struct.  On the host, ss_dispatch hands a
// launch's model to a generic lambda as compile-time (D, OSC), and ss_phases is the fold - scan - restart sequence of every direction
// (ss_scored_phases: with the log-density finish, and the single launch when there is one chunk).
#include "lmm_internal.h"
#include "lmm_statespace.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int SS_THREADS = 256;      // fold / filter / rts: one thread per chunk
constexpr int SS_SCAN = 128;         // aggregates per workgroup of the scan (one per thread; 128 SSFwd<3> are 33 KiB of LDS)
// 128 SSFwd<3, SSDual> would be 66 KiB, above the 64 KiB of static LDS: elements that large are scanned 64 per workgroup
template <typename T> constexpr int ss_scan_width() { return sizeof(T) * SS_SCAN <= 65536 ? SS_SCAN : SS_SCAN / 2; }

// The model of a launch: OSC = false, the Matern model of state dimension D; OSC = true (D = 2), the oscillator
template <int D, bool OSC, typename Sc = double> struct SSModelOf { typedef SSModel<D, Sc> type; };
template <typename Sc> struct SSModelOf<2, true, Sc> { typedef SSOsc<Sc> type; };
// seeded parameters of the forward-mode gradient: variance and lengthscale, and an oscillator's quality
template <bool OSC> constexpr int ss_seeds() { return OSC ? 3 : 2; }

template <int D, bool OSC, typename Sc>
__device__ __forceinline__ typename SSModelOf<D, OSC, Sc>::type ss_make_model(Sc var, Sc inv_ls, Sc quality) {
  typename SSModelOf<D, OSC, Sc>::type M;
  if constexpr (OSC) ss_osc_model<Sc>(var, inv_ls, quality, M);
  else ss_model<D, Sc>(var, inv_ls, M);
  return M;
}

// The model of a latent's (var, inv_ls, quality), of any of the *Lat structs.  Sc = SSDual: with the tangent of parameter `seed` set: 0 =
// variance, 1 = lengthscale (d (1 / l) = -1 / l^2; an oscillator's period), 2 = an oscillator's quality
template <int D, bool OSC, typename Sc = double, typename Lat>
__device__ __forceinline__ typename SSModelOf<D, OSC, Sc>::type ss_lat_model(const Lat& L, int seed = 0) {
  if constexpr (std::is_same<Sc, SSDual>::value)
    return ss_make_model<D, OSC, SSDual>(SSDual(L.var, seed == 0 ? 1.0 : 0.0), SSDual(L.inv_ls, seed == 1 ? -L.inv_ls * L.inv_ls : 0.0),
                                         SSDual(L.quality, seed == 2 ? 1.0 : 0.0));
  else return ss_make_model<D, OSC, double>(L.var, L.inv_ls, L.quality);
}

// Fold and filter in both scalar types.  Sc = double: the value; the aggregates of latent z = blockIdx.z are item z of a.agg.
// Sc = SSDual: (value, tangent) with blockIdx.y the seeded parameter (NS = ss_seeds<OSC>() of them), so a thread carries one tangent;
// the aggregates of (latent z, seed s) are item NS z + s of a.dagg.
// And from both starts (Args).  SSArgs: the prior in front of point 0.  SSFromArgs (Sc = double; DESIGN.md 4.18 "Appending
// observations"): a stored state, L.init at input a.x0 -- the element of point 0 is ss_fwd_element_from, thread 0 restarts from L.init
// over x[0] - x0, and the filtered states go point-major to L.out (rows n .. n + k - 1 of the posterior object's block); every other
// element and the scan are the same.
template <int D, bool OSC, typename Sc, typename Args>
__device__ __forceinline__ SSFwd<D, Sc>& ss_fwd_agg(const Args& a, int z, int s, size_t j) {       // aggregate j of (latent z, seed s)
  if constexpr (std::is_same<Sc, SSDual>::value) return reinterpret_cast<SSFwd<D, Sc>*>(a.dagg)[(size_t)(ss_seeds<OSC>() * z + s) * a.nch + j];
  else return reinterpret_cast<SSFwd<D, Sc>*>(a.agg)[(size_t)z * a.nch + j];
}

template <int D, bool OSC, typename Sc, typename Args = SSArgs>
__global__ __launch_bounds__(SS_THREADS) void ss_fold_kernel(Args a) {
  constexpr bool DUAL = std::is_same<Sc, SSDual>::value, FROM = std::is_same<Args, SSFromArgs>::value;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z, s = DUAL ? blockIdx.y : 0;
  if (j >= a.nch) return;
  const auto& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC, Sc>(L, s);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  SSFwd<D, Sc> acc, el;
  double xp = a.x[t0];
  if constexpr (FROM) {
    if (t0 == 0) {
      double m0[D], P0[D][D];
      ss_load_state<D>(L.init, 1, 0, 0, m0, P0);
      ss_fwd_element_from<D>(M, xp - a.x0, m0, P0, L.w[0], L.r[0], acc);
    } else ss_fwd_element<D>(M, false, xp - a.x[t0 - 1], L.w[t0], L.r[t0], acc);
  } else ss_fwd_element<D, Sc>(M, t0 == 0, t0 == 0 ? 0.0 : xp - a.x[t0 - 1], L.w[t0], L.r[t0], acc);
  for (long long t = t0 + 1; t < t1; ++t) {
    const double xt = a.x[t];
    ss_fwd_element<D, Sc>(M, false, xt - xp, L.w[t], L.r[t], el);
    ss_fwd_combine<D, Sc>(acc, el, acc);
    xp = xt;
  }
  ss_fwd_agg<D, OSC, Sc>(a, z, s, j) = acc;
}

struct FwdOp {
  template <int D, typename Sc>
  static __device__ __forceinline__ void combine(const SSFwd<D, Sc>& a, const SSFwd<D, Sc>& b, SSFwd<D, Sc>& o) { ss_fwd_combine<D, Sc>(a, b, o); }
};
struct BwdOp {
  template <int D> static __device__ __forceinline__ void combine(const SSBwd<D>& a, const SSBwd<D>& b, SSBwd<D>& o) { ss_bwd_combine<D>(a, b, o); }
};

// Inclusive scan of N items per latent, SS_SCAN per workgroup.  REV: a suffix scan -- logical position q is item N - 1 - q, and the
// earlier-in-time operand of the combine is the item itself.  totals (nullptr: none): the workgroups' totals, stored like the items
// (logical workgroup k at nblk - 1 - k when REV), so the same kernel scans them.
template <int D, typename T, typename Op, bool REV>
__global__ __launch_bounds__(SS_SCAN) void ss_scan_kernel(T* items, int N, T* totals) {
  constexpr int W = ss_scan_width<T>();
  __shared__ T sh[W];
  const int tid = threadIdx.x, q = blockIdx.x * W + tid, z = blockIdx.z;
  const int nblk = gridDim.x;
  const bool live = q < N;
  const size_t i = (size_t)z * N + (REV ? N - 1 - q : q);
  T mine;
  if (live) { mine = items[i]; sh[tid] = mine; }
  __syncthreads();
  for (int off = 1; off < W; off <<= 1) {
    const bool take = live && tid >= off;
    T other;
    if (take) other = sh[tid - off];
    __syncthreads();
    if (take) {
      if (REV) Op::template combine<D>(mine, other, mine);
      else Op::template combine<D>(other, mine, mine);
      sh[tid] = mine;
    }
    __syncthreads();
  }
  if (live) {
    items[i] = mine;
    const int last = (N - blockIdx.x * W < W ? N - blockIdx.x * W : W) - 1;
    if (totals != nullptr && tid == last) totals[(size_t)z * nblk + (REV ? nblk - 1 - (int)blockIdx.x : (int)blockIdx.x)] = mine;
  }
}

// items of logical workgroup k >= 1 take the scanned total of workgroup k - 1 in front
template <int D, typename T, typename Op, bool REV>
__global__ __launch_bounds__(SS_SCAN) void ss_addprefix_kernel(T* items, int N, const T* totals) {
  constexpr int W = ss_scan_width<T>();
  const int blk = blockIdx.x + 1, q = blk * W + threadIdx.x, z = blockIdx.z;
  const int nblk = gridDim.x + 1;
  if (q >= N) return;
  const size_t i = (size_t)z * N + (REV ? N - 1 - q : q);
  const T pre = totals[(size_t)z * nblk + (REV ? nblk - 1 - (blk - 1) : blk - 1)];
  T mine = items[i];
  if (REV) Op::template combine<D>(mine, pre, mine);
  else Op::template combine<D>(pre, mine, mine);
  items[i] = mine;
}

template <int D, typename T, typename Op, bool REV>
void scan_levels(T* items, int N, int nb, T* scratch, hipStream_t st) {
  constexpr int W = ss_scan_width<T>();
  const int nblk = (N + W - 1) / W;
  if (nblk == 1) {
    hipLaunchKernelGGL((ss_scan_kernel<D, T, Op, REV>), dim3(1, 1, nb), dim3(W), 0, st, items, N, (T*)nullptr);
    return;
  }
  hipLaunchKernelGGL((ss_scan_kernel<D, T, Op, REV>), dim3(nblk, 1, nb), dim3(W), 0, st, items, N, scratch);
  scan_levels<D, T, Op, REV>(scratch, nblk, nb, scratch + (size_t)nb * nblk, st);
  hipLaunchKernelGGL((ss_addprefix_kernel<D, T, Op, REV>), dim3(nblk - 1, 1, nb), dim3(W), 0, st, items, N, (const T*)scratch);
}

// Sc = double writes the marginals, the states and its log-density partial; Sc = SSDual only the tangent of its partial.  With one
// chunk this kernel alone is the filter (ss_scored_phases).
template <int D, bool OSC, typename Sc, typename Args = SSArgs>
__global__ __launch_bounds__(SS_THREADS) void ss_filter_kernel(Args a) {
  constexpr bool DUAL = std::is_same<Sc, SSDual>::value, FROM = std::is_same<Args, SSFromArgs>::value;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z, s = DUAL ? blockIdx.y : 0;
  if (j >= a.nch) return;
  const auto& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC, Sc>(L, s);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  Sc m[D], P[D][D];
  if (j == 0) {
    if constexpr (FROM) ss_load_state<D>(L.init, 1, 0, 0, m, P);
    else {
      for (int i = 0; i < D; ++i) {
        m[i] = 0.0;
        for (int k = 0; k < D; ++k) P[i][k] = M.Pinf[i][k];
      }
    }
  } else {       // (b, C) of the prefix, written out: through a loader the SSFromArgs instantiation of Matern32 takes 110 VGPRs, not 96
    const SSFwd<D, Sc>& pre = ss_fwd_agg<D, OSC, Sc>(a, z, s, (size_t)j - 1);
    for (int i = 0; i < D; ++i) {
      m[i] = pre.b[i];
      for (int k = 0; k < D; ++k) P[i][k] = pre.C[i][k];
    }
  }
  double* fm = a.fmean ? a.fmean + (size_t)z * a.n : nullptr;
  double* fv = a.fvar ? a.fvar + (size_t)z * a.n : nullptr;
  double* stt = nullptr;
  if constexpr (!FROM) stt = a.state ? a.state + (size_t)z * a.state_stride : nullptr;
  Sc lp = 0.0;
  double xp;
  if constexpr (FROM) xp = t0 == 0 ? a.x0 : a.x[t0 - 1];
  else xp = t0 == 0 ? a.x[0] : a.x[t0 - 1];
  for (long long t = t0; t < t1; ++t) {
    const double xt = a.x[t];
    lp += ss_filter_step<D, Sc>(M, xt - xp, L.w[t], L.r[t], m, P);
    xp = xt;
    if constexpr (!DUAL) {
      if (fm) fm[t] = m[0];
      if (fv) fv[t] = P[0][0];
      if constexpr (FROM) ss_store_state<D>(L.out, 1, D + D * (D + 1) / 2, t, m, P);       // point-major
      else if (stt) {                                                                      // component-major
        for (int i = 0; i < D; ++i) {
          stt[(size_t)i * a.n + t] = m[i];
          for (int k = i; k < D; ++k) stt[(size_t)ss_sym_at(D, i, k) * a.n + t] = P[i][k];
        }
      }
    }
  }
  if constexpr (DUAL) a.dpart[(size_t)(ss_seeds<OSC>() * z + s) * a.nch + j] = lp.t;
  else a.part[(size_t)z * a.nch + j] = lp;
}

// lml[z] = the nch partials of latent z: each thread adds a contiguous strip in order, thread 0 adds the strips in thread order
__global__ __launch_bounds__(SS_THREADS) void ss_finish_kernel(const double* __restrict__ part, int nch, double* __restrict__ lml) {
  __shared__ double sh[SS_THREADS];
  const int z = blockIdx.x, per = (nch + SS_THREADS - 1) / SS_THREADS;
  const int k0 = threadIdx.x * per, k1 = k0 + per < nch ? k0 + per : nch;
  double s = 0.0;
  for (int k = k0; k < k1; ++k) s += part[(size_t)z * nch + k];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < SS_THREADS; ++k) tot += sh[k];
    lml[z] = tot;
  }
}

// ---- gradients: the pointwise part (the forward-mode part is ss_fold_kernel / ss_filter_kernel with Sc = SSDual) -----------------------
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

// The backward recursion reads the filtered states from a.state, component-major, as the filter of the same call left them; KEPT: from
// a.fkeep, point-major -- the posterior object's buffer, whose blocks a.state_stride strides as well.
template <int D, bool OSC, bool KEPT = false>
__global__ __launch_bounds__(SS_THREADS) void ss_bfold_kernel(SSArgs a) {
  constexpr int NC = D + D * (D + 1) / 2;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const auto M = ss_lat_model<D, OSC>(a.lat[z]);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  const double* fst = (KEPT ? a.fkeep : a.state) + (size_t)z * a.state_stride;
  SSBwd<D> acc, el;
  double m[D], P[D][D];
  for (long long t = t0; t < t1; ++t) {
    const bool last = t == a.n - 1;
    ss_load_state<D>(fst, KEPT ? 1 : a.n, KEPT ? NC : 1, t, m, P);
    ss_bwd_element<D>(M, last, last ? 0.0 : a.x[t + 1] - a.x[t], m, P, t == t0 ? acc : el);
    if (t > t0) ss_bwd_combine<D>(acc, el, acc);
  }
  reinterpret_cast<SSBwd<D>*>(a.bagg)[(size_t)z * a.nch + j] = acc;
}

// What the RTS replay writes.  MARGINALS: a.smean (+ the latent's mean) and a.svar.  FULL: the whole smoothed state (without the
// latent's mean) goes to a.sstate as well, and the filtered state it was computed from to a.fkeep, both point-major (a point's
// components side by side, which is how ss_interp_kernel reads them); a.smean may be nullptr.  GX: when the recursion steps from point
// t + 1 to point t it holds the filtered state of t and the smoothed state of t + 1, which is all ss_input_grad takes: a.gdt[t + 1] =
// d lml / d (x_{t+1} - x_t), and a.gdt[0] = 0; no state is stored for it, and every entry of a.gdt is written by exactly one thread.
// KEPT (with ss_bfold_kernel<.., true>; DESIGN.md 4.18 "Appending observations"): the smoother over kept states -- the filtered states
// are read from a.fkeep and only a.sstate is written; neither the data nor a.state is read, and no marginal is written.
enum SSRts { SS_RTS_MARGINALS, SS_RTS_FULL, SS_RTS_GX, SS_RTS_KEPT };
template <int D, bool OSC, SSRts V = SS_RTS_MARGINALS>
__global__ __launch_bounds__(SS_THREADS) void ss_rts_kernel(SSArgs a) {
  constexpr bool FULL = V == SS_RTS_FULL, GX = V == SS_RTS_GX, KEPT = V == SS_RTS_KEPT;
  constexpr int NC = D + D * (D + 1) / 2;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  const double* fst = (KEPT ? a.fkeep : a.state) + (size_t)z * a.state_stride;
  double* sst = KEPT ? a.sstate + (size_t)z * a.state_stride : nullptr;
  double ms[D], Ps[D][D];
  for (int i = 0; i < D; ++i) {       // the last chunk has no successor: its first element has E = 0 and ignores this state.  (Written
    ms[i] = 0.0;                      // out, as the prefix is in ss_filter_kernel: a loader changes the code of all twelve instantiations.)
    for (int k = 0; k < D; ++k) Ps[i][k] = 0.0;
  }
  if (j + 1 < a.nch) {
    const SSBwd<D>& suf = reinterpret_cast<const SSBwd<D>*>(a.bagg)[(size_t)z * a.nch + j + 1];
    for (int i = 0; i < D; ++i) {
      ms[i] = suf.g[i];
      for (int k = 0; k < D; ++k) Ps[i][k] = suf.L[i][k];
    }
  }
  double* sm = (!KEPT && (!FULL || a.smean)) ? a.smean + (size_t)z * a.n : nullptr;
  double* sv = (!KEPT && a.svar) ? a.svar + (size_t)z * a.n : nullptr;
  SSBwd<D> el;
  double m[D], P[D][D];
  for (long long t = t1 - 1; t >= t0; --t) {
    const bool last = t == a.n - 1;
    ss_load_state<D>(fst, KEPT ? 1 : a.n, KEPT ? NC : 1, t, m, P);
    ss_bwd_element<D>(M, last, last ? 0.0 : a.x[t + 1] - a.x[t], m, P, el);
    if constexpr (GX) {
      double* gd = a.gdt + (size_t)z * a.n;
      if (!last) gd[t + 1] = ss_input_grad<D>(M, a.x[t + 1] - a.x[t], m, P, ms, Ps);
      if (t == 0) gd[0] = 0.0;
    }
    ss_rts_step<D>(el, ms, Ps);
    if constexpr (!KEPT) {
      if (!FULL || sm) sm[t] = ms[0] + L.mean;
      if (sv) sv[t] = Ps[0][0];
    }
    if constexpr (KEPT) ss_store_state<D>(sst, 1, NC, t, ms, Ps);
    if constexpr (FULL) {       // both states entry by entry: two ss_store_state calls issue the stores in another order (other code)
      double* so = a.sstate + (size_t)z * a.state_stride + (size_t)t * NC;
      double* fo = a.fkeep + (size_t)z * a.state_stride + (size_t)t * NC;
      for (int i = 0; i < D; ++i) {
        so[i] = ms[i]; fo[i] = m[i];
        for (int k = i; k < D; ++k) { so[ss_sym_at(D, i, k)] = Ps[i][k]; fo[ss_sym_at(D, i, k)] = P[i][k]; }
      }
    }
  }
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

// One thread per (query, latent): the posterior marginal of the latent at xs[q] from the stored filtered and smoothed states
// (ss_interp).  k = #{t : x_t <= s} by binary search over the sorted x (a query equal to a training input comes behind every copy of
// it): at most ceil(log2(n + 1)) probes.  Reads the states of points k - 1 >= 0 and k < n only; a query's result depends on no other
// query.  xs is finite (launch_ss_finite has looked).
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_interp_kernel(SSInterpArgs a) {
  const int q = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (q >= a.ns) return;
  const SSInterpLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
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
  ss_interp<D>(M, k > 0, d1, k < a.n, d2, m, P, ms, Ps);
  a.mean[(size_t)z * a.ns + q] = m[0] + L.mean;
  if (a.var) a.var[(size_t)z * a.ns + q] = P[0][0];
}

// ss_interp_kernel's threads, writing the derivatives of its two outputs with respect to the query instead (ss_interp_dx_state; Matern12:
// ss_interp_dx_ou on ss_interp's inputs).  At a query equal to a training input they are those of the side the search sorts it to
// (behind every copy), which matters for Matern12 alone: its posterior mean has a kink there.
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_interp_dx_kernel(SSInterpArgs a) {
  const int q = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (q >= a.ns) return;
  const SSInterpLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
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

// ---- sampling ------------------------------------------------------------------------------------------------------------------
// The prior path s_t = A(dt_t) s_{t-1} + chol(Q(dt_t)) zeta_t, s_0 = chol(Pinf) zeta_0, is an affine recursion, so the same three
// phases serve it with SSAff<D> elements (D^2 + D doubles): ss_sfold_kernel, the scan with AffOp, ss_path_kernel.  blockIdx.z runs over
// the (latent, sample) pairs of a launch; zeta is read straight from the caller's buffer, component i of point t at z[i n + t].
template <int D>
__device__ __forceinline__ void ss_load_zeta(const double* __restrict__ z, int n, long long t, double zeta[D]) {
  for (int i = 0; i < D; ++i) zeta[i] = z[(size_t)i * n + t];
}

template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_sfold_kernel(SSPathArgs a) {
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSPathLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  SSAff<D> acc, el;
  double zeta[D];
  double xp = a.x[t0];
  ss_load_zeta<D>(L.z, a.n, t0, zeta);
  ss_aff_element<D>(M, t0 == 0, t0 == 0 ? 0.0 : xp - a.x[t0 - 1], zeta, acc);
  for (long long t = t0 + 1; t < t1; ++t) {
    const double xt = a.x[t];
    ss_load_zeta<D>(L.z, a.n, t, zeta);
    ss_aff_element<D>(M, false, xt - xp, zeta, el);
    ss_aff_combine<D>(acc, el, acc);
    xp = xt;
  }
  reinterpret_cast<SSAff<D>*>(a.agg)[(size_t)z * a.nch + j] = acc;
}

struct AffOp {
  template <int D> static __device__ __forceinline__ void combine(const SSAff<D>& a, const SSAff<D>& b, SSAff<D>& o) { ss_aff_combine<D>(a, b, o); }
};

// each thread restarts the recursion from its prefix state (the c of the scanned aggregate before its run) and writes f_t = (s_t)_1 (+ lat.mean)
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_path_kernel(SSPathArgs a) {
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSPathLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const auto [t0, t1] = ss_chunk_range(j, a.chunk, a.n);
  double s[D], zeta[D];
  for (int i = 0; i < D; ++i) s[i] = 0.0;           // the first element has A = 0 and ignores this state
  if (j > 0) {
    const SSAff<D>& pre = reinterpret_cast<const SSAff<D>*>(a.agg)[(size_t)z * a.nch + j - 1];
    for (int i = 0; i < D; ++i) s[i] = pre.c[i];
  }
  SSAff<D> el;
  double xp = t0 == 0 ? a.x[0] : a.x[t0 - 1];
  for (long long t = t0; t < t1; ++t) {
    const double xt = a.x[t];
    ss_load_zeta<D>(L.z, a.n, t, zeta);
    ss_aff_element<D>(M, t == 0, xt - xp, zeta, el);
    ss_aff_step<D>(el, s);
    xp = xt;
    L.f[t] = s[0] + L.mean;
  }
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

// ---- sampling from the posterior object --------------------------------------------------------------------------------------------
// Given the data, the states at the window's points (SSPostArgs: the sorted queries and the training points between the smallest and
// the largest of them) form a Markov chain that runs BACKWARDS: s_j = E_j s_{j+1} + g_j + U(L_j) zeta_j from the posterior state at the
// last point (ss_post_element).  That is an affine recursion again, so the three phases of the prior path serve it from the right:
// ss_pfold_kernel, the suffix scan with AffRevOp, ss_ppath_kernel.  Nothing outside the window is read but the states next to its ends.

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

__device__ __forceinline__ double ss_window_input(const SSWindowArgs& a, long long j) {
  const int s = a.src[j];
  return s >= 0 ? a.x[s] : a.xs[-1 - s];
}

// The element of window point j (input xj, its successor's input xn; xn is not read at the last point).  The filtered state of a
// training point is the stored one; that of a query is the stored one of training point k - 1, k = #{t : x_t <= q} = first + (j - its
// index among the queries), predicted over q - x_{k-1} (the filter's step at an unobserved point), and (0, Pinf) when k = 0.
// Reads fstate of points first - 1 .. first + count - 1 (>= 0) and sstate of point first + count (< n) only.
// ss_lwindow_element below repeats the filtered state of a window point, and the four window kernels their walk over a run, on
// purpose.  One window-point helper (a struct it fills, arrays it fills, or the shared text outside and the element in a lambda) costs
// every window kernel 2 - 8 SGPRs (ss_ppath_kernel<3>: 51 -> 58, ss_lfilter_kernel<1>: 66 -> 74), and one walk taking the body as a
// lambda costs ss_pfold_kernel 2 - 4 VGPRs besides (Matern52: 208 -> 212).
template <int D, typename Mod>
__device__ __forceinline__ void ss_window_element(const SSPostArgs& a, const SSPostLat& L, const Mod& M, long long j, double xj, double xn,
                                                  SSAff<D>& e) {
  constexpr int NC = D + D * (D + 1) / 2;       // the stored states are point-major
  const int s = a.src[j];
  double m[D], P[D][D], ms[D], Ps[D][D], zeta[D];
  int k;
  if (s >= 0) {
    ss_load_state<D>(L.fstate, 1, NC, s, m, P);
    k = s + 1;
  } else {
    k = a.first + (int)(j - (-1 - s));
    if (k > 0) {
      ss_load_state<D>(L.fstate, 1, NC, k - 1, m, P);
      ss_filter_step<D>(M, xj - a.x[k - 1], INFINITY, 0.0, m, P);
    } else {
      for (int i = 0; i < D; ++i) {
        m[i] = 0.0;
        for (int c = 0; c < D; ++c) P[i][c] = M.Pinf[i][c];
      }
    }
  }
  const bool last = j == a.W - 1, has_next = k < a.n;
  double dt = xn - xj;
  for (int i = 0; i < D; ++i) {
    ms[i] = 0.0;
    for (int c = 0; c < D; ++c) Ps[i][c] = 0.0;
  }
  if (last) {
    dt = 0.0;
    if (has_next) {
      ss_load_state<D>(L.sstate, 1, NC, k, ms, Ps);
      dt = a.x[k] - xj;
    }
  }
  for (int i = 0; i < D; ++i) zeta[i] = L.z[(size_t)i * a.W + j];
  ss_post_element<D>(M, last, has_next, dt, m, P, ms, Ps, zeta, e);
}

// the scan's REV hands over (item, what lies to its right): the right operand is applied first
struct AffRevOp {
  template <int D> static __device__ __forceinline__ void combine(const SSAff<D>& a, const SSAff<D>& b, SSAff<D>& o) { ss_aff_combine<D>(b, a, o); }
};

// one thread per run of `chunk` window points, folded from the right: the aggregate maps the state behind the run to the run's first
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_pfold_kernel(SSPostArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSPostLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  // ss_chunk_range's text, written out here and in ss_ppath_kernel: `j1 < a.W` below shares its comparison only when the compiler sees
  // both in the kernel before it inlines, and through the helper these two kernels come out with other code (SHO: 4 more VGPRs)
  const long long j0 = (long long)c * a.chunk;
  const long long j1 = j0 + a.chunk < a.W ? j0 + a.chunk : a.W;
  SSAff<D> acc, el;
  double xn = j1 < a.W ? ss_window_input(a, j1) : 0.0;
  for (long long j = j1 - 1; j >= j0; --j) {
    const double xj = ss_window_input(a, j);
    ss_window_element<D>(a, L, M, j, xj, xn, j == j1 - 1 ? acc : el);
    if (j < j1 - 1) ss_aff_combine<D>(acc, el, acc);
    xn = xj;
  }
  reinterpret_cast<SSAff<D>*>(a.agg)[(size_t)z * a.nch + c] = acc;
}

// each thread restarts the recursion from the state behind its run (the c of the scanned aggregate of the run to its right) and writes
// the query rows f[i] = (s_j)_1 + lat.mean
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_ppath_kernel(SSPostArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSPostLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const long long j0 = (long long)c * a.chunk;           // as in ss_pfold_kernel
  const long long j1 = j0 + a.chunk < a.W ? j0 + a.chunk : a.W;
  double s[D];
  for (int i = 0; i < D; ++i) s[i] = 0.0;           // the last element has A = 0 and ignores this state
  if (c + 1 < a.nch) {
    const SSAff<D>& suf = reinterpret_cast<const SSAff<D>*>(a.agg)[(size_t)z * a.nch + c + 1];
    for (int i = 0; i < D; ++i) s[i] = suf.c[i];
  }
  SSAff<D> el;
  double xn = j1 < a.W ? ss_window_input(a, j1) : 0.0;
  for (long long j = j1 - 1; j >= j0; --j) {
    const double xj = ss_window_input(a, j);
    ss_window_element<D>(a, L, M, j, xj, xn, el);
    ss_aff_step<D>(el, s);
    xn = xj;
    const int q = a.src[j];
    if (q < 0) L.f[-1 - q] = s[0] + L.mean;
  }
}

// ---- predictive log density from the posterior object ------------------------------------------------------------------------------
// Observing data at the queries of the window's backward chain is a Kalman filter that runs from the window's last point down to its
// first, with the affine transitions (E_j, g_j, L_j) (ss_fwd_element_affine, ss_chain_step).  The three phases of the filter serve it
// from the right: ss_lfold_kernel, the suffix scan of SSFwd<D> with FwdRevOp, ss_lfilter_kernel, and ss_finish_kernel adds the
// partials.  A training point of the window is an unobserved step; a query carries (w, r) of the front end, indexed through src.

// The backward element of window point j (input xj, its successor's input xn; xn is not read at the last point) and the point's noise
// and data.  The filtered state is taken as ss_window_element takes it; the last point's element is ss_chain_start.  Reads fstate of
// points first - 1 .. first + count - 1 (>= 0) and sstate of point first + count (< n) only, and w, r of the queries.
template <int D, typename Mod>
__device__ __forceinline__ void ss_lwindow_element(const SSLpdfArgs& a, const SSLpdfLat& L, const Mod& M, long long j, double xj, double xn,
                                                   SSBwd<D>& el, double& w, double& r) {
  constexpr int NC = D + D * (D + 1) / 2;       // the stored states are point-major
  const int s = a.src[j];
  double m[D], P[D][D];
  int k;
  if (s >= 0) {
    ss_load_state<D>(L.fstate, 1, NC, s, m, P);
    k = s + 1;
    w = INFINITY; r = 0.0;
  } else {
    k = a.first + (int)(j - (-1 - s));
    if (k > 0) {
      ss_load_state<D>(L.fstate, 1, NC, k - 1, m, P);
      ss_filter_step<D>(M, xj - a.x[k - 1], INFINITY, 0.0, m, P);
    } else {
      for (int i = 0; i < D; ++i) {
        m[i] = 0.0;
        for (int c = 0; c < D; ++c) P[i][c] = M.Pinf[i][c];
      }
    }
    w = L.w[-1 - s]; r = L.r[-1 - s];
  }
  if (j < a.W - 1) {
    ss_bwd_element<D>(M, false, xn - xj, m, P, el);
    return;
  }
  const bool has_next = k < a.n;
  double ms[D], Ps[D][D], dt = 0.0;
  for (int i = 0; i < D; ++i) {
    ms[i] = 0.0;
    for (int c = 0; c < D; ++c) Ps[i][c] = 0.0;
  }
  if (has_next) {
    ss_load_state<D>(L.sstate, 1, NC, k, ms, Ps);
    dt = a.x[k] - xj;
  }
  ss_chain_start<D>(M, has_next, dt, m, P, ms, Ps, el);
}

// the scan's REV hands over (item, what lies to its right); the run to the right is the earlier one in filter order
struct FwdRevOp {
  template <int D> static __device__ __forceinline__ void combine(const SSFwd<D>& a, const SSFwd<D>& b, SSFwd<D>& o) { ss_fwd_combine<D>(b, a, o); }
};

// one thread per run of `chunk` window points, folded from the right: the aggregate takes the filtered state behind the run to the one
// at the run's first point
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_lfold_kernel(SSLpdfArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSLpdfLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const long long j0 = (long long)c * a.chunk;
  const long long j1 = j0 + a.chunk < a.W ? j0 + a.chunk : a.W;
  SSFwd<D> acc, fe;
  SSBwd<D> el;
  double xn = j1 < a.W ? ss_window_input(a, j1) : 0.0;
  for (long long j = j1 - 1; j >= j0; --j) {
    const double xj = ss_window_input(a, j);
    double w, r;
    ss_lwindow_element<D>(a, L, M, j, xj, xn, el, w, r);
    ss_fwd_element_affine<D>(el.E, el.g, el.L, w, r, j == j1 - 1 ? acc : fe);
    if (j < j1 - 1) ss_fwd_combine<D>(acc, fe, acc);
    xn = xj;
  }
  reinterpret_cast<SSFwd<D>*>(a.agg)[(size_t)z * a.nch + c] = acc;
}

// each thread restarts the sequential filter from the state behind its run ((b, C) of the scanned aggregate of the run to its right;
// the last run starts the chain and reads none) and writes its log-density partial.  With one chunk this kernel alone is the filter.
template <int D, bool OSC>
__global__ __launch_bounds__(SS_THREADS) void ss_lfilter_kernel(SSLpdfArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSLpdfLat& L = a.lat[z];
  const auto M = ss_lat_model<D, OSC>(L);
  const long long j0 = (long long)c * a.chunk;
  const long long j1 = j0 + a.chunk < a.W ? j0 + a.chunk : a.W;
  double m[D], P[D][D];
  for (int i = 0; i < D; ++i) {                     // the start element has E = 0 and ignores this state
    m[i] = 0.0;
    for (int k = 0; k < D; ++k) P[i][k] = 0.0;
  }
  if (c + 1 < a.nch) {
    const SSFwd<D>& suf = reinterpret_cast<const SSFwd<D>*>(a.agg)[(size_t)z * a.nch + c + 1];
    for (int i = 0; i < D; ++i) {
      m[i] = suf.b[i];
      for (int k = 0; k < D; ++k) P[i][k] = suf.C[i][k];
    }
  }
  SSBwd<D> el;
  double lp = 0.0;
  double xn = j1 < a.W ? ss_window_input(a, j1) : 0.0;
  for (long long j = j1 - 1; j >= j0; --j) {
    const double xj = ss_window_input(a, j);
    double w, r;
    ss_lwindow_element<D>(a, L, M, j, xj, xn, el, w, r);
    lp += ss_chain_step<D>(el, w, r, m, P);
    xn = xj;
  }
  a.part[(size_t)z * a.nch + c] = lp;
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

// f(SSModelTag<D, OSC>()) for the model of a launch, so that D and OSC reach the generic lambda f as compile-time constants.  A state
// dimension 1 / 2 / 3 is the number of its Matern model, which is how the element sizes below dispatch on D.
static_assert(SS_MODEL_SHO > 3, "ss_dispatch takes a state dimension 1 / 2 / 3 for its Matern model: none may be the oscillator's number");
template <int D_, bool OSC_> struct SSModelTag { static constexpr int D = D_; static constexpr bool OSC = OSC_; };
template <typename F>
auto ss_dispatch(int model, F&& f) {
  if (model == SS_MODEL_SHO) return f(SSModelTag<2, true>());
  if (model == 1) return f(SSModelTag<1, false>());
  if (model == 2) return f(SSModelTag<2, false>());
  return f(SSModelTag<3, false>());
}

// Phases 1 - 3 with nch threads per item and ny * nb items (grid (., ny, nb)): fold, the scan of the items' aggregates E at agg, restart
template <int D, typename E, typename Op, bool REV, typename Args>
void ss_phases(void (*fold)(Args), void (*restart)(Args), const Args& a, int ny, int nb, double* agg, hipStream_t st) {
  const dim3 grid((a.nch + SS_THREADS - 1) / SS_THREADS, ny, nb);
  hipLaunchKernelGGL(fold, grid, dim3(SS_THREADS), 0, st, a);
  E* e = reinterpret_cast<E*>(agg);
  scan_levels<D, E, Op, REV>(e, a.nch, ny * nb, e + (size_t)ny * nb * a.nch, st);
  hipLaunchKernelGGL(restart, grid, dim3(SS_THREADS), 0, st, a);
}

// Filter-shaped phases over SSFwd<D> with a log-density finish: lml[l] (device, nullptr: none) = the sum of latent l's partials.  One
// chunk: thread 0 of the restart is the whole sequential filter, no aggregate is read, and a latent's one partial is its log density:
// one launch in all.  (launch_ss_filter does not come here: its launch sequence is fold, scan, filter, finish whatever nch is.)
template <int D, typename Op, bool REV, typename Args>
void ss_scored_phases(void (*fold)(Args), void (*restart)(Args), const Args& a, int nb, double* lml, hipStream_t st) {
  if (a.nch == 1) {
    Args b = a;
    if (lml) b.part = lml;
    hipLaunchKernelGGL(restart, dim3(1, 1, nb), dim3(SS_THREADS), 0, st, b);
    return;
  }
  ss_phases<D, SSFwd<D>, Op, REV>(fold, restart, a, 1, nb, a.agg, st);
  if (lml) hipLaunchKernelGGL(ss_finish_kernel, dim3(nb), dim3(SS_THREADS), 0, st, (const double*)a.part, a.nch, lml);
}

}  // namespace

int ss_model_of(int kind) {
  return kind == LMM_KERNEL_MATERN12 ? 1 : kind == LMM_KERNEL_MATERN32 ? 2 : kind == LMM_KERNEL_MATERN52 ? 3 : kind == LMM_KERNEL_SHO ? SS_MODEL_SHO : 0;
}
int ss_model_dim(int model) { return model == SS_MODEL_SHO ? 2 : model; }
int ss_model_seeds(int model) { return model == SS_MODEL_SHO ? ss_seeds<true>() : ss_seeds<false>(); }
int ss_state_dim(int kind) { return ss_model_dim(ss_model_of(kind)); }
int ss_state_comps(int D) { return D + D * (D + 1) / 2; }
int ss_default_chunk(int n) { return n <= 4096 ? 16 : 64; }
size_t ss_fwd_agg_elems(int D, int nch) { return ss_dispatch(D, [&](auto t) { return agg_elems<SSFwd<decltype(t)::D>>(nch); }); }
size_t ss_bwd_agg_elems(int D, int nch) { return ss_dispatch(D, [&](auto t) { return agg_elems<SSBwd<decltype(t)::D>>(nch); }); }
size_t ss_aff_agg_elems(int D, int nch) { return ss_dispatch(D, [&](auto t) { return agg_elems<SSAff<decltype(t)::D>>(nch); }); }
size_t ss_dual_agg_elems(int D, int nch, int nseeds) {
  return nseeds * ss_dispatch(D, [&](auto t) { return agg_elems<SSFwd<decltype(t)::D, SSDual>>(nch); });
}
int ss_point_blocks(int n) { return (n + SS_THREADS * SS_POINT_PER - 1) / (SS_THREADS * SS_POINT_PER); }

void launch_ss_filter(const SSArgs& a, int model, int nb, double* lml, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSFwd<T::D>, FwdOp, false>(ss_fold_kernel<T::D, T::OSC, double>, ss_filter_kernel<T::D, T::OSC, double>, a, 1, nb, a.agg, st);
  });
  if (lml) hipLaunchKernelGGL(ss_finish_kernel, dim3(nb), dim3(SS_THREADS), 0, st, (const double*)a.part, a.nch, lml);
}

void launch_ss_smooth(const SSArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSBwd<T::D>, BwdOp, true>(ss_bfold_kernel<T::D, T::OSC>,
                                              a.sstate ? ss_rts_kernel<T::D, T::OSC, SS_RTS_FULL>
                                                       : a.gdt ? ss_rts_kernel<T::D, T::OSC, SS_RTS_GX> : ss_rts_kernel<T::D, T::OSC>,
                                              a, 1, nb, a.bagg, st);
  });
}

void launch_ss_filter_from(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_scored_phases<T::D, FwdOp, false>(ss_fold_kernel<T::D, T::OSC, double, SSFromArgs>, ss_filter_kernel<T::D, T::OSC, double, SSFromArgs>,
                                         a, nb, lml, st);
  });
}

void launch_ss_smooth_kept(const SSArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSBwd<T::D>, BwdOp, true>(ss_bfold_kernel<T::D, T::OSC, true>, ss_rts_kernel<T::D, T::OSC, SS_RTS_KEPT>, a, 1, nb, a.bagg, st);
  });
}

void launch_ss_any_below(const double* xs, int ns, double bound, int* flag, hipStream_t st) {
  hipLaunchKernelGGL(ss_any_below_kernel, dim3(1), dim3(SS_THREADS), 0, st, xs, ns, bound, flag);
}

void launch_ss_grad(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st) {
  const int NS = ss_model_seeds(model);
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSFwd<T::D, SSDual>, FwdOp, false>(ss_fold_kernel<T::D, T::OSC, SSDual>, ss_filter_kernel<T::D, T::OSC, SSDual>, a, NS, nb,
                                                       a.dagg, st);
  });
  hipLaunchKernelGGL(ss_finish_kernel, dim3(NS * nb), dim3(SS_THREADS), 0, st, (const double*)a.dpart, a.nch, gtheta);
}

void launch_ss_point(const SSArgs& a, int nb, double* alpha, double* grad_w, double* ppart, double* sums, hipStream_t st) {
  const int nblk = ss_point_blocks(a.n);
  hipLaunchKernelGGL(ss_point_kernel, dim3(nblk, 1, nb), dim3(SS_THREADS), 0, st, a, alpha, grad_w, ppart);
  hipLaunchKernelGGL(ss_finish_kernel, dim3(4 * nb), dim3(SS_THREADS), 0, st, (const double*)ppart, nblk, sums);
}

void launch_ss_path(const SSPathArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSAff<T::D>, AffOp, false>(ss_sfold_kernel<T::D, T::OSC>, ss_path_kernel<T::D, T::OSC>, a, 1, nb, a.agg, st);
  });
}

void launch_ss_post_path(const SSPostArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSAff<T::D>, AffRevOp, true>(ss_pfold_kernel<T::D, T::OSC>, ss_ppath_kernel<T::D, T::OSC>, a, 1, nb, a.agg, st);
  });
}

void launch_ss_post_logpdf(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_scored_phases<T::D, FwdRevOp, true>(ss_lfold_kernel<T::D, T::OSC>, ss_lfilter_kernel<T::D, T::OSC>, a, nb, lml, st);
  });
}

void launch_ss_interp(const SSInterpArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((ss_interp_kernel<T::D, T::OSC>), dim3((a.ns + SS_THREADS - 1) / SS_THREADS, 1, nb), dim3(SS_THREADS), 0, st, a);
  });
}

void launch_ss_interp_dx(const SSInterpArgs& a, int model, int nb, hipStream_t st) {
  ss_dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((ss_interp_dx_kernel<T::D, T::OSC>), dim3((a.ns + SS_THREADS - 1) / SS_THREADS, 1, nb), dim3(SS_THREADS), 0, st, a);
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
