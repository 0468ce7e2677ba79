// lmm_kernels_ss.h -- the templated kernels of the state-space path and their launch sequences, shared by the two translation units
// that instantiate them: lmm_kernels_ss.hip (the one-term models: Matern12 / 32 / 52 and the oscillator) and lmm_kernels_ss_sum.hip (the
// seven sums of two of them, SSSum).  Everything here has internal linkage (an anonymous namespace per unit).  The description of
// the phases, of every kernel and of the host helpers is at the top of lmm_kernels_ss.hip.
#pragma once
#include "lmm_internal.h"
#include "lmm_statespace.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int SS_THREADS = 256;      // fold / filter / rts: one thread per chunk
constexpr int SS_SCAN = 128;         // aggregates per workgroup of the scan (one per thread; 128 SSFwd<3> are 33 KiB of LDS)
// 128 SSFwd<3, SSDual> would be 66 KiB, above the 64 KiB of static LDS: elements that large are scanned 64 per workgroup
template <typename T> constexpr int ss_scan_width() { return sizeof(T) * SS_SCAN <= 65536 ? SS_SCAN : SS_SCAN / 2; }

// The model of a launch: MOD = 0, the Matern model of state dimension D; MOD = 1 (D = 2), the oscillator; MOD = SS_PAIR(a, b) (D = D_a +
// D_b), the sum of the term models a and b, each 1 / 2 / 3 (Matern12 / 32 / 52) or SS_MODEL_SHO (lmm_statespace.h SSSum)
constexpr int ss_term_dim(int term) { return term == SS_MODEL_SHO ? 2 : term; }
template <int D, int MOD, typename Sc = double> struct SSModelOf {
  static_assert(MOD >= SS_PAIR(1, 1) && ss_term_dim(MOD / SS_PAIR(1, 0)) + ss_term_dim(MOD % SS_PAIR(1, 0)) == D, "not a model");
  typedef typename SSModelOf<ss_term_dim(MOD / SS_PAIR(1, 0)), MOD / SS_PAIR(1, 0) == SS_MODEL_SHO, Sc>::type A;
  typedef typename SSModelOf<ss_term_dim(MOD % SS_PAIR(1, 0)), MOD % SS_PAIR(1, 0) == SS_MODEL_SHO, Sc>::type B;
  typedef SSSum<A, B, Sc> type;
};
template <int D, typename Sc> struct SSModelOf<D, 0, Sc> { typedef SSModel<D, Sc> type; };
template <typename Sc> struct SSModelOf<2, 1, Sc> { typedef SSOsc<Sc> type; };
// seeded parameters of the forward-mode gradient: variance and lengthscale, and an oscillator's quality; a sum: its terms' own, a's first
constexpr int ss_term_seeds(int term) { return term == SS_MODEL_SHO ? 3 : 2; }
template <int MOD> constexpr int ss_seeds() {
  return MOD >= SS_PAIR(1, 1) ? ss_term_seeds(MOD / SS_PAIR(1, 0)) + ss_term_seeds(MOD % SS_PAIR(1, 0)) : MOD ? 3 : 2;
}

template <int D, int MOD, typename Sc>
__device__ __forceinline__ typename SSModelOf<D, MOD, Sc>::type ss_make_model(Sc var, Sc inv_ls, Sc quality) {
  typename SSModelOf<D, MOD, Sc>::type M;
  if constexpr (MOD) ss_osc_model<Sc>(var, inv_ls, quality, M);
  else ss_model<D, Sc>(var, inv_ls, M);
  return M;
}

// The model of a latent's (var, inv_ls, quality), of any of the *Lat structs.  Sc = SSDual: with the tangent of parameter `seed` set: 0 =
// variance, 1 = lengthscale (d (1 / l) = -1 / l^2; an oscillator's period), 2 = an oscillator's quality.  A sum takes its second term
// from (var2, inv_ls2, quality2), and its seeds count through the first term's parameters, then the second's.
template <int D, int MOD, typename Sc = double, typename Lat>
__device__ __forceinline__ typename SSModelOf<D, MOD, Sc>::type ss_lat_model(const Lat& L, int seed = 0) {
  if constexpr (MOD >= SS_PAIR(1, 1)) {
    constexpr int TA = MOD / SS_PAIR(1, 0), TB = MOD % SS_PAIR(1, 0), NA = ss_term_seeds(TA);
    constexpr int DA = ss_term_dim(TA), DB = ss_term_dim(TB);
    typename SSModelOf<D, MOD, Sc>::type M;
    if constexpr (std::is_same<Sc, SSDual>::value) {
      const int sb = seed - NA;
      ss_sum_model(ss_make_model<DA, TA == SS_MODEL_SHO, SSDual>(SSDual(L.var, seed == 0 ? 1.0 : 0.0), SSDual(L.inv_ls, seed == 1 ? -L.inv_ls * L.inv_ls : 0.0),
                                                                 SSDual(L.quality, NA == 3 && seed == 2 ? 1.0 : 0.0)),
                   ss_make_model<DB, TB == SS_MODEL_SHO, SSDual>(SSDual(L.var2, sb == 0 ? 1.0 : 0.0), SSDual(L.inv_ls2, sb == 1 ? -L.inv_ls2 * L.inv_ls2 : 0.0),
                                                                 SSDual(L.quality2, sb == 2 ? 1.0 : 0.0)), M);
    } else {
      ss_sum_model(ss_make_model<DA, TA == SS_MODEL_SHO, double>(L.var, L.inv_ls, L.quality),
                   ss_make_model<DB, TB == SS_MODEL_SHO, double>(L.var2, L.inv_ls2, L.quality2), M);
    }
    return M;
  } else if constexpr (std::is_same<Sc, SSDual>::value)
    return ss_make_model<D, MOD, SSDual>(SSDual(L.var, seed == 0 ? 1.0 : 0.0), SSDual(L.inv_ls, seed == 1 ? -L.inv_ls * L.inv_ls : 0.0),
                                         SSDual(L.quality, seed == 2 ? 1.0 : 0.0));
  else return ss_make_model<D, MOD, double>(L.var, L.inv_ls, L.quality);
}

// Fold and filter in both scalar types.  Sc = double: the value; the aggregates of latent z = blockIdx.z are item z of a.agg.
// Sc = SSDual: (value, tangent) with blockIdx.y the seeded parameter (NS = ss_seeds<MOD>() of them), so a thread carries one tangent;
// the aggregates of (latent z, seed s) are item NS z + s of a.dagg.
// And from both starts (Args).  SSArgs: the prior in front of point 0.  SSFromArgs (Sc = double; DESIGN.md 4.18 "Appending
// observations"): a stored state, L.init at input a.x0 -- the element of point 0 is ss_fwd_element_from, thread 0 restarts from L.init
// over x[0] - x0, and the filtered states go point-major to L.out (rows n .. n + k - 1 of the posterior object's block); every other
// element and the scan are the same.
template <int D, int MOD, typename Sc, typename Args>
__device__ __forceinline__ SSFwd<D, Sc>& ss_fwd_agg(const Args& a, int z, int s, size_t j) {       // aggregate j of (latent z, seed s)
  if constexpr (std::is_same<Sc, SSDual>::value) return reinterpret_cast<SSFwd<D, Sc>*>(a.dagg)[(size_t)(ss_seeds<MOD>() * z + s) * a.nch + j];
  else return reinterpret_cast<SSFwd<D, Sc>*>(a.agg)[(size_t)z * a.nch + j];
}

template <int D, int MOD, typename Sc, typename Args = SSArgs>
__global__ __launch_bounds__(SS_THREADS) void ss_fold_kernel(Args a) {
  constexpr bool DUAL = std::is_same<Sc, SSDual>::value, FROM = std::is_same<Args, SSFromArgs>::value;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z, s = DUAL ? blockIdx.y : 0;
  if (j >= a.nch) return;
  const auto& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD, Sc>(L, s);
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
  ss_fwd_agg<D, MOD, Sc>(a, z, s, j) = acc;
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
template <int D, int MOD, typename Sc, typename Args = SSArgs>
__global__ __launch_bounds__(SS_THREADS) void ss_filter_kernel(Args a) {
  constexpr bool DUAL = std::is_same<Sc, SSDual>::value, FROM = std::is_same<Args, SSFromArgs>::value;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z, s = DUAL ? blockIdx.y : 0;
  if (j >= a.nch) return;
  const auto& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD, Sc>(L, s);
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
    const SSFwd<D, Sc>& pre = ss_fwd_agg<D, MOD, Sc>(a, z, s, (size_t)j - 1);
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
  if constexpr (DUAL) a.dpart[(size_t)(ss_seeds<MOD>() * z + s) * a.nch + j] = lp.t;
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

// The backward recursion reads the filtered states from a.state, component-major, as the filter of the same call left them; KEPT: from
// a.fkeep, point-major -- the posterior object's buffer, whose blocks a.state_stride strides as well.
template <int D, int MOD, bool KEPT = false>
__global__ __launch_bounds__(SS_THREADS) void ss_bfold_kernel(SSArgs a) {
  constexpr int NC = D + D * (D + 1) / 2;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const auto M = ss_lat_model<D, MOD>(a.lat[z]);
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
template <int D, int MOD, SSRts V = SS_RTS_MARGINALS>
__global__ __launch_bounds__(SS_THREADS) void ss_rts_kernel(SSArgs a) {
  constexpr bool FULL = V == SS_RTS_FULL, GX = V == SS_RTS_GX, KEPT = V == SS_RTS_KEPT;
  constexpr int NC = D + D * (D + 1) / 2;
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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

// One thread per (query, latent): the posterior marginal of the latent at xs[q] from the stored filtered and smoothed states
// (ss_interp).  k = #{t : x_t <= s} by binary search over the sorted x (a query equal to a training input comes behind every copy of
// it): at most ceil(log2(n + 1)) probes.  Reads the states of points k - 1 >= 0 and k < n only; a query's result depends on no other
// query.  xs is finite (launch_ss_finite has looked).
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_interp_kernel(SSInterpArgs a) {
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
  ss_interp<D>(M, k > 0, d1, k < a.n, d2, m, P, ms, Ps);
  a.mean[(size_t)z * a.ns + q] = m[0] + L.mean;
  if (a.var) a.var[(size_t)z * a.ns + q] = P[0][0];
}


// ---- sampling ------------------------------------------------------------------------------------------------------------------
// The prior path s_t = A(dt_t) s_{t-1} + chol(Q(dt_t)) zeta_t, s_0 = chol(Pinf) zeta_0, is an affine recursion, so the same three
// phases serve it with SSAff<D> elements (D^2 + D doubles): ss_sfold_kernel, the scan with AffOp, ss_path_kernel.  blockIdx.z runs over
// the (latent, sample) pairs of a launch; zeta is read straight from the caller's buffer, component i of point t at z[i n + t].
template <int D>
__device__ __forceinline__ void ss_load_zeta(const double* __restrict__ z, int n, long long t, double zeta[D]) {
  for (int i = 0; i < D; ++i) zeta[i] = z[(size_t)i * n + t];
}

template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_sfold_kernel(SSPathArgs a) {
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSPathLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_path_kernel(SSPathArgs a) {
  const int j = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (j >= a.nch) return;
  const SSPathLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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

// ---- sampling from the posterior object --------------------------------------------------------------------------------------------
// Given the data, the states at the window's points (SSPostArgs: the sorted queries and the training points between the smallest and
// the largest of them) form a Markov chain that runs BACKWARDS: s_j = E_j s_{j+1} + g_j + U(L_j) zeta_j from the posterior state at the
// last point (ss_post_element).  That is an affine recursion again, so the three phases of the prior path serve it from the right:
// ss_pfold_kernel, the suffix scan with AffRevOp, ss_ppath_kernel.  Nothing outside the window is read but the states next to its ends.

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
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_pfold_kernel(SSPostArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSPostLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_ppath_kernel(SSPostArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSPostLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_lfold_kernel(SSLpdfArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSLpdfLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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
template <int D, int MOD>
__global__ __launch_bounds__(SS_THREADS) void ss_lfilter_kernel(SSLpdfArgs a) {
  const int c = blockIdx.x * SS_THREADS + threadIdx.x, z = blockIdx.z;
  if (c >= a.nch) return;
  const SSLpdfLat& L = a.lat[z];
  const auto M = ss_lat_model<D, MOD>(L);
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



// The model of a launch as a type: D and MOD reach a generic lambda as compile-time constants.  A sum's model SS_PAIR(a, b) is its own
// template argument MOD, beside D = D_a + D_b (PAIR: whether the model is a sum).
template <int D_, int MOD_> struct SSModelTag { static constexpr int D = D_, MOD = MOD_; static constexpr bool PAIR = MOD_ >= SS_PAIR(1, 1); };
template <int A, int B> using SSPairTag = SSModelTag<ss_term_dim(A) + ss_term_dim(B), SS_PAIR(A, B)>;

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


// The launches of one set of models: Models::dispatch hands a launch's model to a generic lambda as compile-time (D, MOD).  The two
// translation units instantiate these with their own set (lmm_kernels_ss.hip: SSOneTermModels; lmm_kernels_ss_sum.hip: SSPairModels).
template <typename Models>
void ss_launch_filter(const SSArgs& a, int model, int nb, double* lml, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSFwd<T::D>, FwdOp, false>(ss_fold_kernel<T::D, T::MOD, double>, ss_filter_kernel<T::D, T::MOD, double>, a, 1, nb, a.agg, st);
  });
  if (lml) hipLaunchKernelGGL(ss_finish_kernel, dim3(nb), dim3(SS_THREADS), 0, st, (const double*)a.part, a.nch, lml);
}

template <typename Models>
void ss_launch_smooth(const SSArgs& a, int model, int nb, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    auto rts = ss_rts_kernel<T::D, T::MOD>;
    if (a.sstate) rts = ss_rts_kernel<T::D, T::MOD, SS_RTS_FULL>;
    else if constexpr (!T::PAIR) {      // a sum has no location gradients (the entry points refuse them): a.gdt is nullptr
      if (a.gdt) rts = ss_rts_kernel<T::D, T::MOD, SS_RTS_GX>;
    }
    ss_phases<T::D, SSBwd<T::D>, BwdOp, true>(ss_bfold_kernel<T::D, T::MOD>, rts, a, 1, nb, a.bagg, st);
  });
}

template <typename Models>
void ss_launch_filter_from(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_scored_phases<T::D, FwdOp, false>(ss_fold_kernel<T::D, T::MOD, double, SSFromArgs>, ss_filter_kernel<T::D, T::MOD, double, SSFromArgs>,
                                         a, nb, lml, st);
  });
}

template <typename Models>
void ss_launch_smooth_kept(const SSArgs& a, int model, int nb, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSBwd<T::D>, BwdOp, true>(ss_bfold_kernel<T::D, T::MOD, true>, ss_rts_kernel<T::D, T::MOD, SS_RTS_KEPT>, a, 1, nb, a.bagg, st);
  });
}

template <typename Models>
void ss_launch_grad(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st) {
  const int NS = ss_model_seeds(model);
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSFwd<T::D, SSDual>, FwdOp, false>(ss_fold_kernel<T::D, T::MOD, SSDual>, ss_filter_kernel<T::D, T::MOD, SSDual>, a, NS, nb,
                                                       a.dagg, st);
  });
  hipLaunchKernelGGL(ss_finish_kernel, dim3(NS * nb), dim3(SS_THREADS), 0, st, (const double*)a.dpart, a.nch, gtheta);
}

template <typename Models>
void ss_launch_path(const SSPathArgs& a, int model, int nb, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSAff<T::D>, AffOp, false>(ss_sfold_kernel<T::D, T::MOD>, ss_path_kernel<T::D, T::MOD>, a, 1, nb, a.agg, st);
  });
}

template <typename Models>
void ss_launch_post_path(const SSPostArgs& a, int model, int nb, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_phases<T::D, SSAff<T::D>, AffRevOp, true>(ss_pfold_kernel<T::D, T::MOD>, ss_ppath_kernel<T::D, T::MOD>, a, 1, nb, a.agg, st);
  });
}

template <typename Models>
void ss_launch_post_logpdf(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    ss_scored_phases<T::D, FwdRevOp, true>(ss_lfold_kernel<T::D, T::MOD>, ss_lfilter_kernel<T::D, T::MOD>, a, nb, lml, st);
  });
}

template <typename Models>
void ss_launch_interp(const SSInterpArgs& a, int model, int nb, hipStream_t st) {
  Models::dispatch(model, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((ss_interp_kernel<T::D, T::MOD>), dim3((a.ns + SS_THREADS - 1) / SS_THREADS, 1, nb), dim3(SS_THREADS), 0, st, a);
  });
}

}  // namespace

// The launches of the pair models (lmm_kernels_ss_sum.hip), which the launch_ss_* of lmm_kernels_ss.hip hand a sum's model to
void launch_ss_filter_pair(const SSArgs& a, int model, int nb, double* lml, hipStream_t st);
void launch_ss_smooth_pair(const SSArgs& a, int model, int nb, hipStream_t st);
void launch_ss_filter_from_pair(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st);
void launch_ss_smooth_kept_pair(const SSArgs& a, int model, int nb, hipStream_t st);
void launch_ss_grad_pair(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st);
void launch_ss_path_pair(const SSPathArgs& a, int model, int nb, hipStream_t st);
void launch_ss_post_path_pair(const SSPostArgs& a, int model, int nb, hipStream_t st);
void launch_ss_post_logpdf_pair(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st);
void launch_ss_interp_pair(const SSInterpArgs& a, int model, int nb, hipStream_t st);
