// statespace_post_rand_host_check.hip -- ss_post_element and ss_chol_upper of csrc/lmm_statespace.h (the backward recursion that samples
// the posterior at new inputs from the stored states; DESIGN.md 4.18 "Sampling from the posterior object") run on the CPU.  For
// Matern12 / 32 / 52 and the oscillator (Q = 0.51, 2, 50), n = 1, 2, 3 and 200 with a quarter of the points unobserved and a run of equal
// inputs, the window of a set of sorted queries is built by a stable merge and the recursion is run once with zero normals and once per
// unit vector of the D W normals.  With zero normals every query must return the mean of ss_interp; the squares of the unit-vector
// responses must add up to ss_interp's variance, to 1e-11 of the prior scale; every result must be finite.  Queries: in front of,
// between, on (also on the tie) and behind the training inputs, 1e-9 beyond either end, 1e-9 and 1e-12 beside training inputs, and
// duplicates.  A stand-alone program for host sanitizers; it needs no GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -std=c++17 -I linearmixingmodels.jl_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tools/statespace_post_rand_host_check.hip -o statespace_post_rand_host_check && ./statespace_post_rand_host_check
#include "lmm_statespace.h"
#include <cstdio>
#include <vector>
#include <cmath>
#include <algorithm>

template <int D> struct State { double m[D], P[D][D]; };

// the sequential filter and the sequential full-state smoother
template <int D, typename Mod>
void states(const Mod& M, const std::vector<double>& x, const std::vector<double>& w, const std::vector<double>& r,
            std::vector<State<D>>& f, std::vector<State<D>>& s) {
  const int n = (int)x.size();
  f.resize(n); s.resize(n);
  State<D> c;
  for (int i = 0; i < D; ++i) { c.m[i] = 0.0; for (int k = 0; k < D; ++k) c.P[i][k] = M.Pinf[i][k]; }
  for (int t = 0; t < n; ++t) { ss_filter_step<D>(M, t ? x[t] - x[t - 1] : 0.0, w[t], r[t], c.m, c.P); f[t] = c; }
  State<D> g;
  for (int i = 0; i < D; ++i) { g.m[i] = 0.0; for (int k = 0; k < D; ++k) g.P[i][k] = 0.0; }
  for (int t = n - 1; t >= 0; --t) {
    SSBwd<D> el;
    ss_bwd_element<D>(M, t == n - 1, t == n - 1 ? 0.0 : x[t + 1] - x[t], f[t].m, f[t].P, el);
    ss_rts_step<D>(el, g.m, g.P);
    s[t] = g;
  }
}

// One run of the recursion over the window src (training point t >= 0, query -1 - i) on the normals zeta (D W, component-major):
// out[i] = the first component of the state at query i
template <int D, typename Mod>
void run(const Mod& M, const std::vector<double>& x, const std::vector<State<D>>& f, const std::vector<State<D>>& s,
         const std::vector<double>& q, const std::vector<int>& src, int first, const std::vector<double>& zeta, std::vector<double>& out) {
  const int n = (int)x.size(), W = (int)src.size();
  auto input = [&](int j) { return src[j] >= 0 ? x[src[j]] : q[-1 - src[j]]; };
  double st[D];
  for (int i = 0; i < D; ++i) st[i] = 0.0;
  State<D> zero;
  for (int i = 0; i < D; ++i) { zero.m[i] = 0.0; for (int j = 0; j < D; ++j) zero.P[i][j] = 0.0; }
  for (int j = W - 1; j >= 0; --j) {
    State<D> c;
    int k;
    if (src[j] >= 0) { c = f[src[j]]; k = src[j] + 1; }
    else {
      k = first + (j - (-1 - src[j]));
      if (k > 0) { c = f[k - 1]; ss_filter_step<D>(M, input(j) - x[k - 1], INFINITY, 0.0, c.m, c.P); }
      else { c = zero; for (int a = 0; a < D; ++a) for (int b = 0; b < D; ++b) c.P[a][b] = M.Pinf[a][b]; }
    }
    const bool last = j == W - 1, has_next = k < n;
    const double dt = last ? (has_next ? x[k] - input(j) : 0.0) : input(j + 1) - input(j);
    const State<D>& nx = last && has_next ? s[k] : zero;
    double z[D];
    for (int i = 0; i < D; ++i) z[i] = zeta[(size_t)i * W + j];
    SSAff<D> e;
    ss_post_element<D>(M, last, has_next, dt, c.m, c.P, nx.m, nx.P, z, e);
    ss_aff_step<D>(e, st);
    if (src[j] < 0) out[-1 - src[j]] = st[0];
  }
}

template <int D, typename Mod>
int check_model(const Mod& M, const char* name, int n, unsigned seed) {
  std::vector<double> x(n), w(n), r(n);
  unsigned sd = seed; auto u = [&]() { sd = sd * 1664525u + 1013904223u; return (sd >> 8) / 16777216.0; };
  double xx = 0;
  for (int t = 0; t < n; ++t) { xx += 0.7 * std::pow(10.0, -2.0 * u()); x[t] = xx; w[t] = u() < 0.25 ? INFINITY : 0.05 + 0.45 * u(); r[t] = 2 * u() - 1; }
  if (n > 12) { x[11] = x[10]; x[12] = x[10]; }
  std::vector<State<D>> f, s;
  states<D>(M, x, w, r, f, s);
  int bad = 0;
  double worst = 0.0;
  // three query sets: around everything, behind the data only, inside a stretch of it
  for (int set = 0; set < 3; ++set) {
    std::vector<double> q;
    if (set == 0) {
      q = {x[0] - 1.5, x[0] - 1e-9, x[0], x[n - 1], x[n - 1] + 1e-9, x[n - 1] + 2.5};
      for (int k = 0; k < 12; ++k) q.push_back(x[0] + (x[n - 1] - x[0]) * u());
      if (n > 12) { q.push_back(x[10]); q.push_back(x[40]); q.push_back(x[40]); q.push_back(x[50] + 1e-9); q.push_back(x[60] - 1e-12); }
    } else if (set == 1) q = {x[n - 1] + 0.01, x[n - 1] + 0.3, x[n - 1] + 0.3, x[n - 1] + 4.0};
    else if (n > 12) { for (int k = 0; k < 7; ++k) q.push_back(x[20] + (x[30] - x[20]) * u()); }
    else q = {x[0] + 1e-5};
    std::stable_sort(q.begin(), q.end());
    const int ns = (int)q.size();
    const int first = (int)(std::upper_bound(x.begin(), x.end(), q[0]) - x.begin());
    const int count = (int)(std::upper_bound(x.begin(), x.end(), q[ns - 1]) - x.begin()) - first;
    const int W = ns + count;
    std::vector<int> src(W, 1 << 30);
    for (int t = first; t < first + count; ++t) src[(t - first) + (std::lower_bound(q.begin(), q.end(), x[t]) - q.begin())] = t;
    for (int i = 0; i < ns; ++i) src[i + (std::upper_bound(x.begin(), x.end(), q[i]) - x.begin()) - first] = -1 - i;
    for (int j = 0; j < W; ++j) if (src[j] == 1 << 30) ++bad;
    std::vector<double> zeta((size_t)D * W, 0.0), mean(ns, 0.0), resp(ns, 0.0), var(ns, 0.0);
    run<D>(M, x, f, s, q, src, first, zeta, mean);
    for (int c = 0; c < D * W; ++c) {
      zeta[c] = 1.0;
      run<D>(M, x, f, s, q, src, first, zeta, resp);
      zeta[c] = 0.0;
      for (int i = 0; i < ns; ++i) var[i] += (resp[i] - mean[i]) * (resp[i] - mean[i]);
    }
    for (int i = 0; i < ns; ++i) {
      const int k = (int)(std::upper_bound(x.begin(), x.end(), q[i]) - x.begin());
      State<D> a, zero;
      for (int c = 0; c < D; ++c) { zero.m[c] = 0.0; for (int j = 0; j < D; ++j) zero.P[c][j] = 0.0; }
      a = k > 0 ? f[k - 1] : zero;
      const State<D>& nx = k < n ? s[k] : zero;
      ss_interp<D>(M, k > 0, k > 0 ? q[i] - x[k - 1] : 0.0, k < n, k < n ? x[k] - q[i] : 0.0, a.m, a.P, nx.m, nx.P);
      if (!std::isfinite(mean[i]) || !std::isfinite(var[i])) ++bad;
      worst = std::max(worst, std::fabs(mean[i] - a.m[0]) / std::sqrt(M.Pinf[0][0]));
      worst = std::max(worst, std::fabs(var[i] - a.P[0][0]) / M.Pinf[0][0]);
    }
  }
  if (!(worst <= 1e-11)) ++bad;
  std::printf("%-14s D=%d n=%3d worst %.2e %s\n", name, D, n, worst, bad ? "BAD" : "ok");
  return bad;
}

template <int D> int check_matern(const char* name) {
  SSModel<D> M; ss_model<D>(1.3, 1.0 / 0.7, M);
  int bad = 0;
  for (int n : {1, 2, 3, 200}) bad += check_model<D>(M, name, n, 777u + 31u * D + n);
  return bad;
}

// ss_count_le / ss_count_lt (the kernels' binary searches) against std::upper_bound / std::lower_bound on sorted arrays with ties,
// n = 0, 1, 2, 7, queries on, between and outside the values, over the whole array and over every sub-range [lo, hi)
int check_counts() {
  int bad = 0;
  const std::vector<double> all = {-1.0, 0.5, 0.5, 0.5, 2.0, 3.0, 3.0};
  for (int n : {0, 1, 2, 7}) {
    const std::vector<double> x(all.begin(), all.begin() + n);
    for (double s : {-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0})
      for (int lo = 0; lo <= n; ++lo)
        for (int hi = lo; hi <= n; ++hi) {
          if (ss_count_le(x.data(), lo, hi, s) != (int)(std::upper_bound(x.begin() + lo, x.begin() + hi, s) - x.begin())) ++bad;
          if (ss_count_lt(x.data(), lo, hi, s) != (int)(std::lower_bound(x.begin() + lo, x.begin() + hi, s) - x.begin())) ++bad;
        }
  }
  std::printf("ss_count_le / ss_count_lt %s\n", bad ? "BAD" : "ok");
  return bad;
}

int main() {
  int bad = check_matern<1>("matern12") + check_matern<2>("matern32") + check_matern<3>("matern52") + check_counts();
  for (double Q : {0.51, 2.0, 50.0}) {
    SSOsc<double> M; ss_osc_model<double>(1.3, 1.0 / 0.7, Q, M);
    char name[32]; std::snprintf(name, sizeof name, "sho Q=%g", Q);
    for (int n : {1, 2, 3, 200}) bad += check_model<2>(M, name, n, 991u + n);
  }
  std::printf(bad ? "FAILED (%d)\n" : "all checks passed\n", bad);
  return bad ? 1 : 0;
}
