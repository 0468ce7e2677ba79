// statespace_posterior_host_check.hip -- ss_interp of csrc/lmm_statespace.h (the posterior at a new input from the filtered state of
// the training point before it and the smoothed state of the one after it; DESIGN.md 4.18 "Posterior object") run on the CPU.  For
// Matern12 / 32 / 52 and the oscillator (Q = 0.51, 2, 50), n = 1, 2, 3 and 200 with a quarter of the points unobserved and a run of equal
// inputs, every query is answered twice: by ss_interp from the stored states, and by merging it into the inputs as an unobserved point
// and running the sequential filter and smoother over all n + 1 points (the `xs=` route).  The two must agree to 1e-11 of the prior
// scale; a query on a training input must return that input's smoothed state; every result must be finite.  Queries: in front of,
// between, on (also on the tie) and behind the training inputs, and 1e-9 beyond either end.  A stand-alone program for host
// sanitizers; it needs no GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -std=c++17 -I linearmixingmodels.jl_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tools/statespace_posterior_host_check.hip -o statespace_posterior_host_check && ./statespace_posterior_host_check
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

template <int D, typename Mod>
int check_model(const Mod& M, const char* name, int n, unsigned seed) {
  std::vector<double> x(n), w(n), r(n);
  unsigned sd = seed; auto u = [&]() { sd = sd * 1664525u + 1013904223u; return (sd >> 8) / 16777216.0; };
  double xx = 0;
  for (int t = 0; t < n; ++t) { xx += 0.7 * std::pow(10.0, -2.0 * u()); x[t] = xx; w[t] = u() < 0.25 ? INFINITY : 0.05 + 0.45 * u(); r[t] = 2 * u() - 1; }
  if (n > 12) { x[11] = x[10]; x[12] = x[10]; }
  std::vector<State<D>> f, s;
  states<D>(M, x, w, r, f, s);
  std::vector<double> q = {x[0] - 1.5, x[0] - 1e-9, x[0], x[n - 1], x[n - 1] + 1e-9, x[n - 1] + 2.5};
  for (int k = 0; k < 12; ++k) q.push_back(x[0] + (x[n - 1] - x[0]) * u());
  if (n > 12) { q.push_back(x[10]); q.push_back(x[40]); q.push_back(0.5 * (x[12] + x[13])); }
  int bad = 0;
  double worst = 0.0;
  for (double sq : q) {
    const int k = (int)(std::upper_bound(x.begin(), x.end(), sq) - x.begin());
    State<D> a, zero;
    for (int i = 0; i < D; ++i) { zero.m[i] = 0.0; for (int j = 0; j < D; ++j) zero.P[i][j] = 0.0; }
    a = k > 0 ? f[k - 1] : zero;
    const State<D>& nx = k < n ? s[k] : zero;
    ss_interp<D>(M, k > 0, k > 0 ? sq - x[k - 1] : 0.0, k < n, k < n ? x[k] - sq : 0.0, a.m, a.P, nx.m, nx.P);
    // the same by merging the query into the inputs as an unobserved point
    std::vector<double> x2(x), w2(w), r2(r);
    x2.insert(x2.begin() + k, sq); w2.insert(w2.begin() + k, INFINITY); r2.insert(r2.begin() + k, 0.0);
    std::vector<State<D>> f2, s2;
    states<D>(M, x2, w2, r2, f2, s2);
    for (int i = 0; i < D; ++i) {
      const double si = std::sqrt(M.Pinf[i][i]);
      if (!std::isfinite(a.m[i])) ++bad;
      worst = std::max(worst, std::fabs(a.m[i] - s2[k].m[i]) / si);
      for (int j = 0; j < D; ++j) {
        if (!std::isfinite(a.P[i][j])) ++bad;
        worst = std::max(worst, std::fabs(a.P[i][j] - s2[k].P[i][j]) / (si * std::sqrt(M.Pinf[j][j])));
      }
    }
    if (k > 0 && sq == x[k - 1])                 // on a training input: its smoothed state
      for (int i = 0; i < D; ++i) {
        worst = std::max(worst, std::fabs(a.m[i] - s[k - 1].m[i]) / std::sqrt(M.Pinf[i][i]));
        for (int j = 0; j < D; ++j)
          worst = std::max(worst, std::fabs(a.P[i][j] - s[k - 1].P[i][j]) / std::sqrt(M.Pinf[i][i] * M.Pinf[j][j]));
      }
  }
  if (!(worst <= 1e-11)) ++bad;
  std::printf("%-14s D=%d n=%3d queries=%2d worst %.2e %s\n", name, D, n, (int)q.size(), worst, bad ? "BAD" : "ok");
  return bad;
}

template <int D> int check_matern(const char* name) {
  SSModel<D> M; ss_model<D>(1.3, 1.0 / 0.7, M);
  int bad = 0;
  for (int n : {1, 2, 3, 200}) bad += check_model<D>(M, name, n, 777u + 31u * D + n);
  return bad;
}

int main() {
  int bad = check_matern<1>("matern12") + check_matern<2>("matern32") + check_matern<3>("matern52");
  for (double Q : {0.51, 2.0, 50.0}) {
    SSOsc<double> M; ss_osc_model<double>(1.3, 1.0 / 0.7, Q, M);
    char name[32]; std::snprintf(name, sizeof name, "sho Q=%g", Q);
    for (int n : {1, 2, 3, 200}) bad += check_model<2>(M, name, n, 991u + n);
  }
  std::printf(bad ? "FAILED (%d)\n" : "all checks passed\n", bad);
  return bad ? 1 : 0;
}
