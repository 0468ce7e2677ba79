// statespace_input_grad_host_check.hip -- ss_input_grad, ss_interp_dx_state and ss_interp_dx_ou of csrc/lmm_statespace.h (the gradients
// with respect to locations; DESIGN.md 4.18 "Gradients with respect to locations") run on the CPU.  For Matern12 / 32 / 52 and the
// oscillator (Q = 0.51, 2, 50), n = 1, 2, 3 and 200 with a quarter of the points unobserved, the sequential filter and full-state
// smoother give the states; d lml / d x_t = g_t - g_{t+1} from ss_input_grad is compared with central differences of the filter's log
// density in x_t (step 1e-6, tolerance 1e-6 of max|gradient|: the spacings are >= 0.01, so the truncation is (h / dt)^2 = 1e-8 and the
// rounding eps |lml| / h < 1e-7), and the query derivatives with central differences of ss_interp's mean and variance at queries in
// front of, between and behind the training inputs, at least 1e-4 from any of them.  Every result must be finite, and g_t = g_{t+1}
// to 1e-9 of max(1, max|g|) at an unobserved point.  A stand-alone program for host sanitizers; it needs no GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -std=c++17 -I linearmixingmodels.jl_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tools/statespace_input_grad_host_check.hip -o statespace_input_grad_host_check && ./statespace_input_grad_host_check
#include "lmm_statespace.h"
#include <cstdio>
#include <vector>
#include <cmath>
#include <algorithm>

template <int D> struct State { double m[D], P[D][D]; };

// the sequential filter (returns lml) and the sequential full-state smoother
template <int D, typename Mod>
double states(const Mod& M, const std::vector<double>& x, const std::vector<double>& w, const std::vector<double>& r,
              std::vector<State<D>>& f, std::vector<State<D>>& s) {
  const int n = (int)x.size();
  f.resize(n); s.resize(n);
  State<D> c;
  for (int i = 0; i < D; ++i) { c.m[i] = 0.0; for (int k = 0; k < D; ++k) c.P[i][k] = M.Pinf[i][k]; }
  double lml = 0.0;
  for (int t = 0; t < n; ++t) { lml += ss_filter_step<D>(M, t ? x[t] - x[t - 1] : 0.0, w[t], r[t], c.m, c.P); f[t] = c; }
  State<D> g;
  for (int i = 0; i < D; ++i) { g.m[i] = 0.0; for (int k = 0; k < D; ++k) g.P[i][k] = 0.0; }
  for (int t = n - 1; t >= 0; --t) {
    SSBwd<D> el;
    ss_bwd_element<D>(M, t == n - 1, t == n - 1 ? 0.0 : x[t + 1] - x[t], f[t].m, f[t].P, el);
    ss_rts_step<D>(el, g.m, g.P);
    s[t] = g;
  }
  return lml;
}

// ss_interp_kernel's and ss_interp_dx_kernel's arithmetic at one query: (mean, var) and their derivatives
template <int D, typename Mod>
void query(const Mod& M, const std::vector<double>& x, const std::vector<State<D>>& f, const std::vector<State<D>>& s, double q,
           double& mu, double& v, double& dmu, double& dv) {
  const int n = (int)x.size();
  const int k = ss_count_le(x.data(), 0, n, q);
  State<D> a, b;
  for (int i = 0; i < D; ++i) { a.m[i] = b.m[i] = 0.0; for (int j = 0; j < D; ++j) a.P[i][j] = b.P[i][j] = 0.0; }
  double d1 = 0.0, d2 = 0.0;
  if (k > 0) { a = f[k - 1]; d1 = q - x[k - 1]; }
  if (k < n) { b = s[k]; d2 = x[k] - q; }
  if constexpr (D == 1) ss_interp_dx_ou(M, k > 0, d1, k < n, d2, a.m[0], a.P[0][0], b.m[0], b.P[0][0], dmu, dv);
  ss_interp<D>(M, k > 0, d1, k < n, d2, a.m, a.P, b.m, b.P);
  if constexpr (D >= 2) ss_interp_dx_state<D>(a.m, a.P, dmu, dv);
  mu = a.m[0]; v = a.P[0][0];
}

static int failures = 0;
static double worst_x = 0.0, worst_q = 0.0;

template <int D, typename Mod>
void check(const char* name, const Mod& M, int n, unsigned seed) {
  unsigned st = seed * 2654435761u + 12345u;
  auto uni = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) + 0.5) / 16777216.0; };
  std::vector<double> x(n), w(n), r(n);
  double c = -1.0;
  for (int t = 0; t < n; ++t) {
    c += 0.7 * pow(10.0, -2.0 * uni());
    x[t] = c;
    w[t] = (t == 0 || uni() < 0.25) ? INFINITY : 0.05 + 0.45 * uni();
    r[t] = 2.0 * uni() - 1.0 + sin(3.0 * c);
  }
  if (n == 3) w[0] = 0.2;
  std::vector<State<D>> f, s;
  states<D>(M, x, w, r, f, s);
  // the spacings' derivatives and d lml / d x
  std::vector<double> g(n + 1, 0.0), gx(n), fd(n);
  for (int t = 1; t < n; ++t) g[t] = ss_input_grad<D>(M, x[t] - x[t - 1], f[t - 1].m, f[t - 1].P, s[t].m, s[t].P);
  double gmax = 0.0, scale = 0.0;
  for (int t = 0; t <= n; ++t) gmax = std::max(gmax, fabs(g[t]));
  const double h = 1e-6;
  for (int t = 0; t < n; ++t) {
    gx[t] = w[t] < INFINITY ? g[t] - g[t + 1] : 0.0;
    if (!(w[t] < INFINITY) && fabs(g[t] - g[t + 1]) > 1e-9 * std::max(gmax, 1.0)) { printf("FAIL %s n=%d: g does not telescope at the unobserved point %d\n", name, n, t); ++failures; }
    std::vector<double> xp(x), xm(x);
    std::vector<State<D>> f2, s2;
    xp[t] += h; xm[t] -= h;
    fd[t] = (states<D>(M, xp, w, r, f2, s2) - states<D>(M, xm, w, r, f2, s2)) / (2.0 * h);
    scale = std::max(scale, fabs(fd[t]));
  }
  for (int t = 0; t < n; ++t) {
    const double e = scale > 0.0 ? fabs(gx[t] - fd[t]) / scale : fabs(gx[t]);
    worst_x = std::max(worst_x, e);
    if (!std::isfinite(gx[t]) || e > 1e-6) { printf("FAIL %s n=%d: d lml / d x[%d] = %.12g, differences %.12g\n", name, n, t, gx[t], fd[t]); ++failures; }
  }
  // the queries
  std::vector<double> qs = {x[0] - 0.5, x[0] - 1e-3, x[n - 1] + 1e-3, x[n - 1] + 0.7};
  for (int t = 0; t + 1 < n; t += std::max(1, n / 20))
    if (x[t + 1] - x[t] > 4e-4) qs.push_back(0.5 * (x[t] + x[t + 1]));
  const double hq = 1e-6;
  double sm = 1e-300, sv = 1e-300;
  std::vector<double> em(qs.size()), ev(qs.size());
  for (size_t i = 0; i < qs.size(); ++i) {
    double mu, v, dmu, dv, mp, vp, mm, vm, d0, d1;
    query<D>(M, x, f, s, qs[i], mu, v, dmu, dv);
    query<D>(M, x, f, s, qs[i] + hq, mp, vp, d0, d1);
    query<D>(M, x, f, s, qs[i] - hq, mm, vm, d0, d1);
    const double fm = (mp - mm) / (2.0 * hq), fv = (vp - vm) / (2.0 * hq);
    sm = std::max(sm, fabs(fm)); sv = std::max(sv, fabs(fv));
    em[i] = fabs(dmu - fm); ev[i] = fabs(dv - fv);
    if (!std::isfinite(dmu) || !std::isfinite(dv)) { printf("FAIL %s n=%d: query %g is not finite\n", name, n, qs[i]); ++failures; }
  }
  for (size_t i = 0; i < qs.size(); ++i) {
    // nothing observed (n = 1 with w = +Inf): the posterior is the prior, both derivatives are 0 up to the differences' rounding
    const double e = std::max(em[i] / std::max(sm, 1e-3), ev[i] / std::max(sv, 1e-3));
    worst_q = std::max(worst_q, e);
    if (e > 1e-6) { printf("FAIL %s n=%d: query %g off by %.3e\n", name, n, qs[i], e); ++failures; }
  }
}

int main() {
  const int sizes[] = {1, 2, 3, 200};
  for (int n : sizes) {
    SSModel<1> m1; ss_model<1>(1.3, 1.0 / 0.7, m1); check<1>("matern12", m1, n, 1);
    SSModel<2> m2; ss_model<2>(1.3, 1.0 / 0.7, m2); check<2>("matern32", m2, n, 2);
    SSModel<3> m3; ss_model<3>(1.3, 1.0 / 0.7, m3); check<3>("matern52", m3, n, 3);
    const double Q[] = {0.51, 2.0, 50.0};
    for (double q : Q) { SSOsc<double> o; ss_osc_model<double>(1.3, 1.0 / 0.7, q, o); check<2>("sho", o, n, 4 + (unsigned)q); }
  }
  printf("worst d lml / d x against differences %.3e, worst query derivative %.3e (of the largest in the case)\n", worst_x, worst_q);
  printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
