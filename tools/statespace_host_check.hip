// statespace_host_check.hip -- the double and the SSDual instantiations of csrc/lmm_statespace.h run on the CPU, with the chunked schedule
// of lmm_kernels_ss.hip (fold, a sequential scan of the aggregates, filter restarted from the prefix) for chunk = 1, 7, 64 and n, Matern12 /
// 32 / 52, a quarter of the points unobserved and a run of equal inputs.  Checks that the value of the dual instantiation is bitwise the
// double one's and that both tangents agree with central differences of the value (step 1e-5: 1e-6 relative).  Sampling: ss_chol_psd on a
// zero, a rank-deficient and a slightly indefinite matrix, and the affine fold / scan / restart of the prior path at the same chunks
// against the sequential recursion (1e-12 sqrt(v); an equal input repeats the state bitwise).  The oscillator model of an SHO latent
// (SSOsc) goes through the same checks at Q = 0.51, 2 and 50 with its three tangents (variance, period, quality), and A(0) = I, Q(0) = 0
// exactly.  A stand-alone program for host sanitizers; it needs no GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -std=c++17 -I linearmixingmodels.jl_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tools/statespace_host_check.hip -o statespace_host_check && ./statespace_host_check
#include "lmm_statespace.h"
#include <cstdio>
#include <vector>
#include <cmath>
#include <algorithm>
template <int D, typename Sc, typename Mod>
Sc run_model(const Mod& M, const std::vector<double>& x, const std::vector<double>& w, const std::vector<double>& r, int chunk) {
  const int n = (int)x.size(), nch = (n + chunk - 1) / chunk;
  std::vector<SSFwd<D, Sc>> agg(nch);
  for (int j = 0; j < nch; ++j) {
    int t0 = j * chunk, t1 = std::min(n, t0 + chunk);
    SSFwd<D, Sc> acc, el;
    ss_fwd_element<D, Sc>(M, t0 == 0, t0 == 0 ? 0.0 : x[t0] - x[t0 - 1], w[t0], r[t0], acc);
    for (int t = t0 + 1; t < t1; ++t) { ss_fwd_element<D, Sc>(M, false, x[t] - x[t - 1], w[t], r[t], el); ss_fwd_combine<D, Sc>(acc, el, acc); }
    agg[j] = acc;
  }
  for (int j = 1; j < nch; ++j) ss_fwd_combine<D, Sc>(agg[j - 1], agg[j], agg[j]);
  Sc tot = 0.0;
  for (int j = 0; j < nch; ++j) {
    int t0 = j * chunk, t1 = std::min(n, t0 + chunk);
    Sc m[D], P[D][D];
    for (int i = 0; i < D; ++i) { m[i] = j ? agg[j - 1].b[i] : Sc(0.0); for (int k = 0; k < D; ++k) P[i][k] = j ? agg[j - 1].C[i][k] : M.Pinf[i][k]; }
    double xp = t0 == 0 ? x[0] : x[t0 - 1];
    for (int t = t0; t < t1; ++t) { tot += ss_filter_step<D, Sc>(M, x[t] - xp, w[t], r[t], m, P); xp = x[t]; }
  }
  return tot;
}
template <int D, typename Sc>
Sc run(Sc var, Sc il, const std::vector<double>& x, const std::vector<double>& w, const std::vector<double>& r, int chunk) {
  SSModel<D, Sc> M; ss_model<D, Sc>(var, il, M);
  return run_model<D, Sc>(M, x, w, r, chunk);
}
template <typename Sc>
Sc run_osc(Sc var, Sc ip, Sc q, const std::vector<double>& x, const std::vector<double>& w, const std::vector<double>& r, int chunk) {
  SSOsc<Sc> M; ss_osc_model<Sc>(var, ip, q, M);
  return run_model<2, Sc>(M, x, w, r, chunk);
}
template <int D> int check() {
  const int n = 200; std::vector<double> x(n), w(n), r(n);
  unsigned s = 12345u + D; auto u = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  double xx = 0; for (int t = 0; t < n; ++t) { xx += 0.7 * std::pow(10.0, -2.0 * u()); x[t] = xx; w[t] = u() < 0.25 ? INFINITY : 0.05 + 0.45 * u(); r[t] = 2 * u() - 1; }
  x[11] = x[10]; x[12] = x[10];
  const double v = 1.3, ell = 0.7, il = 1 / ell; int bad = 0;
  for (int chunk : {1, 7, 64, 200}) {
    double val = run<D, double>(v, il, x, w, r, chunk);
    SSDual gv = run<D, SSDual>(SSDual(v, 1.0), SSDual(il, 0.0), x, w, r, chunk);
    SSDual gl = run<D, SSDual>(SSDual(v, 0.0), SSDual(il, -il * il), x, w, r, chunk);
    const double h = 1e-5;
    double fv = (run<D, double>(v + h, il, x, w, r, chunk) - run<D, double>(v - h, il, x, w, r, chunk)) / (2 * h);
    double fl = (run<D, double>(v, 1 / (ell + h), x, w, r, chunk) - run<D, double>(v, 1 / (ell - h), x, w, r, chunk)) / (2 * h);
    std::printf("D=%d chunk=%3d val=%.15g dual.v==val:%d dv %.12g fd %.12g dl %.12g fd %.12g\n", D, chunk, val, gv.v == val && gl.v == val, gv.t, fv, gl.t, fl);
    if (!(gv.v == val) || std::fabs(gv.t - fv) > 1e-6 * std::fabs(fv) + 1e-7 || std::fabs(gl.t - fl) > 1e-6 * std::fabs(fl) + 1e-7) ++bad;
  }
  return bad;
}
// the prior path by the chunked schedule: fold the affine elements, scan the aggregates, restart from the prefix state
template <int D, typename Mod>
std::vector<double> path_model(const Mod& M, const std::vector<double>& x, const std::vector<double>& z, int chunk) {
  const int n = (int)x.size(), nch = (n + chunk - 1) / chunk;
  auto zeta = [&](int t, double* o) { for (int i = 0; i < D; ++i) o[i] = z[(size_t)i * n + t]; };
  std::vector<SSAff<D>> agg(nch);
  double zt[D];
  for (int j = 0; j < nch; ++j) {
    int t0 = j * chunk, t1 = std::min(n, t0 + chunk);
    SSAff<D> acc, el;
    zeta(t0, zt);
    ss_aff_element<D>(M, t0 == 0, t0 == 0 ? 0.0 : x[t0] - x[t0 - 1], zt, acc);
    for (int t = t0 + 1; t < t1; ++t) { zeta(t, zt); ss_aff_element<D>(M, false, x[t] - x[t - 1], zt, el); ss_aff_combine<D>(acc, el, acc); }
    agg[j] = acc;
  }
  for (int j = 1; j < nch; ++j) ss_aff_combine<D>(agg[j - 1], agg[j], agg[j]);
  std::vector<double> f(n);
  for (int j = 0; j < nch; ++j) {
    int t0 = j * chunk, t1 = std::min(n, t0 + chunk);
    double s[D];
    for (int i = 0; i < D; ++i) s[i] = j ? agg[j - 1].c[i] : 0.0;
    SSAff<D> el;
    for (int t = t0; t < t1; ++t) { zeta(t, zt); ss_aff_element<D>(M, t == 0, t == 0 ? 0.0 : x[t] - x[t - 1], zt, el); ss_aff_step<D>(el, s); f[t] = s[0]; }
  }
  return f;
}
template <int D>
std::vector<double> path(double var, double il, const std::vector<double>& x, const std::vector<double>& z, int chunk) {
  SSModel<D> M; ss_model<D>(var, il, M);
  return path_model<D>(M, x, z, chunk);
}
template <int D> int check_chol() {
  int bad = 0;
  double X[D][D], L[D][D];
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) X[i][j] = 0.0;
  ss_chol_psd<D>(X, L);                                                  // zero matrix: zero factor
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) if (L[i][j] != 0.0) ++bad;
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) X[i][j] = (i + 1.0) * (j + 1.0);      // rank one: only the first column
  X[D - 1][D - 1] += (D > 1 ? -1e-18 : 0.0);                             // and a last pivot that rounding has made negative
  ss_chol_psd<D>(X, L);
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
    const double want = j == 0 ? i + 1.0 : 0.0;
    if (!(std::fabs(L[i][j] - want) <= 1e-15) || (j > 0 && L[i][j] != 0.0)) ++bad;
  }
  SSModel<D> M; ss_model<D>(1.3, 1 / 0.7, M);                            // Q of a tiny step: finite, non-negative diagonal, L L' = Q to rounding
  double A[D][D], Q[D][D];
  ss_AQ<D>(M, 1e-4, A, Q);
  ss_chol_psd<D>(Q, L);
  for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) if (!std::isfinite(L[i][j]) || (i == j && L[i][j] < 0.0) || (j > i && L[i][j] != 0.0)) ++bad;
  std::printf("D=%d chol_psd bad=%d\n", D, bad);
  return bad;
}
template <int D> int check_path() {
  const int n = 200; std::vector<double> x(n), z((size_t)D * n);
  unsigned s = 777u + D; auto u = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  double xx = 0; for (int t = 0; t < n; ++t) { xx += 0.7 * (0.5 + 1.5 * u()); x[t] = xx; }
  for (auto& v : z) v = 2 * u() - 1 + 2 * u() - 1;
  x[11] = x[10]; x[12] = x[10];
  for (int t = 100; t < n; ++t) x[t] += 7000.0;                           // one gap of 1e4 lengthscales
  const double v = 1.3, il = 1 / 0.7; int bad = 0;
  const std::vector<double> seq = path<D>(v, il, x, z, n);
  if (seq[11] != seq[10] || seq[12] != seq[10]) ++bad;
  for (int chunk : {1, 7, 64, 200}) {
    const std::vector<double> f = path<D>(v, il, x, z, chunk);
    double err = 0; for (int t = 0; t < n; ++t) err = std::max(err, std::fabs(f[t] - seq[t]));
    std::printf("D=%d chunk=%3d path err %.3g\n", D, chunk, err);
    if (!(err <= 1e-12 * std::sqrt(v))) ++bad;
  }
  return bad;
}
// the oscillator: value and three tangents at every chunk, A(0) = I and Q(0) = 0 exactly, the chunked path against the sequential one
int check_osc(double q) {
  const int n = 200; std::vector<double> x(n), w(n), r(n), z(2 * (size_t)n);
  unsigned s = 4242u + (unsigned)(100 * q); auto u = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  double xx = 0; for (int t = 0; t < n; ++t) { xx += 0.7 * std::pow(10.0, -2.0 * u()); x[t] = xx; w[t] = u() < 0.25 ? INFINITY : 0.05 + 0.45 * u(); r[t] = 2 * u() - 1; }
  for (auto& v : z) v = 2 * u() - 1 + 2 * u() - 1;
  x[11] = x[10]; x[12] = x[10];
  const double v = 1.3, P = 0.7, ip = 1 / P; int bad = 0;
  SSOsc<double> M; ss_osc_model<double>(v, ip, q, M);
  double A[2][2], Q[2][2];
  ss_AQ<2>(M, 0.0, A, Q);
  if (A[0][0] != 1.0 || A[1][1] != 1.0 || A[0][1] != 0.0 || A[1][0] != 0.0 || Q[0][0] != 0.0 || Q[0][1] != 0.0 || Q[1][0] != 0.0 || Q[1][1] != 0.0) ++bad;
  for (int chunk : {1, 7, 64, 200}) {
    const double val = run_osc<double>(v, ip, q, x, w, r, chunk);
    const SSDual g[3] = {run_osc<SSDual>(SSDual(v, 1.0), SSDual(ip, 0.0), SSDual(q, 0.0), x, w, r, chunk),
                         run_osc<SSDual>(SSDual(v, 0.0), SSDual(ip, -ip * ip), SSDual(q, 0.0), x, w, r, chunk),
                         run_osc<SSDual>(SSDual(v, 0.0), SSDual(ip, 0.0), SSDual(q, 1.0), x, w, r, chunk)};
    const double h = q > 0.6 ? 1e-5 : 1e-7;                              // d/dq is of size 1 / (2 q - 1) near q = 1/2, and so is its curvature
    const double fd[3] = {(run_osc<double>(v + h, ip, q, x, w, r, chunk) - run_osc<double>(v - h, ip, q, x, w, r, chunk)) / (2 * h),
                          (run_osc<double>(v, 1 / (P + h), q, x, w, r, chunk) - run_osc<double>(v, 1 / (P - h), q, x, w, r, chunk)) / (2 * h),
                          (run_osc<double>(v, ip, q + h, x, w, r, chunk) - run_osc<double>(v, ip, q - h, x, w, r, chunk)) / (2 * h)};
    std::printf("Q=%g chunk=%3d val=%.15g dual.v==val:%d dv %.10g fd %.10g dP %.10g fd %.10g dQ %.10g fd %.10g\n", q, chunk, val,
                g[0].v == val && g[1].v == val && g[2].v == val, g[0].t, fd[0], g[1].t, fd[1], g[2].t, fd[2]);
    for (int k = 0; k < 3; ++k)
      if (!(g[k].v == val) || std::fabs(g[k].t - fd[k]) > (q > 0.6 ? 1e-6 : 1e-4) * std::fabs(fd[k]) + 1e-6) ++bad;
  }
  std::vector<double> xs(n);                                                // separated inputs for the path, as check_path
  xx = 0; for (int t = 0; t < n; ++t) { xx += 0.7 * (0.5 + 1.5 * u()); xs[t] = xx; }
  xs[11] = xs[10]; xs[12] = xs[10];
  for (int t = 100; t < n; ++t) xs[t] += 7000.0;
  const std::vector<double> seq = path_model<2>(M, xs, z, n);
  if (seq[11] != seq[10] || seq[12] != seq[10]) ++bad;
  for (int chunk : {1, 7, 64, 200}) {
    const std::vector<double> f = path_model<2>(M, xs, z, chunk);
    double err = 0; for (int t = 0; t < n; ++t) err = std::max(err, std::fabs(f[t] - seq[t]));
    std::printf("Q=%g chunk=%3d path err %.3g\n", q, chunk, err);
    if (!(err <= 1e-12 * std::sqrt(v))) ++bad;
  }
  return bad;
}
int main() {
  int bad = check<1>() + check<2>() + check<3>();
  bad += check_osc(0.51) + check_osc(2.0) + check_osc(50.0);
  bad += check_chol<1>() + check_chol<2>() + check_chol<3>() + check_path<1>() + check_path<2>() + check_path<3>();
  std::printf("bad=%d\n", bad);
  return bad != 0;
}
