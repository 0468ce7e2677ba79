// lmm_statespace.h -- the per-point arithmetic of the state-space (Kalman / RTS) path for Matern and SHO latents over a one-dimensional
// input (include/lmm_hip.h "state space").  Everything is templated on the state dimension D (Matern12 / 32 / 52: 1 / 2 /
// 3; SHO: 2) and on the latent's model (SSModel<D>: Matern; SSOsc: the damped oscillator), and fully unrolled, so every matrix lives in
// registers.  The functions are __host__ __device__: lmm_kernels_ss.hip runs them on the
// GPU, and a host build of the same text can be stepped through on the CPU.
//
// Model: F is the companion matrix of (s + lam)^D, N = F + lam I is nilpotent (N^D = 0), A(dt) = exp(-lam dt) (I + N dt + N^2 dt^2 / 2),
// Q(dt) = Pinf - A Pinf A', prior state N(0, Pinf), observation h = e_1'.
// The oscillator (SSOsc, D = 2): F = [0 1; -w0^2 -w0 / Q] with w0 = 2 pi / P, a = w0 / (2 Q), eta = w0 sqrt(1 - 1 / (4 Q^2)); N = F + a I
// has N^2 = -eta^2 I, so A(dt) = exp(-a dt) (cos(eta dt) I + sin(eta dt) / eta N); Pinf = diag(v, w0^2 v), Q(dt) and h as above.  Only
// A(dt) differs between the models: everything from ss_fwd_element down is one text, instantiated on the model's type.
//
// The forward (filtering) arithmetic is also templated on its scalar type Sc.  Sc = double (the default) is the arithmetic of the value;
// Sc = SSDual carries one tangent beside every value, which makes the same text the forward-mode derivative of the filter with respect
// to one kernel parameter (the gradient of the log density with respect to variance and lengthscale).  The inputs x, the spacings dt,
// the noise w and the data r stay plain doubles, and the branches (`first`, w = +Inf) do not depend on the parameters.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define SS_HD __host__ __device__ __forceinline__

// value and tangent of one scalar; comparisons look at the value
struct SSDual {
  double v, t;
  SSDual() = default;
  SS_HD SSDual(double v_) : v(v_), t(0.0) {}
  SS_HD SSDual(double v_, double t_) : v(v_), t(t_) {}
};
SS_HD SSDual operator-(SSDual a) { return SSDual(-a.v, -a.t); }
SS_HD SSDual operator+(SSDual a, SSDual b) { return SSDual(a.v + b.v, a.t + b.t); }
SS_HD SSDual operator+(SSDual a, double b) { return SSDual(a.v + b, a.t); }
SS_HD SSDual operator+(double a, SSDual b) { return SSDual(a + b.v, b.t); }
SS_HD SSDual operator-(SSDual a, SSDual b) { return SSDual(a.v - b.v, a.t - b.t); }
SS_HD SSDual operator-(SSDual a, double b) { return SSDual(a.v - b, a.t); }
SS_HD SSDual operator-(double a, SSDual b) { return SSDual(a - b.v, -b.t); }
SS_HD SSDual operator*(SSDual a, SSDual b) { return SSDual(a.v * b.v, a.t * b.v + a.v * b.t); }
SS_HD SSDual operator*(SSDual a, double b) { return SSDual(a.v * b, a.t * b); }
SS_HD SSDual operator*(double a, SSDual b) { return SSDual(a * b.v, a * b.t); }
SS_HD SSDual operator/(SSDual a, SSDual b) { const double q = a.v / b.v; return SSDual(q, (a.t - q * b.t) / b.v); }
SS_HD SSDual operator/(SSDual a, double b) { return SSDual(a.v / b, a.t / b); }
SS_HD SSDual operator/(double a, SSDual b) { const double q = a / b.v; return SSDual(q, -q * b.t / b.v); }
SS_HD SSDual& operator+=(SSDual& a, SSDual b) { a.v += b.v; a.t += b.t; return a; }
SS_HD SSDual& operator+=(SSDual& a, double b) { a.v += b; return a; }
SS_HD SSDual& operator-=(SSDual& a, SSDual b) { a.v -= b.v; a.t -= b.t; return a; }
SS_HD SSDual& operator-=(SSDual& a, double b) { a.v -= b; return a; }
SS_HD SSDual exp(SSDual a) { const double e = exp(a.v); return SSDual(e, e * a.t); }
SS_HD SSDual log(SSDual a) { return SSDual(log(a.v), a.t / a.v); }
SS_HD SSDual sqrt(SSDual a) { const double r = sqrt(a.v); return SSDual(r, 0.5 * a.t / r); }
// (sin x, cos x) of one argument
SS_HD void ss_sincos(double x, double& s, double& c) { s = sin(x); c = cos(x); }
SS_HD void ss_sincos(SSDual x, SSDual& s, SSDual& c) {
  double sv, cv;
  ss_sincos(x.v, sv, cv);
  s = SSDual(sv, cv * x.t); c = SSDual(cv, -sv * x.t);
}
SS_HD bool operator<(SSDual a, SSDual b) { return a.v < b.v; }
SS_HD bool operator>(SSDual a, SSDual b) { return a.v > b.v; }
SS_HD bool operator<=(SSDual a, SSDual b) { return a.v <= b.v; }
SS_HD bool operator>=(SSDual a, SSDual b) { return a.v >= b.v; }
SS_HD bool operator==(SSDual a, SSDual b) { return a.v == b.v; }
SS_HD bool operator!=(SSDual a, SSDual b) { return a.v != b.v; }

// ---- index arithmetic shared by the kernels of lmm_kernels_ss.hip ------------------------------------------------------------------
// [t0, t1): the run of thread j over n items, `chunk` per thread
struct SSRange { long long t0, t1; };
SS_HD SSRange ss_chunk_range(long long j, int chunk, int n) {
  const long long t0 = j * chunk;
  return SSRange{t0, t0 + chunk < n ? t0 + chunk : n};
}

// lo + #{t in [lo, hi) : x_t <= s} (ss_count_lt: x_t < s) for non-decreasing x, by binary search: at most ceil(log2(hi - lo + 1)) probes
SS_HD int ss_count_le(const double* x, int lo, int hi, double s) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x[mid] <= s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
SS_HD int ss_count_lt(const double* x, int lo, int hi, double s) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// packed index of the symmetric entry (i, j), i <= j, behind the D mean components of a stored state
__host__ __device__ constexpr int ss_sym_at(int D, int i, int j) { return D + i * D - i * (i - 1) / 2 + (j - i); }

// The stored state of point t (mean, then the packed upper triangle of the covariance) into m, P: component c lies at
// st[c comp_stride + t point_stride] ((n, 1): component-major; (1, D + D (D + 1) / 2): point-major)
template <int D>
SS_HD void ss_load_state(const double* st, size_t comp_stride, size_t point_stride, long long t, double m[D], double P[D][D]) {
  const double* f = st + (size_t)t * point_stride;
  for (int i = 0; i < D; ++i) {
    m[i] = f[(size_t)i * comp_stride];
    for (int k = i; k < D; ++k) P[i][k] = P[k][i] = f[(size_t)ss_sym_at(D, i, k) * comp_stride];
  }
}
// its counterpart: m and the upper triangle of P become the stored state of point t
template <int D>
SS_HD void ss_store_state(double* st, size_t comp_stride, size_t point_stride, long long t, const double m[D], const double P[D][D]) {
  double* f = st + (size_t)t * point_stride;
  for (int i = 0; i < D; ++i) {
    f[(size_t)i * comp_stride] = m[i];
    for (int k = i; k < D; ++k) f[(size_t)ss_sym_at(D, i, k) * comp_stride] = P[i][k];
  }
}

template <int D, typename Sc = double>
struct SSModel {
  Sc lam;
  Sc N[D][D], N2[D][D], Pinf[D][D];
};

// lam = sqrt(2 nu) / lengthscale and the stationary covariance of (f, f', f'') for variance v
template <int D, typename Sc = double>
SS_HD void ss_model(Sc var, Sc inv_ls, SSModel<D, Sc>& M) {
  const Sc lam = (D == 1 ? 1.0 : D == 2 ? 1.7320508075688772 : 2.23606797749979) * inv_ls;
  M.lam = lam;
  Sc F[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) { F[i][j] = (j == i + 1) ? 1.0 : 0.0; M.Pinf[i][j] = 0.0; }
  if (D == 1) F[0][0] = -lam;
  if (D == 2) { F[D - 1][0] = -lam * lam; F[D - 1][D - 1] = -2.0 * lam; }
  if (D == 3) { F[D - 1][0] = -lam * lam * lam; F[D - 1][D == 3 ? 1 : 0] = -3.0 * lam * lam; F[D - 1][D - 1] = -3.0 * lam; }
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) M.N[i][j] = F[i][j] + (i == j ? lam : 0.0);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      Sc s = 0.0;
      for (int k = 0; k < D; ++k) s += M.N[i][k] * M.N[k][j];
      M.N2[i][j] = s;
    }
  const Sc l2 = lam * lam;
  M.Pinf[0][0] = var;
  if (D == 2) M.Pinf[D - 1][D - 1] = l2 * var;
  if (D == 3) {
    M.Pinf[0][D - 1] = M.Pinf[D - 1][0] = -l2 * var / 3.0;
    M.Pinf[D == 3 ? 1 : 0][D == 3 ? 1 : 0] = l2 * var / 3.0;
    M.Pinf[D - 1][D - 1] = l2 * l2 * var;
  }
}

// Q = Pinf - A Pinf A' (symmetric by construction)
template <int D, typename Sc = double>
SS_HD void ss_stationary_Q(const Sc Pinf[D][D], const Sc A[D][D], Sc Q[D][D]) {
  Sc T[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      Sc s = 0.0;
      for (int k = 0; k < D; ++k) s += A[i][k] * Pinf[k][j];
      T[i][j] = s;
    }
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) {
      Sc s = 0.0;
      for (int k = 0; k < D; ++k) s += T[i][k] * A[j][k];
      Q[i][j] = Q[j][i] = Pinf[i][j] - s;
    }
}

// A(dt) and Q(dt); dt = 0 gives A = I and Q = 0 exactly
template <int D, typename Sc = double>
SS_HD void ss_AQ(const SSModel<D, Sc>& M, double dt, Sc A[D][D], Sc Q[D][D]) {
  const Sc e = exp(-M.lam * dt);
  const double h = 0.5 * dt * dt;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) A[i][j] = e * ((i == j ? 1.0 : 0.0) + M.N[i][j] * dt + (D > 2 ? M.N2[i][j] * h : 0.0));
  ss_stationary_Q<D, Sc>(M.Pinf, A, Q);
}

// ---- the stochastically driven damped harmonic oscillator (SHO; underdamped, Q > 1 / 2) --------------------------------------------
template <typename Sc = double>
struct SSOsc {
  Sc a, eta;
  Sc N[2][2], Pinf[2][2];
};

// inv_p = 1 / P (the undamped period), q the quality factor.  1 - 1 / (4 q^2) is taken as (2 q - 1) (2 q + 1) / (4 q^2), which keeps
// its relative accuracy as q -> 1 / 2: eta = a sqrt((2 q - 1) (2 q + 1)).
template <typename Sc = double>
SS_HD void ss_osc_model(Sc var, Sc inv_p, Sc q, SSOsc<Sc>& M) {
  const Sc w0 = 6.283185307179586 * inv_p;
  const Sc a = w0 / (2.0 * q);
  const Sc w2 = w0 * w0;
  M.a = a;
  M.eta = a * sqrt((2.0 * q - 1.0) * (2.0 * q + 1.0));
  M.N[0][0] = a; M.N[0][1] = 1.0; M.N[1][0] = -w2; M.N[1][1] = -a;
  M.Pinf[0][0] = var; M.Pinf[0][1] = 0.0; M.Pinf[1][0] = 0.0; M.Pinf[1][1] = w2 * var;
}

// A(dt) and Q(dt) of the oscillator; dt = 0 gives e = c = 1 and s = 0, so A = I and Q = 0 exactly
template <int D, typename Sc = double>
SS_HD void ss_AQ(const SSOsc<Sc>& M, double dt, Sc A[D][D], Sc Q[D][D]) {
  static_assert(D == 2, "the oscillator has a two-dimensional state");
  const Sc e = exp(-M.a * dt);
  Sc sn, cs;
  ss_sincos(M.eta * dt, sn, cs);
  const Sc c = e * cs, s = e * sn / M.eta;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) A[i][j] = (i == j ? c : Sc(0.0)) + s * M.N[i][j];
  ss_stationary_Q<D, Sc>(M.Pinf, A, Q);
}

// ---- the sum of two models inside one latent (DESIGN.md 4.18 "Sum latents") --------------------------------------------------------
// f = f_a + f_b with independent f_a, f_b of models MA, MB is again a state-space model: the state s = (s_a, s_b) has dimension
// D = D_a + D_b, block-diagonal A, Q, Pinf and F, and the observation e_1' s_a + e_1' s_b.  Everything below ss_fwd_element is written
// against h = e_1', so the state is held in the basis s' = T s with T = I + e_1 e_{D_a+1}': its first component is f_a + f_b and every
// other component is the one of s.  T and T^-1 = I - e_1 e_{D_a+1}' differ from I in one entry: T X adds row D_a + 1 of X to row 1,
// X T' adds column D_a + 1 to column 1, and X T^-1 takes column 1 off column D_a + 1.
template <typename M> struct SSDimOf;
template <int D, typename Sc> struct SSDimOf<SSModel<D, Sc>> { static constexpr int value = D; };
template <typename Sc> struct SSDimOf<SSOsc<Sc>> { static constexpr int value = 2; };

template <typename MA, typename MB, typename Sc = double>
struct SSSum {
  static constexpr int DA = SSDimOf<MA>::value, DB = SSDimOf<MB>::value;
  MA a;
  MB b;
  Sc Pinf[DA + DB][DA + DB];
};

// X = T blkdiag(Xa, Xb) T' (COV: a covariance) or T blkdiag(Xa, Xb) T^-1 (a transition)
template <int DA, int DB, bool COV, typename Sc>
SS_HD void ss_sum_basis(const Sc Xa[DA][DA], const Sc Xb[DB][DB], Sc X[DA + DB][DA + DB]) {
  constexpr int D = DA + DB;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      if (i < DA && j < DA) X[i][j] = Xa[i][j];
      else if (i >= DA && j >= DA) X[i][j] = Xb[i - DA][j - DA];
      else X[i][j] = 0.0;
    }
  for (int j = 0; j < D; ++j) X[0][j] += X[DA][j];
  for (int i = 0; i < D; ++i) {
    if (COV) X[i][0] += X[i][DA];
    else X[i][DA] -= X[i][0];
  }
}

template <typename MA, typename MB, typename Sc>
SS_HD void ss_sum_model(const MA& a, const MB& b, SSSum<MA, MB, Sc>& M) {
  M.a = a; M.b = b;
  ss_sum_basis<SSSum<MA, MB, Sc>::DA, SSSum<MA, MB, Sc>::DB, true, Sc>(a.Pinf, b.Pinf, M.Pinf);
}

// A(dt) and Q(dt) of the sum from its terms' own: A' = T blkdiag(A_a, A_b) T^-1, and Q' = Pinf' - A' Pinf' A'' taken block by block,
// T blkdiag(Q_a, Q_b) T' with Q_c = Pinf_c - A_c Pinf_c A_c' (the same matrix; the blocks' zeros stay exact and the products are
// those of the terms).  dt = 0: A_a = A_b = I and Q_a = Q_b = 0 exactly, so A' = I (its entry (1, D_a + 1) is 1 - 1) and Q' = 0 exactly.
template <int D, typename Sc = double, typename MA, typename MB>
SS_HD void ss_AQ(const SSSum<MA, MB, Sc>& M, double dt, Sc A[D][D], Sc Q[D][D]) {
  constexpr int DA = SSSum<MA, MB, Sc>::DA, DB = SSSum<MA, MB, Sc>::DB;
  static_assert(D == DA + DB, "the sum's state dimension is that of its terms together");
  Sc Aa[DA][DA], Qa[DA][DA], Ab[DB][DB], Qb[DB][DB];
  ss_AQ<DA, Sc>(M.a, dt, Aa, Qa);
  ss_AQ<DB, Sc>(M.b, dt, Ab, Qb);
  ss_sum_basis<DA, DB, false, Sc>(Aa, Ab, A);
  ss_sum_basis<DA, DB, true, Sc>(Qa, Qb, Q);
}

template <int D, typename Sc = double>
SS_HD void ss_mm(const Sc X[D][D], const Sc Y[D][D], Sc Z[D][D]) {      // Z = X Y
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      Sc s = 0.0;
      for (int k = 0; k < D; ++k) s += X[i][k] * Y[k][j];
      Z[i][j] = s;
    }
}
template <int D, typename Sc = double>
SS_HD void ss_mmt(const Sc X[D][D], const Sc Y[D][D], Sc Z[D][D]) {     // Z = X Y'
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      Sc s = 0.0;
      for (int k = 0; k < D; ++k) s += X[i][k] * Y[j][k];
      Z[i][j] = s;
    }
}
template <int D, typename Sc = double>
SS_HD void ss_sym(Sc X[D][D]) {
  for (int i = 0; i < D; ++i)
    for (int j = i + 1; j < D; ++j) X[i][j] = X[j][i] = 0.5 * (X[i][j] + X[j][i]);
}

// X^-1 of a general D x D matrix by cofactors (relative accuracy is invariant under the diagonal scalings that separate f, f', f'').
// D = 4 (a sum model): the adjugate through the twelve 2 x 2 minors of rows (0, 1) and rows (2, 3), not a block inverse.  The
// matrices inverted here are I + C J with C, J positive semi-definite, whose entries scale like X_ij ~ s_i / s_j with s = (1, lam,
// lam^2, ..) per block.  Every product in a minor, in a cofactor and in the determinant takes one entry from each of its rows and
// columns, so all the terms of one sum carry the same power of the s_i: the scalings factor out of every sum and the rounding is
// that of the well-scaled matrix.  A block inverse divides by a Schur complement of the leading block instead, which is exact in
// the same sense only while that block stays well conditioned, and costs a second 2 x 2 inverse on the critical path.
template <int D, typename Sc = double>
SS_HD void ss_inv(const Sc X[D][D], Sc Y[D][D]) {
  if constexpr (D == 4) {
    const Sc s0 = X[0][0] * X[1][1] - X[1][0] * X[0][1], s1 = X[0][0] * X[1][2] - X[1][0] * X[0][2], s2 = X[0][0] * X[1][3] - X[1][0] * X[0][3];
    const Sc s3 = X[0][1] * X[1][2] - X[1][1] * X[0][2], s4 = X[0][1] * X[1][3] - X[1][1] * X[0][3], s5 = X[0][2] * X[1][3] - X[1][2] * X[0][3];
    const Sc c5 = X[2][2] * X[3][3] - X[3][2] * X[2][3], c4 = X[2][1] * X[3][3] - X[3][1] * X[2][3], c3 = X[2][1] * X[3][2] - X[3][1] * X[2][2];
    const Sc c2 = X[2][0] * X[3][3] - X[3][0] * X[2][3], c1 = X[2][0] * X[3][2] - X[3][0] * X[2][2], c0 = X[2][0] * X[3][1] - X[3][0] * X[2][1];
    const Sc r = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    Y[0][0] = (X[1][1] * c5 - X[1][2] * c4 + X[1][3] * c3) * r;
    Y[0][1] = (X[0][2] * c4 - X[0][1] * c5 - X[0][3] * c3) * r;
    Y[0][2] = (X[3][1] * s5 - X[3][2] * s4 + X[3][3] * s3) * r;
    Y[0][3] = (X[2][2] * s4 - X[2][1] * s5 - X[2][3] * s3) * r;
    Y[1][0] = (X[1][2] * c2 - X[1][0] * c5 - X[1][3] * c1) * r;
    Y[1][1] = (X[0][0] * c5 - X[0][2] * c2 + X[0][3] * c1) * r;
    Y[1][2] = (X[3][2] * s2 - X[3][0] * s5 - X[3][3] * s1) * r;
    Y[1][3] = (X[2][0] * s5 - X[2][2] * s2 + X[2][3] * s1) * r;
    Y[2][0] = (X[1][0] * c4 - X[1][1] * c2 + X[1][3] * c0) * r;
    Y[2][1] = (X[0][1] * c2 - X[0][0] * c4 - X[0][3] * c0) * r;
    Y[2][2] = (X[3][0] * s4 - X[3][1] * s2 + X[3][3] * s0) * r;
    Y[2][3] = (X[2][1] * s2 - X[2][0] * s4 - X[2][3] * s0) * r;
    Y[3][0] = (X[1][1] * c1 - X[1][0] * c3 - X[1][2] * c0) * r;
    Y[3][1] = (X[0][0] * c3 - X[0][1] * c1 + X[0][2] * c0) * r;
    Y[3][2] = (X[3][1] * s1 - X[3][0] * s3 - X[3][2] * s0) * r;
    Y[3][3] = (X[2][0] * s3 - X[2][1] * s1 + X[2][2] * s0) * r;
    return;
  }
  if (D == 1) { Y[0][0] = 1.0 / X[0][0]; return; }
  if (D == 2) {
    const Sc a = X[0][0], b = X[0][D - 1], c = X[D - 1][0], d = X[D - 1][D - 1];
    const Sc r = 1.0 / (a * d - b * c);
    Y[0][0] = d * r; Y[0][D - 1] = -b * r; Y[D - 1][0] = -c * r; Y[D - 1][D - 1] = a * r;
    return;
  }
  Sc Cf[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      const int i1 = (i + 1) % D, i2 = (i + 2) % D, j1 = (j + 1) % D, j2 = (j + 2) % D;
      Cf[i][j] = X[i1][j1] * X[i2][j2] - X[i1][j2] * X[i2][j1];      // cofactor (cyclic indices carry the sign)
    }
  Sc det = 0.0;
  for (int j = 0; j < D; ++j) det += X[0][j] * Cf[0][j];
  const Sc r = 1.0 / det;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) Y[i][j] = Cf[j][i] * r;
}

// X^-1 of a symmetric positive definite matrix through its Cholesky factor
template <int D>
SS_HD void ss_inv_spd(const double X[D][D], double Y[D][D]) {
  double L[D][D], W[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) { L[i][j] = 0.0; W[i][j] = 0.0; }
  for (int j = 0; j < D; ++j) {
    double s = X[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    const double dj = sqrt(s);
    L[j][j] = dj;
    for (int i = j + 1; i < D; ++i) {
      double t = X[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / dj;
    }
  }
  for (int j = 0; j < D; ++j) {               // W = L^-1 (lower)
    W[j][j] = 1.0 / L[j][j];
    for (int i = j + 1; i < D; ++i) {
      double t = 0.0;
      for (int k = j; k < i; ++k) t -= L[i][k] * W[k][j];
      W[i][j] = t / L[i][i];
    }
  }
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) {
      double s = 0.0;
      for (int k = j; k < D; ++k) s += W[k][i] * W[k][j];
      Y[i][j] = Y[j][i] = s;
    }
}

// ---- forward (filtering) elements of Sarkka & Garcia-Fernandez, "Temporal parallelization of Bayesian smoothers" ------------------
template <int D, typename Sc = double>
struct SSFwd { Sc A[D][D], b[D], C[D][D], eta[D], J[D][D]; };

// The element of one point.  first: the prior takes the place of the transition (A = 0, Q = Pinf).  w = +Inf: unobserved.
template <int D, typename Sc = double, typename Mod>
SS_HD void ss_fwd_element(const Mod& M, bool first, double dt, double w, double r, SSFwd<D, Sc>& e) {
  Sc A[D][D], Q[D][D];
  if (first) {
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) { A[i][j] = 0.0; Q[i][j] = M.Pinf[i][j]; }
  } else ss_AQ<D, Sc>(M, dt, A, Q);
  if (!(w < INFINITY)) {
    for (int i = 0; i < D; ++i) {
      e.b[i] = 0.0; e.eta[i] = 0.0;
      for (int j = 0; j < D; ++j) { e.A[i][j] = A[i][j]; e.C[i][j] = Q[i][j]; e.J[i][j] = 0.0; }
    }
    return;
  }
  const Sc Sinv = 1.0 / (Q[0][0] + w);
  for (int i = 0; i < D; ++i) {
    const Sc K = Q[i][0] * Sinv;
    e.b[i] = K * r;
    e.eta[i] = A[0][i] * r * Sinv;
    for (int j = 0; j < D; ++j) {
      e.A[i][j] = A[i][j] - K * A[0][j];
      e.C[i][j] = Q[i][j] - K * Q[0][j];
      e.J[i][j] = A[0][i] * A[0][j] * Sinv;
    }
  }
}

// out = a (.) b with a the earlier run; out may alias a or b
template <int D, typename Sc = double>
SS_HD void ss_fwd_combine(const SSFwd<D, Sc>& a, const SSFwd<D, Sc>& b, SSFwd<D, Sc>& out) {
  Sc T[D][D], Ti[D][D], Mx[D][D], Mp[D][D], X[D][D];
  ss_mm<D, Sc>(a.C, b.J, T);
  for (int i = 0; i < D; ++i) T[i][i] += 1.0;
  ss_inv<D, Sc>(T, Ti);
  ss_mm<D, Sc>(b.A, Ti, Mx);                      // M = A_j (I + C_i J_j)^-1
  ss_mm<D, Sc>(Ti, a.A, X);                       // M' = A_i' (I + J_j C_i)^-1 = ((I + C_i J_j)^-1 A_i)'
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) Mp[i][j] = X[j][i];
  SSFwd<D, Sc> o;
  ss_mm<D, Sc>(Mx, a.A, o.A);
  Sc u[D], v[D];
  for (int i = 0; i < D; ++i) {
    Sc s = a.b[i], t = b.eta[i];
    for (int k = 0; k < D; ++k) { s += a.C[i][k] * b.eta[k]; t -= b.J[i][k] * a.b[k]; }
    u[i] = s; v[i] = t;
  }
  for (int i = 0; i < D; ++i) {
    Sc s = b.b[i], t = a.eta[i];
    for (int k = 0; k < D; ++k) { s += Mx[i][k] * u[k]; t += Mp[i][k] * v[k]; }
    o.b[i] = s; o.eta[i] = t;
  }
  ss_mm<D, Sc>(Mx, a.C, X);
  ss_mmt<D, Sc>(X, b.A, o.C);
  ss_mm<D, Sc>(Mp, b.J, X);
  ss_mm<D, Sc>(X, a.A, o.J);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) { o.C[i][j] += b.C[i][j]; o.J[i][j] += a.J[i][j]; }
  ss_sym<D, Sc>(o.C); ss_sym<D, Sc>(o.J);
  out = o;
}

// One step of the ordinary Kalman filter: (m, P) at the previous point -> (m, P) at this one.  Returns the point's log-density term
// (0 for an unobserved point, which takes the predict step only).
template <int D, typename Sc = double, typename Mod>
SS_HD Sc ss_filter_step(const Mod& M, double dt, double w, double r, Sc m[D], Sc P[D][D]) {
  Sc A[D][D], Q[D][D], T[D][D], mp[D];
  ss_AQ<D, Sc>(M, dt, A, Q);
  ss_mm<D, Sc>(A, P, T);
  for (int i = 0; i < D; ++i) {
    Sc s = 0.0;
    for (int k = 0; k < D; ++k) s += A[i][k] * m[k];
    mp[i] = s;
    for (int j = i; j < D; ++j) {
      Sc q = Q[i][j];
      for (int k = 0; k < D; ++k) q += T[i][k] * A[j][k];
      P[i][j] = P[j][i] = q;
    }
  }
  for (int i = 0; i < D; ++i) m[i] = mp[i];
  if (!(w < INFINITY)) return Sc(0.0);
  const Sc S = P[0][0] + w, Sinv = 1.0 / S, e = r - m[0];
  Sc K[D], p0[D];
  for (int i = 0; i < D; ++i) { p0[i] = P[0][i]; K[i] = P[i][0] * Sinv; }
  for (int i = 0; i < D; ++i) {
    m[i] += K[i] * e;
    for (int j = 0; j < D; ++j) P[i][j] -= K[i] * p0[j];
  }
  ss_sym<D, Sc>(P);
  return -0.5 * (log(6.283185307179586 * S) + e * e * Sinv);
}

// The element of the first of a run of points whose predecessor is not the prior but a given state (m0, P0) lying dt in front of it
// (DESIGN.md 4.18 "Appending observations"): ss_fwd_element's `first` with the prediction m- = A m0, P- = A P0 A' + Q in the prior's
// place, i.e. A = 0, b = m- + K (r - m-[0]), C = P- - K P-[0, :], eta = 0, J = 0; w = +Inf: b = m-, C = P-.  (b, C) is what
// ss_filter_step makes of (m0, P0), in its arithmetic; dt = 0 keeps (m0, P0) exactly through the prediction.
template <int D, typename Mod>
SS_HD void ss_fwd_element_from(const Mod& M, double dt, const double m0[D], const double P0[D][D], double w, double r, SSFwd<D>& e) {
  double m[D], P[D][D];
  for (int i = 0; i < D; ++i) {
    m[i] = m0[i];
    for (int j = 0; j < D; ++j) P[i][j] = P0[i][j];
  }
  ss_filter_step<D>(M, dt, w, r, m, P);
  for (int i = 0; i < D; ++i) {
    e.b[i] = m[i]; e.eta[i] = 0.0;
    for (int j = 0; j < D; ++j) { e.A[i][j] = 0.0; e.C[i][j] = P[i][j]; e.J[i][j] = 0.0; }
  }
}

// ---- backward (smoothing) elements -----------------------------------------------------------------------------------------------
template <int D>
struct SSBwd { double E[D][D], g[D], L[D][D]; };

// The element of a point with filtered state (m, P) whose successor lies dt further; last: the final point (0, m, P).
template <int D, typename Mod>
SS_HD void ss_bwd_element(const Mod& M, bool last, double dt, const double m[D], const double P[D][D], SSBwd<D>& e) {
  if (last) {
    for (int i = 0; i < D; ++i) {
      e.g[i] = m[i];
      for (int j = 0; j < D; ++j) { e.E[i][j] = 0.0; e.L[i][j] = P[i][j]; }
    }
    return;
  }
  double A[D][D], Q[D][D], T[D][D], Pp[D][D], Pi[D][D], X[D][D];
  ss_AQ<D>(M, dt, A, Q);
  ss_mm<D>(A, P, T);                          // A P
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) {
      double q = Q[i][j];
      for (int k = 0; k < D; ++k) q += T[i][k] * A[j][k];
      Pp[i][j] = Pp[j][i] = q;
    }
  ss_inv_spd<D>(Pp, Pi);
  for (int i = 0; i < D; ++i)                 // E = (A P)' Pp^-1
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
      for (int k = 0; k < D; ++k) s += T[k][i] * Pi[k][j];
      e.E[i][j] = s;
    }
  ss_mm<D>(e.E, T, X);                        // E A P
  double Am[D];
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += A[i][k] * m[k];
    Am[i] = s;
  }
  for (int i = 0; i < D; ++i) {
    double s = m[i];
    for (int k = 0; k < D; ++k) s -= e.E[i][k] * Am[k];
    e.g[i] = s;
    for (int j = 0; j < D; ++j) e.L[i][j] = P[i][j] - X[i][j];
  }
  ss_sym<D>(e.L);
}

// out = a (.) b with a the earlier run: (E_a E_b, E_a g_b + g_a, E_a L_b E_a' + L_a); out may alias a or b
template <int D>
SS_HD void ss_bwd_combine(const SSBwd<D>& a, const SSBwd<D>& b, SSBwd<D>& out) {
  SSBwd<D> o;
  double X[D][D];
  ss_mm<D>(a.E, b.E, o.E);
  ss_mm<D>(a.E, b.L, X);
  ss_mmt<D>(X, a.E, o.L);
  for (int i = 0; i < D; ++i) {
    double s = a.g[i];
    for (int k = 0; k < D; ++k) s += a.E[i][k] * b.g[k];
    o.g[i] = s;
    for (int j = 0; j < D; ++j) o.L[i][j] += a.L[i][j];
  }
  ss_sym<D>(o.L);
  out = o;
}

// One step of the Rauch-Tung-Striebel recursion: the smoothed state (ms, Ps) of the successor -> that of the point with element e.
template <int D>
SS_HD void ss_rts_step(const SSBwd<D>& e, double ms[D], double Ps[D][D]) {
  double X[D][D], Y[D][D], t[D];
  ss_mm<D>(e.E, Ps, X);
  ss_mmt<D>(X, e.E, Y);
  for (int i = 0; i < D; ++i) {
    double s = e.g[i];
    for (int k = 0; k < D; ++k) s += e.E[i][k] * ms[k];
    t[i] = s;
  }
  for (int i = 0; i < D; ++i) {
    ms[i] = t[i];
    for (int j = 0; j < D; ++j) Ps[i][j] = Y[i][j] + e.L[i][j];
  }
  ss_sym<D>(Ps);
}

// ---- the posterior at a new input (DESIGN.md 4.18 "Posterior object") ---------------------------------------------------------------
// The posterior state at an input s that lies d1 behind training point k - 1 and d2 in front of training point k.  By the Markov
// property it needs the FILTERED state of k - 1 (in: m, P) and the SMOOTHED state of k (ms, Ps) and nothing else: one predict step
// over d1 (the filter's step at an unobserved point; d1 = 0 keeps the state exactly), then one RTS step back over d2.  has_prev =
// false (s in front of every training point): the prior takes the place of the prediction and m, P are not read.  has_next = false
// (s behind every training point): the prediction is the answer and ms, Ps are not read.  Out: m, P.
template <int D, typename Mod>
SS_HD void ss_interp(const Mod& M, bool has_prev, double d1, bool has_next, double d2, double m[D], double P[D][D], const double ms[D],
                     const double Ps[D][D]) {
  if (!has_prev) {
    for (int i = 0; i < D; ++i) {
      m[i] = 0.0;
      for (int j = 0; j < D; ++j) P[i][j] = M.Pinf[i][j];
    }
  } else ss_filter_step<D>(M, d1, INFINITY, 0.0, m, P);
  if (!has_next) return;
  SSBwd<D> el;
  ss_bwd_element<D>(M, false, d2, m, P, el);
  for (int i = 0; i < D; ++i) {
    m[i] = ms[i];
    for (int j = 0; j < D; ++j) P[i][j] = Ps[i][j];
  }
  ss_rts_step<D>(el, m, P);
}

// ---- gradients with respect to locations (DESIGN.md 4.18 "Gradients with respect to locations") --------------------------------------
// The drift F of the model's SDE, dA / dt = F A: N - lam I (Matern), N - a I (oscillator)
template <int D>
SS_HD void ss_drift(const SSModel<D>& M, double F[D][D]) {
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) F[i][j] = M.N[i][j] - (i == j ? M.lam : 0.0);
}
template <int D>
SS_HD void ss_drift(const SSOsc<double>& M, double F[D][D]) {
  static_assert(D == 2, "the oscillator has a two-dimensional state");
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) F[i][j] = M.N[i][j] - (i == j ? M.a : 0.0);
}
// (A sum, SSSum, has none yet: its drift would be T blkdiag(F_a, F_b) T^-1, and gradients with respect to locations refuse sum latents.)

// g = d lml / d dt of ONE transition: the spacing dt between point t - 1, with FILTERED state (m, P), and point t, with SMOOTHED state
// (ms, Ps).  lml depends on dt only through the predicted state mp = A m, Pp = A P A' + Q of point t, with d mp / d dt = F mp and
// d Pp / d dt = F (Pp - Pinf) + (Pp - Pinf) F' (dA / dt = F A and dQ / dt = -F (A Pinf A') - (A Pinf A') F'), and
// d lml / d mp = Pp^-1 delta, d lml / d Pp = Pp^-1 (delta delta' + Ps - Pp) Pp^-1 / 2 with delta = ms - mp (Fisher's identity), so
//   g = (Pp^-1 delta)' F mp + tr(Pp^-1 (delta delta' + Ps - Pp) Pp^-1 F (Pp - Pinf)).
// The first lines are those of ss_bwd_element, which the smoother evaluates beside this for the same transition.
template <int D, typename Mod>
SS_HD double ss_input_grad(const Mod& M, double dt, const double m[D], const double P[D][D], const double ms[D], const double Ps[D][D]) {
  double A[D][D], Q[D][D], T[D][D], Pp[D][D], Pi[D][D], F[D][D], G[D][D], X[D][D], Y[D][D], mp[D];
  ss_AQ<D>(M, dt, A, Q);
  ss_mm<D>(A, P, T);                          // A P
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) {
      double q = Q[i][j];
      for (int k = 0; k < D; ++k) q += T[i][k] * A[j][k];
      Pp[i][j] = Pp[j][i] = q;
    }
  ss_inv_spd<D>(Pp, Pi);
  ss_drift<D>(M, F);
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += A[i][k] * m[k];
    mp[i] = s;
  }
  for (int i = 0; i < D; ++i)                 // G = delta delta' + Ps - Pp
    for (int j = 0; j < D; ++j) G[i][j] = (ms[i] - mp[i]) * (ms[j] - mp[j]) + (Ps[i][j] - Pp[i][j]);
  double g = 0.0;
  for (int i = 0; i < D; ++i) {
    double s = 0.0, f = 0.0;
    for (int k = 0; k < D; ++k) { s += Pi[i][k] * (ms[k] - mp[k]); f += F[i][k] * mp[k]; }
    g += s * f;
  }
  ss_mm<D>(Pi, G, X);
  ss_mm<D>(X, Pi, Y);                         // Pp^-1 G Pp^-1
  for (int i = 0; i < D; ++i)                 // X = F (Pp - Pinf)
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
      for (int k = 0; k < D; ++k) s += F[i][k] * (Pp[k][j] - M.Pinf[k][j]);
      X[i][j] = s;
    }
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) g += Y[i][j] * X[j][i];
  return g;
}

// The derivative with respect to s of ss_interp's first-component mean and variance at the query s (d d1 / ds = 1, d d2 / ds = -1),
// given ss_interp's OUTPUT (m, P) there.  A mean-square differentiable latent (D >= 2) carries f' as its second state component:
// d E[f(s) | y] / ds = m[1] and d Var[f(s) | y] / ds = 2 P[0][1].
template <int D>
SS_HD void ss_interp_dx_state(const double m[D], const double P[D][D], double& dmu, double& dv) {
  static_assert(D >= 2, "Matern12 has no derivative component: ss_interp_dx_ou");
  dmu = m[D >= 2 ? 1 : 0];
  dv = 2.0 * P[0][D >= 2 ? 1 : 0];
}
// Matern12 (D = 1, the Ornstein-Uhlenbeck process) has no such component; its predict-then-RTS step is differentiated in closed form.
// In: ss_interp's INPUTS (the filtered state (m, P) of point k - 1, the smoothed state (ms, Ps) of point k).  With e1 = exp(-lam d1),
// e2 = exp(-lam d2) and v = Pinf: mp = e1 m, Pp = v + e1^2 (P - v), so d mp = -lam mp and d Pp = -2 lam (Pp - v) (both 0 in front of
// every training point, where the prior stands).  The prediction (mn, Pn) of point k does not depend on s, so with E = Pp e2 / Pn,
// d E = (d Pp + lam Pp) e2 / Pn: d mean = d mp + d E (ms - mn) and d var = d Pp + 2 E d E (Ps - Pn).
SS_HD void ss_interp_dx_ou(const SSModel<1>& M, bool has_prev, double d1, bool has_next, double d2, double m, double P, double ms,
                           double Ps, double& dmu, double& dv) {
  const double v = M.Pinf[0][0], lam = M.lam;
  double mp = 0.0, Pp = v;
  if (has_prev) {
    const double e1 = exp(-lam * d1);
    mp = e1 * m;
    Pp = v + e1 * e1 * (P - v);
  }
  const double dmp = -lam * mp, dPp = -2.0 * lam * (Pp - v);
  if (!has_next) { dmu = dmp; dv = dPp; return; }
  const double e2 = exp(-lam * d2);
  const double mn = e2 * mp, Pn = v + e2 * e2 * (Pp - v);
  const double E = Pp * e2 / Pn, dE = (dPp + lam * Pp) * e2 / Pn;
  dmu = dmp + dE * (ms - mn);
  dv = dPp + 2.0 * E * dE * (Ps - Pn);
}

// ---- sampling: the prior path as an affine scan ------------------------------------------------------------------------------------
// Lower Cholesky factor with non-negative diagonal of a symmetric positive SEMI-definite X (its lower triangle is read).  A pivot that
// is not > 0 gives a zero column (its diagonal and everything below it), so X = 0 gives L = 0 exactly and a Q that rounding has made
// slightly indefinite (Q = Pinf - A Pinf A' is a difference) is served.
template <int D>
SS_HD void ss_chol_psd(const double X[D][D], double L[D][D]) {
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) L[i][j] = 0.0;
  for (int j = 0; j < D; ++j) {
    double s = X[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > 0.0)) continue;
    const double dj = sqrt(s);
    L[j][j] = dj;
    for (int i = j + 1; i < D; ++i) {
      double t = X[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / dj;
    }
  }
}

// UPPER triangular factor with non-negative diagonal, U U' = X, of a symmetric positive semi-definite X (its upper triangle is read):
// the elimination runs from component D down to component 1, the highest derivative first.  A pivot that is not > 0 gives a zero
// column (its diagonal and everything above it), ss_chol_psd's rule.  For the differences L = P - E A P and Q = Pinf - A Pinf A' at a
// small spacing the (1, 1) entry (~ dt^5 for Matern52) is pure rounding: ss_chol_psd pivots on it first and spoils the whole factor,
// this order takes it last, where nothing depends on it (DESIGN.md 4.18 "Sampling from the posterior object").
template <int D>
SS_HD void ss_chol_upper(const double X[D][D], double U[D][D]) {
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) U[i][j] = 0.0;
  for (int j = D - 1; j >= 0; --j) {
    double s = X[j][j];
    for (int k = j + 1; k < D; ++k) s -= U[j][k] * U[j][k];
    if (!(s > 0.0)) continue;
    const double dj = sqrt(s);
    U[j][j] = dj;
    for (int i = 0; i < j; ++i) {
      double t = X[i][j];
      for (int k = j + 1; k < D; ++k) t -= U[i][k] * U[j][k];
      U[i][j] = t / dj;
    }
  }
}

// s -> A s + c
template <int D>
struct SSAff { double A[D][D], c[D]; };

// The element of one point of the prior path s_t = A(dt) s_{t-1} + chol(Q(dt)) zeta_t.  first: (0, chol(Pinf) zeta_0).
template <int D, typename Mod>
SS_HD void ss_aff_element(const Mod& M, bool first, double dt, const double zeta[D], SSAff<D>& e) {
  double Q[D][D], L[D][D];
  if (first) {
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) { e.A[i][j] = 0.0; Q[i][j] = M.Pinf[i][j]; }
  } else ss_AQ<D>(M, dt, e.A, Q);
  ss_chol_psd<D>(Q, L);
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
    for (int k = 0; k <= i; ++k) s += L[i][k] * zeta[k];
    e.c[i] = s;
  }
}

// out = a (.) b with a the earlier run: (A_b A_a, A_b c_a + c_b); out may alias a or b
template <int D>
SS_HD void ss_aff_combine(const SSAff<D>& a, const SSAff<D>& b, SSAff<D>& out) {
  SSAff<D> o;
  ss_mm<D>(b.A, a.A, o.A);
  for (int i = 0; i < D; ++i) {
    double s = b.c[i];
    for (int k = 0; k < D; ++k) s += b.A[i][k] * a.c[k];
    o.c[i] = s;
  }
  out = o;
}

// One step of the path: the state s of the previous point -> that of the point with element e
template <int D>
SS_HD void ss_aff_step(const SSAff<D>& e, double s[D]) {
  double t[D];
  for (int i = 0; i < D; ++i) {
    double v = e.c[i];
    for (int k = 0; k < D; ++k) v += e.A[i][k] * s[k];
    t[i] = v;
  }
  for (int i = 0; i < D; ++i) s[i] = t[i];
}

// ---- sampling from the posterior object (DESIGN.md 4.18 "Sampling from the posterior object") ---------------------------------------
// Given the data the states of a window of inputs are a Markov chain that runs backwards: s_j | s_{j+1}, y = N(g_j + E_j s_{j+1}, L_j)
// with (E_j, g_j, L_j) the smoother's element of point j (ss_bwd_element on its FILTERED state (m, P) and the spacing dt to its
// successor).  The element of the affine recursion s_j = E_j s_{j+1} + g_j + U(L_j) zeta_j, U = ss_chol_upper.  last: the window's
// final point, which starts the chain: A = 0 and c = m* + U(P*) zeta with (m*, P*) the posterior state there -- has_next: one RTS step
// back from (ms, Ps), the smoothed state of the training point dt further (the second half of ss_interp); else (m, P) itself (a
// forecast behind the last training point), and dt, ms, Ps are not read.
template <int D, typename Mod>
SS_HD void ss_post_element(const Mod& M, bool last, bool has_next, double dt, const double m[D], const double P[D][D], const double ms[D],
                           const double Ps[D][D], const double zeta[D], SSAff<D>& e) {
  SSBwd<D> el;
  ss_bwd_element<D>(M, last && !has_next, dt, m, P, el);
  if (last) {
    if (has_next) {
      double mm[D], PP[D][D];
      for (int i = 0; i < D; ++i) {
        mm[i] = ms[i];
        for (int j = 0; j < D; ++j) PP[i][j] = Ps[i][j];
      }
      ss_rts_step<D>(el, mm, PP);
      for (int i = 0; i < D; ++i) {
        el.g[i] = mm[i];
        for (int j = 0; j < D; ++j) el.L[i][j] = PP[i][j];
      }
    }
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) el.E[i][j] = 0.0;
  }
  double U[D][D];
  ss_chol_upper<D>(el.L, U);
  for (int i = 0; i < D; ++i) {
    double s = el.g[i];
    for (int k = i; k < D; ++k) s += U[i][k] * zeta[k];
    e.c[i] = s;
    for (int j = 0; j < D; ++j) e.A[i][j] = el.E[i][j];
  }
}

// ---- predictive log density from the posterior object (DESIGN.md 4.18 "Predictive log density from the posterior object") -----------
// Observing held-out data at the queries of the backward chain above is a Kalman filter over the window that runs from its last point
// down to its first, with the AFFINE transitions s_j = E_j s_{j+1} + g_j + N(0, L_j) in the place of s_t = A(dt) s_{t-1} + N(0, Q(dt)).
// The forward element of one such step, observed through h = e_1' with noise w and data r: with S = L_00 + w and K = L[:, 0] / S,
// A = E - K E[0, :], b = g + K (r - g_0), C = L - K L[0, :], eta = E[0, :]' (r - g_0) / S, J = E[0, :]' E[0, :] / S; w = +Inf
// (unobserved): (E, g, L, 0, 0).  ss_fwd_element is the case g = 0.  The window's last point starts the chain with E = 0 and (g, L)
// the posterior state (m*, P*) there, which gives A = 0, eta = 0, J = 0 and (b, C) that state after its own update.
template <int D>
SS_HD void ss_fwd_element_affine(const double E[D][D], const double g[D], const double L[D][D], double w, double r, SSFwd<D>& e) {
  if (!(w < INFINITY)) {
    for (int i = 0; i < D; ++i) {
      e.b[i] = g[i]; e.eta[i] = 0.0;
      for (int j = 0; j < D; ++j) { e.A[i][j] = E[i][j]; e.C[i][j] = L[i][j]; e.J[i][j] = 0.0; }
    }
    return;
  }
  const double Sinv = 1.0 / (L[0][0] + w), d = r - g[0];
  for (int i = 0; i < D; ++i) {
    const double K = L[i][0] * Sinv;
    e.b[i] = g[i] + K * d;
    e.eta[i] = E[0][i] * d * Sinv;
    for (int j = 0; j < D; ++j) {
      e.A[i][j] = E[i][j] - K * E[0][j];
      e.C[i][j] = L[i][j] - K * L[0][j];
      e.J[i][j] = E[0][i] * E[0][j] * Sinv;
    }
  }
}

// The backward element of the window's last point: E = 0 and (g, L) = (m*, P*), the posterior state there as ss_post_element takes it
// -- has_next: one RTS step back from (ms, Ps), the smoothed state of the training point dt further; else the filtered (m, P) itself.
template <int D, typename Mod>
SS_HD void ss_chain_start(const Mod& M, bool has_next, double dt, const double m[D], const double P[D][D], const double ms[D],
                          const double Ps[D][D], SSBwd<D>& el) {
  ss_bwd_element<D>(M, !has_next, dt, m, P, el);
  if (has_next) {
    double mm[D], PP[D][D];
    for (int i = 0; i < D; ++i) {
      mm[i] = ms[i];
      for (int j = 0; j < D; ++j) PP[i][j] = Ps[i][j];
    }
    ss_rts_step<D>(el, mm, PP);
    for (int i = 0; i < D; ++i) {
      el.g[i] = mm[i];
      for (int j = 0; j < D; ++j) el.L[i][j] = PP[i][j];
    }
  }
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) el.E[i][j] = 0.0;
}

// One step of the sequential filter along the chain: (m, P) at window point j + 1 -> (m, P) at point j with element el, m <- E m + g
// and P <- E P E' + L, then ss_filter_step's update.  Returns the point's log-density term, 0 for an unobserved point.  The start
// element (E = 0) makes (m*, P*) of any finite (m, P).
template <int D>
SS_HD double ss_chain_step(const SSBwd<D>& el, double w, double r, double m[D], double P[D][D]) {
  double X[D][D], mp[D];
  ss_mm<D>(el.E, P, X);
  for (int i = 0; i < D; ++i) {
    double s = el.g[i];
    for (int k = 0; k < D; ++k) s += el.E[i][k] * m[k];
    mp[i] = s;
  }
  for (int i = 0; i < D; ++i) {
    m[i] = mp[i];
    for (int j = i; j < D; ++j) {
      double q = el.L[i][j];
      for (int k = 0; k < D; ++k) q += X[i][k] * el.E[j][k];
      P[i][j] = P[j][i] = q;
    }
  }
  if (!(w < INFINITY)) return 0.0;
  const double S = P[0][0] + w, Sinv = 1.0 / S, e = r - m[0];
  double K[D], p0[D];
  for (int i = 0; i < D; ++i) { p0[i] = P[0][i]; K[i] = P[i][0] * Sinv; }
  for (int i = 0; i < D; ++i) {
    m[i] += K[i] * e;
    for (int j = 0; j < D; ++j) P[i][j] -= K[i] * p0[j];
  }
  ss_sym<D>(P);
  return -0.5 * (log(6.283185307179586 * S) + e * e * Sinv);
}
