// lmm_kernels_toeplitz.hip -- symmetric positive definite Toeplitz systems in O(n^2): the Schur recursion of one
// matrix per workgroup, and the Gohberg-Semencul products that turn its generators into K^-1 r and the diagonal sums of K^-1.
// All Float64, no atomics, no scratch memory; every sum has a fixed order, so results are bitwise reproducible.
#include "lmm_toeplitz.h"

// ---------------------------------------------------------------------------------------------------
// The recursion.  K = L L' with column k of L = a (rows >= k); after step k the generator pair (a, b) describes the Schur complement of
// the leading k + 1 rows and (p, q) the same elimination applied to the identity, so that at the end
//     K^-1 = L(q) L(q)' - L(p) L(p)'          (L(v): lower triangular Toeplitz with first column v).
// Step k: shift a and p down by one row, rho = b[k + 1] / a[k + 1], c = sqrt((1 - rho)(1 + rho)), and on the rows > k of (a, b) and
// the rows <= k + 1 of (p, q) the hyperbolic rotation in its mixed form  alpha' = (alpha - rho beta) / c,  beta' = c beta - rho alpha'.
//
// One workgroup of TOEP_THREADS threads per matrix, all n steps in one launch, one barrier per step.  Row i belongs to thread
// i mod TOEP_THREADS, which keeps two values per row in registers (EPT of each, loops unrolled).  The first, bq, is b[i] while the
// row is below the pivot and q[i] from then on: b lives on the rows > k + 1, q on the rows <= k + 1, and row k + 1 changes sides at
// step k, where its beta' is exactly 0 (never stored) and its q starts from 0.  So every row takes exactly one rotation per step.
// The vectors that shift live in LDS under a storage index that moves with the step -- a's row i at i - k - 1, p's at
// n + (i - k - 1) + (n - 1) while step k rotates (p's n slots follow a's) -- so a shift moves nothing, and within a step a slot is read and written
// by the one thread that owns its row: steps are separated by the barrier, and inside a step there is no hazard.
// The forward substitution z = L^-1 r rides on the same reads: before it rotates, the slot of row i holds L[i - 1, k], column k of
// the factor one row up.  The second register is therefore the right-hand side of row i - 1, and r[i - 1] -= L[i - 1, k] z_k costs
// no LDS traffic of its own (row n - 1's, which has no row below it, is kept by thread 0 in a register of its own; its slot
// n - 1 - k is not touched by step k's rotations).
// What a step needs from other threads goes through piv[k & 1]: the pivot a[k] = L[k, k] from the owner of row k, and b[k + 1] and
// the finished r[k] from the owner of row k + 1.  Step k reads piv[k & 1] and writes piv[(k + 1) & 1], which was last read before the
// previous barrier.  Every thread forms rho and z_k = r[k] / L[k, k] from them; log det = 2 log prod L[k, k] is kept as a running
// product with its exponent pulled out every step, and r' K^-1 r = sum z_k^2 is added in step order.
// A pivot that is not > 0 or a rho outside (-1, 1) is read by every thread alike: they leave the loop together.
// ---------------------------------------------------------------------------------------------------
template <int EPT>
__global__ __launch_bounds__(TOEP_THREADS) void toep_schur_kernel(const double* __restrict__ t, const double* __restrict__ r, int n,
                                                                   double* __restrict__ out2, double* __restrict__ pg,
                                                                   double* __restrict__ qg, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double toep_lds[];      // a: n doubles, then p: n doubles
  __shared__ double piv[2][3];
  const int l = blockIdx.x, tid = threadIdx.x;
  t += (size_t)l * n; r += (size_t)l * n; pg += (size_t)l * n; qg += (size_t)l * n;
  const double s = sqrt(t[0]), is = 1.0 / s;
  double bq[EPT], rr[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * TOEP_THREADS;
    const bool act = i < n;
    const int ii = act ? i : 0;
    const double v = t[ii] * is, rv = r[ii ? ii - 1 : 0];
    if (act) { toep_lds[i] = v; toep_lds[n + i] = (i == n - 1) ? is : 0.0; }
    bq[e] = act ? (i ? v : is) : 0.0;   // b[i], or q[0]
    rr[e] = (act && i) ? rv : 0.0;      // r[i - 1]
  }
  if (tid == 0) { piv[0][0] = s; piv[0][1] = n > 1 ? t[1] * is : 0.0; piv[0][2] = r[0]; }
  __syncthreads();
  int bad = 0, ex = 0;
  double prod = 1.0, quad = 0.0;
  double rlast = tid == 0 ? r[n - 1] : 0.0;      // row n - 1's right-hand side (thread 0)
  // The registers are updated by selects and only stores sit under branches: a conditional update of one element makes the compiler
  // keep a second copy of both arrays across the branch, and two copies of 4 EPT registers do not fit 128 VGPRs at EPT = 7, 8.
  for (int k = 0; k < n; ++k) {
    const int par = k & 1;
    const double pa = piv[par][0], pb = piv[par][1], num = piv[par][2];
    const double ipa = 1.0 / pa, z = num * ipa, rho = pb * ipa;
    const bool last = k == n - 1;
    if (!(pa > 0.0) || (!last && !(fabs(rho) < 1.0))) { bad = k + 1; break; }
    quad = __builtin_fma(z, z, quad);
    prod *= pa;
    const bool big = prod > 0x1p+500, small = prod < 0x1p-500;
    prod *= big ? 0x1p-500 : small ? 0x1p+500 : 1.0;
    ex += big ? 500 : small ? -500 : 0;
    if (last) break;
    const double c = sqrt((1.0 - rho) * (1.0 + rho)), ic = 1.0 / c;
    double qnew = 0.0;                  // row k + 1 becomes final: (p, q) gain it with q = 0, and its owner rotates that pair too
    if (tid == ((k + 1) & (TOEP_THREADS - 1))) {
      const double pn = toep_lds[2 * n - 1] * ic;
      toep_lds[2 * n - 1] = pn;
      qnew = -(rho * pn);
    }
    if (tid == 0) {
      rlast = __builtin_fma(-toep_lds[n - 1 - k], z, rlast);
      if (k == n - 2) piv[par ^ 1][2] = rlast;
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int i = tid + e * TOEP_THREADS;
      const bool act = i < n;
      const int j = act ? i - k - 1 + (i > k ? 0 : 2 * n - 1) : 0;
      const double al = toep_lds[j], be = bq[e];
      const double an = (al - rho * be) * ic;
      const double bn = (i == k + 1) ? qnew : c * be - rho * an;
      const double rn = (act && i > k + 1) ? __builtin_fma(-al, z, rr[e]) : rr[e];
      if (act) toep_lds[j] = an;
      if (i == k + 1 && act) piv[par ^ 1][0] = an;
      if (i == k + 2 && act) { piv[par ^ 1][1] = bn; piv[par ^ 1][2] = rn; }
      bq[e] = act ? bn : bq[e];
      rr[e] = rn;
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * TOEP_THREADS;
    if (i < n) {
      pg[i] = i ? toep_lds[n + i - 1] : 0.0;      // the last step's shift
      qg[i] = bq[e];
    }
  }
  if (tid == 0) {
    out2[2 * l] = 2.0 * (log(prod) + (double)ex * 0.6931471805599453);
    out2[2 * l + 1] = quad;
    info[l] = bad;
  }
}

// ---------------------------------------------------------------------------------------------------
// Products with L(q), L(p) and their transposes.  LOWER: out[o] = sum_{s <= o} q[o - s] xq[s] - p[o - s] xp[s]; else the transposes,
// outq[o] = sum_{s >= o} q[s - o] xq[s] and outp[o] likewise with p, kept apart.  Workgroup (tile of 256 outputs, matrix): per tile of
// 256 values of x it stages them and the 511 lags of q and p that the pair of tiles spans in LDS (zeros outside [0, n)); a thread owns
// one output and walks the tile in order, tiles in ascending order.
// ---------------------------------------------------------------------------------------------------
template <bool LOWER>
__global__ __launch_bounds__(256) void toep_tri_kernel(const double* __restrict__ p, const double* __restrict__ q,
                                                       const double* __restrict__ xq, const double* __restrict__ xp, int n,
                                                       double* __restrict__ outq, double* __restrict__ outp) {
  __shared__ double vq[512], vp[512], sq[256], sp[256];
  const int l = blockIdx.y, tid = threadIdx.x, o0 = blockIdx.x * 256;
  const size_t off = (size_t)l * n;
  p += off; q += off; xq += off; xp += off;
  double aq = 0.0, ap = 0.0;
  const int s_beg = LOWER ? 0 : o0, s_end = LOWER ? o0 + 256 : n;
  for (int s0 = s_beg; s0 < s_end && s0 < n; s0 += 256) {
    const int base = (LOWER ? o0 - s0 : s0 - o0) - 255;
    __syncthreads();
    for (int w = tid; w < 512; w += 256) {
      const int lag = base + w;
      const bool ok = lag >= 0 && lag < n;
      vq[w] = ok ? q[lag] : 0.0; vp[w] = ok ? p[lag] : 0.0;
    }
    sq[tid] = s0 + tid < n ? xq[s0 + tid] : 0.0;
    sp[tid] = s0 + tid < n ? xp[s0 + tid] : 0.0;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 256; ++j) {
      const int w = LOWER ? tid - j + 255 : j - tid + 255;
      aq = __builtin_fma(vq[w], sq[j], aq);
      ap = __builtin_fma(vp[w], sp[j], ap);
    }
  }
  const int o = o0 + tid;
  if (o < n) {
    if (LOWER) outq[off + o] = aq - ap;
    else { outq[off + o] = aq; outp[off + o] = ap; }
  }
}

// ---------------------------------------------------------------------------------------------------
// Sums along the diagonals: sd[d] = sum_i (K^-1)_{i, i + d} = sum_j (n - d - j) (q_j q_{j + d} - p_j p_{j + d}) and the autocorrelation
// ad[d] = sum_j alpha_j alpha_{j + d}.  Workgroup (tile of 256 lags, matrix), a thread per lag; per tile of 256 values of j the three
// vectors at j and the 511 values at j + d are staged in LDS (zeros from n on, which ends every sum where it must).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void toep_lag_kernel(const double* __restrict__ p, const double* __restrict__ q,
                                                       const double* __restrict__ alpha, int n, double* __restrict__ sd,
                                                       double* __restrict__ ad) {
  __shared__ double wq[512], wp[512], wa[512], jq[256], jp[256], ja[256];
  const int l = blockIdx.y, tid = threadIdx.x, d0 = blockIdx.x * 256, d = d0 + tid;
  const size_t off = (size_t)l * n;
  p += off; q += off; alpha += off;
  double as = 0.0, aa = 0.0;
  for (int j0 = 0; j0 + d0 < n; j0 += 256) {
    __syncthreads();
    for (int w = tid; w < 512; w += 256) {
      const int i = j0 + d0 + w;
      const bool ok = i < n;
      wq[w] = ok ? q[i] : 0.0; wp[w] = ok ? p[i] : 0.0; wa[w] = ok ? alpha[i] : 0.0;
    }
    const bool ok = j0 + tid < n;
    jq[tid] = ok ? q[j0 + tid] : 0.0; jp[tid] = ok ? p[j0 + tid] : 0.0; ja[tid] = ok ? alpha[j0 + tid] : 0.0;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 256; ++j) {
      const double wgt = (double)(n - d - j0 - j);
      as = __builtin_fma(wgt, __builtin_fma(jq[j], wq[j + tid], -(jp[j] * wp[j + tid])), as);
      aa = __builtin_fma(ja[j], wa[j + tid], aa);
    }
  }
  if (d < n) { sd[off + d] = as; ad[off + d] = aa; }
}

template <int EPT>
static void toep_schur_launch(const double* t, const double* r, int n, int nb, double* out2, double* p, double* q, int* info,
                              hipStream_t st) {
  const int bytes = 2 * n * (int)sizeof(double);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(toep_schur_kernel<EPT>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  hipLaunchKernelGGL(toep_schur_kernel<EPT>, dim3(nb), dim3(TOEP_THREADS), bytes, st, t, r, n, out2, p, q, info);
}
void launch_toep_schur(const double* t, const double* r, int n, int nb, double* out2, double* p, double* q, int* info, hipStream_t st) {
  if (nb <= 0) return;
  switch ((n + TOEP_THREADS - 1) / TOEP_THREADS) {
    case 1: toep_schur_launch<1>(t, r, n, nb, out2, p, q, info, st); break;
    case 2: toep_schur_launch<2>(t, r, n, nb, out2, p, q, info, st); break;
    case 3: toep_schur_launch<3>(t, r, n, nb, out2, p, q, info, st); break;
    case 4: toep_schur_launch<4>(t, r, n, nb, out2, p, q, info, st); break;
    case 5: toep_schur_launch<5>(t, r, n, nb, out2, p, q, info, st); break;
    case 6: toep_schur_launch<6>(t, r, n, nb, out2, p, q, info, st); break;
    case 7: toep_schur_launch<7>(t, r, n, nb, out2, p, q, info, st); break;
    default: toep_schur_launch<TOEP_MAX_EPT>(t, r, n, nb, out2, p, q, info, st); break;
  }
}
void launch_toep_solve(const double* p, const double* q, const double* r, int n, int nb, double* u, double* alpha, hipStream_t st) {
  if (nb <= 0) return;
  const dim3 grid((n + 255) / 256, nb);
  double* uq = u;
  double* up = u + (size_t)nb * n;
  hipLaunchKernelGGL(toep_tri_kernel<false>, grid, dim3(256), 0, st, p, q, r, r, n, uq, up);
  hipLaunchKernelGGL(toep_tri_kernel<true>, grid, dim3(256), 0, st, p, q, (const double*)uq, (const double*)up, n, alpha, (double*)nullptr);
}
void launch_toep_lags(const double* p, const double* q, const double* alpha, int n, int nb, double* sd, double* ad, hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_lag_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, p, q, alpha, n, sd, ad);
}
