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

// ---------------------------------------------------------------------------------------------------
// The blocked schedule (DESIGN.md 4.22 "Blocked schedule"): the same recursion with one latent spread over many workgroups, TOEPB_J
// steps per launch, for n beyond what one workgroup's LDS holds.  Between launches the state lives in global memory: a, b, p, q in two
// copies each (a launch reads one and writes the other), r updated in place by its row's owner, and a four-double record per latent
// (running product, sum z^2, exponent, info), also in two copies.  (p, q) are kept on every row: p_k and q_k are exactly 0 on the rows
// > k, and the rotation of a zero pair is zero, so row k + 1 "enters" with q = 0 without a rule of its own.
//
// A launch at step k0 is (row windows x latents) workgroups of TOEPB_WAVES waves.  Wave 0 of every workgroup first replays the block on
// its leading rows, one row per lane: lane j holds a[k0 + j], b[k0 + j + 1] and r[k0 + j]; step s reads pivot, b and r from lane s,
// rotates, and moves a down one lane.  It leaves (rho, c, 1 / c, z) of the TOEPB_J steps in LDS; steps past n - 1 (and step n - 1,
// which has no rotation) are the identity (0, 1, 1, 0).  Every workgroup of a latent computes the same numbers with the same code, so
// nothing waits for a panel; workgroup 0 alone writes the latent's record.  After the one barrier each wave applies the steps to a
// window of 64 TOEPB_EPT rows held in registers, lane j rows g0 + j TOEPB_EPT + e.  Per step: r -= a z (the a side), a (or p) moves
// down one row, the rotation.  The move is a rename inside the lane -- the step loop is unrolled by TOEPB_EPT and row e of step s
// lives in register (e - s) mod TOEPB_EPT -- plus one __shfl_up of the register that leaves the lane.  What comes in at the top of
// the window is wrong, one row more per step: the first TOEPB_J rows are a halo that is loaded and never stored, and a wave stores the
// TOEPB_V rows below it.  The (p, q) windows tile the rows [0, k0 + J], the (a, b) windows the rows [k0 + J, n); rows above 0 and
// p, q above k0 load as 0.  In the last block only jr < J steps rotate; the identity steps still move p down, so p is stored J - jr
// rows up.  No barrier but the one, no LDS but the coefficients, no atomics, no flags: launches are ordered by the stream.
// A latent whose record already has info != 0, or whose replay meets a bad pivot, stores nothing but the record.
// ---------------------------------------------------------------------------------------------------
static_assert(TOEPB_J == 64, "the replay holds one row per lane");
static_assert(TOEPB_J % TOEPB_EPT == 0, "the register rename closes after TOEPB_EPT steps");

__device__ __forceinline__ double toepb_lane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// One wave's window.  ASIDE: x = a, y = b over the rows [0, n), r updated; else x = p, y = q over the rows [0, hi], x stored sh rows up.
template <bool ASIDE>
__device__ __forceinline__ void toepb_window(const double* __restrict__ xin, const double* __restrict__ yin, double* __restrict__ xout,
                                             double* __restrict__ yout, double* r, const double4* coef, int n, int g0, int hi, int sh,
                                             int lane) {
  double P[TOEPB_EPT], B[TOEPB_EPT], R[TOEPB_EPT];
  const int i0 = g0 + lane * TOEPB_EPT;
  const bool own = lane * TOEPB_EPT >= TOEPB_J;      // below the halo (TOEPB_J is a multiple of TOEPB_EPT: a lane is all halo or none)
#pragma unroll
  for (int e = 0; e < TOEPB_EPT; ++e) {
    const int i = i0 + e;
    const bool ok = i >= 0 && i <= hi;
    const int ii = ok ? i : 0;
    const double xv = xin[ii], yv = yin[ii];
    P[e] = ok ? xv : 0.0;
    B[e] = ok ? yv : 0.0;
    R[e] = 0.0;
    if (ASIDE && ok && own) R[e] = r[i];      // r is read by its row's owner alone
  }
  for (int s0 = 0; s0 < TOEPB_J; s0 += TOEPB_EPT) {
#pragma unroll
    for (int s = 0; s < TOEPB_EPT; ++s) {
      const double4 cf = coef[s0 + s];
      const double rho = cf.x, c = cf.y, ic = cf.z, z = cf.w;
      if (ASIDE) {
#pragma unroll
        for (int e = 0; e < TOEPB_EPT; ++e) R[e] = __builtin_fma(-P[(e - s + TOEPB_EPT) % TOEPB_EPT], z, R[e]);
      }
      const int ps = (2 * TOEPB_EPT - 1 - s) % TOEPB_EPT;      // the row that leaves the lane
      P[ps] = __shfl_up(P[ps], 1);
#pragma unroll
      for (int e = 0; e < TOEPB_EPT; ++e) {
        const int x = (e - s - 1 + 2 * TOEPB_EPT) % TOEPB_EPT;
        const double an = (P[x] - rho * B[e]) * ic;
        B[e] = c * B[e] - rho * an;
        P[x] = an;
      }
    }
  }
  if (own) {
#pragma unroll
    for (int e = 0; e < TOEPB_EPT; ++e) {
      const int i = i0 + e;
      if (i < n) yout[i] = B[e];
      if (i - sh >= 0 && i - sh < n) xout[i - sh] = P[e];
      if (ASIDE && i < n) r[i] = R[e];
    }
  }
}

// work: see launch_toep_schur_blocked.  np: the workgroups on the (p, q) side (they come first).
__global__ __launch_bounds__(64 * TOEPB_WAVES) void toep_schur_block_kernel(
    const double* __restrict__ ain, const double* __restrict__ bin, const double* __restrict__ pin, const double* __restrict__ qin,
    double* __restrict__ aout, double* __restrict__ bout, double* __restrict__ pout, double* __restrict__ qout, double* r,
    const double* __restrict__ stin, double* __restrict__ stout, int n, int k0, int np) {
  __shared__ double4 coef[TOEPB_J];
  __shared__ int sbad;
  const int l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t off = (size_t)l * n;
  stin += 4 * l; stout += 4 * l;
  if (stin[3] != 0.0) {      // failed in an earlier block: pass the record on
    if (blockIdx.x == 0 && tid < 4) stout[tid] = stin[tid];
    return;
  }
  r += off;
  const int js = min(TOEPB_J, n - k0);      // steps of this block, the last of the recursion (n - 1) included
  const int jr = min(TOEPB_J, n - 1 - k0);  // of which rotate
  if (wave == 0) {
    const int i = k0 + lane;
    const double av = ain[off + (i < n ? i : k0)], bv = bin[off + (i + 1 < n ? i + 1 : k0)], rv = r[i < n ? i : k0];
    double X = i < n ? av : 0.0, Bq = i + 1 < n ? bv : 0.0, R = i < n ? rv : 0.0;
    double prod = stin[0], quad = stin[1];
    int ex = (int)stin[2], bad = 0, s = 0;
    for (; s < js; ++s) {
      const double pa = toepb_lane(X, s), pb = toepb_lane(Bq, s), num = toepb_lane(R, s);
      const double ipa = 1.0 / pa, z = num * ipa, rho = pb * ipa;
      const bool last = k0 + s == n - 1;
      if (!(pa > 0.0) || (!last && !(fabs(rho) < 1.0))) { bad = k0 + s + 1; break; }
      quad = __builtin_fma(z, z, quad);
      prod *= pa;
      const bool big = prod > 0x1p+500, small = prod < 0x1p-500;
      prod *= big ? 0x1p-500 : small ? 0x1p+500 : 1.0;
      ex += big ? 500 : small ? -500 : 0;
      if (last) break;
      const double c = sqrt((1.0 - rho) * (1.0 + rho)), ic = 1.0 / c;
      if (lane == 0) coef[s] = make_double4(rho, c, ic, z);
      R = lane > s ? __builtin_fma(-X, z, R) : R;
      const double an = (X - rho * Bq) * ic;
      Bq = c * Bq - rho * an;
      X = __shfl_up(an, 1);
    }
    if (lane >= jr) coef[lane] = make_double4(0.0, 1.0, 1.0, 0.0);
    if (lane == 0) sbad = bad;
    if (blockIdx.x == 0 && lane == 0) { stout[0] = prod; stout[1] = quad; stout[2] = (double)ex; stout[3] = (double)bad; }
  }
  __syncthreads();
  if (sbad) return;
  const int v = ((int)blockIdx.x < np ? (int)blockIdx.x : (int)blockIdx.x - np) * TOEPB_WAVES + wave;
  if ((int)blockIdx.x < np) {
    const int g0 = v * TOEPB_V - TOEPB_J;
    if (g0 > k0) return;                    // its rows lie above k0 + J
    toepb_window<false>(pin + off, qin + off, pout + off, qout + off, nullptr, coef, n, g0, k0, TOEPB_J - jr, lane);
  } else {
    const int g0 = k0 + v * TOEPB_V;
    if (g0 + TOEPB_J >= n) return;
    toepb_window<true>(ain + off, bin + off, aout + off, bout + off, r, coef, n, g0, n - 1, 0, lane);
  }
}

// Before the first block: a = t / sqrt(t0) (a[0] the square root itself), b = a, p[0] = q[0] = 1 / sqrt(t0), r copied, the record.
__global__ __launch_bounds__(256) void toep_block_init_kernel(const double* __restrict__ t, const double* __restrict__ r, int n,
                                                              double* __restrict__ a, double* __restrict__ b, double* __restrict__ p,
                                                              double* __restrict__ q, double* __restrict__ rw, double* __restrict__ st) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const size_t off = (size_t)l * n;
  if (i >= n) return;
  const double s = sqrt(t[off]), is = 1.0 / s, v = i ? t[off + i] * is : s;
  a[off + i] = v; b[off + i] = v; rw[off + i] = r[off + i];
  if (i == 0) {
    p[off] = is; q[off] = is;
    st[4 * l] = 1.0; st[4 * l + 1] = 0.0; st[4 * l + 2] = 0.0; st[4 * l + 3] = 0.0;
  }
}
// After the last: the generators with p's last shift, log det, the sum, info.
__global__ __launch_bounds__(256) void toep_block_finish_kernel(const double* __restrict__ p, const double* __restrict__ q,
                                                                const double* __restrict__ st, int n, double* __restrict__ pg,
                                                                double* __restrict__ qg, double* __restrict__ out2, int* __restrict__ info) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const size_t off = (size_t)l * n;
  if (i >= n) return;
  pg[off + i] = i ? p[off + i - 1] : 0.0;
  qg[off + i] = q[off + i];
  if (i == 0) {
    out2[2 * l] = 2.0 * (log(st[4 * l]) + st[4 * l + 2] * 0.6931471805599453);
    out2[2 * l + 1] = st[4 * l + 1];
    info[l] = (int)st[4 * l + 3];
  }
}

ToepBlockPlan toep_block_plan(int n, int nb) {
  ToepBlockPlan P;
  P.steps = TOEPB_J; P.rows = TOEPB_ROWS;
  P.launches = (n + TOEPB_J - 1) / TOEPB_J;
  P.windows = (n - 1) / TOEPB_ROWS + 2;      // most workgroups a launch gives a latent (both sides)
  P.work = 9 * (size_t)nb * n + 8 * (size_t)nb;
  return P;
}
void launch_toep_schur_blocked(const double* t, const double* r, int n, int nb, double* out2, double* p, double* q, int* info,
                               double* work, hipStream_t st) {
  if (nb <= 0) return;
  const size_t N = (size_t)nb * n;
  double* a[2] = {work, work + N};
  double* b[2] = {work + 2 * N, work + 3 * N};
  double* pp[2] = {work + 4 * N, work + 5 * N};
  double* qq[2] = {work + 6 * N, work + 7 * N};
  double* rw = work + 8 * N;
  double* rec[2] = {work + 9 * N, work + 9 * N + 4 * (size_t)nb};
  const dim3 flat((n + 255) / 256, nb);
  hipLaunchKernelGGL(toep_block_init_kernel, flat, dim3(256), 0, st, t, r, n, a[0], b[0], pp[0], qq[0], rw, rec[0]);
  int cur = 0;
  for (int k0 = 0; k0 < n; k0 += TOEPB_J, cur ^= 1) {
    const int np = (k0 + TOEPB_J + TOEPB_ROWS) / TOEPB_ROWS;      // rows [0, k0 + J]
    const int na = k0 + TOEPB_J < n ? (n - k0 - TOEPB_J + TOEPB_ROWS - 1) / TOEPB_ROWS : 0;
    hipLaunchKernelGGL(toep_schur_block_kernel, dim3(np + na, nb), dim3(64 * TOEPB_WAVES), 0, st, (const double*)a[cur],
                       (const double*)b[cur], (const double*)pp[cur], (const double*)qq[cur], a[cur ^ 1], b[cur ^ 1], pp[cur ^ 1],
                       qq[cur ^ 1], rw, (const double*)rec[cur], rec[cur ^ 1], n, k0, np);
  }
  hipLaunchKernelGGL(toep_block_finish_kernel, flat, dim3(256), 0, st, (const double*)pp[cur], (const double*)qq[cur],
                     (const double*)rec[cur], n, p, q, out2, info);
}

// ---------------------------------------------------------------------------------------------------
// Sampling (DESIGN.md 4.22 "Sampling"): f = L zeta with L L' = Toeplitz(t), the factor never stored.  Before step k shifts it, a holds
// column k of L on the rows >= k, so f[i] += a[i] zeta[k] rides on the recursion where r[i] -= a[i] z rides in the blocked schedule,
// whose launches (TOEPB_J steps each, ordered by the stream), one-wave replay and register windows this kernel keeps.  Only the
// (a, b) side exists: a launch is max(na, 1) workgroups per latent and the state between launches is a, b in two copies, the samples
// (in f itself, a row read and written by its owner alone) and one int of record per latent, in two copies.
// A pass carries TOEPS_NS samples: a lane keeps TOEPS_NS accumulators for each of its TOEPB_EPT rows, and the TOEPB_J x TOEPS_NS
// normals of the block are staged once in LDS beside the coefficients and read as broadcasts.  The rows k0 .. k0 + J - 1 turn into
// pivots inside the block: they are finished by the replay wave, lane j row k0 + j, diagonal term included, and stored by workgroup 0
// alone, as the record is.  Sample slots past the call's N read zeros and are never stored, and every accumulator is one chain of
// fmas in step order whatever its slot: column q of an N-sample call is bitwise the one-sample call on its normals.
// A bad pivot (or |rho| >= 1) stores nothing but the record, which holds 1 + the step.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void toeps_window(const double* __restrict__ ain, const double* __restrict__ bin, double* __restrict__ aout,
                                             double* __restrict__ bout, double* f, int nq, const double4* coef, const double* zeta, int n,
                                             int g0, int lane) {
  double P[TOEPB_EPT], B[TOEPB_EPT], F[TOEPS_NS][TOEPB_EPT];
  const int i0 = g0 + lane * TOEPB_EPT;              // g0 >= 0: no row above 0
  const bool own = lane * TOEPB_EPT >= TOEPB_J;      // below the halo
#pragma unroll
  for (int e = 0; e < TOEPB_EPT; ++e) {
    const int i = i0 + e;
    const bool ok = i < n;
    const int ii = ok ? i : 0;
    const double xv = ain[ii], yv = bin[ii];
    P[e] = ok ? xv : 0.0;
    B[e] = ok ? yv : 0.0;
#pragma unroll
    for (int q = 0; q < TOEPS_NS; ++q) {
      F[q][e] = 0.0;
      if (ok && own && q < nq) F[q][e] = f[(size_t)q * n + i];      // a row's samples are read by its owner alone
    }
  }
  for (int s0 = 0; s0 < TOEPB_J; s0 += TOEPB_EPT) {
#pragma unroll
    for (int s = 0; s < TOEPB_EPT; ++s) {
      const double4 cf = coef[s0 + s];
      const double rho = cf.x, c = cf.y, ic = cf.z;
      const double* zt = zeta + (s0 + s) * TOEPS_NS;
#pragma unroll
      for (int q = 0; q < TOEPS_NS; ++q) {
        const double zq = zt[q];
#pragma unroll
        for (int e = 0; e < TOEPB_EPT; ++e) F[q][e] = __builtin_fma(P[(e - s + TOEPB_EPT) % TOEPB_EPT], zq, F[q][e]);
      }
      const int ps = (2 * TOEPB_EPT - 1 - s) % TOEPB_EPT;      // the row that leaves the lane
      P[ps] = __shfl_up(P[ps], 1);
#pragma unroll
      for (int e = 0; e < TOEPB_EPT; ++e) {
        const int x = (e - s - 1 + 2 * TOEPB_EPT) % TOEPB_EPT;
        const double an = (P[x] - rho * B[e]) * ic;
        B[e] = c * B[e] - rho * an;
        P[x] = an;
      }
    }
  }
  if (own) {
#pragma unroll
    for (int e = 0; e < TOEPB_EPT; ++e) {
      const int i = i0 + e;
      if (i < n) {
        bout[i] = B[e]; aout[i] = P[e];
#pragma unroll
        for (int q = 0; q < TOEPS_NS; ++q)
          if (q < nq) f[(size_t)q * n + i] = F[q][e];
      }
    }
  }
}

// z, f: [latent][N][n]; this pass serves the samples [q0, min(q0 + TOEPS_NS, N)).  stin, stout: the record, one int per latent.
__global__ __launch_bounds__(64 * TOEPB_WAVES) void toep_schur_sample_kernel(
    const double* __restrict__ ain, const double* __restrict__ bin, double* __restrict__ aout, double* __restrict__ bout,
    const double* __restrict__ z, double* f, const int* __restrict__ stin, int* __restrict__ stout, int n, int k0, int N, int q0) {
  __shared__ double4 coef[TOEPB_J];                  // (rho, c, 1 / c, -)
  __shared__ double zeta[TOEPB_J * TOEPS_NS];        // zeta[s][q]: the normal of step k0 + s, sample q0 + q
  __shared__ int sbad;
  const int l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t off = (size_t)l * n;
  if (stin[l] != 0) {      // failed in an earlier block: pass the record on
    if (blockIdx.x == 0 && tid == 0) stout[l] = stin[l];
    return;
  }
  const int nq = min(TOEPS_NS, N - q0);
  z += ((size_t)l * N + q0) * n; f += ((size_t)l * N + q0) * n;
  const int js = min(TOEPB_J, n - k0);      // steps of this block, the last of the recursion (n - 1) included
  const int jr = min(TOEPB_J, n - 1 - k0);  // of which rotate
  for (int w = tid; w < TOEPB_J * TOEPS_NS; w += 64 * TOEPB_WAVES) {
    const int s = w % TOEPB_J, q = w / TOEPB_J;
    const bool ok = s < js && q < nq;
    const double v = z[ok ? (size_t)q * n + k0 + s : 0];
    zeta[s * TOEPS_NS + q] = ok ? v : 0.0;
  }
  __syncthreads();
  if (wave == 0) {
    const int i = k0 + lane;
    const bool in = i < n;
    const double av = ain[off + (in ? i : k0)], bv = bin[off + (i + 1 < n ? i + 1 : k0)];
    double X = in ? av : 0.0, Bq = i + 1 < n ? bv : 0.0, F[TOEPS_NS];
#pragma unroll
    for (int q = 0; q < TOEPS_NS; ++q) {
      F[q] = 0.0;
      if (in && q < nq && blockIdx.x == 0) F[q] = f[(size_t)q * n + i];      // workgroup 0 alone keeps these rows
    }
    int bad = 0;
    for (int s = 0; s < js; ++s) {
      const double pa = toepb_lane(X, s), pb = toepb_lane(Bq, s);
      const double ipa = 1.0 / pa, rho = pb * ipa;
      const bool last = k0 + s == n - 1;
      if (!(pa > 0.0) || (!last && !(fabs(rho) < 1.0))) { bad = k0 + s + 1; break; }
#pragma unroll
      for (int q = 0; q < TOEPS_NS; ++q) F[q] = lane >= s ? __builtin_fma(X, zeta[s * TOEPS_NS + q], F[q]) : F[q];
      if (last) break;
      const double c = sqrt((1.0 - rho) * (1.0 + rho)), ic = 1.0 / c;
      if (lane == 0) coef[s] = make_double4(rho, c, ic, 0.0);
      const double an = (X - rho * Bq) * ic;
      Bq = c * Bq - rho * an;
      X = __shfl_up(an, 1);
    }
    if (lane >= jr) coef[lane] = make_double4(0.0, 1.0, 1.0, 0.0);
    if (lane == 0) sbad = bad;
    if (blockIdx.x == 0) {
      if (lane == 0) stout[l] = bad;
      if (!bad && lane < js) {
#pragma unroll
        for (int q = 0; q < TOEPS_NS; ++q)
          if (q < nq) f[(size_t)q * n + i] = F[q];
      }
    }
  }
  __syncthreads();
  if (sbad) return;
  const int g0 = k0 + ((int)blockIdx.x * TOEPB_WAVES + wave) * TOEPB_V;
  if (g0 + TOEPB_J >= n) return;
  toeps_window(ain + off, bin + off, aout + off, bout + off, f, nq, coef, zeta, n, g0, lane);
}

// Before a pass: a = t / sqrt(t0) (a[0] the square root itself), b = a, the pass's samples 0, the record 0
__global__ __launch_bounds__(256) void toep_sample_init_kernel(const double* __restrict__ t, int n, int N, int q0, double* __restrict__ a,
                                                               double* __restrict__ b, double* __restrict__ f, int* __restrict__ st) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const size_t off = (size_t)l * n;
  if (i >= n) return;
  const double s = sqrt(t[off]), v = i ? t[off + i] / s : s;
  a[off + i] = v; b[off + i] = v;
  for (int q = q0; q < min(q0 + TOEPS_NS, N); ++q) f[((size_t)l * N + q) * n + i] = 0.0;
  if (i == 0) st[l] = 0;
}
__global__ void toep_sample_info_kernel(const int* __restrict__ st, int nb, int* __restrict__ info) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < nb) info[l] = st[l];
}

size_t toep_sample_work(int n, int nb) { return 4 * (size_t)nb * n + (size_t)nb; }
void launch_toep_sample(const double* t, const double* z, int n, int nb, int N, double* f, int* info, double* work, hipStream_t st) {
  if (nb <= 0 || N <= 0) return;
  const size_t M = (size_t)nb * n;
  double* a[2] = {work, work + M};
  double* b[2] = {work + 2 * M, work + 3 * M};
  int* rec[2] = {reinterpret_cast<int*>(work + 4 * M), reinterpret_cast<int*>(work + 4 * M) + nb};
  int cur = 0;
  for (int q0 = 0; q0 < N; q0 += TOEPS_NS) {
    cur = 0;
    hipLaunchKernelGGL(toep_sample_init_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, t, n, N, q0, a[0], b[0], f, rec[0]);
    for (int k0 = 0; k0 < n; k0 += TOEPB_J, cur ^= 1) {
      const int na = k0 + TOEPB_J < n ? (n - k0 - TOEPB_J + TOEPB_ROWS - 1) / TOEPB_ROWS : 0;
      hipLaunchKernelGGL(toep_schur_sample_kernel, dim3(std::max(na, 1), nb), dim3(64 * TOEPB_WAVES), 0, st, (const double*)a[cur],
                         (const double*)b[cur], a[cur ^ 1], b[cur ^ 1], z, f, (const int*)rec[cur], rec[cur ^ 1], n, k0, N, q0);
    }
  }
  hipLaunchKernelGGL(toep_sample_info_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, (const int*)rec[cur], nb, info);
}

// ---------------------------------------------------------------------------------------------------
// Pathwise conditioning around the products (lmm_api.hip, toep_rand): elementwise kernels, a thread per point, blockIdx.y the latent.
// ---------------------------------------------------------------------------------------------------
// zt[l][q][i] = z[q zs + l n + i]: the callers' normals ([sample][latent][n], samples zs apart) in the layout of launch_toep_sample
__global__ __launch_bounds__(256) void toep_gather_kernel(const double* __restrict__ z, size_t zs, int n, int N, double* __restrict__ zt) {
  const int l = blockIdx.y, q = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) zt[((size_t)l * N + q) * n + i] = z[(size_t)q * zs + (size_t)l * n + i];
}
// tj = t + jitter e0, and e = t[0] e0 (so that L(e) = t[0] I); e may be nullptr
__global__ __launch_bounds__(256) void toep_prior_kernel(const double* __restrict__ t, double jitter, int n, double* __restrict__ tj,
                                                         double* __restrict__ e) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t off = (size_t)blockIdx.y * n;
  if (i >= n) return;
  const double v = t[off + i];
  tj[off + i] = i ? v : v + jitter;
  if (e) e[off + i] = i ? 0.0 : v;
}
// d[l][i] = f[l][q][i] + sw[l] xi[l n + i], i < n: the prior path's pseudo-observation (f: [latent][N][nt], sample q)
__global__ __launch_bounds__(256) void toep_obs_kernel(const double* __restrict__ f, int nt, int N, int q, const double* __restrict__ sw,
                                                       const double* __restrict__ xi, int n, double* __restrict__ d) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[(size_t)l * n + i] = __builtin_fma(sw[l], xi[(size_t)l * n + i], f[((size_t)l * N + q) * nt + i]);
}
// g[l][i] = alpha[l][i] - beta[l][i] for i < n, 0 for n <= i < nt
__global__ __launch_bounds__(256) void toep_gap_kernel(const double* __restrict__ alpha, const double* __restrict__ beta, int n, int nt,
                                                       double* __restrict__ gp) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i < nt) gp[(size_t)l * nt + i] = i < n ? alpha[(size_t)l * n + i] - beta[(size_t)l * n + i] : 0.0;
}
// out[l][i] = mu[l] + f[l][q][i] (+ lo[l][i] + up[l][i]): the latent paths of sample q, [latent][nt]
__global__ __launch_bounds__(256) void toep_path_kernel(const double* __restrict__ f, int nt, int N, int q, const double* __restrict__ mu,
                                                        const double* __restrict__ lo, const double* __restrict__ up,
                                                        double* __restrict__ out) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nt) return;
  const size_t o = (size_t)l * nt + i;
  double v = mu[l] + f[((size_t)l * N + q) * nt + i];
  if (lo) v += lo[o] + up[o];
  out[o] = v;
}

void launch_toep_gather(const double* z, size_t zs, int n, int nb, int N, double* zt, hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_gather_kernel, dim3((n + 255) / 256, nb, N), dim3(256), 0, st, z, zs, n, N, zt);
}
void launch_toep_prior(const double* t, double jitter, int n, int nb, double* tj, double* e, hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_prior_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, t, jitter, n, tj, e);
}
void launch_toep_obs(const double* f, int nt, int N, int q, const double* sw, const double* xi, int n, int nb, double* d, hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_obs_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, f, nt, N, q, sw, xi, n, d);
}
void launch_toep_gap(const double* alpha, const double* beta, int n, int nt, int nb, double* gp, hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_gap_kernel, dim3((nt + 255) / 256, nb), dim3(256), 0, st, alpha, beta, n, nt, gp);
}
void launch_toep_sym(const double* t, const double* e, const double* v, int n, int nb, double* lo, double* up, double* waste, hipStream_t st) {
  if (nb <= 0) return;
  const dim3 grid((n + 255) / 256, nb);
  hipLaunchKernelGGL(toep_tri_kernel<true>, grid, dim3(256), 0, st, e, t, v, v, n, lo, (double*)nullptr);      // L(t) v - t[0] v
  hipLaunchKernelGGL(toep_tri_kernel<false>, grid, dim3(256), 0, st, e, t, v, v, n, up, waste);                // L(t)' v (and t[0] v)
}
void launch_toep_path(const double* f, int nt, int N, int q, const double* mu, const double* lo, const double* up, int nb, double* out,
                      hipStream_t st) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(toep_path_kernel, dim3((nt + 255) / 256, nb), dim3(256), 0, st, f, nt, N, q, mu, lo, up, out);
}
