// lmm_toeplitz.h -- the Toeplitz path for stationary latents over an evenly spaced one-dimensional input.  All Float64.
// lmm_kernels_toeplitz.hip holds the factorisation and the products; the two kernels that evaluate a latent's kernel (the first column
// and the gradient contraction) stand beside the per-kind evaluators they call, in lmm_kernels.hip.
#pragma once
#include "lmm_internal.h"

#define TOEP_THREADS 1024                     // threads of the one workgroup that factors a latent
#define TOEP_MAX_EPT 8                        // most rows a thread owns
#define TOEP_MAX_N (TOEP_THREADS * TOEP_MAX_EPT)      // 8192: a and p (n doubles each) stay in LDS, 128 KB of the CU's 160

// t[l n + j] = kappa_l(x_j, x_0) (+ w[l n] at j = 0) for the nb latents lat[0 .. nb) (device descriptors as the dense kernels take them:
// Latent::dev()); w: [latent][n] noise, of which element 0 is read, or nullptr; mode: the kernel instantiation (0, 1 sums, 2 periodic)
void launch_toep_row(const double* x, int n, const LatentDev* lat, const double* w, int nb, int mode, double* t, hipStream_t st);
// The Schur recursion of nb symmetric positive definite Toeplitz matrices with first columns t[l n ..] and right-hand sides r[l n ..]:
// out2[2 l] = log det, out2[2 l + 1] = r' K^-1 r, p / q [l n ..] the Gohberg-Semencul generators of K^-1, info[l] = 0 or 1 + the step
// whose pivot was not > 0 (or whose reflection coefficient was not inside (-1, 1)).  n <= TOEP_MAX_N.
void launch_toep_schur(const double* t, const double* r, int n, int nb, double* out2, double* p, double* q, int* info, hipStream_t st);
// The same recursion for any n <= TOEPB_MAX_N, a latent spread over many workgroups and TOEPB_J steps per launch (DESIGN.md 4.22
// "Blocked schedule").  A wave holds 64 TOEPB_EPT rows in registers, of which the first TOEPB_J are the halo of the block's steps.
#define TOEPB_J 64                            // steps of a block (a launch)
#define TOEPB_EPT 8                           // rows a lane holds
#define TOEPB_WAVES 4                         // waves of a workgroup
#define TOEPB_V (64 * TOEPB_EPT - TOEPB_J)    // rows a wave stores: 448
#define TOEPB_ROWS (TOEPB_WAVES * TOEPB_V)    // rows a workgroup stores: 1792
#define TOEPB_MAX_N 131072                    // the largest n that has been run; memory is O(n)
struct ToepBlockPlan {
  int steps, rows;                            // TOEPB_J, TOEPB_ROWS
  int windows, launches;                      // most workgroups per latent of a launch; block launches
  size_t work;                                // doubles of workspace: a, b, p, q twice, r, the records twice
};
ToepBlockPlan toep_block_plan(int n, int nb);
// Outputs as launch_toep_schur's; work: toep_block_plan(n, nb).work doubles.
void launch_toep_schur_blocked(const double* t, const double* r, int n, int nb, double* out2, double* p, double* q, int* info,
                               double* work, hipStream_t st);
// Joint samples (DESIGN.md 4.22 "Sampling"): f[l][q][..] = L_l z[l][q][..] with L_l L_l' = Toeplitz(t[l n ..]), for the N samples
// q of each of the nb matrices, TOEPS_NS samples per pass of the blocked recursion; the factor is never stored.  Any n <= TOEPB_MAX_N.
// info[l] = 0 or 1 + the failing step (f is then not a sample); work: toep_sample_work(n, nb) doubles.
#define TOEPS_NS 4                            // samples of a pass: 4 x TOEPB_EPT accumulators (64 VGPRs) beside a and b (32)
size_t toep_sample_work(int n, int nb);
void launch_toep_sample(const double* t, const double* z, int n, int nb, int N, double* f, int* info, double* work, hipStream_t st);
// out = T(t) v = L(t) v + L(t)' v - t[0] v in two parts on toep_tri_kernel: lo = L(t) v - t[0] v, up = L(t)' v; e = t[0] e0
// (launch_toep_prior); v, lo, up, waste: [matrix][n]
void launch_toep_sym(const double* t, const double* e, const double* v, int n, int nb, double* lo, double* up, double* waste, hipStream_t st);
// The elementwise steps of pathwise conditioning (lmm_kernels_toeplitz.hip, above their kernels)
void launch_toep_gather(const double* z, size_t zs, int n, int nb, int N, double* zt, hipStream_t st);
void launch_toep_prior(const double* t, double jitter, int n, int nb, double* tj, double* e, hipStream_t st);
void launch_toep_obs(const double* f, int nt, int N, int q, const double* sw, const double* xi, int n, int nb, double* d, hipStream_t st);
void launch_toep_gap(const double* alpha, const double* beta, int n, int nt, int nb, double* gp, hipStream_t st);
void launch_toep_path(const double* f, int nt, int N, int q, const double* mu, const double* lo, const double* up, int nb, double* out,
                      hipStream_t st);
// alpha[l n ..] = K_l^-1 r_l = L(q) L(q)' r - L(p) L(p)' r; u: 2 nb n doubles of scratch
void launch_toep_solve(const double* p, const double* q, const double* r, int n, int nb, double* u, double* alpha, hipStream_t st);
// sd[l n + d] = sum_i (K_l^-1)_{i, i + d} and ad[l n + d] = sum_i alpha_i alpha_{i + d}
void launch_toep_lags(const double* p, const double* q, const double* alpha, int n, int nb, double* sd, double* ad, hipStream_t st);
// One latent of the gradient contraction: its nterms gradient descriptors (KernelTerm::gd)
struct ToepGradLat { LatentDev gd[LMM_SUM_MAX_TERMS]; int nterms; int pad; };
// red[(LMM_SUM_MAX_TERMS l + c) LMM_NGRAD ..]: term c's record in the layout of grad_reduce_kernel -- [0] d/d lengthscale, [7] sum w K_c,
// [8] d/d alpha, rho or quality, [9] d/d decay over the pairs i > j, w_ij = alpha_i alpha_j - (K^-1)_ij summed along the diagonals
// (ad - sd); term 0's also [1] tr K^-1, [2] alpha.alpha, [3] alpha.r, [4] sum alpha.  mode as launch_toep_row's.
void launch_toep_contract(const double* x, int n, const ToepGradLat* lat, const double* sd, const double* ad, const double* alpha,
                          const double* r, int nb, int mode, double* red, hipStream_t st);

// ---- the posterior at new inputs (DESIGN.md 4.22 "Posterior handle") ----
#define TOEP_PRED_R 256                       // rows of a row block of toep_predict_kernel
#define TOEP_PRED_Q 32                        // queries of a query block
// x[i] = x0 + i h, i < n: the grid as the predict kernel forms it
void launch_toep_grid(double x0, double h, int n, double* x, hipStream_t st);
// var[l ldv + c] = k0[l] - k*_c' K_l^-1 k*_c for the ns queries xs and the nb latents lat[0 .. nb) with generators p, q [l n ..] over the
// grid x0 + s h, s < n; k0[l] = kappa_l(0) (device); part: toep_predict_scratch(n, ns, nb) doubles; mode as launch_toep_row's.
// ns <= 65535 TOEP_PRED_Q.
size_t toep_predict_scratch(int n, int ns, int nb);
void launch_toep_predict(double x0, double h, int n, const LatentDev* lat, const double* k0, const double* p, const double* q,
                         const double* xs, int ns, int nb, int mode, double* part, double* var, size_t ldv, hipStream_t st);

// ---- gradients with respect to the queries (DESIGN.md 4.22 "Gradients with respect to the queries") ----
#define TOEP_GRAD_Q 16                        // queries of a query block of toep_predict_grad_kernel: kappa and d kappa / d xs share the B tile
// dvar[l ldv + c] = d var_l(xs_c) / d xs_c = -2 (u_q . u'_q - u_p . u'_p); part: toep_predict_grad_scratch(n, ns, nb) doubles.
// ctol: |xs_c - (x0 + s h)| <= ctol counts as a coincident pair, whose derivative is 0 for every kind (it matters at the cusp of
// Matern12 only).  Arguments otherwise as launch_toep_predict's.  ns <= 65535 TOEP_GRAD_Q.
size_t toep_predict_grad_scratch(int n, int ns, int nb);
void launch_toep_predict_grad(double x0, double h, double ctol, int n, const LatentDev* lat, const double* p, const double* q,
                              const double* xs, int ns, int nb, int mode, double* part, double* dvar, size_t ldv, hipStream_t st);
// dmean[l ldm + c] = sum_s d kappa_l(x0 + s h, xs_c) / d xs_c alpha[l n + s]
void launch_toep_mean_grad(double x0, double h, double ctol, int n, const LatentDev* lat, const double* alpha, const double* xs, int ns,
                           int nb, int mode, double* dmean, size_t ldm, hipStream_t st);

// ---- the joint predictive at new inputs (DESIGN.md 4.22 "Joint predictive") ----
// C_l = K_l(xs, xs) - (Uq' Uq - Up' Up), Uq = L(q)' K*, Up = L(p)' K*: the storing variant of the predict GEMM leaves Uq and Up of a
// chunk of whole row blocks in U[latent][generator][row of the chunk][nsp], nsp = toep_joint_nsp(ns); the Gram kernel folds the chunk
// into G; the finish kernel turns G into C + d I in place, in the layout potrf_batch takes.
#define TOEP_JOINT_T 128                      // edge of the tile of G a workgroup of toep_gram_kernel owns
#define TOEP_JOINT_MAX_NS 4096                // 32 latents' C: 4.3 GB
#define TOEP_JOINT_BUDGET (size_t(1) << 28)   // bytes of U a pass may hold: 256 MB
inline int toep_joint_nsp(int ns) { return (ns + TOEP_PRED_Q - 1) / TOEP_PRED_Q * TOEP_PRED_Q; }
// What a call over nb latents runs: `lat` latents per pass (<= LMM_MAX_BATCH) and chunks of `rows` rows (whole row blocks, at most the
// row blocks of n), so that lat 2 rows nsp doubles stay within TOEP_JOINT_BUDGET -- but for one latent and one row block, the least a
// pass can hold (16 MB at ns = 4096).  rows_forced (a multiple of TOEP_PRED_R; 0: none): chunks of that many rows, lat sized to them.
struct ToepJointPlan { int lat, rows; };
ToepJointPlan toep_joint_plan(int n, int ns, int nb, int rows_forced = 0);
// U of the rows [row0, row0 + rows) (row0, rows: multiples of TOEP_PRED_R) for the nb latents lat[0 .. nb): rows >= n and the padding
// queries ns .. nsp - 1 are zeros.  U: nb 2 rows nsp doubles.  Arguments otherwise as launch_toep_predict's.
void launch_toep_predict_store(double x0, double h, int n, const LatentDev* lat, const double* p, const double* q, const double* xs, int ns,
                               int nb, int mode, int row0, int rows, double* U, hipStream_t st);
// G_l (+)= sum over the chunk's row blocks, in ascending order, of (Uq' Uq over the block's rows, then - Up' Up over them): element
// (i, j) of latent l at G.p[l][j ld + i], the TOEP_JOINT_T tiles of the lower triangle (whole tiles: i, j < rup(ns, TOEP_JOINT_T), the
// diagonal tiles on both sides).  first: the sum starts here (G is not read).  The sum is carried in the accumulators from chunk to
// chunk, so G does not depend on how the rows are chunked.
void launch_toep_gram(const double* U, int n, int row0, int rows, int ns, const BatchPtr& G, int ld, int nb, bool first, hipStream_t st);
// out.p[l][j ldo + i] = kappa_l(xs_i - xs_j) - G.p[l][j ldg + i] + (i == j) diag[l] for ns > i >= j.  With pad (out as Dims(ns, 1) lays a
// factor matrix out: NC columns, NR rows) the whole 64 x 64 tiles of the lower triangle are written: also i < j inside a diagonal tile,
// the identity on the padding columns, rider[l ns + j] in row NC (rider == nullptr: zeros) and zeros in the other rows from ns on.
// diag: nb values, rider: [latent][ns], both on the device.  out may be G.
void launch_toep_cov_finish(const LatentDev* lat, const double* xs, int ns, const BatchPtr& G, int ldg, const BatchPtr& out, int ldo, int NR,
                            int NC, const double* diag, const double* rider, bool pad, int nb, int mode, hipStream_t st);

// ---- missing observations (DESIGN.md 4.22 "Missing observations") ----
#define TOEP_MISSING_MAX_K TOEP_JOINT_MAX_NS  // the same Cholesky and the same k^2 memory as the joint predictive
// B_l[i][j] = (T_l^-1)[idx[i], idx[j]] from the generators p, q [l n ..] of the nb latents, element (i, j) at B.p[l][j ld + i]; idx: k
// ascending distinct points in [0, n) (device), the same for every latent.  whole: the TOEP_JOINT_T tiles on and below the diagonal
// are written whole (i, j < rup(k, TOEP_JOINT_T); zeros from k on); else the lower triangle i >= j, i < k and nothing else.
void launch_toep_inverse_block(const double* p, const double* q, int n, const int* idx, int k, const BatchPtr& B, int ld, int nb, bool whole,
                               hipStream_t st);
// Rows of T_l^-1 K* (DESIGN.md 4.22 "Posterior handle for gappy grids"): V_l[i][j] (+)= sum over the rows c of [row0, row0 + rows) of
// q[idx[i] - c] Uq[c][j] - p[idx[i] - c] Up[c][j], with U as launch_toep_predict_store left it for that chunk of rows and the ns
// queries; element (i, j) at V.p[l][i ld + j] (the query runs along the memory: one row per query, one column per point, as the rider
// rows of a triangular solve).  first: the sum starts here (V is not read); it is carried through V from chunk to chunk, so V does not
// depend on how the rows are chunked.  last: row i is scaled by d[l k + i] (d == nullptr: by 1).  whole: the TOEP_JOINT_T tiles are
// written whole (i < rup(k, TOEP_JOINT_T), j < rup(ns, TOEP_JOINT_T); zeros from k and from ns on); else i < k, j < ns and nothing else.
void launch_toep_inverse_rows(const double* p, const double* q, int n, const int* idx, int k, const double* U, int row0, int rows, int ns,
                              const double* d, const BatchPtr& V, int ld, int nb, bool first, bool last, bool whole, hipStream_t st);
// rhs[l n + idx[i]] = d[l k + i] g.p[l][i], i < k (the other elements of rhs are not written)
void launch_toep_gap_scatter(const BatchPtr& g, const double* d, const int* idx, int k, int n, int nb, double* rhs, hipStream_t st);
// d, f [l k ..] of the points idx from the per-point noise w ([latent][n]; +Inf: no observed output) and the complete-data noise w0[l];
// w[l n] becomes w0[l], which launch_toep_row then reads
void launch_toep_missing_prep(double* w, int n, const int* idx, int k, const double* w0, int nb, double* d, double* f, hipStream_t st);
// M_l = D B_l D + F in place (B as launch_toep_inverse_block leaves it with `whole`), in the layout of Dims(k, 2): the identity on the
// padding columns, the rider d o alpha_l[idx] in row NC, zeros in row NC + 1 and the other rows from k on
void launch_toep_missing_finish(const BatchPtr& M, int ld, int NR, int NC, int k, const int* idx, const double* d, const double* f,
                                const double* alpha, int n, int nb, hipStream_t st);
