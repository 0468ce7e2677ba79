// lmm_internal.h -- shared between lmm_kernels.hip (device) and lmm_api.hip (host orchestration).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/lmm_hip.h"
#include "lmm_potrf_plan.h"
// the planner names the profile classes without seeing lmm_hip.h
static_assert((int)POTRF_CLS_UPDATE == LMM_PROF_UPDATE && (int)POTRF_CLS_UPDATE_NARROW == LMM_PROF_UPDATE_NARROW && (int)POTRF_CLS_TRSM == LMM_PROF_TRSM &&
              (int)POTRF_CLS_DIAG == LMM_PROF_DIAG && (int)POTRF_CLS_REGION == LMM_PROF_REGION && (int)POTRF_CLS_UPDATE_SHORT == LMM_PROF_UPDATE_SHORT,
              "the POTRF_CLS_* values of lmm_potrf_plan.h are lmm_prof_class values");

extern int g_f32;              // compute dtype of the matrices: 0 = Float64, 1 = Float32 (lmm_kernels.hip)
#define LMM_MAX_BATCH 32
struct BatchPtr { double* p[LMM_MAX_BATCH]; };   // base pointers of the matrices of one batch (kernel argument, by value)
struct BatchInfo { int* p[LMM_MAX_BATCH]; };

// kind: the BASE kernel kind (lmm_kernel_kind); ils: nullptr (isotropic, inv_ls) or the latent's d per-dimension inverse lengthscales
// (device; an ARD latent, d > 1).  An ARD latent keeps inv_ls = 1 / its common multiplier (the gradient reduction's d/d multiplier).
// alpha: the RQ shape; for a periodic latent (LMM_KERNEL_PERIODIC) the slot carries 1 / rho^2, inv_ls 1 / period and ils the
// per-dimension 1 / P_k (unused by the other kinds).  A locally periodic latent (LMM_KERNEL_LOCALLY_PERIODIC) is described as a periodic
// one, plus inv_decay = 1 / (its SE lengthscale) (0 for every other kind).
// A sum latent (kind LMM_KERNEL_SUM) has nterms (1..LMM_SUM_MAX_TERMS) resolved terms in `terms` (device): each an ordinary base-kind
// descriptor whose var = v0 v_c, inv_ls = 1 / (s0 l_c) and ils = its per-dimension 1 / (s0 l_c ard_c[k]) (or nullptr); var and inv_ls
// of the sum latent itself are v0 and 1 / s0.  terms is nullptr and nterms 0 for every other latent.
struct LatentDev {
  int kind;
  int nterms;              // (next to kind: the descriptor keeps the 64 bytes it had before inv_decay)
  double var, inv_ls, mean;
  const double* ils;
  double alpha;
  const LatentDev* terms;
  double inv_decay;
};
static_assert(sizeof(LatentDev) == 64, "LatentDev is read per element by the dense and sum kernels: keep it at 64 bytes");

// Gram / factor-matrix assembly arguments (see gram_kernel).
struct GramArgs {
  double* A;            // factor matrix base (row 0 = matrix row `row_shift`)
  int ld, nrows, ncols; // nrows = rows covered by the launch (multiple of 64), ncols multiple of 64
  int row_tile0;        // first 64-row tile of the launch (rider-only launches start at ncols/64)
  int row_shift;        // row index stored at A[0]
  int full;             // 1: no lower-triangle skip (rectangular rider matrix)
  const double* x; int d, n;
  int kind; double var, inv_ls, diag_add, pad_diag;
  const double* ils;                           // per-dimension inverse lengthscales (device, d of them; nullptr: isotropic inv_ls)
  const double* diag_vec;                      // optional per-point diagonal term (length n), added to diag_add
  const double* rider; int rider_ld, nrider;   // rows ncols + r  <- rider[r*rider_ld + j] - rider_sub
  double rider_sub;                            // constant subtracted from the rider rows (latent mean: delta = T y - mean)
  const double* xs; int ns;                    // rows ncols + r  <- kappa(xs_r, x_j)
  int* info_zero;                              // optional: the matrix's pivot-info word, zeroed by the launch (saves a memset per call)
  int cpw;                                     // column tiles per workgroup (set by the launcher: 4, or 1 when the grid would be small)
  double alpha;                                // RQ shape; periodic: 1 / rho^2 (unused by the other kinds)
  const LatentDev* terms; int nterms;          // kind LMM_KERNEL_SUM: the resolved terms (device; see LatentDev)
  int sum_per;                                 // kind LMM_KERNEL_SUM: some term is periodic or locally periodic (the instantiation that evaluates one)
  double inv_decay;                            // locally periodic: 1 / decay (unused by the other kinds)
  // optional (Float64 storage only; row_shift = 0): this matrix's zero extents (lmm_emul.h), one int per 64-row block of the matrix,
  // set to LMM_ZERO_EXT_NONE on the stream ahead of the launch; args[j] of a batched launch has zext = args[0].zext + j * zext_ld
  int* zext; int zext_ld;
};

// The same assembly for up to LMM_MAX_BATCH same-shaped matrices in ONE launch (blockIdx.z = matrix): everything in `base`
// is shared; the fields below replace base's per matrix.  All matrices of a launch have base.kind.
struct GramBatchArgs {
  GramArgs base;
  double* A[LMM_MAX_BATCH];
  double var[LMM_MAX_BATCH], inv_ls[LMM_MAX_BATCH], diag_add[LMM_MAX_BATCH];
  const double* ils[LMM_MAX_BATCH];
  const double* diag_vec[LMM_MAX_BATCH];
  const double* rider[LMM_MAX_BATCH];
  double rider_sub[LMM_MAX_BATCH];
  int* info_zero[LMM_MAX_BATCH];
  double alpha[LMM_MAX_BATCH];
  const LatentDev* terms[LMM_MAX_BATCH];
  int nterms[LMM_MAX_BATCH];
  double inv_decay[LMM_MAX_BATCH];
};
static_assert(sizeof(GramBatchArgs) <= 4096, "GramBatchArgs is passed by value: kernel arguments are limited to 4096 bytes");

struct DenseArgs {
  double* A; int ld, nrows, ncols;
  const double* x; int d, n, m;
  const LatentDev* lat;      // device, m entries
  const double* sigmaT;      // device, m x m column-major (nbatch of them when sig_idx != nullptr)
  const int* sig_idx;        // optional, device, n entries: which sigmaT the point's noise block uses (sequential conditioning)
  const double* rider; int rider_ld, nrider;
  int has_sum;               // 1: some lat[l] is a sum latent (the kernel instantiation that evaluates kappa_sum); 2: some latent is
                             // periodic or locally periodic or has such a term (the instantiation that also evaluates kappa_per / kappa_lp)
};

void launch_gram(const GramArgs& a, hipStream_t st);
// nb same-shaped assemblies (differing only in A, kind, var, inv_ls, ils, alpha, inv_decay, terms, diag_add, diag_vec, rider): one launch per run of
// equal kinds (sum latents form runs too; their terms may differ per matrix)
void launch_gram_batch(const GramArgs* args, int nb, hipStream_t st);
void launch_dense_assemble(const DenseArgs& a, hipStream_t st);
void launch_dense_cov(const double* S, int lds, int ns, int m, const double* Hm, int p, double jitter, double sigma2, double* T,
                      double* out, hipStream_t st);
void launch_dense_cross(double* R, int ldr, int nrows, int ncols, const double* xs, int ns, const double* x, int n, int d,
                        int m, const LatentDev* lat, int has_sum, hipStream_t st);
size_t dense_var_partial_elems(int ns, int p, int Ncols);
void launch_dense_var(const double* R, int ldr, int ns, int m, int Ncols, const double* Hm, int p, const LatentDev* lat,
                      double jitter, double sigma2, double* partial, double* out, hipStream_t st);
// Arguments of potrf_node_kernel (lmm_kernels.hip K2c): the trailing update of the columns [j0 + h, j0 + h + N) with the factored
// columns [j0, j0 + h), fused with the factorisation of the next 128-column panel's diagonal block; or that panel's bulk rows.
struct NodeArgs {
  BatchPtr A, W, W2;      // factor matrices; 64 x 64 inverse blocks; 128 x 128 inverse panels (scratch)
  BatchInfo info;
  int ld, M, j0, h, N, n_real;   // M: rows of the region (from row j0 + h) this launch covers
  int MT, nb;             // 128-row tiles of the region; matrices in the batch
  int rest_items, full_items, splitk;     // work items of the column tiles 1.. (gemm_work_item's enumeration and split-K tail)
  int full_items_last, splitk_last;       // the same for the LAST matrix of the batch, which carries the launch's tail
  int mode;               // NODE_UPDATE | NODE_LEAF [| NODE_FUSE], or NODE_BULK
  // NODE_FUSE: the bulk rows of the panel this launch's leaf factors run as the LAST work items of the same launch, behind
  // device-side flags (nflags: per matrix [0] abort word, [1] leaf done, [2 + ti] column-0 tile ti updated; values epoch * 32 + 1)
  int* nflags; int nf_stride, epoch;
  int strip_n, strip0;    // column tiles of the ragged last 64 rows run as work items of this launch (0: none / separate launch); their first item
  int Mb, MTb, bulk0;     // rows / 128-row tiles the bulk items cover (a ragged last 64 rows included); index of the first bulk item
  // the screen's flag bytes (lmm_potrf_plan.h, f64_screen_flag_at with MT and scr_nt): a "rest" item whose tile's byte is 0 returns at once; nullptr: no screen
  const unsigned char* scr; int scr_nt;
  // zero extents (lmm_emul.h; matrix b at zext + b * zext_ld, nullptr: none): a rest item, or a column-0 item ti >= 1 of a launch without
  // NODE_FUSE, whose rows are zero across the panel returns at entry; zstat (may be nullptr) counts them, split parts once
  const int* zext; int zext_ld; int* zstat;
};
// Arguments of potrf_region_kernel (lmm_kernels.hip K2d): the columns [c0, c0 + 128 P) of every matrix of the batch, rows c0 .. c0 + M - 1.
struct RegionArgs {
  BatchPtr A, W, W2;
  BatchInfo info, flags;  // flags: P * R readiness words + 1 abort word per matrix (zeroed once per factorisation)
  int ld, M, c0, P, R, n_real, nb, epoch, first_done;
  int M_real;             // rows c0 .. c0 + M_real - 1 hold data, the rest of the M rows is zero padding (rider rows are padded to 64)
  BatchPtr S;             // optional scratch (LMM_REGION_ASST_TILES 64 x 64 tiles per matrix): partial products of the ASSISTANT tasks
  int na;                 // assistant tasks per matrix (square rows LMM_REGION_ASST_MIN_R .. 2P - 1), 0: none
  int ntasks;             // workgroups per matrix (trace layout)
  int n128;               // the first n128 row tiles below the square are 128 rows high, the following ones 64
  long long* trace;       // optional (LMM_REGION_TRACE=1, tools/region_trace.py): start / end wall-clock ticks of every workgroup
  unsigned* claim; unsigned* claim_next;      // strict-progress build: this launch's claim counters, and the set it zeroes for the next one
  int claim_scramble;     // test hook (lmm_dev_claim_scramble): workgroups ask for the indices in REVERSE order, as if dispatched last-first
  // zero extents (as in NodeArgs): a row task whose rows are zero across the block column returns before its first wait; zstat counts them
  const int* zext; int zext_ld; int* zstat;
};
// The zero extents of a batch as the launchers take them (lmm_emul.h): matrix b's at p + b * ld, one int per 64-row block from matrix
// row 0 and LMM_ZERO_EXT_PAD more; stat (may be nullptr): this step's counter of void work items.  p == nullptr: none, nothing is left out.
struct ZeroExt { const int* p = nullptr; int ld = 0; int* stat = nullptr; };
// Strict forward progress (lmm_set_strict_progress, default on): potrf_region_kernel's workgroups take their task INDEX in turn from a
// per-matrix counter (region_claim) instead of reading it from blockIdx.x, and the fused update launches (NODE_FUSE: bulk items that wait for earlier items of the same launch)
// are not used -- no kernel then relies on the order in which workgroups are dispatched.
extern int g_strict_progress;
extern int g_claim_scramble;              // test hook: see RegionArgs.claim_scramble
void strict_ticket_reset();               // drop the claim counters (after an error drained the device; at shutdown)
// (LMM_REGION_MAX_PANELS, LMM_REGION_ASST_MIN_C / _MIN_R / _TILES: lmm_potrf_plan.h)
// the assistant of a row takes the blocks [0, LMM_REGION_ASST_SPLIT(c)) of the helper's K-long product for column block c.  Round 3:
// c / 2; round 4: 3 c / 4 -- once the chain's hand-offs got cheaper (sc1 loads instead of acquire fences) the helpers of rows >= 9 were
// again the slower side of the walker <-> helper cycle (walker waits of 3-10 us at n = 1024), and what a helper does per column AFTER
// W_c arrives cannot shrink, so the part before it must: the blocks [0, 3 c / 4) are final c / 4 - 1 block periods before they are needed.
#define LMM_REGION_ASST_SPLIT(c) ((3 * (c)) / 4)
// Bound of every dependency spin of the dataflow kernels, in ticks of the 100 MHz wall clock (4 s).  The deadlock argument (a workgroup
// only waits for workgroups dispatched before it, the walker excepted) covers one launch on an otherwise free device; kernels of other
// streams holding CUs or a serialising profiler can delay the one later-dispatched workgroup a walker waits for, hence seconds, not ms.
#define LMM_REGION_SPIN_TICKS 400000000LL
#define LMM_INFO_SYNC_TIMEOUT (-7777)     // pivot-info value a region launch leaves when a dependency wait timed out (never expected)
void region_flags_register(int* base, size_t ints);     // the context's persistent flag array (cleared when the launch epoch wraps)
int device_cus();                         // compute units of the current device (256 when it cannot be asked); read once
extern FactorSwitches g_switches;         // the factorisation's knobs; the lmm_dev_set_* hooks write it, everything else reads it through ...
const FactorSwitches& factor_switches();  // ... which fills it from the environment at its first call
void region_plan_probe(int P, int nb, int Mb, int Mb_real, int cus, int na_full, int out[3]);   // lmm_dev_region_plan
int region_flag_epoch(int set_to);                       // lmm_dev_flag_epoch: returns the current launch epoch; set_to >= 0 replaces it
size_t region_flag_ints(int NR);          // ints per matrix that the flags of any region of a matrix with NR rows need
// returns the number of 128-row row tasks of the launch (the following row tasks are 64 rows high)
int launch_region(const BatchPtr& A, const BatchPtr& W, const BatchPtr& W2, const BatchInfo& info, const BatchInfo& flags, int ld, int NR,
                   int c0, int width, int n_real, int nb, bool first_done, hipStream_t st, int rows_real = -1, const BatchPtr* S = nullptr,
                   const ZeroExt& zx = ZeroExt());
void launch_leaf128(const BatchPtr& A, size_t offD, int ld, const BatchPtr& W, size_t offW, const BatchPtr& W2, size_t offW2,
                    int gcol0, int n_real, const BatchInfo& info, int nb, hipStream_t st);
// bulk rows of the panel at column r0 (its diagonal block factored, its inverse in W2): X = P Dinv' in place
void launch_panel_bulk(const BatchPtr& A, const BatchPtr& W2, int ld, int NR, int r0, int nb, hipStream_t st);
// C -= A B' for the region at r0 = j0 + h (N columns, multiple of 128) + leaf128 on its top-left block
// strip (POTRF_STRIP_*): where the plan puts a ragged last 64 rows; nflags != nullptr (the plan's fused_bulk): also the bulk rows of that
// panel, in the same launch (NODE_FUSE, flags of nf_stride ints per matrix)
void launch_update_leaf(const BatchPtr& A, const BatchPtr& W, const BatchPtr& W2, const BatchInfo& info, int ld, int NR, int j0, int h,
                        int N, int n_real, int nb, hipStream_t st, int strip, int* nflags = nullptr, int nf_stride = 0, const unsigned char* scr = nullptr,
                        const ZeroExt& zx = ZeroExt());
// lmm_kernels_f32w.hip: fp32 C -= A B' on 256 x 256 tiles (one workgroup per CU); false: not launched (shape / switch), use the 128-tile kernel
bool launch_gemm32w(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& A, size_t offA, int lda, const BatchPtr& B, size_t offB, int ldb,
                    int M, int N, int K, int lower, int nb, int cus, bool deterministic, hipStream_t st);
// lmm_kernels_i8.hip: Float64 C_m -= P_m P_m[0:N]' (C_m at C.p[m] + offC, the M x K panel P_m at P.p[m] + offP; lower trapezoid, i >= j) as exact int8 modular GEMMs.  emul_shape_ok:
// M >= N, K a multiple of 128 within the int32 accumulator bound.  Matrices go through `scratch` (emul_scratch_bytes) in groups of G.
// (emul_shape_ok, emul_scratch_bytes: lmm_emul.h)
void emul_set_gemm_workgroups(int wgs);      // cap of the persistent GEMM grid (tests); 0: one workgroup per CU
void emul_set_scratch_poison(int on);        // tests: != 0 fills a group's residue scratch with a non-zero byte before its convert
void emul_set_screen(int on);                // 0: every tile counts as live (the live id list is the identity); 1: tiles whose update cannot change a bit of C are skipped; < 0: LMM_EMUL_SCREEN (default 1)
void emul_set_zero_skip(int on);             // 0: the GEMM walks every K block (all-ones live masks); 1: only the live ones; < 0: LMM_EMUL_ZERO_SKIP (default 1)
// Row maxima that outlive the update (potrf_batch; emul_amax_cover of lmm_potrf_plan.h): out = this update's array, out[m ld + r] for
// matrix m and the ABSOLUTE row r of the matrix (the panel's row i is row row0 + i), written for all nb matrices; src[0 .. n) = arrays
// of the same layout that earlier updates wrote, which together hold the maxima over the panel's columns [0, scan0), so that only
// the columns [scan0, K) are read.  bmax: the factorisation's block maxima (lmm_emul.h), bmax[(m ncb + c) ld + r] for matrix m, the
// ABSOLUTE 128-column block c < ncb and row r; the panel begins at column block cb0.  The scan writes the blocks it reads, and the
// blocks of the columns [0, scan0) are there from the updates that scanned them, whose rows began no later than row0 (the entries
// below a factored block column never change).  nullptr: the maxima live in the scratch and in aux, per group, and the whole panel
// is read.
// aux: emul_aux(M, G, K).total bytes (lmm_emul.h) for the live K blocks and the dead pieces of one group's panels; without a keep,
// .total_bmax bytes: the group's block maxima follow them.  screen: emul_screen_layout(M, N, G, nmod).total bytes for the tile flags,
// the live id list and its counts.
struct EmulAmaxKeep { unsigned long long* out; int ld, row0, n; const unsigned long long* src[LMM_EMUL_COVER_MAX]; int scan0; unsigned long long* bmax; int cb0, ncb; };
hipError_t launch_emul_update(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& P, size_t offP, int ldp, int M, int N, int K, int nb,
                              int G, int nmod, void* scratch, void* aux, void* screen, hipStream_t st, const EmulAmaxKeep* keep = nullptr,
                              const ZeroExt& zx = ZeroExt(), int zrow0 = 0);      // the first HIP error of its host-side calls
// zx, zrow0 (both screens): the zero extents and the matrix row of the region's first row, which is also the panel's end: a tile whose
// row blocks are zero there is stored as not live without reading C (and counted in zx.stat by the emulation's screen, in stat[0] by the f64 one)
// lmm_kernels_i8.hip: the scan and the screen in front of a screened f64 update launch.  keep: as for an emulated
// update (bmax may be nullptr: no block maxima are kept).  flags: f64_screen_flag_bytes; stat[0] += dead rest tiles, stat[1] = 1 when
// the screen did its work; vote (may be nullptr): a word an earlier screen of the factorisation left its dead count in -- when it is
// zero the scan and the screen return at entry and the flags say "live".  M, strip: the step's; the screen covers the rows the node launch takes.
hipError_t launch_f64_screen(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& P, size_t offP, int ldp, int M, int N, int K, int strip, int nb,
                             const EmulAmaxKeep& keep, unsigned char* flags, int* stat, const int* vote, hipStream_t st, const ZeroExt& zx = ZeroExt(), int zrow0 = 0);
void launch_diag64(const BatchPtr& A, size_t offA, int ld, const BatchPtr& W, size_t offW, int gcol0, int n_real,
                   const BatchInfo& info, int nb, hipStream_t st);
// no_splitk: never split the last round's tiles along K (their f64 atomics make the sum order run-dependent): bitwise reproducible
void launch_gemm_nt(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& A, size_t offA, int lda, const BatchPtr& B,
                    size_t offB, int ldb, int M, int N, int K, int lower, bool set, int nb, hipStream_t st, bool no_splitk = false);
void launch_gemm_nt(double* C, int ldc, const double* A, int lda, const double* B, int ldb, int M, int N, int K,
                    int lower, bool set, hipStream_t st);
void launch_lml_reduce(const double* A, int ld, int n, int rider_row0, int nrhs, double* out, hipStream_t st);
// out[b*nrhs + r]; info_out != nullptr: also info_out[b] = *info.p[b] (out / info_out may be device-mapped pinned host memory: the
// results then need no copy back)
void launch_lml_reduce(const BatchPtr& A, int nb, int ld, int n, int rider_row0, int nrhs, double* out, hipStream_t st,
                       const BatchInfo* info = nullptr, int* info_out = nullptr);
void launch_extract_row(const double* A, int ld, int row, int n, double* out, hipStream_t st);
void launch_extract_rows(const BatchPtr& A, int nb, int ld, int row, int n, int nfill, const BatchPtr& o1, const BatchPtr& o2,
                         hipStream_t st);
int strip_kc(int nk);
size_t strip_partial_elems(int nr, int nk, int nv);
void launch_rider_stats(const double* R, int ld, int nr, int nk, const double* z, double mu, double base, double* partial,
                        double* mean_out, double* var_out, hipStream_t st);
void launch_backsolve(const BatchPtr& L, int ld, const BatchPtr& W, int nblk, const BatchPtr& z, int nb, hipStream_t st);
void launch_tall_skinny(const double* In, int ldi, int n, int K, const double* Mx, int ldm, int C, double* Out, int ldo,
                        const double* sub, const double* Ref, int ldr, double* partial, int mode, hipStream_t st);
int tall_skinny_partials(int n, int C);
void launch_sum_partials(const double* partial, int count, double* out, hipStream_t st);
size_t post_mean_partial_elems(int ns, int n);
void launch_post_mean(const double* xs, int ns, const double* x, int n, int d, const double* alpha, LatentDev g,
                      double* partial, double* out, hipStream_t st);
void launch_mix(const double* lat, int ns, int ml, const double* Hm, int p, int pw, double lat_add, double out_add,
                const double* eps, double eps_scale, double* out, hipStream_t st);
void launch_mix_bf16(const double* lat, int ns, int ml, const double* Hm, int p, int pw, double lat_add, double out_add,
                     int terms, double* out, hipStream_t st);
void launch_cov_mix(const BatchPtr& Cl, int ldcl, int nl, const double* Hs, int p, int ns, double jitter, double sigma2,
                    int init, double* out, hipStream_t st);
void launch_trmv_lower(const double* L, int ld, int n, const double* z, double mu, double* partial, double* out,
                       hipStream_t st);
void launch_syrk_upper_set(double* C, int ldc, const double* X, int ldx, int N, hipStream_t st);
void launch_syrk_upper_set(const BatchPtr& C, int ldc, const BatchPtr& X, int ldx, int N, int nb, hipStream_t st);
void launch_set_identity(double* R, int ld, int nc, hipStream_t st);
int grad_partials(int n, int d_ard = 0);      // partial-buffer elements of launch_grad_reduce (d_ard: the d of an ARD latent, else 0)
#define LMM_NGRAD 10                          // sums of one reduction: the 9 common ones and a locally periodic latent's d/d decay ([9], written for that kind only)
#define LMM_ARD_GRAD_DMAX 32                  // widest ARD latent the gradient reduction serves (per-dimension sums in registers)
// g.ils != nullptr (an ARD latent, d <= LMM_ARD_GRAD_DMAX): out8[0] is d/d multiplier and out_ard[k] = d/d l_k (d values)
void launch_grad_reduce(const double* Kinv, int ld, int n, int nsplit, const double* alpha, const double* delta, const double* x, int d,
                        LatentDev g, double* partial, double* out7, hipStream_t st, double* out_ard = nullptr);
// Input gradient of one latent (grad_x_kernel): gx (d x n, column-major) = d logpdf_l / d x from the lower triangle of Kinv, alpha and
// x; accumulate: gx += instead of gx =.  partial: grad_x_partial_elems(n, d) doubles.  d <= LMM_ARD_GRAD_DMAX.
size_t grad_x_partial_elems(int n, int d);
void launch_grad_x(const double* Kinv, int ld, int n, const double* alpha, const double* x, int d, LatentDev g, double* partial,
                   double* gx, bool accumulate, hipStream_t st);
// Predictive-marginal input gradients.  C (M x N) {=, -=} A (M x K) B (K x N), NN form (trsm_nn_kernel): the products
// of the right solve R <- R L^-1; set = true is the in-place 64-column leaf (C == A, N = K = 64).
void launch_trsm_nn(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& A, size_t offA, int lda, const BatchPtr& B, size_t offB,
                    int ldb, int M, int N, int K, bool set, int nb, hipStream_t st);
// gx (d x ns) {=, +=} d/d xs of sum_s mbar_s mean_l(xs_s) + vbar_s var_l(xs_s) for one latent (pred_grad_x_kernel): W = R L^-1 (ns rows,
// ldw), or nullptr for the mean-only form.  partial: pred_grad_x_partial_elems(n, ns, d) doubles.  d <= LMM_ARD_GRAD_DMAX.
size_t pred_grad_x_partial_elems(int n, int ns, int d);
void launch_pred_grad_x(const double* xs, int ns, const double* x, int n, int d, const double* alpha, const double* mbar,
                        const double* vbar, const double* W, int ldw, LatentDev g, double* partial, double* gx, bool accumulate,
                        hipStream_t st);
void launch_vec_axpby(const double* a, double sa, const double* b, double sb, size_t n, double* out, hipStream_t st);
void launch_block_trace(const double* Minv, int ld, int n, int m, int i0, int i1, double* out, hipStream_t st);   // points i0..i1-1
// Consecutive point ranges [off[b], off[b + 1]) that carry the observation-noise variance s2[b]: the conditioning batches of a
// sequentially conditioned posterior followed by the test points (gradient of the predictive logpdf).
#define LMM_MAX_NOISE_BLOCKS 8
struct NoiseBlocks {
  int nblk;
  int off[LMM_MAX_NOISE_BLOCKS + 1];
  double s2[LMM_MAX_NOISE_BLOCKS];
  int count(int b) const { return off[b + 1] - off[b]; }
};
// out[k] = a[k] + (num / s2[block of row k]) * b[k]   with row(k) = k mod N  (column-major N x p operands)
void launch_vec_lin_blocks(const double* a, const double* b, const NoiseBlocks& nb, double num, int N, size_t count, double* out, hipStream_t st);
// Missing observations (NaN in y).  p outputs, nw = ceil(p / 64) mask words per point or pattern; all Float64.
#define LMM_MISSING_MMAX 128                  // widest m the per-pattern m x m work serves
// masks[t nw + w], pt[t]: observed-output bits and their count for every point of y (n x p column-major, device)
void launch_missing_masks(const double* y, int n, int p, unsigned long long* masks, int* pt, hipStream_t st);
// per pattern: Tpat (m x p, zero columns at missing outputs) = G^-1 H_O', dinv (m) = diag G^-1, logdet = log det G, info = failed pivot
// or 0.  scratch: missing_pattern_scratch_elems(m, npat) doubles (0 for m <= 64: the m x m work is in LDS).
size_t missing_pattern_scratch_elems(int m, int npat);
void launch_missing_patterns(const double* H, int p, int m, const unsigned long long* pmask, int npat, double* scratch, double* Tpat,
                             double* dinv, double* logdet, int* info, hipStream_t st);
// out_z, out_noise: [l1 - l0][n] (z - means, s2 dinv); resid: n x p or nullptr; part: 3 n doubles; sums3: sum_t |resid_t|^2, sum_t p_t,
// sum_t log det G_t (fixed order)
void launch_missing_apply(const double* y, int n, int p, int m, const int* pat_of, const unsigned long long* pmask, const double* Tpat,
                          const double* dinv, const double* logdet, const int* pt, const double* H, double s2, const double* means,
                          int l0, int l1, double* out_z, double* out_noise, double* resid, double* part, double* sums3,
                          hipStream_t st);
// out2 = [sum_t w_t alpha_t^2, sum_t w_t Kinv_tt]
void launch_missing_wdiag(const double* Kinv, int ld, int n, const double* alpha, const double* w, double* out2, hipStream_t st);
// gy (n x p) = -T_t' alpha_t - resid / s2 at observed entries (resid nullptr: first term only), 0 at missing ones; alpha: [ms][lda]
void launch_missing_grad_y(int n, int p, int m, const int* pat_of, const unsigned long long* pmask, const double* Tpat,
                           const double* alpha, int lda, int l0, int ms, const double* resid, double s2, double* gy, hipStream_t st);
// Inducing-point (VFE) moments.  All Float64 in both compute dtypes.
#define LMM_SPARSE_MMAX 1024                  // most inducing points
#define LMM_SPARSE_DMAX 32                    // widest input
// One latent of a moments launch: its kernel, per-point noise w (device, n values; nullptr: the constant wconst), the projected data r
// (device, n values; rsub is subtracted) and kdiag = kappa(0).
struct SparseLat { LatentDev g; const double* w; const double* r; double wconst, rsub, kdiag; int sum_per; };   // sum_per: a sum with a (locally) periodic term
struct SparseMomArgs {
  const double* x; const double* z;           // d x n inputs, d x nz inducing inputs (device)
  int d, n, nz, chunk, nch;                   // chunk points per partial, nch = ceil(n / chunk) partials
  double* scratch;                            // nb * nch * sparse_partial_stride(nz) doubles
  SparseLat lat[LMM_MAX_BATCH];
};
static_assert(sizeof(SparseMomArgs) <= 4096, "SparseMomArgs is passed by value: kernel arguments are limited to 4096 bytes");
size_t sparse_partial_stride(int nz);         // doubles of one (latent, chunk) partial: the 64 x 64 tiles of Phi's lower triangle, b, 3 scalars
int sparse_default_chunk(int n, int nz, int nb);
// Phi (the lower 64 x 64 tiles with nz padded to 64, zero rows beyond nz), b, (s, kappa, lambda) of nb latents in one launch
// (blockIdx.z = latent) into a.scratch, one partial per chunk; no atomics.  mode: as launch_sparse_grad's, of these nb latents.
void launch_sparse_moments(const SparseMomArgs& a, int nb, int mode, hipStream_t st);
// The partials added in chunk order: Phi.p[l] (nz x nz, column-major ld; the lower triangle, mirror: also the upper), b.p[l] (nz),
// scal.p[l] (3).
void launch_sparse_finish(const double* scratch, int nch, int nz, const BatchPtr& Phi, int ld, bool mirror, const BatchPtr& b,
                          const BatchPtr& scal, int nb, hipStream_t st);
// Out.p[l] (N x N, ld) = In.p[l]'
void launch_sparse_transpose(const BatchPtr& In, const BatchPtr& Out, int ld, int N, int nb, hipStream_t st);
// Bm.p[l] (NR x NC, ld) = [I + sym(Q.p[l]) on the leading M x M, identity pad; rider row NC = row NC of Au.p[l]]; trace[l] = tr Q.p[l]
void launch_sparse_bmat(const BatchPtr& Q, const BatchPtr& Au, const BatchPtr& Bm, int ld, int NC, int NR, int M, double* trace,
                        int nb, hipStream_t st);
// Gradient of the bound: the second pass over the points (sparse_grad_kernel).  One latent of a launch: its kernel as
// the forward pass evaluates it (g), its nterms gradient descriptors (gd, device: a plain latent has one), w / r as SparseLat, PhiBar
// (nz x nz, both triangles, leading dimension SparseGradArgs.ld), beta (nz) and the output d elbo / d r (n values, or nullptr).
struct SparseGradLat {
  LatentDev g; const LatentDev* gd; int nterms;
  const double* w; const double* r; double wconst, rsub;
  const double* PhiBar; const double* beta; double* grad_r;
};
struct SparseGradArgs {
  const double* x; const double* z;           // d x n inputs, d x nz inducing inputs (device)
  int d, n, nz, chunk, nch, ld;
  double* scratch;                            // nb * nch * ceil(nz / 64) * sparse_grad_partial_stride(d) doubles
  const SparseGradLat* lat;                   // device, one per latent of the launch (blockIdx.z)
};
size_t sparse_grad_partial_stride(int d);     // doubles of one (latent, chunk, tile row) partial: LMM_SUM_MAX_TERMS (4 + d) sums and 64 x d input sums
void launch_sparse_grad(const SparseGradArgs& a, int nb, int mode, hipStream_t st);
// recs.p[l]: LMM_SUM_MAX_TERMS records of LMM_NGRAD + d sums ([0], [7], [8], [9] and the d per-dimension ones; zeros elsewhere);
// gz.p[l]: d x nz input sums (or nullptr).  Partials added in chunk order, then in tile-row order.
void launch_sparse_grad_finish(const double* scratch, int nch, int nz, int d, const BatchPtr& recs, const BatchPtr& gz, int nb,
                               hipStream_t st);
// beta.p[l] (M) = R.p[l] c.p[l] for the upper triangular R (M x M, ld)
void launch_sparse_beta(const BatchPtr& R, int ld, int M, const BatchPtr& c, const BatchPtr& beta, int nb, hipStream_t st);
// PB.p[l] = (Ki - Si - beta beta') / 2 (both triangles); lower(Si.p[l]) <- -2 PB + sym(T2)
void launch_sparse_phibar(const BatchPtr& Ki, const BatchPtr& Si, const BatchPtr& T2, const BatchPtr& beta, const BatchPtr& PB, int ld,
                          int M, int nb, hipStream_t st);
// State-space inference for Matern and SHO latents over a one-dimensional input (lmm_kernels_ss.hip).  All Float64.
// One latent of a launch: variance, 1 / lengthscale (an SHO latent's 1 / period), the constant added to the smoothed means, per-point
// noise w (device, n values; +Inf: unobserved), data r (device, n values) and an SHO latent's quality factor (unused by the Matern models).
struct SSLat { double var, inv_ls, mean; const double* w; const double* r; double quality; double var2, inv_ls2, quality2; };
struct SSArgs {
  const double* x; int n, chunk, nch;         // sorted inputs (device); points per thread; nch = ceil(n / chunk) threads per latent
  double* agg;                                // nb * ss_fwd_agg_elems(D, nch) doubles: the forward aggregates and the scan's levels
  double* bagg;                               // nb * ss_bwd_agg_elems(D, nch) doubles (smoother only)
  double* fmean; double* fvar;                // filtered first-component mean / variance, [latent][n] (nullptr: not written)
  double* state; size_t state_stride;         // filtered states, [latent][ss_state_comps(D)][n] (nullptr: not kept); doubles per latent
  double* part;                               // nb * nch log-density partials
  double* smean; double* svar;                // smoothed first-component mean (+ lat.mean) / variance, [latent][n]
  double* sstate; double* fkeep;              // kept for the posterior object (nullptr: not kept; else both, and smean may be nullptr): the
                                              // full smoothed (zero-mean) and the filtered states POINT-major, [latent][n][ss_state_comps(D)]
  double* dagg;                               // nb * ss_dual_agg_elems(D, nch, seeds) doubles: the (value, tangent) aggregates (gradients only)
  double* dpart;                              // nb * seeds * nch tangents of the log-density partials (gradients only)
  SSLat lat[LMM_MAX_BATCH];
  double* gdt;                                // d lml / d (x_t - x_{t-1}), [latent][n] with 0 at t = 0 (nullptr: not written; behind lat, so that
                                              // the kernels from before it read their arguments where they did)
};
static_assert(sizeof(SSArgs) <= 4096, "SSArgs is passed by value: kernel arguments are limited to 4096 bytes");
// The model of a launch: 1 / 2 / 3 = Matern12 / 32 / 52 (the state dimension), SS_MODEL_SHO = the damped oscillator (state dimension 2)
#define SS_MODEL_SHO 4
// The model of a sum of two terms inside one latent (DESIGN.md 4.18 "Sum latents"): SS_PAIR(a, b) of the term models a, b above, in the
// library's one order of the terms (Matern12, Matern32, SHO, Matern52) and with a state dimension D_a + D_b <= 4.  Every *Lat struct
// carries the second term's (var2, inv_ls2, quality2) behind its own fields, which the one-term models do not read.
#define SS_PAIR(a, b) (16 * (a) + (b))
int ss_model_of(int kind);                    // the model of a base kind, 0 for a kind without one
int ss_pair_model(int a, int b, int* swapped);// the model of the sum of the term models a, b (*swapped: b comes first in it); 0: not served
int ss_model_dim(int model);                  // its state dimension
int ss_model_seeds(int model);                // parameters its forward-mode gradient seeds: 2 (variance, lengthscale), SHO 3 (+ quality); a sum: its terms' together
int ss_state_dim(int kind);                   // 1 / 2 / 3 for Matern12 / 32 / 52, 2 for SHO, 0 for every other kind
int ss_state_comps(int D);                    // doubles of one filtered state: D + D (D + 1) / 2
int ss_default_chunk(int n);                  // the library's plan: a function of n alone
size_t ss_fwd_agg_elems(int D, int nch);      // per latent
size_t ss_bwd_agg_elems(int D, int nch);
// fold, scan, filter (and, lml != nullptr, lml[l] = latent l's log density) of nb latents of one model
void launch_ss_filter(const SSArgs& a, int model, int nb, double* lml, hipStream_t st);
// the same in reverse over the filtered states a.state: smoothed marginals into a.smean / a.svar
// a.gdt != nullptr: and every spacing's d lml / d dt into a.gdt, from what the backward recursion holds when it steps from t + 1 to t
void launch_ss_smooth(const SSArgs& a, int model, int nb, hipStream_t st);
// grad_x[t] = sum over the ms latents, in their order, of g_l[t] - g_l[t + 1] (g_l[n] = 0) where w_l[t] < +Inf, and exactly 0 where
// it is not: d lml / d x_t from the spacings' derivatives g ([latent][n], SSArgs::gdt) and the noise w ([latent][n])
void launch_ss_grad_x(const double* g, const double* w, int n, int ms, double* grad_x, hipStream_t st);
// Gradients.  gtheta[NS l + s], NS = ss_model_seeds(model): d lml_l / d variance (s = 0), d lml_l / d lengthscale (s = 1) and, SHO,
// d lml_l / d quality (s = 2) by the forward-mode (dual number) instantiation of fold, scan and filter; a.dagg and a.dpart are its workspace
size_t ss_dual_agg_elems(int D, int nch, int nseeds);     // per latent, all seeds
void launch_ss_grad(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st);
// from a.smean / a.svar (no mean added): alpha, grad_w ([latent][n]) = -d lml / d r_t, d lml / d w_t (0 at unobserved points) and
// sums[4 l + q] = sum_t alpha, w alpha^2, w c, grad_w in a fixed order; ppart: nb * 4 * ss_point_blocks(n) doubles
int ss_point_blocks(int n);
void launch_ss_point(const SSArgs& a, int nb, double* alpha, double* grad_w, double* ppart, double* sums, hipStream_t st);
// Sampling.  One (latent, sample) pair of a launch: variance, 1 / lengthscale, its standard normals z (device, D n values, component i
// of point t at z[i n + t]), the constant added to the path, the path it writes (device, n values: the first component of the state)
// and an SHO latent's quality factor.
struct SSPathLat { double var, inv_ls, mean; const double* z; double* f; double quality; double var2, inv_ls2, quality2; };
struct SSPathArgs {
  const double* x; int n, chunk, nch;         // as SSArgs
  double* agg;                                // nb * ss_aff_agg_elems(D, nch) doubles: the affine aggregates and the scan's levels
  SSPathLat lat[LMM_MAX_BATCH];
};
size_t ss_aff_agg_elems(int D, int nch);      // per pair
// fold, scan and restart of the prior paths of nb pairs of one model
void launch_ss_path(const SSPathArgs& a, int model, int nb, hipStream_t st);
// rp[latent k][sample q][n] = r_k - f[q][k] - sqrt(w_k) xi[q xi_stride + k n] at observed points, r_k where w = +Inf (xi not read)
void launch_ss_pathwise(const double* r, const double* w, const double* f, const double* xi, size_t xi_stride, int n, int ms, int N,
                        double* rp, hipStream_t st);
// f[sample q][latent k][n] += sm[k][q][n]
void launch_ss_addpath(double* f, const double* sm, int n, int ms, int N, hipStream_t st);
// *flag (preset to INT_MAX) = the first t with !(x_t >= x_{t-1})
void launch_ss_sorted(const double* x, int n, int* flag, hipStream_t st);
// The posterior at new inputs from stored states (DESIGN.md 4.18 "Posterior object").  One latent of a launch: variance, 1 / lengthscale,
// the constant added to the means and an SHO latent's quality.  Component c of point t of latent z's filtered (smoothed) state is
// fstate (sstate)[z state_stride + c comp_stride + t point_stride]: comp_stride = 1, point_stride = ss_state_comps(D) is the point-major
// layout the posterior object keeps (SSArgs::sstate, fkeep); comp_stride = n, point_stride = 1 the component-major one of SSArgs::state.
struct SSInterpLat { double var, inv_ls, mean, quality; double var2, inv_ls2, quality2; };
struct SSInterpArgs {
  const double* x; int n;                     // sorted training inputs (device)
  const double* xs; int ns;                   // the queries (device), in any order
  const double* fstate; const double* sstate; size_t state_stride, comp_stride, point_stride;
  double* mean; double* var;                  // [latent][ns]: first-component mean (+ lat.mean) and variance
  SSInterpLat lat[LMM_MAX_BATCH];
  double* dmean; double* dvar;                // launch_ss_interp_dx only, [latent][ns]: their derivatives with respect to the query
};
// one thread per (query, latent) of nb latents of one model
void launch_ss_interp(const SSInterpArgs& a, int model, int nb, hipStream_t st);
// the same threads write a.dmean, a.dvar (not nullptr) instead: d mean / d xs and d var / d xs per (query, latent); a.mean, a.var not read
void launch_ss_interp_dx(const SSInterpArgs& a, int model, int nb, hipStream_t st);
// grad_xs[q] = sum over the ms latents, in their order, of (sum_o dmean[q + o ns] H[o + l p]) dmu[l ns + q] + (sum_o dvar[q + o ns]
// H[o + l p]^2) dv[l ns + q]; dmean or dvar may be nullptr (its term is left out), H is p x ms column-major; one thread per query
void launch_ss_contract_dx(const double* dmean, const double* dvar, const double* H, int p, int ms, const double* dmu, const double* dv,
                           int ns, double* grad_xs, hipStream_t st);
// *flag (preset to INT_MAX) = the first t with xs_t NaN or +-Inf
void launch_ss_finite(const double* xs, int ns, int* flag, hipStream_t st);
// Sampling from the posterior object (DESIGN.md 4.18 "Sampling from the posterior object").  The window of the sorted queries xs: the
// ns queries and the training points first .. first + count - 1 that lie between the smallest and the largest of them, W = ns + count
// points ordered by input (a training point before an equal query, equal queries in their order).
// out[0] = #{t : x_t <= lo}, out[1] = #{t : x_t <= hi} (device); xs != nullptr: lo = xs[0], hi = xs[ns - 1] are read on the device
void launch_ss_window_bounds(const double* x, int n, const double* xs, int ns, double lo, double hi, int* out, hipStream_t st);
// src[W] (device): window position j holds training point src[j] >= 0, or query -1 - src[j]; one thread per point, no atomics
void launch_ss_window(const double* x, int n, const double* xs, int ns, int first, int count, int* src, hipStream_t st);
// One (latent, sample) pair of a launch: the latent's parameters, its stored states (device, point-major n x ss_state_comps(D)), the
// pair's standard normals z (device, D W values, component i of window point j at z[i W + j]) and the path it writes (device, ns values
// in the order of the sorted queries: the first component of the state + mean).
struct SSPostLat { double var, inv_ls, mean, quality; const double* fstate; const double* sstate; const double* z; double* f; double var2, inv_ls2, quality2; };
// what every scan over a window takes, in front of its own fields (the kernels read their arguments by offset)
struct SSWindowArgs {
  const double* x; int n;                     // sorted training inputs (device)
  const double* xs; int ns;                   // sorted queries (device)
  const int* src; int first, W;               // the window (launch_ss_window)
  int chunk, nch;                             // window points per thread; nch = ceil(W / chunk) threads per entry
  double* agg;                                // nb * ss_aff_agg_elems(D, nch) (SSLpdfArgs: ss_fwd_agg_elems, not read when nch == 1) doubles:
                                              // the aggregates and the scan's levels
};
struct SSPostArgs : SSWindowArgs {
  SSPostLat lat[LMM_MAX_BATCH];
};
static_assert(sizeof(SSPostArgs) <= 4096, "SSPostArgs is passed by value: kernel arguments are limited to 4096 bytes");
// fold from the right, suffix scan and restart of the backward recursion for nb pairs of one model
void launch_ss_post_path(const SSPostArgs& a, int model, int nb, hipStream_t st);
// Predictive log density from the posterior object (DESIGN.md 4.18 "Predictive log density from the posterior object"): the Kalman
// filter over the window's backward chain, from its last point down to its first.  One latent of a launch: its parameters, its stored
// states (as SSPostLat) and the noise w and data r of the ns sorted queries (device; +Inf: an unobserved query).  Training points of
// the window are unobserved steps.
struct SSLpdfLat { double var, inv_ls, mean, quality; const double* fstate; const double* sstate; const double* w; const double* r; double var2, inv_ls2, quality2; };
struct SSLpdfArgs : SSWindowArgs {
  double* part;                               // nb * nch log-density partials
  SSLpdfLat lat[LMM_MAX_BATCH];
};
static_assert(sizeof(SSLpdfArgs) <= 4096, "SSLpdfArgs is passed by value: kernel arguments are limited to 4096 bytes");
// fold from the right, suffix scan and restart (nch == 1: the restart alone, which is then the sequential filter) and lml[l] = latent
// l's log p(queries' data | training data)
void launch_ss_post_logpdf(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st);
// Appending observations (DESIGN.md 4.18 "Appending observations").  The filter over k new points whose predecessor is a stored state.
// One latent of a launch: its parameters, the noise w and data r of the k points (device), the packed state `init` (device,
// ss_state_comps(D) values: mean, then the upper triangle of the covariance) of the point in front of them, and `out` (device), where
// the k filtered states go point-major, k x ss_state_comps(D): row n of the latent's block of the posterior object.
struct SSFromLat { double var, inv_ls, quality; const double* w; const double* r; const double* init; double* out; double var2, inv_ls2, quality2; };
struct SSFromArgs {
  const double* x; int n, chunk, nch;         // the k = n new inputs, sorted (device); points per thread; threads per latent
  double x0;                                  // the input of the stored state, <= x[0]
  double* agg;                                // nb * ss_fwd_agg_elems(D, nch) doubles (not read when nch == 1)
  double* fmean; double* fvar;                // filtered first-component mean / variance, [latent][k] (nullptr: not written)
  double* part;                               // nb * nch log-density partials
  SSFromLat lat[LMM_MAX_BATCH];
};
static_assert(sizeof(SSFromArgs) <= 4096, "SSFromArgs is passed by value: kernel arguments are limited to 4096 bytes");
// fold, scan, restart from the stored state (nch == 1: the restart alone, which is then the sequential filter) and lml[l] = the log
// density of latent l's new points given everything in front of them
void launch_ss_filter_from(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st);
// The smoother over kept states: reads the filtered states point-major from a.fkeep and writes the full smoothed states point-major
// to a.sstate, latent z's block z * a.state_stride doubles in (the stride is the capacity's, not n's).  a.state, a.smean, a.svar,
// lat.w and lat.r are not read: the recursion consumes filtered states and inputs only.
void launch_ss_smooth_kept(const SSArgs& a, int model, int nb, hipStream_t st);
// *flag (device) = 1 when some xs_t < bound, else 0; one workgroup, no atomics
void launch_ss_any_below(const double* xs, int ns, double bound, int* flag, hipStream_t st);
// rows idx[0 .. nsel) of an n x p column-major matrix into an nsel x p one, and back
void launch_ss_gather_rows(const double* in, int n, int p, const int* idx, int nsel, double* out, hipStream_t st);
void launch_ss_scatter_rows(const double* in, int n, int p, const int* idx, int nsel, double* out, hipStream_t st);
void launch_atb(const double* X, int ldx, const double* Z, int ldz, int n, int na, int nb, double* out, hipStream_t st);
void launch_fill(double* p, int n, double v, hipStream_t st);
void launch_reorder(const double* in, int n, int p, int to_outputs, double* out, hipStream_t st);
void launch_vec_lin(const double* a, const double* b, double sb, int n, double* out, hipStream_t st);  // out = a + sb*b
// out[(row0 + i rs) + (col0 + j cs) ldo] = src[i + j lds] (src a MATRIX in the compute dtype, out Float64): a block of cov(f, x, y)
void launch_block_scatter(const double* src, int lds, int nr, int nc, double* out, size_t ldo, size_t row0, int rs, size_t col0, int cs,
                          hipStream_t st);
void launch_normals(unsigned long long seed, unsigned long long stream, size_t count, double* out, hipStream_t st);
void launch_mfma_peak(double* out, int blocks, int iters, hipStream_t st);
