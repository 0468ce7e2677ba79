// lmm_potrf_plan.h -- what the batched blocked Cholesky launches for a shape (DESIGN.md "what is launched for a shape").  Plain C++17,
// no HIP: plan_potrf is a pure function of the shape, the batch, the device's CU count and the switches, so the schedule can be read
// and tested without a GPU (lmm_dev_potrf_plan, tests/test_potrf_plan_host.py).  The plan also owns the factorisation's scratch list,
// every step's wiring to it (kept row maxima and their covers, the f64 screen's flags and vote) and the extent invariants between
// them (plan_potrf_finish, plan_potrf_check; tests/c/potrf_scratch_check.cpp).  potrf_batch (lmm_api.hip) allocates what the plan
// lists and launches the step list.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "lmm_emul.h"

#define LMM_REGION_MAX_PANELS 8
#define LMM_REGION_ASST_MIN_C 4           // a helper's product for column block c >= this is split with its row's assistant
#define LMM_REGION_ASST_MIN_R (LMM_REGION_ASST_MIN_C + 2)
#define LMM_REGION_ASST_TILES ((2 * LMM_REGION_MAX_PANELS - LMM_REGION_ASST_MIN_R) * 16)

// Every knob of the factorisation.  The LMM_* values are read from the environment once, all together, by the first factor_switches()
// call of the process (lmm_kernels.hip) -- a factorisation, or one of the host-only plan hooks; the lmm_dev_set_* test hooks write the
// emulation fields.
enum { LMM_REGION_BY_RULE = 0, LMM_REGION_EVERYWHERE = 1, LMM_REGION_NEVER = 2 };
constexpr int kRuleAlways = 4096, kRuleShape = 2048;
constexpr double kRuleOuts = 4.0e7;      // between 16 x (2112 x 2048), which gains under 5 % emulated, and 4 x (6208 x 2048), which gains 20 %
struct FactorSwitches {
  int panel128 = 1;          // LMM_PANEL128=0: the round-2 path (64-column recursion) for every matrix
  int region = 1024;         // LMM_REGION=<columns>: widest block column potrf_region_kernel takes in one launch (at most 1024; 0: off)
  // LMM_REGION_ALL: the region kernel as the base case of matrices wider than `region`.  Unset: the rule of plan_potrf decides; a
  // non-zero value: always; 0 (or anything atoi reads as 0): never.  (Matrices of at most `region` columns are one region launch
  // whatever this says; LMM_REGION=0 turns those off.)
  int region_all = LMM_REGION_BY_RULE;
  int region_small = 512;    // LMM_REGION_SMALL=<columns>: the base case when the rule refuses `region` (a multiple of 128, else 0: panel launches)
  int fuse_bulk = 1;         // LMM_FUSE_BULK=0: a panel's bulk rows never ride in the update launch that factors its diagonal block
  int strip_items = 1;       // LMM_STRIP_ITEMS=0: the ragged last 64 rows of a long update as a separate launch; 2: in-launch also beside other batches
  int deterministic = 0;     // LMM_DETERMINISTIC=1: no split-K atomics in the update launches (bitwise reproducible sums)
  int region_asst = 1;       // LMM_REGION_ASST=0: no assistants; 2: also when they are not resident from the start (measured slower)
  int region_occ = 0;        // LMM_REGION_OCC=1 / 2: force the one- / two-workgroups-per-CU build of the region kernel
  int region_th = 0;         // LMM_REGION_TH=128 / 64: all row tiles of a region launch that high
  int region_trace = 0;      // LMM_REGION_TRACE=1: per-workgroup ticks of every region launch on stderr (synchronises the stream)
  // Float64 updates run as exact int8 modular GEMMs (lmm_kernels_i8.hip) where that pays: LMM_F64_EMUL=0 keeps them all
  // on the f64 MFMA kernel.  An explicit threshold -- LMM_F64_EMUL_MINK or lmm_dev_set_f64_emul(on, min_k, nmod) -- emulates every
  // update with K >= min_k.  With none the shape rule decides, emul_pays.  (-1: not read from the environment yet; counts as the default.)
  int emul_on = -1, emul_mink = -1, emul_nmod = LMM_EMUL_MAXMOD;
  int rule_always = kRuleAlways, rule_shape = kRuleShape;      // lmm_dev_set_f64_emul_rule
  double rule_outs = kRuleOuts;
  int emul_group_cap = 0;    // lmm_dev_set_emul_group: at most this many matrices per group of an emulated update (0: no cap)
  int emul_amax_reuse = 1;   // lmm_dev_set_emul_amax_reuse: 0 = every scanning update reads its whole panel for the row maxima (emul_amax_cover)
  // The f64 update launches leave out the 128 x 128 tiles whose update cannot change a bit of C (DESIGN.md 4.17 "the same screen on
  // the f64 kernel"): LMM_F64_SCREEN=0 turns that off, LMM_F64_SCREEN_MINK is the least K that earns its scan;
  // lmm_dev_set_f64_screen(on, min_k) writes both.  LMM_F64_SCREEN_VOTE=0: every screened update scans and screens, whatever the first one found.
  int f64_screen = 1, f64_screen_mink = 512, f64_screen_vote = 1;
  // Zero extents (lmm_emul.h): the Gram launch of a per-latent logpdf keeps, per 64-row block, how many leading columns it stored as +0, and
  // the region row tasks, update items and screens leave out work on rows that are zero across their panel.  LMM_ZERO_EXTENTS=0 (or
  // lmm_dev_set_zero_extents(0)): no extents are kept and every launch does what it did without them.
  int zero_extents = 1;
  // ... and only for matrices of more than this many columns (LMM_ZERO_EXTENTS_MINCOLS, lmm_dev_set_zero_extents_min_cols): at 2048
  // columns (`small`) the memset and the per-tile reduction cost 0.3 % and next to nothing is void, at 4096 (C1) the extents gain 17 %
  // (profiles/zero_extents/ab_summary.txt).  A matrix one region launch factors whole has no item that can be void at any setting.
  int zero_extents_min_cols = 2048;
  int f64_screen_rounds = 1; // f64_screen_pays: a screened launch has more work items than this many rounds of 2 per CU (0: no such rule; LMM_F64_SCREEN_ROUNDS)
};

enum PotrfStepKind {
  POTRF_DIAG64 = 0,          // diag64m_kernel: the 64 x 64 diagonal block at j0 (factor + inverse)
  POTRF_SOLVE64,             // the M rows below it, by the inverse block (launch_gemm_nt, set)
  POTRF_UPDATE,              // plain trailing update (launch_gemm_nt): columns [j0 + h, j0 + h + N) -= with the h columns from j0
  POTRF_LEAF128,             // leaf128_kernel: the 128 x 128 diagonal block at j0
  POTRF_PANEL_BULK,          // the M rows below that block (launch_panel_bulk)
  POTRF_UPDATE_LEAF,         // launch_update_leaf: the update + the leaf of the panel at j0 + h; fused_bulk: + that panel's bulk rows
  POTRF_EMUL_UPDATE_LEAF,    // the same update through the int8 emulation (group matrices at a time), then that leaf as a launch of its own
  POTRF_REGION,              // potrf_region_kernel: the whole block column [j0, j0 + N) in one launch; first_done: its first diagonal block is factored
  POTRF_STEP_KINDS
};
enum { POTRF_STRIP_NONE = 0, POTRF_STRIP_IN_LAUNCH = 1, POTRF_STRIP_SEPARATE = 2 };
// Profile classes: the lmm_prof_class values of include/lmm_hip.h, which this header does not see (lmm_internal.h asserts they agree)
enum { POTRF_CLS_UPDATE = 1, POTRF_CLS_UPDATE_NARROW = 2, POTRF_CLS_TRSM = 3, POTRF_CLS_DIAG = 4, POTRF_CLS_REGION = 5, POTRF_CLS_UPDATE_SHORT = 6 };

// The kept row-maximum arrays a scanning step reads instead of scanning (emul_amax_cover, below): those of step[0 .. n), which hold
// the maxima over the columns [j0, scan0) of its panel; the columns [scan0, j0 + h) are left to scan.
#define LMM_EMUL_COVER_MAX 8
struct EmulCover { int n = 0; int step[LMM_EMUL_COVER_MAX] = {}; int scan0 = 0; };

struct PotrfStep {
  int kind;
  int j0, h, N, M;           // first column; depth K of the product (the block's width for the other kinds); columns; rows (from row j0 + h of an update)
  int cls;                   // profile class
  double work, bytes;        // what ProfScope books for the step
  bool first_done = false, fused_bulk = false;
  int strip = POTRF_STRIP_NONE;      // UPDATE_LEAF: where a ragged last 64 rows of a K >= 1024 update go
  bool screened = false;             // UPDATE_LEAF: its panel's row maxima are scanned and kept, and the tiles of the column tiles 1.. are screened
  int update = -1;                   // UPDATE_LEAF, EMUL_UPDATE_LEAF: the step's entry in PotrfPlan.updates
  int group = 0; size_t scratch = 0; // EMUL_UPDATE_LEAF: matrices per group, scratch bytes at that group size (that entry's)
  // The step's wiring to the plan's scratch (plan_potrf_finish):
  bool keeps_amax = false;           // an emulated or screened update: it scans its panel's row maxima into a kept array of its own
  EmulCover cover;                   // ... reading these earlier steps' kept arrays for the columns [j0, cover.scan0) instead
  size_t flag_bytes = 0;             // screened: the bytes of the flag block its screen writes (f64_screen_flag_bytes)
  int vote_from = -1;                // screened: the step whose counters carry the vote it listens to (-1: it scans and screens whatever was found)
  size_t screen_bytes = 0;           // EMUL_UPDATE_LEAF: the bytes of the emulation's screen block one of its groups uses (emul_screen_layout)
  // the (M, N, K) ProfScope names: the 64-column path's diagonal blocks and solves go unnamed
  bool named() const { return kind != POTRF_DIAG64 && kind != POTRF_SOLVE64; }
};
// A trailing update with at least 128 columns, whether it is a launch of its own or runs inside a region launch (lmm_dev_emul_plan lists these)
struct PotrfUpdate { int M, N, K; bool emulated; int group; size_t scratch; };
struct PotrfPlan {
  bool panel128 = false;     // the 128-column panel path (else the round-2 recursion on 64 columns, which needs no scratch)
  int region_cols = 0;       // widest block column that becomes ONE region launch (0: none; then no region flags are needed)
  size_t w2_doubles = 0;     // per matrix: one 128 x 128 inverse per panel
  size_t node_flag_ints = 0; // per matrix: flags of the fused bulk rows, zeroed per factorisation (0: no launch fuses them)
  size_t asst_doubles = 0;   // per matrix: scratch tiles of the region launches' assistants (0: none)
  // The scratch block of the emulated updates: sized for the widest emulated level at G = min(4, nb, 12 GB / that level) matrices.  The
  // sizing also counts updates that end up inside a region launch, which only makes it generous.
  size_t emul_bytes = 0; int emul_G = 0, emul_nmod = 0;
  // ---- what plan_potrf_finish adds: every other array of the factorisation, in the bytes potrf_batch requests (scratch_round) ----
  // Each is an allocation of its own, so that the extent guard checks an access against the array it belongs to; all live until
  // the API call ends, like W2.
  // Row maxima: one array per step with keeps_amax, [matrix][NR] 8-byte words -- a later update whose panel contains an earlier one's
  // reads its maxima there instead of scanning those columns again (PotrfStep.cover).
  int amax_arrays = 0; size_t amax_bytes = 0;      // how many; bytes of each
  // The f64 screen: one flag byte per 128 x 128 tile in ONE block, sized for the screened step that needs most and
  // rewritten by every screened step in stream order, and two counters per step of the plan (dead tiles; 1 when the screen ran), zeroed
  // before the first launch.  The dead count of the first screened step with at least LMM_F64_SCREEN_VOTE_NT tile columns is the vote:
  // zero there and the later scans and screens of this factorisation return at entry (decaying data has dead tiles from the third or
  // fourth tile column on; a narrower update finds none either way and says nothing).  vote_step is that step whether or not
  // FactorSwitches.f64_screen_vote lets the later ones listen (PotrfStep.vote_from).
  size_t f64_flag_bytes = 0, f64_stat_bytes = 0; int vote_step = -1;
  // The emulated updates' small arrays, each rewritten by every group of every update in stream order.  Aux: live K blocks and dead
  // pieces of the panels (emul_aux), sized for the deepest emulated step, emul_kmax.  Screen: tile flags, live id list and counts
  // (emul_screen_layout), sized for the step that needs most.  Block maxima: ONE array for the factorisation, [matrix][128-column
  // block][NR], up to the last column block an emulated step's panel holds, emul_ncb; the scan of an update writes the blocks it reads,
  // a later update that covers them decides its live blocks and pieces from them without reading those columns.  batch_plan budgets
  // the block maxima by emul_stream_budget, which counts all NC / 128 blocks.
  int emul_kmax = 0, emul_ncb = 0; size_t emul_aux_bytes = 0, emul_screen_bytes = 0, emul_bmax_bytes = 0;
  // Zero extents (lmm_emul.h): taken when the caller has them, the matrices are Float64 and FactorSwitches.zero_extents is on; then
  // the caller's array holds zext_bytes, and, when the test hook asks, one counter of void work items per step, zeroed likewise.
  bool zext = false; size_t zext_bytes = 0, zext_stat_bytes = 0;
  std::vector<PotrfStep> steps;        // in launch order
  std::vector<PotrfUpdate> updates;    // in the order of the recursion
};

inline int potrf_split(int w) {      // left width of the recursive split (multiple of 64; of 128 when w >= 256)
  if (w >= 256) return (w / 2 + 127) / 128 * 128;
  return (w == 192) ? 128 : 64;
}
// Does emulating the M x N (x K) trailing update of nb matrices pay?  The ONE place that decides.  Between rule_shape and rule_always
// it does when the batch's trapezoid has at least rule_outs outputs -- at a fixed K = N both paths grow linearly with the rows and the
// matrix count, but the emulated one carries fixed costs (launches per group, the leaf and bulk launches of their own) that only a
// large enough update earns back (the crossover table of DESIGN.md 4.17).
inline bool emul_pays(int M, int N, int K, int nb, const FactorSwitches& sw) {
  if (sw.emul_mink > 0) return K >= sw.emul_mink;
  if (K >= sw.rule_always) return true;
  if (K < sw.rule_shape) return false;
  const double outs = (double)N * (N + 1.0) / 2.0 + ((double)M - N) * N;
  return nb * outs >= sw.rule_outs;
}
inline bool emul_takes(int M, int N, int K, int nb, const FactorSwitches& sw) { return emul_shape_ok(M, N, K) && emul_pays(M, N, K, nb, sw); }
// The block for a factorisation's emulated updates (PotrfPlan.emul_bytes, .emul_G); kEmulBlockCap: what G is cut to fit
constexpr double kEmulBlockCap = 12e9;
inline void emul_block_plan(PotrfPlan& P, int nb) {
  auto need = [&](int G) {
    size_t n = 0;
    for (const PotrfUpdate& u : P.updates) if (u.emulated) n = std::max(n, emul_scratch_bytes(u.M, u.N, u.K, G, P.emul_nmod));
    return n;
  };
  const size_t one = need(1);
  if (one == 0) return;
  P.emul_G = (int)std::max<size_t>(1, std::min<size_t>(std::min(4, nb), (size_t)kEmulBlockCap / one));
  P.emul_bytes = need(P.emul_G);
}
// Matrices per group of ONE update inside that block: as many as fit (a level below the widest needs less per matrix, so fewer groups
// and fewer launches), never fewer than the G the block was sized for
inline int emul_group(int M, int N, int K, int nb, const PotrfPlan& P, const FactorSwitches& sw) {
  int gs = (int)std::min<size_t>((size_t)nb, P.emul_bytes / emul_scratch_bytes(M, N, K, 1, P.emul_nmod));
  gs = std::max(gs, std::min(P.emul_G, nb));
  if (sw.emul_group_cap > 0) gs = std::min(gs, sw.emul_group_cap);
  return gs;
}

// ---- the f64 update launches' screen: flag bytes of one launch ----
// potrf_node_kernel's tiles are 128 x 128; the screen leaves one byte per (matrix, tile row, tile column) of the launch's MT x NT
// tile grid, flags[f64_screen_flag_at(MT, NT, z, ti, tj)] != 0 when some entry of the tile that the kernel would write -- i >= j,
// i < M, j < N -- is not negligible (emul_negligible, lmm_emul.h).  Only the bytes of the "rest" tiles, 1 <= tj <= ti < MT, are
// written and read.  MT counts the rows the node launch takes: a ragged last 64 rows that go to the strip are not among them.
#define LMM_F64_SCREEN_TILE 128
#define LMM_F64_SCREEN_VOTE_NT 4      // the vote is taken by the first screened update with at least this many tile columns (PotrfPlan.vote_step)
LMM_HD inline size_t f64_screen_flag_at(int MT, int NT, int z, int ti, int tj) { return ((size_t)z * MT + ti) * NT + tj; }
inline int f64_screen_rows(int M, int strip) { return strip != POTRF_STRIP_NONE ? M - 64 : M; }
inline size_t f64_screen_flag_bytes(int M, int N, int strip, int nb) {
  const int MT = (f64_screen_rows(M, strip) + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE, NT = (N + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE;
  return ((size_t)nb * MT * NT + 7) & ~size_t(7);
}
// rest tiles of one matrix: sum over tj = 1 .. NT - 1 of (MT - tj)
inline long long f64_screen_rest_tiles(int MT, int NT) {
  long long T = 0;
  for (int tj = 1; tj < NT && tj < MT; ++tj) T += MT - tj;
  return T;
}
// Does screening the M x N (x K) update of nb matrices pay?  Only a launch of more than `rounds` rounds of workgroups (two resident per
// CU) can get shorter by leaving tiles out: one that fits the device at once takes a tile time whatever is skipped, and the scan, the
// screen and their launches are pure cost (8 x 2048, one K = 1024 update of 288 work items: 1.16 -> 1.20 ms per evaluation with it
// screened).  An explicit threshold (LMM_F64_SCREEN_MINK, lmm_dev_set_f64_screen) sets rounds to 0: every update with K >= min_k and
// more than one tile column is screened, as the tests' small shapes need.
inline bool f64_screen_pays(int M, int N, int strip, int nb, int cus, const FactorSwitches& sw) {
  if (sw.f64_screen_rounds <= 0) return true;
  const int MT = (f64_screen_rows(M, strip) + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE, NT = (N + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE;
  return (long long)nb * (MT + f64_screen_rest_tiles(MT, NT)) > 2LL * cus * sw.f64_screen_rounds;
}

// The walk over the columns [0, NC) of nb matrices of NR rows.  rows_real: rows that hold data (the Gram rows + the real rider rows; -1:
// all NR) -- the work figures count those, not the 64-row padding of the riders.
struct PotrfPlanner {
  PotrfPlan P;
  const FactorSwitches& sw;
  int NR, nbi, rows; double nb;
  bool emul, node_fuse = false; int in_flight;
  int cus = 256;

  PotrfStep& add(int kind, int cls, int j0, int h, int N, int M, double work, double bytes = 0.0) {
    PotrfStep s{}; s.kind = kind; s.cls = cls; s.j0 = j0; s.h = h; s.N = N; s.M = M; s.work = work; s.bytes = bytes;
    P.steps.push_back(s);
    return P.steps.back();
  }
  // Round 2: columns [j0, j0 + w) by 64-column blocks -- diag64 + solve by its inverse, plain updates between the halves
  void cols64(int j0, int w) {
    if (w <= 64) {
      add(POTRF_DIAG64, POTRF_CLS_DIAG, j0, 64, 64, 64, nb * 2.0 * 64.0 * 64.0 * 64.0 / 3.0);
      const int M = NR - (j0 + 64);
      if (M > 0) add(POTRF_SOLVE64, POTRF_CLS_TRSM, j0, 64, 64, M, nb * (double)M * 64.0 * 64.0);      // triangular solve: M * 64^2 flops
      return;
    }
    const int h = potrf_split(w), r0 = j0 + h;
    cols64(j0, h);
    const double Mr = NR - r0, Nc = w - h;     // lower trapezoid: Nc(Nc+1)/2 + (Mr-Nc)Nc outputs, 2h flops each
    const double outs = Nc * (Nc + 1.0) / 2.0 + (Mr - Nc) * Nc;
    // algorithmic bytes: C read + written once (16 B per output), the A panel (Mr x h, which contains B) read once
    add(POTRF_UPDATE, Nc <= 64 ? POTRF_CLS_UPDATE_NARROW : POTRF_CLS_UPDATE, j0, h, w - h, NR - r0, nb * 2.0 * h * outs, nb * (16.0 * outs + 8.0 * Mr * h));
    cols64(r0, w - h);
  }
  // The updates with at least 128 columns of the recursion over [j0, j0 + w), in order (those of a region launch run inside it)
  bool note_update(int M, int N, int K) {
    const bool takes = sw.emul_on != 0 && emul_takes(M, N, K, nbi, sw);
    P.updates.push_back(PotrfUpdate{M, N, K, takes, 0, 0});
    return takes;
  }
  void inside_region(int j0, int w) {
    if (w < 256) return;
    const int h = potrf_split(w);
    inside_region(j0, h);
    note_update(NR - (j0 + h), w - h, h);
    inside_region(j0 + h, w - h);
  }
  // Round 3: the same recursion with 128-column panels.  A panel = leaf128 (its 128 x 128 diagonal block: factor, 64 x 64 inverse blocks,
  // full inverse into the W2 scratch) + ONE bulk GEMM (rows below: X = P Dinv'); and every trailing update also runs the leaf of the
  // panel that follows it, so that per 128 columns the stream sees two launches (update + leaf, bulk) instead of six.  first_done: the
  // diagonal block of the first panel of [j0, j0 + w) is already factored; bulk_done (implies first_done): the rows below that block
  // are solved as well (the update launch that factored it ran them too).  Widths that are not multiples of 128 (NC = 64 mod 128) end
  // in the round-2 path for their last 64 columns.
  void panels(int j0, int w, bool first_done, bool bulk_done) {
    if (P.region_cols > 0 && w <= P.region_cols && w >= 128 && (w % 128) == 0) {
      // the whole block column as ONE dataflow launch (lmm_kernels.hip K2d): leaves, bulk products and all updates inside it
      const double Mr = rows - j0, Wd = w;
      const double fl = Mr * Wd * Wd - 2.0 * Wd * Wd * Wd / 3.0;           // flops of factoring an Mr x Wd tall panel: Mr Wd^2 - 2 Wd^3 / 3
      add(POTRF_REGION, POTRF_CLS_REGION, j0, w, w, NR - j0, nb * fl).first_done = first_done;
      inside_region(j0, w);
      return;
    }
    if (w == 128) {
      if (!first_done) add(POTRF_LEAF128, POTRF_CLS_DIAG, j0, 128, 128, 128, nb * 2.0 * 128.0 * 128.0 * 128.0 / 3.0);
      const int M = NR - (j0 + 128);
      if (M > 0 && !bulk_done) {
        const double Mreal = rows - (j0 + 128);
        add(POTRF_PANEL_BULK, POTRF_CLS_TRSM, j0, 128, 128, M, nb * Mreal * 128.0 * 128.0);       // triangular solve: (real rows) * 128^2 flops
      }
      return;
    }
    if (w <= 64) { cols64(j0, w); return; }          // a trailing 64-column leaf (never pre-factored)
    const int h = potrf_split(w), r0 = j0 + h, Nc = w - h;
    panels(j0, h, first_done, bulk_done);
    const double Mr = rows - r0;
    const double outs = (double)Nc * (Nc + 1.0) / 2.0 + (Mr - Nc) * Nc;
    if (Nc < 128) {
      add(POTRF_UPDATE, POTRF_CLS_UPDATE_NARROW, j0, h, Nc, NR - r0, nb * 2.0 * h * outs, nb * (16.0 * outs + 8.0 * Mr * h));
      cols64(r0, Nc);
      return;
    }
    // K >= 1024: potrf_node_kernel<2> (+ gemm16h_kernel for a ragged last 64 rows) -- the dominant kernel; below: potrf_node_kernel<1>.
    // + the leaf's 2 * 128^3 / 3 flops, run by one workgroup of the launch.  Emulated: convert + int8 GEMMs + combine in place of the f64
    // update, then the leaf as a launch of its own; the same flop count, so the class's rate reads as an f64-EQUIVALENT rate.
    const int M = NR - r0;
    const bool emulated = note_update(M, Nc, h) && emul;
    // The bulk rows of the panel at r0 ride in the launches with 512 <= K <= 2048: below, the chain update -> leaf -> bulk inside one
    // launch is no shorter than two launches (K = 128: 115 us against 72 + 34); above, the fused build's 3-4 spilled registers cost the
    // long launches more (0.3 % of 11-30 ms) than the bulk launch they absorb (33 us).  + their Mb * 128^2 flops and 16 B per entry
    const bool fuse_k = !emulated && node_fuse && h >= 512 && h <= 2048;
    const double Mb = fuse_k ? std::max(0.0, Mr - 128.0) : 0;
    PotrfStep& s = add(emulated ? POTRF_EMUL_UPDATE_LEAF : POTRF_UPDATE_LEAF, h >= 1024 ? POTRF_CLS_UPDATE : POTRF_CLS_UPDATE_SHORT, j0, h, Nc, M,
                       nb * (2.0 * h * outs + 2.0 * 128.0 * 128.0 * 128.0 / 3.0 + Mb * 128.0 * 128.0), nb * (16.0 * outs + 8.0 * Mr * h + 16.0 * Mb * 128.0));
    s.update = (int)P.updates.size() - 1;
    if (!emulated) {
      s.screened = sw.f64_screen != 0 && h >= sw.f64_screen_mink && (h % 128) == 0 && (j0 % 128) == 0 && Nc > 128;
      s.fused_bulk = fuse_k && (M + 127) / 128 > 1;
      // ragged last row tile (the rider rows make the row count an odd multiple of 64): on the long products the node kernel takes the
      // full 128-row tiles and gemm16h_kernel the last 64 rows (two idle waves for a whole tile time otherwise) -- as work items of the
      // same launch, but only while no other batch runs beside this one: with two batches in flight (C2 at N = 1) the other stream's
      // kernels fill the CUs a separate launch leaves idle, and the in-launch items measured slower (687.2 -> 689.9 ms per step)
      if ((M % 128) == 64 && M - 64 >= Nc && (Nc % 128) == 0 && h >= 1024)
        s.strip = sw.strip_items && (in_flight <= 1 || sw.strip_items == 2) ? POTRF_STRIP_IN_LAUNCH : POTRF_STRIP_SEPARATE;
      s.screened = s.screened && f64_screen_pays(M, Nc, s.strip, nbi, cus, sw);
    }
    const bool fused = s.fused_bulk;
    panels(r0, Nc, true, fused);
  }
};

// Row maxima kept across the emulated updates of one factorisation.  An emulated update scans its panel -- columns
// [j0, j0 + h), rows from j0 + h -- for the largest |entry| of every row, and that array is kept until the factorisation ends
// (PotrfStep.keeps_amax).  The entries below a factored block column never change again, so a later update whose panel contains those columns, and
// whose rows begin at or below the kept array's first row, finds the exact maximum of that column range in it.  emul_amax_cover
// covers a prefix [j0, scan0) of the panel of steps[si] with the kept arrays of earlier scanning steps: from c = j0, the widest
// earlier panel that begins at c and ends at or before j0 + h (so its rows begin no later than ours, at j0 + h), then on from its
// end.  The columns [scan0, j0 + h) are left to scan.  It reads the step list only: no shape of the recursion is assumed.
// A scanning step is an emulated update or, with f64_too, a screened f64 update (PotrfStep.screened), which keeps the same array.
// An f64 step's array holds maxima only while the vote of the f64 screen has not switched its scans off, and an f64 step keeps no
// block maxima.  So plan_potrf_finish passes f64_too for the cover of a screened f64 step, which the same vote switches off and
// which reads no block maxima, and never for the cover of an emulated step: that one takes from emulated steps' arrays only.
inline bool emul_step_scans(const PotrfStep& e, bool f64_too) {
  return e.kind == POTRF_EMUL_UPDATE_LEAF || (f64_too && e.kind == POTRF_UPDATE_LEAF && e.screened);
}
inline EmulCover emul_amax_cover(const std::vector<PotrfStep>& steps, int si, bool reuse, bool f64_too = false) {
  const PotrfStep& s = steps[si];
  EmulCover c;
  c.scan0 = s.j0;
  const int end = s.j0 + s.h;
  while (reuse && c.n < LMM_EMUL_COVER_MAX && c.scan0 < end) {
    int best = -1;
    for (int t = 0; t < si; ++t) {
      const PotrfStep& e = steps[t];
      if (emul_step_scans(e, f64_too) && e.j0 == c.scan0 && e.j0 + e.h <= end && (best < 0 || e.h > steps[best].h)) best = t;
    }
    if (best < 0) break;
    c.step[c.n++] = best;
    c.scan0 += steps[best].h;
  }
  return c;
}

// ---- the factorisation's scratch and the steps' wiring to it ----
// The scratch allocator counts in doubles, so every array is requested in whole doubles.  scratch_round is the ONE place that rounds:
// a *_bytes field of the plan is the bytes actually requested, a multiple of 8, and potrf_batch asks for bytes / 8 doubles.
inline size_t scratch_round(size_t bytes) { return (bytes + 7) & ~size_t(7); }
inline size_t scratch_ints(size_t ints) { return scratch_round(ints * sizeof(int)); }
// The last pass of plan_potrf, pure like the rest: reads the step list, NR, nb and the switches.  zext: the caller has zero extents
// for this factorisation; zext_counters: the test hook wants the void work items counted.
inline void plan_potrf_finish(PotrfPlan& P, int NR, int nb, bool f32, bool zext, bool zext_counters, const FactorSwitches& sw) {
  const int n = (int)P.steps.size();
  P.amax_bytes = scratch_round((size_t)nb * NR * 8);
  if (P.emul_bytes > 0) P.emul_kmax = 128;
  for (int i = 0; i < n; ++i) {
    PotrfStep& s = P.steps[i];
    const bool screened = s.kind == POTRF_UPDATE_LEAF && s.screened, emulated = s.kind == POTRF_EMUL_UPDATE_LEAF;
    s.keeps_amax = screened || emulated;
    if (!s.keeps_amax) continue;
    ++P.amax_arrays;
    s.cover = emul_amax_cover(P.steps, i, sw.emul_amax_reuse != 0, screened);
    if (screened) {
      s.flag_bytes = scratch_round(f64_screen_flag_bytes(s.M, s.N, s.strip, nb));
      P.f64_flag_bytes = std::max(P.f64_flag_bytes, s.flag_bytes);
      if (P.vote_step >= 0) s.vote_from = sw.f64_screen_vote ? P.vote_step : -1;
      else if ((s.N + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE >= LMM_F64_SCREEN_VOTE_NT) P.vote_step = i;
    } else {
      s.screen_bytes = scratch_round(emul_screen_layout(s.M, s.N, std::min(s.group, nb), P.emul_nmod).total);
      P.emul_screen_bytes = std::max(P.emul_screen_bytes, s.screen_bytes);
      P.emul_kmax = std::max(P.emul_kmax, s.h);
      P.emul_ncb = std::max(P.emul_ncb, (s.j0 + s.h) / 128);
    }
  }
  if (P.f64_flag_bytes > 0) P.f64_stat_bytes = scratch_ints(2 * (size_t)n);
  if (P.emul_bytes > 0) {
    P.emul_aux_bytes = scratch_round(emul_aux(NR, nb, P.emul_kmax).total);
    P.emul_bmax_bytes = scratch_round(emul_block_max_bytes(NR, P.emul_ncb, nb));
  }
  P.zext = zext && !f32 && sw.zero_extents != 0;
  if (P.zext) P.zext_bytes = scratch_ints((size_t)zero_ext_ld(NR) * nb);
  if (P.zext && zext_counters) P.zext_stat_bytes = scratch_ints((size_t)n);
}
// What batch_plan sets aside per stream for a batch with this plan, in bytes: upper bounds that need no second plan when the batch
// is halved -- the emulation block at its cap, and block maxima for all NC / 128 column blocks (PotrfPlan.emul_bmax_bytes stops at
// emul_ncb <= NC / 128, the same formula).  0 when nothing is emulated.
inline double emul_stream_budget(const PotrfPlan& P, int NR, int NC, int nb) {
  return P.emul_bytes > 0 ? kEmulBlockCap + (double)emul_block_max_bytes(NR, NC / 128, nb) : 0.0;
}

// ---- the extent invariants of a finished plan ----
// Every one compares a step's figure with the plan's (or with NR); potrf_batch checks them once, before its first allocation.
enum PotrfInvariant {
  POTRF_INV_NONE = 0,
  POTRF_INV_FLAG_BYTES,      // screened: its flag bytes fit the flag block
  POTRF_INV_ROWS,            // screened, emulated: the update's rows j0 + h + M end within the NR rows of the matrix (and of a kept array)
  POTRF_INV_SCREEN_COLS,     // screened: its N columns lie within the rows the screen covers (f64_screen_rows)
  POTRF_INV_EMUL_SCRATCH,    // emulated: its scratch fits the emulation block
  POTRF_INV_EMUL_SCREEN,     // emulated: its screen bytes fit the emulation's screen block
  POTRF_INV_PANEL_BLOCKS,    // emulated: j0, h and scan0 - j0 are whole 128-column blocks (the block maxima are kept per block)
  POTRF_INV_BMAX_BLOCKS,     // emulated: its panel ends within the emul_ncb column blocks of the block maxima
  POTRF_INVARIANTS
};
struct PotrfViolation {
  int which = POTRF_INV_NONE, step = -1;
  long long needs = 0, has = 0;      // the two numbers of the relation (PANEL_BLOCKS: the offending column count and 128)
  explicit operator bool() const { return which != POTRF_INV_NONE; }
};
inline const char* potrf_invariant_text(int which) {
  static const char* const text[POTRF_INVARIANTS] = {"", "flag bytes of the screened update", "last row of the update against the matrix rows",
    "columns of the screened update against the rows its screen covers", "scratch bytes of the emulated update", "screen bytes of the emulated update",
    "columns of the emulated update's panel that are not whole 128-column blocks", "last column block of the emulated update's panel against the block maxima"};
  return which > POTRF_INV_NONE && which < POTRF_INVARIANTS ? text[which] : "";
}
// The first violated invariant in step order (nothing: all hold)
inline PotrfViolation plan_potrf_check(const PotrfPlan& P, int NR) {
  for (int i = 0; i < (int)P.steps.size(); ++i) {
    const PotrfStep& s = P.steps[i];
    const int r0 = s.j0 + s.h;
    auto bad = [&](int which, long long needs, long long has) { return PotrfViolation{which, i, needs, has}; };
    if (s.kind == POTRF_UPDATE_LEAF && s.screened) {
      if (s.flag_bytes > P.f64_flag_bytes) return bad(POTRF_INV_FLAG_BYTES, (long long)s.flag_bytes, (long long)P.f64_flag_bytes);
      if (r0 + s.M > NR) return bad(POTRF_INV_ROWS, r0 + s.M, NR);
      if (s.N > f64_screen_rows(s.M, s.strip)) return bad(POTRF_INV_SCREEN_COLS, s.N, f64_screen_rows(s.M, s.strip));
    }
    if (s.kind == POTRF_EMUL_UPDATE_LEAF) {
      if (s.scratch > P.emul_bytes) return bad(POTRF_INV_EMUL_SCRATCH, (long long)s.scratch, (long long)P.emul_bytes);
      if (s.screen_bytes > P.emul_screen_bytes) return bad(POTRF_INV_EMUL_SCREEN, (long long)s.screen_bytes, (long long)P.emul_screen_bytes);
      if (r0 + s.M > NR) return bad(POTRF_INV_ROWS, r0 + s.M, NR);
      for (int v : {s.j0, s.h, s.cover.scan0 - s.j0})
        if ((v % 128) != 0) return bad(POTRF_INV_PANEL_BLOCKS, v, 128);
      if (r0 / 128 > P.emul_ncb) return bad(POTRF_INV_BMAX_BLOCKS, r0 / 128, P.emul_ncb);
    }
  }
  return PotrfViolation{};
}

// in_flight: batches that run concurrently on the slot streams; ld_odd: the leading dimension is odd (the panel kernels' 16-byte
// accesses need an even one); emul_allowed: false once the API call could not get an emulation block (its remaining batches take the
// f64 path without asking again); zext, zext_counters: plan_potrf_finish
inline PotrfPlan plan_potrf(int NR, int NC, int nb, int rows_real, int in_flight, int cus, bool f32, bool ld_odd, bool strict, bool emul_allowed,
                            const FactorSwitches& sw, bool zext = false, bool zext_counters = false) {
  PotrfPlanner W{PotrfPlan{}, sw, NR, nb, rows_real >= 0 ? std::min(NR, rows_real) : NR, (double)nb, false, false, in_flight};
  PotrfPlan& P = W.P;
  W.cus = cus;
  // Float64 batches take the 128-column panel path; its W2 scratch -- one 128 x 128 inverse per panel and matrix -- lives until the API call ends
  P.panel128 = !(f32 || !sw.panel128 || NC < 128 || ld_odd);
  if (!P.panel128) { W.cols64(0, NC); plan_potrf_finish(P, NR, nb, f32, zext, zext_counters, sw); return P; }
  P.w2_doubles = (size_t)(NC / 128) * 16384;
  // Default: the region kernel serves matrices that are ONE region (NC <= 1024: the whole factorisation in one launch, the small-n
  // path); larger matrices take it as the base case of the panel recursion where the rule below says so.
  // Mid sizes / few matrices (round 3, tools/mid_probe.py): while a block column's dataflow launch -- 2 P square tasks + one per
  // 128-row tile below, per matrix -- is at most ~2.3 workgroups per CU, it beats the panel launches it replaces (8 latents: n = 1536
  // 1.34 -> 0.96 ms, 2048 1.97 -> 1.51, 3072 3.50 -> 2.93, 4096 5.80 -> 5.2, 8192 27.1 -> 26.5; 16 x 2048: 2.19 -> 2.01; a rank's
  // 4-latent share of C2: 94.5 -> 93.9); with more work per launch it does not (16 x 4096: a tie; the two concurrent 16-latent batches
  // of C2 at N = 1: 696 -> 706 ms).
  const bool by_rule = sw.region_all == LMM_REGION_BY_RULE && sw.region >= 1024 && NC > sw.region && (NC % 128) == 0;
  bool region_base = sw.region_all == LMM_REGION_EVERYWHERE;
  int region_cols = sw.region;
  if (by_rule) {
    const long long tasks = 2LL * (sw.region / 128) + ((NR + 127) / 128 - sw.region / 128);      // of the first (tallest) block column
    // (concurrent batches count together: configs[3]'s 8-latent batches at n = 8192 fit the rule one by one, but four of them in
    // flight do not -- 724 -> 748 ms per step with the dataflow base case, the same effect as for C2's two 16-latent batches)
    region_base = tasks * nb * in_flight <= (long long)(2.3 * cus);
    // Round 4: when the 1024-column block column is over that bound -- many matrices per launch: C2's 16-latent batches, 32 latents at
    // n = 2048 ... 4096 -- the base case is a 512-column block column instead of the panel launches: its row chains are 10 units long
    // instead of 36 (finer tasks for a machine that is oversubscribed many times over), the square's workgroups hold their CUs half as
    // long, and the K = 512 update between two of them runs at 60-64 TFLOP/s.  32 x 2048: 2.98 -> 2.64 ms, 32 x 4096: 15.2 -> 14.0,
    // 16 x 16384 on one stream: 346.8 -> 343.6, C2 at N = 1: 685.7-687.5 -> 683.1-684.2 ms.
    if (!region_base && sw.region_small > 0) { region_cols = sw.region_small; region_base = true; }
  }
  const bool region_here = region_cols > 0 && (region_base || (NC <= region_cols && (NC % 128) == 0));
  P.region_cols = region_here ? region_cols : 0;
  // The bulk rows of a panel ride in the update launch that factors its diagonal block (NODE_FUSE), behind per-call flags; not under
  // strict progress (bulk items wait for earlier items of the same launch), and not when the region kernel serves as the base case
  // (it solves the first panel's rows itself)
  W.node_fuse = sw.fuse_bulk && !strict && !region_here && NC > 128;
  if (W.node_fuse) P.node_flag_ints = (size_t)(2 + (NR + 127) / 128 + 1);
  if (region_here && std::min(NC, region_cols) > 64 * LMM_REGION_ASST_MIN_R) P.asst_doubles = (size_t)LMM_REGION_ASST_TILES * 4096;      // block columns with assistant rows
  W.emul = emul_allowed;
  P.emul_nmod = sw.emul_nmod;
  W.panels(0, NC, false, false);
  if (!emul_allowed) for (PotrfUpdate& u : P.updates) u.emulated = false;
  emul_block_plan(P, nb);
  for (PotrfUpdate& u : P.updates)
    if (u.emulated) { u.group = emul_group(u.M, u.N, u.K, nb, P, sw); u.scratch = emul_scratch_bytes(u.M, u.N, u.K, u.group, P.emul_nmod); }
  for (PotrfStep& s : P.steps)
    if (s.kind == POTRF_EMUL_UPDATE_LEAF) { s.group = P.updates[s.update].group; s.scratch = P.updates[s.update].scratch; }
  plan_potrf_finish(P, NR, nb, f32, zext, zext_counters, sw);
  return P;
}
// The emulation side of a Float64 factorisation's plan, whatever path and base case the other switches choose (lmm_dev_emul_plan, batch_plan)
inline PotrfPlan plan_potrf_emul_view(int NR, int NC, int nb, FactorSwitches sw) {
  sw.panel128 = 1;
  return plan_potrf(NR, NC, nb, -1, 1, 256, false, false, true, true, sw);
}

