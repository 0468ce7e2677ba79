// lmm_emul.h -- exact int8 modular emulation of a Float64 product C -= A B' (DESIGN.md 4.17): constants and the scalar steps (row
// scaling, residues, CRT reconstruction) shared by the device kernels (lmm_kernels_i8.hip) and the host-only test entry
// lmm_dev_emul_host (lmm_api.hip), so that the CPU test checks the very code the GPU runs.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LMM_HD __host__ __device__
#else
#define LMM_HD
#endif

#define LMM_EMUL_MAXMOD 16
#define LMM_EMUL_MINMOD 8
#define LMM_EMUL_MAXBITS 58      // |a'| <= 2^58: the bit budget of 16 moduli at K = 128 (emul_residues takes any |v| < 2^63)

// The 16 largest pairwise-coprime integers <= 256; the first nmod of them are used.
static constexpr int kEmulModuli[LMM_EMUL_MAXMOD] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193};

// By-value kernel argument.  w_t = (P / p_t) ((P / p_t)^-1 mod p_t) < P; every w_t and P itself are cut at bits 85 and 44 into three
// doubles (41 + 41 + 44 bits, each exact).
struct EmulConst {
  int nmod;
  int p[LMM_EMUL_MAXMOD];
  double w1[LMM_EMUL_MAXMOD], w2[LMM_EMUL_MAXMOD], w3[LMM_EMUL_MAXMOD];
  double P1, P2, P3, Pinv, Phalf;
};

typedef unsigned __int128 emul_u128;

inline emul_u128 emul_modulus_product(int nmod) {
  emul_u128 P = 1;
  for (int t = 0; t < nmod; ++t) P *= (emul_u128)kEmulModuli[t];
  return P;
}
inline void emul_split3(emul_u128 v, double& a, double& b, double& c) {
  a = std::ldexp((double)(uint64_t)(v >> 85), 85);
  b = std::ldexp((double)(uint64_t)((v >> 44) & ((uint64_t(1) << 41) - 1)), 44);
  c = (double)(uint64_t)(v & ((uint64_t(1) << 44) - 1));
}
inline EmulConst emul_make_const(int nmod) {
  EmulConst c{};
  c.nmod = nmod;
  const emul_u128 P = emul_modulus_product(nmod);
  emul_split3(P, c.P1, c.P2, c.P3);
  c.Pinv = 1.0 / ((c.P1 + c.P2) + c.P3);
  c.Phalf = 0.5 * ((c.P1 + c.P2) + c.P3);
  for (int t = 0; t < nmod; ++t) {
    const int p = kEmulModuli[t];
    c.p[t] = p;
    const emul_u128 Mt = P / (emul_u128)p;
    const int r = (int)(Mt % (emul_u128)p);
    int inv = 1;
    while ((r * inv) % p != 1) ++inv;
    emul_split3(Mt * (emul_u128)inv, c.w1[t], c.w2[t], c.w3[t]);
  }
  return c;
}
// Largest b <= LMM_EMUL_MAXBITS with K 2^(2b) < P / 2: a depth-K dot product of integers |a'| <= 2^b is determined by its residues.
inline int emul_bits(int nmod, long long K) {
  const emul_u128 half = emul_modulus_product(nmod) / 2;
  int b = LMM_EMUL_MAXBITS;
  while (b > 0 && (emul_u128)K > ((half - 1) >> (2 * b))) --b;      // K 2^(2b) <= half - 1, without overflowing 128 bits
  return b;
}

// Shapes the emulation takes, and the scratch one update needs: host arithmetic shared by the launcher (lmm_kernels_i8.hip) and the
// factorisation's planner (lmm_potrf_plan.h).  M x N outputs (M >= N) of depth K in 256 x 256 tiles; int32 accumulators: K 128^2 <= 2^28.
#define LMM_EMUL_TILE 256
inline bool emul_shape_ok(int M, int N, int K) { return M >= N && N >= 1 && K >= 128 && K % 128 == 0 && K <= 16384; }
// byte offsets in the scratch of G matrices going through it together: residues of the panel, of the product, row maxima, scales, exponents
struct EmulLayout { size_t R, U, amax, sc, ex, total; int Mp, Np; };
inline EmulLayout emul_layout(int M, int N, int K, int G, int nmod) {
  auto rup256 = [](size_t v) { return (v + 255) & ~size_t(255); };
  EmulLayout L{};
  L.Mp = (M + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE * LMM_EMUL_TILE; L.Np = (N + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE * LMM_EMUL_TILE;
  size_t o = 0;
  L.R = o; o += rup256((size_t)G * nmod * L.Mp * K);
  L.U = o; o += rup256((size_t)G * nmod * L.Np * L.Mp);
  L.amax = o; o += rup256((size_t)G * L.Mp * 8);
  L.sc = o; o += rup256((size_t)G * L.Mp * 8);
  L.ex = o; o += rup256((size_t)G * L.Mp * 4);
  L.total = o;
  return L;
}
inline size_t emul_scratch_bytes(int M, int N, int K, int G, int nmod) { return emul_layout(M, N, K, G, nmod).total; }

// ---- live K blocks (zero skip) ----
// Per matrix and per 256-row tile row of the panel, one bit per 128-wide K block (K <= 16384: 128 bits, bit = k / 128, two 64-bit
// words): set by the convert when any truncated integer of that block of rows is non-zero.  A block whose bit is clear holds zero
// residues for every modulus and adds exactly zero to every integer dot product, so the GEMM may leave its stage out.  The stage list
// of a tile is the set bits of (mask of its A rows) & (mask of its B rows) below K / 128, in increasing k; an empty intersection is
// replaced by bit 0 alone (one stage of zeros), so that every tile has at least one stage.  Both sides of the GEMM's pipeline take
// the list from here: the staging cursor walks it (emul_mask_first, emul_mask_pop), the MFMA loop counts it (emul_mask_count).
#define LMM_EMUL_MASK_WORDS 2
struct EmulMask { unsigned long long w0, w1; };
inline size_t emul_mask_bytes(int M, int G) { return (size_t)G * ((M + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE) * LMM_EMUL_MASK_WORDS * 8; }
LMM_HD inline EmulMask emul_live_stages(EmulMask a, EmulMask b, int nk) {      // 1 <= nk <= 128
  const unsigned long long ones = ~0ull;
  EmulMask m;
  m.w0 = a.w0 & b.w0 & (nk >= 64 ? ones : ones >> (64 - nk));
  m.w1 = nk > 64 ? (a.w1 & b.w1 & (ones >> (128 - nk))) : 0ull;
  if ((m.w0 | m.w1) == 0ull) m.w0 = 1ull;
  return m;
}
LMM_HD inline bool emul_mask_empty(EmulMask m) { return (m.w0 | m.w1) == 0ull; }
LMM_HD inline int emul_mask_count(EmulMask m) { return __builtin_popcountll(m.w0) + __builtin_popcountll(m.w1); }
LMM_HD inline int emul_mask_first(EmulMask m) { return m.w0 != 0ull ? __builtin_ctzll(m.w0) : 64 + __builtin_ctzll(m.w1); }      // m not empty
LMM_HD inline EmulMask emul_mask_pop(EmulMask m) {      // m without its first bit; m not empty
  if (m.w0 != 0ull) m.w0 &= m.w0 - 1ull; else m.w1 &= m.w1 - 1ull;
  return m;
}

// ---- the GEMM's walk: work ids per XCD ----
// Workgroups b and b + 8 share an XCD.  The nids work ids are cut into min(nwg, 8) contiguous ranges, as equal as they can be (the
// first nids % parts ranges hold one more); range x belongs to the workgroups b with b % 8 == x, emul_range_wgs of them.  The ranges
// tile [0, nids) exactly, whatever nids and nwg >= 1.
struct EmulRange { int start, len; };
LMM_HD inline int emul_range_parts(int nwg) { return nwg < 8 ? nwg : 8; }
LMM_HD inline EmulRange emul_xcd_range(int nids, int nwg, int x) {      // 0 <= x < emul_range_parts(nwg)
  const int parts = emul_range_parts(nwg), q = nids / parts, r = nids - q * parts;
  return EmulRange{x * q + (x < r ? x : r), q + (x < r ? 1 : 0)};
}
LMM_HD inline int emul_range_wgs(int nwg, int x) { return (nwg >> 3) + (x < (nwg & 7) ? 1 : 0); }

// ---- dead pieces (dead blocks are never written) ----
// The convert works on pieces of 16 rows x 128 k, 16 per block.  A piece whose truncated integers are all zero is dead: it is neither
// read nor turned into residues.  emul_live_kernel finds the dead pieces from the block maxima (below) before the convert starts and
// sets their bits here, 16 bits per (matrix, tile row, K block), two blocks per 32-bit word -- one 16-bit store per block, every
// block of a group written, so nothing is cleared beforehand.  The convert writes zero residues into the dead pieces of the blocks the
// GEMM may stage -- the live ones, and block 0 for the empty-intersection fallback of emul_live_stages -- and into no other block.
#define LMM_EMUL_PIECE_ROWS 16
#define LMM_EMUL_PIECES (LMM_EMUL_TILE / LMM_EMUL_PIECE_ROWS)
LMM_HD inline size_t emul_piece_block(int tile_rows, int nkb, int z, int trow, int kb) { return ((size_t)z * tile_rows + trow) * nkb + kb; }
LMM_HD inline size_t emul_piece_word(size_t block) { return block >> 1; }
LMM_HD inline unsigned emul_piece_shift(size_t block) { return (unsigned)(block & 1) * LMM_EMUL_PIECES; }
inline size_t emul_piece_bytes(int M, int G, int K) {
  const size_t blocks = (size_t)G * ((M + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE) * (K / 128);
  return (blocks + 1) / 2 * 4;
}
// The small arrays of one group beside its residues: the live masks, then the dead-piece bitmap (byte offsets; a multiple of 8 each;
// `total` bytes for a caller that keeps the block maxima elsewhere: a factorisation).  An update on its own keeps the block maxima of
// its group behind them, [matrix][K block][row] with M rows per block, and needs `total_bmax` bytes.
struct EmulAux { size_t masks, pieces, total, bmax, total_bmax; };
inline EmulAux emul_aux(int M, int G, int K) {
  EmulAux a{};
  a.masks = 0;
  a.pieces = emul_mask_bytes(M, G);
  a.total = a.pieces + ((emul_piece_bytes(M, G, K) + 7) & ~size_t(7));
  a.bmax = a.total;
  a.total_bmax = a.bmax + (size_t)G * (K / 128) * M * 8;
  return a;
}

// ceil(log2 amax) for a finite amax > 0
LMM_HD inline int emul_row_exp(double amax) {
  int q;
  const double f = frexp(amax, &q);
  return f == 0.5 ? q - 1 : q;
}
// a' = trunc(a 2^sh), sh = b - e_row: an exact power-of-two scaling, |a'| <= 2^b
LMM_HD inline long long emul_trunc(double a, int sh) { return (long long)ldexp(a, sh); }
// ---- block maxima: liveness without reading the panel ----
// The scan that finds a row's maximum keeps, per row and 128-wide K block, the largest |a| of the block as a bit pattern (order-
// preserving for non-negative doubles).  |trunc(a 2^sh)| does not decrease with |a|, so the truncated integers of a (row, block) pair
// are all zero exactly when the block maximum's is: the pair is live iff emul_trunc(block maximum, b - e_row) != 0, for a row whose
// own maximum is finite and not zero (any other row is all zeros to the GEMM).  The very functions of the convert decide, so a
// subnormal scale or a maximum that is an exact power of two cannot fall on the other side.
// bytes of a factorisation's block maxima: nb matrices of NR rows, the first ncb 128-column blocks (all 8 bytes of a maximum are kept:
// the upper half would decide only where the threshold 2^(e_row - b) is a normal number)
inline size_t emul_block_max_bytes(int NR, int ncb, int nb) { return (size_t)nb * ncb * NR * 8; }
LMM_HD inline double emul_bits_as_double(unsigned long long u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)u);
#else
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
#endif
}
// row: bit pattern of the row's max |a| (a NaN is above everything); returns false for an all-zero row and for one with a NaN or an infinity
LMM_HD inline bool emul_row_live(unsigned long long row) { return row != 0ull && row < 0x7FF0000000000000ull; }
LMM_HD inline bool emul_block_live(unsigned long long row, unsigned long long blk, int bits) {
  return emul_row_live(row) && emul_trunc(emul_bits_as_double(blk), bits - emul_row_exp(emul_bits_as_double(row))) != 0;
}
// ---- negligible updates: tiles whose update cannot change a bit of C (the screen) ----
// Output (i, j) of an update of depth K is NEGLIGIBLE when C_ij is finite and not zero, both rows' maxima are finite, and either one
// of the rows is all zeros or
//     ceil(log2 K) + e_i + e_j + LMM_EMUL_NEG_MARGIN <= ilogb(C_ij),      e = emul_row_exp(row maximum), the convert's own exponent.
// Then fl(C_ij - T_ij) has the bits of C_ij, T_ij being the update the GEMM and the combine would form.  Proof, from the code: the
// convert makes |a'| <= 2^b (emul_trunc), so the integer X = sum_k a'_ik a'_jk has |X| <= K 2^(2b); the CRT returns X rounded once
// to Float64, |X~| <= K 2^(2b) (1 + 2^-53).  Both rows being live, sc = 1 and ex = e - b, so the combine subtracts
// T = ldexp(X~, e_i + e_j - 2b): an exact scaling, or a rounding to the subnormal grid, which gives 0 or at most doubles |T| (see
// the margin's spare binade below).  With L = ceil(log2 K), |T| <= 2^(L + e_i + e_j) (1 + 2^-52) <= 2^(q - 56) (1 + 2^-52) for q = ilogb(C_ij).
// The spacing of the doubles just BELOW |C_ij| is at least 2^(q - 53) (at a power of two; 2^(q - 52) elsewhere; the fixed 2^-1074 of
// the subnormals is no smaller than either, and ilogb is taken of the value, not of the exponent field), so |T| is below a quarter
// of the smaller of the two gaps around C_ij: the exact C_ij - T is strictly closer to C_ij than to either neighbour, and round-to-
// nearest returns C_ij.  (With an exact ldexp the derivation closes at a margin of 55 already -- |T| < half the lower gap; the 56th
// bit is the binade that a rounding of ldexp into the subnormals may use up, so 56 is what the code as written needs.)  An all-zero row gives X = 0 and
// T = 0 exactly.  A row with a NaN or an infinity is never negligible: its scale is NaN and must reach row i and column j of C.
// C_ij = +-0 counts as live (0 - T = -T), and so do an infinite or NaN C_ij (kept out of the argument, they cost nothing).
// The f64 kernel (potrf_node_kernel, screened by f64_screen_kernel with the same predicate and margin).  It forms acc = sum_k a_ik a_jk
// by f64 MFMAs -- fused multiply-adds, one rounding per term, in some order -- over the K columns of the panel or, with split-K, over
// a part of them, and stores fl(C_ij - acc), or adds -acc to C_ij atomically once per part.  |a_ik| <= 2^e_i, so every partial sum
// is at most K 2^(e_i + e_j) <= B = 2^(q - 56) in exact arithmetic, and, while the roundings are relative ones of 2^-53 each,
// |acc| <= B (1 + 2^-53)^K <= B (1 + 2^-38) for K <= 16384.  Roundings into the subnormal grid are absolute, at most 2^-1075 each:
// if q >= L - 1019 their sum K 2^-1075 <= 2^(L - 1075) <= B, so |acc| <= 2 B (1 + 2^-38) < 2^(q - 54), still below HALF the smaller
// gap 2^(q - 53) around C_ij -- the spare binade again; if q < L - 1019 every product is below 2^-1075, each fused add returns the
// zero it started from, and acc = 0.  Either way the exact C_ij - acc is strictly closer to C_ij than to a neighbour: the store keeps
// the bits of C_ij, and so does each atomic add of a part, whose bound is the same with fewer terms (C_ij is C_ij again before the
// next part arrives).  The cases kept live above stay live here; an all-zero row gives acc = 0 exactly.
// The kernels' screens and the host entry lmm_dev_emul_negligible all decide through emul_negligible.
#define LMM_EMUL_NEG_MARGIN 56
#define LMM_EMUL_NEG_NEVER 0x7FFFFFFF
#define LMM_EMUL_NEG_ALWAYS (-0x7FFFFFFF - 1)
LMM_HD inline int emul_ceil_log2(int K) {      // K >= 1
  int l = 0;
  while ((1 << l) < K) ++l;
  return l;
}
LMM_HD inline unsigned long long emul_double_bits(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned long long)__double_as_longlong(d);
#else
  unsigned long long u;
  __builtin_memcpy(&u, &d, 8);
  return u;
#endif
}
// ri, rj: bit patterns of the two rows' max |a| (as the scan keeps them); lgk = emul_ceil_log2(K).  The least ilogb(C_ij) at which the
// output is negligible; NEVER for a row with a NaN or an infinity, ALWAYS for an all-zero row
LMM_HD inline int emul_neg_bound(int lgk, unsigned long long ri, unsigned long long rj) {
  if (ri >= 0x7FF0000000000000ull || rj >= 0x7FF0000000000000ull) return LMM_EMUL_NEG_NEVER;
  if (ri == 0ull || rj == 0ull) return LMM_EMUL_NEG_ALWAYS;
  return lgk + emul_row_exp(emul_bits_as_double(ri)) + emul_row_exp(emul_bits_as_double(rj)) + LMM_EMUL_NEG_MARGIN;
}
LMM_HD inline bool emul_neg_at(int bound, double c) {
  const unsigned long long u = emul_double_bits(c) & 0x7FFFFFFFFFFFFFFFull;
  if (u == 0ull || u >= 0x7FF0000000000000ull || bound == LMM_EMUL_NEG_NEVER) return false;
  int q;
  (void)frexp(c, &q);      // |c| = f 2^q, 0.5 <= f < 1, subnormals included: ilogb(c) = q - 1
  return bound <= q - 1;
}
LMM_HD inline bool emul_negligible(int K, unsigned long long ri, unsigned long long rj, double c) {
  return emul_neg_at(emul_neg_bound(emul_ceil_log2(K), ri, rj), c);
}

// ---- zero extents: rows whose panel is exactly zero (void work) ----
// The ZERO EXTENT of a block of 64 rows of a factor matrix is the number of leading columns, in whole 64-column blocks of the lower
// triangle, in which every entry of those rows was stored as +0 by the launch that assembled the matrix.  The Gram launch keeps one
// int per 64-row block and matrix (gram_body: every thread ORs the bits of what it stores, one __syncthreads_or per tile, atomicMin
// of the tile's first column for a tile with a set bit; a row block that is all zeros keeps the memset's LMM_ZERO_EXT_NONE, larger
// than any column).  The test is on all 64 bits: a stored -0 counts as an entry.  An update would keep it (-0 - (+0) = -0), but the
// solve REPLACES the entry by its sum, +0, so leaving a solve out under a -0 would change a sign bit.  The kernels store products of
// non-negative factors, so only a rider value of -0 or a negative variance can put one there, and such a tile is simply live.
// Claim.  If every entry of the factor is finite, then L[i, p] = +0 for every row i of the block and every p < ext, at every point of
// the factorisation, whatever the schedule.  Induction on p: C[i, p] starts as +0.  Every update of it subtracts
// acc = sum_q L[i, q] L[p, q] over some q < p < ext, where L[i, q] = +0 by hypothesis: the accumulators start at +0 and every term is
// fma(+0, finite, +0) = +0 (the product may be -0; +0 + -0 = +0 in round-to-nearest), so acc = +0 and +0 - (+0) = +0: the store
// writes the bits that are there.  The solve multiplies the row's zeros by the finite inverse block, again sums of +-0 from +0: +0.
// Consequences, for rows [r, r + 64 k) with ext = the minimum over their blocks:
//   * an update item with the panel [j0, j0 + h) has acc = +0 in every entry when ext >= j0 + h, and stores what it loaded -- whatever
//     C is there, zero or not (C - (+0) = C for every C, -0 and NaN included);
//   * the atomic split-K form adds -acc = -0 once per part: C + (-0) = C for every C (+0 + -0 = +0, -0 + -0 = -0);
//   * the emulation: the rows' maxima are 0, the convert's integers are 0, X = 0 and the CRT returns +0 (emul_crt_finish: sums of
//     0 w_t from +0, q = +0), the combine subtracts ldexp(+0 sc_i sc_j, ..) = +0 for finite scales: T = +0, C - T = C bit for bit;
//   * a region row task over the block column [c0, c0 + 128 P) reads only +0 of its own row and writes only +0 when ext >= c0 + 128 P.
// A non-finite factor: the parent spreads 0 NaN into such rows, a build that leaves the work out does not.  A non-finite entry of a
// square reaches a diagonal entry of its block column or the next (d - sum l^2 is NaN or -Inf), whose pivot test !(d > 0) fails and
// records the pivot (diag_info_of / atomicCAS(info, 0, ..)): the status and the first failing pivot are the parent's; what lies
// below and right of a failed pivot is unspecified in either build.
#define LMM_ZERO_EXT_NONE 0x7F7F7F7F      // the value of a 0x7F memset: "no stored bit in this row block"
#define LMM_ZERO_EXT_PAD 4                // entries past the last row block that a 256-row tile may read; they hold LMM_ZERO_EXT_NONE
// ints per matrix of a batch's extents, [matrix][zero_ext_ld(NR)]: one per 64-row block and the pad
inline int zero_ext_ld(int NR) { return NR / 64 + LMM_ZERO_EXT_PAD; }
// zx: one matrix's extents.  True when the nblk 64-row blocks from row `row` are zero in every column below `need`.
LMM_HD inline bool zero_ext_void(const int* zx, int row, int nblk, int need) {
  int m = LMM_ZERO_EXT_NONE;
  for (int q = 0; q < nblk; ++q) { const int e = zx[row / 64 + q]; m = e < m ? e : m; }
  return m >= need;
}

// ---- the trapezoid's tile list, the live flags and the live id list ----
// Lower-trapezoid tiles (tm tile rows, tn tile columns, j <= i) in supertiles of 8 tile rows x 4 tile columns: 32 consecutive tiles
// share at most 12 operand panels.  xy (may be nullptr): 2 ints per tile, (tile row, tile column).  Returns the number of tiles.
inline int emul_tile_list(int tm, int tn, int* xy) {
  int n = 0;
  for (int I = 0; I < tm; I += 8)
    for (int J = 0; J < tn; J += 4)
      for (int i = I; i < (I + 8 < tm ? I + 8 : tm); ++i)
        for (int j = J; j < (J + 4 < tn ? J + 4 : tn); ++j)
          if (j <= i) {
            if (xy) { xy[2 * n] = i; xy[2 * n + 1] = j; }
            ++n;
          }
  return n;
}
// The screen leaves one byte per (matrix, tile): flags[(z tm + tile row) tn + tile column] != 0 when some entry the combine would write
// is not negligible (the bytes above the diagonal are never written or read).  The GEMM's work ids -- item-major, item = (matrix,
// modulus), the tile list inside -- are then compacted IN ORDER into the live id list: with `before` live tiles in the matrices
// before z and lc live tiles in z, the r-th live tile of z (in tile-list order) under modulus t sits at emul_live_slot, so the list
// is the increasing sequence of the live ids and an XCD's consecutive entries stay on one item's supertiles.  count[0] = entries
// (live ids), count[1] = live (matrix, tile) pairs.  emul_compact_host is the same arithmetic in plain C++ (tests/c).
LMM_HD inline size_t emul_flag_at(int tm, int tn, int z, int ti, int tj) { return ((size_t)z * tm + ti) * tn + tj; }
LMM_HD inline size_t emul_live_slot(int nmod, int before, int lc, int t, int r) { return (size_t)nmod * before + (size_t)t * lc + r; }
inline int emul_compact_host(const unsigned char* flags, const int* xy, int ntiles, int tm, int tn, int gc, int nmod, int* list) {
  int before = 0;
  for (int z = 0; z < gc; ++z) {
    int lc = 0;
    for (int k = 0; k < ntiles; ++k) lc += flags[emul_flag_at(tm, tn, z, xy[2 * k], xy[2 * k + 1])] != 0;
    int r = 0;
    for (int k = 0; k < ntiles; ++k) {
      if (flags[emul_flag_at(tm, tn, z, xy[2 * k], xy[2 * k + 1])] == 0) continue;
      for (int t = 0; t < nmod; ++t) list[emul_live_slot(nmod, before, lc, t, r)] = (z * nmod + t) * ntiles + k;
      ++r;
    }
    before += lc;
  }
  return nmod * before;
}
// byte offsets in the screen's own block for groups of G matrices (beside the scratch and the aux block, whose layouts stand)
struct EmulScreen { size_t flags, count, list, total; int ntiles; };
inline EmulScreen emul_screen_layout(int M, int N, int G, int nmod) {
  const int tm = (M + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE, tn = (N + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE;
  EmulScreen s{};
  s.ntiles = emul_tile_list(tm, tn, nullptr);
  s.flags = 0;
  s.count = ((size_t)G * tm * tn + 15) & ~size_t(15);
  s.list = s.count + 16;
  s.total = s.list + (size_t)G * nmod * s.ntiles * 4;
  s.total = (s.total + 7) & ~size_t(7);
  return s;
}

// ---- the convert kernel's residue step: no branch, no division, no 32-bit multiply per modulus ----
// |v| <= 2^58 is cut into its 8 bytes d_i.  For an odd modulus p, x = sum_i d_i (256^i mod p) <= 8 255 (p - 1) < 2^19 is congruent
// to |v|; the eight products are two 4-byte dot products against the packed constants lo and hi.  q = rint(x fl(1 / p)) is THE
// nearest integer to x / p: the float product is off by less than 2^-11.6 (x / p < 2^11.5, two roundings of 2^-24 each), and x / p
// is at least 1 / (2 p) >= 1 / 510 away from every half-integer because p is odd.  So x - q p lies in [-(p - 1) / 2, (p - 1) / 2]
// with no correction step.  Modulo 256 the residue is the low byte of v itself.
struct EmulDot { unsigned lo[LMM_EMUL_MAXMOD], hi[LMM_EMUL_MAXMOD]; float p[LMM_EMUL_MAXMOD], rp[LMM_EMUL_MAXMOD]; int xmax[LMM_EMUL_MAXMOD]; };
constexpr EmulDot emul_make_dot() {
  EmulDot d{};
  for (int t = 0; t < LMM_EMUL_MAXMOD; ++t) {
    const unsigned p = (unsigned)kEmulModuli[t];
    unsigned c = 1 % p, sum = 0;
    for (int i = 0; i < 8; ++i) {
      if (i < 4) d.lo[t] |= c << (8 * i); else d.hi[t] |= c << (8 * (i - 4));
      sum += c;
      c = (c * 256u) % p;
    }
    d.p[t] = (float)p;
    d.rp[t] = 1.0f / (float)p;
    d.xmax[t] = (int)(255u * sum);      // the largest x the reduction can see
  }
  return d;
}
static constexpr EmulDot kEmulDot = emul_make_dot();

#define LMM_EMUL_MAGIC 12582912.0f      // 1.5 2^23 = the float with the bits 0x4B400000: MAGIC + x has the bits 0x4B400000 + x for 0 <= x < 2^22
#define LMM_EMUL_MAGIC_BITS 0x4B400000u

LMM_HD inline unsigned emul_udot4(unsigned a, unsigned b, unsigned c) {      // c + sum of the four byte products of a and b
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
#endif
}
LMM_HD inline float emul_bits_as_float(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}
// sgn x mod p_t for 0 <= x <= xmax[t], sgn = +-1.0f and t >= 1, given xb = LMM_EMUL_MAGIC_BITS + x.  Every float operation is exact
// but the product with rp: sgn (MAGIC + x) - sgn MAGIC = +-x, and x - q p is a small integer.
LMM_HD inline int emul_reduce_odd(unsigned xb, float sgn, int t) {
  const float xf = fmaf(emul_bits_as_float(xb), sgn, -sgn * LMM_EMUL_MAGIC);
  const float q = rintf(xf * kEmulDot.rp[t]);
  return (int)fmaf(-q, kEmulDot.p[t], xf);
}
// The residues of v modulo the first NMOD moduli, as int8 bit patterns in the low bytes of r[0 .. NMOD - 1]
template <int NMOD>
LMM_HD inline void emul_residues(long long v, int* r) {
  const bool neg = v < 0;
  const unsigned long long m = neg ? (unsigned long long)(-v) : (unsigned long long)v;
  const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
  const float sgn = neg ? -1.0f : 1.0f;
  r[0] = (int)((unsigned)v & 0xFFu);
#pragma unroll
  for (int t = 1; t < NMOD; ++t) r[t] = emul_reduce_odd(emul_udot4(hi, kEmulDot.hi[t], emul_udot4(lo, kEmulDot.lo[t], LMM_EMUL_MAGIC_BITS)), sgn, t) & 0xFF;
}

// ---- the GEMM kernel's epilogue: an int32 accumulator, |x| <= 2^28 (K <= 16384 products of int8), modulo p ----
// x = hi 2^16 + lo with hi = x >> 16 (arithmetic, |hi| <= 2^12) and 0 <= lo < 2^16.  With c = 2^16 mod p in the symmetric range
// (|c| <= 127), y = hi c + lo is congruent to x and |y| <= 2^12 127 + 65535 < 2^19.2.  For an odd p, q = rint(y fl(1 / p)) is THE
// nearest integer to y / p: y is exact in float, the product carries two roundings of 2^-24 each, so it is off by less than
// 2^-23 |y| / p < 2^-23 2^19.2 / 193 < 2^-11.3, and y / p is at least 1 / (2 p) >= 1 / 510 > 2^-9 away from every half-integer.  So
// r = y - q p lies in [-(p - 1) / 2, (p - 1) / 2]: the symmetric residue, with no correction step.  The float steps run on MAGIC + y
// (bits LMM_EMUL_MAGIC_BITS + y for |y| < 2^22), and fma(-q, p, MAGIC + y) = MAGIC + r is exact, so the low byte of its bit pattern
// is r as an int8 and no int <-> float conversion is issued.  p = 256 takes the same steps: c = 0, y = lo, and whichever way the
// tie at lo mod 256 = 128 rounds, r = -+128 is congruent to x and has the low byte of x, which is the int8 residue in [-128, 127].
LMM_HD inline int emul_fold_const(int p) {
  const int r = 65536 % p;
  return r > p / 2 ? r - p : r;
}
// LMM_EMUL_MAGIC_BITS + y: lo is ORed into the zero low half of the constant, and hi c fits the 24-bit multiply-add
LMM_HD inline unsigned emul_acc_fold(int x, int c) {
  const int lo = (int)(((unsigned)x & 0xFFFFu) | LMM_EMUL_MAGIC_BITS);
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)(__mul24(x >> 16, c) + lo);
#else
  return (unsigned)((x >> 16) * c + lo);
#endif
}
// the largest |y| the quotient can see for |x| <= 2^28
LMM_HD inline int emul_acc_fold_max(int c) { return 4096 * (c < 0 ? -c : c) + 65535; }
// y mod p as an int8 bit pattern in the low byte, given yb = LMM_EMUL_MAGIC_BITS + y, |y| < 2^22; pf = (float)p, rp = 1.0f / pf
LMM_HD inline unsigned emul_fold_reduce(unsigned yb, float pf, float rp) {
  const float ym = emul_bits_as_float(yb);                                     // MAGIC + y
  const float q = rintf((ym - LMM_EMUL_MAGIC) * rp);
  const float rm = fmaf(-q, pf, ym);                                           // MAGIC + (y - q p)
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(rm) & 0xFFu;
#else
  unsigned u;
  __builtin_memcpy(&u, &rm, 4);
  return u & 0xFFu;
#endif
}
// x mod p as an int8 bit pattern in the low byte; c = emul_fold_const(p)
LMM_HD inline unsigned emul_acc_residue(int x, int c, float pf, float rp) { return emul_fold_reduce(emul_acc_fold(x, c), pf, rp); }

// The integer X, |X| < P / 2, with X = u_t mod p_t for all t, rounded once to Float64.  S1 and S2 are exact (41-bit chunks, 8-bit
// residues, 16 terms); S1 - q P1 and S2 - q P2 are exact; their sum rounds X to 53 bits; the third term is below one ulp of P.
LMM_HD inline double emul_crt_at(double S1, double S2, double S3, double q, const EmulConst& c) {
  return ((S1 - q * c.P1) + (S2 - q * c.P2)) + (S3 - q * c.P3);
}
// one modulus' term of the three sums, and the reconstruction from them: emul_crt in two pieces, for a caller that runs the sums of
// several outputs side by side (the combine kernel)
LMM_HD inline void emul_crt_term(int u, int t, const EmulConst& c, double& S1, double& S2, double& S3) {
  const double ut = (double)u;
  S1 += ut * c.w1[t];
  S2 += ut * c.w2[t];
  S3 += ut * c.w3[t];
}
LMM_HD inline double emul_crt_finish(double S1, double S2, double S3, const EmulConst& c) {
  double q = rint((S1 + S2) * c.Pinv);
  double X = emul_crt_at(S1, S2, S3, q, c);
  if (X > c.Phalf) X = emul_crt_at(S1, S2, S3, q + 1.0, c);
  else if (X < -c.Phalf) X = emul_crt_at(S1, S2, S3, q - 1.0, c);
  return X;
}
LMM_HD inline double emul_crt(const int* u, const EmulConst& c) {
  double S1 = 0.0, S2 = 0.0, S3 = 0.0;
#pragma unroll
  for (int t = 0; t < LMM_EMUL_MAXMOD; ++t)
    if (t < c.nmod) emul_crt_term(u[t], t, c, S1, S2, S3);
  return emul_crt_finish(S1, S2, S3, c);
}
