// lmm_kernels_i8.hip -- the large Float64 trailing updates C -= A B' of the factorisation as exact int8 modular GEMMs.
// Built WITHOUT -amdgpu-mfma-vgpr-form=1.  Three steps per update, for groups of matrices:
//   1. emul_rowmax_kernel + emul_live_kernel + emul_convert_kernel: per panel row the exponent e_i = ceil(log2 max_k |a_ik|), the
//      integers a' = trunc(a 2^(b - e_i)) and their residues modulo nmod small coprime moduli as K-contiguous int8 rows (inside a
//      factorisation the maxima outlive the update, and a later update reads them for the columns it shares: emul_amax_fold_kernel).
//      The scan keeps the maximum of every row and 128-wide K block too; from those emul_live_kernel decides, before the convert
//      starts, which 256-row blocks and which of their pieces of 16 rows x 128 k hold a non-zero integer.  The convert loads live
//      pieces only; a dead piece gets zeros, without a load, where the GEMM may stage it, and no store anywhere else;
//   2. emul_gemm_kernel: one int8 SYRK-shaped GEMM per (matrix, modulus) on 256 x 256 tiles of the lower trapezoid, int32
//      accumulators, reduced mod p to one byte per output, as a persistent kernel whose tiles walk only the K blocks that are live
//      (not all zeros) in both operands (tools/i8_gemm_probe.hip holds a copy of the kernel without that skip,
//      i8_syrk_mod_kernel_ps with ABL = 6, beside the loops and kernels this one replaced; the probe stands alone: its numbers
//      speak for a K step and a tile's fixed cost, not for a level's time);
//   3. emul_combine_kernel: CRT reconstruction in Float64 (lmm_emul.h) and C_ij -= X 2^(e_i + e_j - 2b) for i >= j.
// Between 1 and 2, emul_screen_kernel marks the tiles in which no output can change by a bit (from the row maxima of 1 and C itself:
// emul_negligible, lmm_emul.h) and emul_compact_kernel lists the work ids of the others; 2 walks that list and 3 returns on a dead
// tile's flag.
// Integer sums are exact in any order: the result is bitwise reproducible.
#include "lmm_internal.h"
#include "lmm_emul.h"
#include <algorithm>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int TILE = LMM_EMUL_TILE, BK = 128;
constexpr int STAGE_BYTES = 2 * TILE * BK;      // A tile + B tile of one K step
constexpr unsigned long long ABS_MASK = 0x7FFFFFFFFFFFFFFFull, INF_BITS = 0x7FF0000000000000ull;

// Block maxima of a group's panels (lmm_emul.h): p[z zs + kblock ld + i] = max |a_ik| over the 128 columns of K block `kblock` of
// the panel, for its row i of matrix z, as a bit pattern.  p points at (first matrix, K block 0, row 0) of the panel inside whatever
// array holds it: the one of a factorisation (absolute column blocks and rows, ld = its rows) or the aux block of a single update.
struct EmulBlockMax { unsigned long long* p; size_t zs, ld; };

// One thread per row and K block of 128 columns, for the blocks kb / 128 .. K / 128 - 1 (kb, K multiples of 128): the block's maximum
// |a_ik| as a bit pattern (order-preserving for non-negative doubles; a NaN is above everything) goes to bm -- one plain store per
// entry, coalesced over the rows -- and amax[z as + i] = max(what is there, that maximum).  as: entries per matrix of amax.
// The scans of the f64 updates' screen keep no block maxima (bm.p == nullptr) and obey that screen's vote: a zero there means the
// factorisation's data does not decay, and the scan returns at entry (uniform over the grid; nobody reads its array then).
__global__ __launch_bounds__(256) void emul_rowmax_kernel(BatchPtr A, int g0, size_t off, int ld, int M, int as, int kb, unsigned long long* amax, EmulBlockMax bm,
                                                          const int* __restrict__ vote) {
  if (vote != nullptr && *vote == 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x, z = blockIdx.z;
  if (i >= M) return;
  const int k0 = kb + blockIdx.y * BK;
  const double* P = A.p[g0 + z] + off + i + (size_t)k0 * ld;
  unsigned long long m = 0;
#pragma unroll 8
  for (int k = 0; k < BK; ++k) m = max(m, (unsigned long long)__double_as_longlong(P[(size_t)k * ld]) & ABS_MASK);
  if (bm.p != nullptr) bm.p[(size_t)z * bm.zs + (size_t)(k0 / BK) * bm.ld + i] = m;
  atomicMax(&amax[(size_t)z * as + i], m);
}
// The first write of an update's kept row maxima: per row the largest of the maxima that earlier updates kept for parts of its panel
// (bit patterns again, so a NaN or an infinity found then is still there), 0 when there are none.  emul_rowmax_kernel adds the
// columns nobody has scanned yet.
__global__ __launch_bounds__(256) void emul_amax_fold_kernel(EmulAmaxKeep k, int M) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const size_t at = (size_t)blockIdx.y * k.ld + k.row0 + i;
  unsigned long long m = 0;
  for (int s = 0; s < k.n; ++s) m = max(m, k.src[s][at]);
  k.out[at] = m;
}

constexpr int CV_ROWS = 16, CV_K = 128, CV_PITCH = 130;
constexpr int CV_NO_ROW = -0x7FFFFFFF - 1;      // in place of a row's shift b - e_i: the row is all zeros to the GEMM
constexpr int CV_SPLIT = 4;                     // workgroups of the convert per (tile row, K block): each walks 16 / CV_SPLIT of the pieces
constexpr int CV_WG_ROWS = TILE / CV_SPLIT;     // (per batch of C2: 5.34 ms with 1, 4.94 with 2, 4.78 with 4, 4.76 with 16 = one per piece)

// Liveness of a group's panels from the block maxima, before the convert reads anything of the panel (zero skip on).  One workgroup
// per (256-row tile row, matrix), one thread per row: for every K block, emul_block_live (lmm_emul.h) of the row's maximum and the
// block's, ORed over the 16 rows of a piece by a wave ballot (a wave holds 4 pieces).  Thread k < K / 128 then stores the 16 dead-piece
// bits of K block k, and the first two waves store the tile row's two live-mask words (a block is live iff one of its pieces is):
// plain stores, every word of the group written, nothing cleared beforehand.  Padding rows and rows with a NaN, an infinity or only
// zeros are dead, as their truncated integers are zeros.
__global__ __launch_bounds__(256) void emul_live_kernel(int M, int Mp, int K, int bits, const unsigned long long* __restrict__ amax, int as, EmulBlockMax bm,
                                                        unsigned long long* masks, unsigned short* dead) {
  __shared__ unsigned char nib[LMM_EMUL_MASK_WORDS * 64][4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, trow = blockIdx.x, z = blockIdx.y, nkb = K / BK, tr = Mp / TILE;
  const int i = trow * TILE + tid;
  const unsigned long long row = i < M ? amax[(size_t)z * as + i] : 0ull;
  const bool ok = emul_row_live(row);
  const unsigned long long* b = bm.p + (size_t)z * bm.zs + i;
  for (int kb = 0; kb < nkb; ++kb) {
    const bool lv = ok && emul_block_live(row, b[(size_t)kb * bm.ld], bits);
    const unsigned long long bal = __ballot(lv);
    if (lane == 0) {
      unsigned n = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) n |= ((bal >> (16 * q)) & 0xFFFFull) != 0ull ? 1u << q : 0u;
      nib[kb][w] = (unsigned char)n;
    }
  }
  __syncthreads();
  if (tid < LMM_EMUL_MASK_WORDS * 64) {      // K block tid: waves 0 and 1 hold the two mask words
    unsigned lp = 0;
    if (tid < nkb) {
      lp = (unsigned)nib[tid][0] | (unsigned)nib[tid][1] << 4 | (unsigned)nib[tid][2] << 8 | (unsigned)nib[tid][3] << 12;
      dead[emul_piece_block(tr, nkb, z, trow, tid)] = (unsigned short)(~lp & 0xFFFFu);      // 16-bit field emul_piece_word / emul_piece_shift
    }
    const unsigned long long word = __ballot(lp != 0u);
    if (lane == 0) masks[((size_t)z * tr + trow) * LMM_EMUL_MASK_WORDS + w] = word;
  }
}

// CV_SPLIT workgroups of 256 threads per (256-row tile row, K block, matrix), NMOD moduli; each walks 16 / CV_SPLIT of the block's 16
// pieces of 16 rows x 128 k (blockIdx.x = tile row * CV_SPLIT + part).
// With the zero skip on (dead != nullptr) it first reads its live bit and its dead-piece bits (emul_live_kernel): a dead block other
// than block 0 returns at once, having read nothing of the panel and stored nothing; the dead pieces of a live block, and all of a
// dead block 0 (which emul_live_stages stages for an empty intersection), get zero residues for all planes -- 8 lanes of 16 B per row
// and plane -- without a panel load.  dead == nullptr: every piece is converted.
// A live piece: each thread issues its 8 loads (8 k of one row; 16 lanes cover 128 contiguous bytes of a column of the column-major
// panel), truncates them and writes the integers to LDS, [row][k] with a pitch of 130.  It then takes 4 consecutive k of two rows
// from LDS, forms the residues (emul_residues: constants folded into the instructions) and stores one dword per modulus straight to
// the K-contiguous int8 rows R[(z NMOD + t) Mp + i][k]: 32 lanes write 128 contiguous bytes.  The loads of the next live piece are
// issued before the current one is truncated, so they fly while its residues are formed.  Rows M .. Mp - 1 (padding up to the GEMM
// tile), all-zero rows and rows with a NaN or an infinity are not loaded and get zero residues.  The workgroups of K block 0 also write the row scales and exponents.
template <int NMOD>
__global__ __launch_bounds__(256) void emul_convert_kernel(BatchPtr A, int g0, size_t off, int ld, int M, int Mp, int K, int bits,
                                                           const unsigned long long* __restrict__ amax, int as, int8_t* __restrict__ R, double* sc, int* ex,
                                                           const unsigned long long* __restrict__ masks, const unsigned short* __restrict__ dead) {
  __shared__ long long lds[CV_ROWS * CV_PITCH];
  __shared__ int shift[TILE];
  const int tid = threadIdx.x, ti = tid & 15, tk = tid >> 4, trow = blockIdx.x / CV_SPLIT, part = blockIdx.x % CV_SPLIT, kbi = blockIdx.y, z = blockIdx.z, k0 = kbi * CV_K;
  const unsigned mine = ((1u << (LMM_EMUL_PIECES / CV_SPLIT)) - 1u) << (part * (LMM_EMUL_PIECES / CV_SPLIT));      // this workgroup's pieces
  unsigned dm = 0;      // the dead pieces
  if (dead != nullptr) {
    const unsigned long long mw = masks[((size_t)z * (Mp / TILE) + trow) * LMM_EMUL_MASK_WORDS + (kbi >> 6)];
    if (kbi != 0 && ((mw >> (kbi & 63)) & 1ull) == 0ull) return;
    dm = dead[emul_piece_block(Mp / TILE, K / CV_K, z, trow, kbi)] & mine;
  }
  if (tid / CV_WG_ROWS == part) {
    const int i = trow * TILE + tid;
    unsigned long long mb = 0;
    if (i < M) mb = amax[(size_t)z * as + i];      // as: entries per matrix of amax
    const bool finite = mb < INF_BITS, live = emul_row_live(mb);
    int e = 0;
    if (live) e = emul_row_exp(__longlong_as_double((long long)mb));
    shift[tid] = live ? bits - e : CV_NO_ROW;
    if (kbi == 0) {      // row scale: 0 for an all-zero (or padding) row, NaN for a row with a non-finite entry
      sc[(size_t)z * Mp + i] = live ? 1.0 : (finite ? 0.0 : __longlong_as_double(0x7FF8000000000000ll));
      ex[(size_t)z * Mp + i] = live ? e - bits : 0;
    }
  }
  __syncthreads();
  for (unsigned u = dm; u != 0u; u &= u - 1u) {
    const int pc = __builtin_ctz(u);
    for (int q = tid; q < NMOD * CV_ROWS * 8; q += 256) {
      const int t = q / (CV_ROWS * 8), row = (q >> 3) % CV_ROWS, col = q & 7;
      int8_t* dst = R + (((size_t)z * NMOD + t) * Mp + trow * TILE + pc * CV_ROWS + row) * K + k0 + col * 16;
      *reinterpret_cast<v4u*>(dst) = (v4u){0u, 0u, 0u, 0u};
    }
  }
  const double* P = A.p[g0 + z] + off + (size_t)(k0 + tk) * ld + trow * TILE + ti;
  auto load = [&](int pc, double (&a)[CV_K / 16]) {
    const bool live = shift[pc * CV_ROWS + ti] != CV_NO_ROW;
#pragma unroll
    for (int s = 0; s < CV_K / 16; ++s) a[s] = live ? P[pc * CV_ROWS + (size_t)(16 * s) * ld] : 0.0;
  };
  unsigned rest = ~dm & mine;
  double a[CV_K / 16], an[CV_K / 16];
  if (rest != 0u) load(__builtin_ctz(rest), a);
  const int kg = tid & 31;
  while (rest != 0u) {
    const int pc = __builtin_ctz(rest);
    rest &= rest - 1u;
    if (rest != 0u) load(__builtin_ctz(rest), an);
    const int sh = shift[pc * CV_ROWS + ti];
#pragma unroll
    for (int s = 0; s < CV_K / 16; ++s) lds[ti * CV_PITCH + tk + 16 * s] = sh != CV_NO_ROW ? emul_trunc(a[s], sh) : 0ll;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = (tid >> 5) + 8 * h;
      unsigned w[NMOD];
#pragma unroll
      for (int t = 0; t < NMOD; ++t) w[t] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int r[NMOD];
        emul_residues<NMOD>(lds[row * CV_PITCH + 4 * kg + j], r);
#pragma unroll
        for (int t = 0; t < NMOD; ++t) w[t] |= (unsigned)r[t] << (8 * j);
      }
      int8_t* dst = R + ((size_t)z * NMOD * Mp + trow * TILE + pc * CV_ROWS + row) * K + k0 + 4 * kg;
#pragma unroll
      for (int t = 0; t < NMOD; ++t) *reinterpret_cast<unsigned*>(dst + (size_t)t * Mp * K) = w[t];
    }
    __syncthreads();      // the next piece overwrites the integers
    if (rest != 0u) {
#pragma unroll
      for (int s = 0; s < CV_K / 16; ++s) a[s] = an[s];
    }
  }
}
template <int NMOD>
void launch_convert(int nmod, dim3 grid, hipStream_t st, const BatchPtr& P, int g0, size_t off, int ld, int M, int Mp, int K, int bits,
                    const unsigned long long* amax, int as, int8_t* R, double* sc, int* ex, const unsigned long long* masks, const unsigned short* dead) {
  if constexpr (NMOD > LMM_EMUL_MINMOD) {
    if (nmod != NMOD) return launch_convert<NMOD - 1>(nmod, grid, st, P, g0, off, ld, M, Mp, K, bits, amax, as, R, sc, ex, masks, dead);
  }
  emul_convert_kernel<NMOD><<<grid, 256, 0, st>>>(P, g0, off, ld, M, Mp, K, bits, amax, as, R, sc, ex, masks, dead);
}

// The tile list (emul_tile_list, lmm_emul.h) is built on the host once per (tile rows, tile columns) and kept on the device for the
// life of the process (a few KB per shape; one process drives one GPU).  nullptr: the allocation or the copy failed (*err says why).
const int2* emul_tiles(int tm, int tn, hipError_t* err) {
  static std::map<std::pair<int, int>, int2*> cache;
  auto it = cache.find({tm, tn});
  if (it != cache.end()) return it->second;
  std::vector<int2> v(emul_tile_list(tm, tn, nullptr));
  emul_tile_list(tm, tn, reinterpret_cast<int*>(v.data()));
  int2* d = nullptr;
  *err = hipMalloc((void**)&d, v.size() * sizeof(int2));
  if (*err != hipSuccess) return nullptr;
  *err = hipMemcpy(d, v.data(), v.size() * sizeof(int2), hipMemcpyHostToDevice);
  if (*err != hipSuccess) { (void)hipFree(d); return nullptr; }
  cache[{tm, tn}] = d;
  return d;
}

// The screen (lmm_emul.h, negligible updates): one workgroup per (tile of the trapezoid's list, matrix), one thread per row of the
// tile.  It tests the entries the combine would write -- i >= j, i < M, j < N -- with emul_negligible against the row maxima the
// convert takes its exponents from, SCR_COLS columns at a time (all loads of a chunk issued before the first is used), and stops at
// the first chunk that holds an entry that is not negligible: a live tile, and any tile of data that does not decay, reads one
// chunk; a dead tile reads its C once.  Thread 0 stores the tile's byte: a plain store, every byte the compaction and the combine
// read is written by each group.
constexpr int SCR_COLS = 16;
__global__ __launch_bounds__(256) void emul_screen_kernel(BatchPtr A, int g0, size_t offC, int ldc, int M, int N, int K, const unsigned long long* __restrict__ amax, int as,
                                                          const int2* __restrict__ tiles, int tm, int tn, unsigned char* flags,
                                                          const int* __restrict__ zext, int zext_ld, int zrow0, int* zstat) {
  const int tid = threadIdx.x, z = blockIdx.y;
  const int2 t = tiles[blockIdx.x];
  // zero extents (lmm_emul.h): the tile's four row blocks are zero across the panel, T = 0: not live, C unread.  Uniform, ahead of the barriers
  if (zext != nullptr && zero_ext_void(zext + (size_t)(g0 + z) * zext_ld, zrow0 + t.x * TILE, TILE / 64, zrow0)) {
    if (tid == 0) { flags[emul_flag_at(tm, tn, z, t.x, t.y)] = 0; if (zstat != nullptr) atomicAdd(zstat, 1); }
    return;
  }
  const int i = t.x * TILE + tid, j0 = t.y * TILE, jn = min(N, j0 + TILE), lgk = emul_ceil_log2(K);
  const unsigned long long* az = amax + (size_t)z * as;
  const unsigned long long ri = i < M ? az[i] : 0ull;
  const double* C = A.p[g0 + z] + offC + i;
  bool live = false;
  for (int jc = j0; jc < jn && !live; jc += SCR_COLS) {
    double cv[SCR_COLS];
    bool on[SCR_COLS];
#pragma unroll
    for (int q = 0; q < SCR_COLS; ++q) {
      const int j = jc + q;
      on[q] = j < jn && i >= j && i < M;
      cv[q] = on[q] ? C[(size_t)j * ldc] : 0.0;
    }
    bool lv = false;
#pragma unroll
    for (int q = 0; q < SCR_COLS; ++q)
      if (on[q]) lv |= !emul_neg_at(emul_neg_bound(lgk, ri, az[jc + q]), cv[q]);      // j < N <= M: the row maximum of column j's panel row exists
    live = __syncthreads_or(lv ? 1 : 0) != 0;
  }
  if (tid == 0) flags[emul_flag_at(tm, tn, z, t.x, t.y)] = live ? 1 : 0;
}
// The same screen in front of an f64 update launch (potrf_node_kernel, lmm_kernels.hip), over that launch's 128 x 128 tiles with tile
// column >= 1 -- its "rest" items; column 0 carries the leaf and what fused bulk tiles wait for, and is never screened.  One workgroup
// of 128 threads per (tile row, tile column - 1, matrix), one thread per row; the entries tested are the ones the kernel would write
// below or on the diagonal: i >= j, i < M, j < N.  Depth K of f64 MFMAs in any order: |acc| <= K 2^(e_i + e_j) (1 + 2^-52)^K, within
// the bound the predicate was proved for (lmm_emul.h, "the f64 kernel").  amax: the kept row maxima, row 0 = the region's first row.
// Thread 0 stores the tile's byte (f64_screen_flag_at): a plain store, every byte the node launch reads is written by every launch.
// stat[0] counts the dead tiles, stat[1] says that the screen ran.  vote: a zero there (the first screened update of this
// factorisation found no dead tile) makes every workgroup store "live" and return without reading C.
__global__ __launch_bounds__(128) void f64_screen_kernel(BatchPtr A, size_t offC, int ldc, int M, int N, int K, const unsigned long long* __restrict__ amax, int as,
                                                         int MT, int NT, unsigned char* flags, int* stat, const int* __restrict__ vote,
                                                         const int* __restrict__ zext, int zext_ld, int zrow0) {
  constexpr int T = LMM_F64_SCREEN_TILE;
  const int tid = threadIdx.x, ti = blockIdx.x, tj = blockIdx.y + 1, z = blockIdx.z;
  if (ti < tj) return;                                  // above the diagonal: no such item, the byte is never read
  unsigned char* flag = flags + f64_screen_flag_at(MT, NT, z, ti, tj);
  if (vote != nullptr && *vote == 0) {
    if (tid == 0) *flag = 1;
    return;
  }
  // zero extents (lmm_emul.h): the node kernel leaves this item out whatever the byte says; dead, C unread.  Uniform, ahead of the barriers
  if (zext != nullptr && zero_ext_void(zext + (size_t)z * zext_ld, zrow0 + ti * T, T / 64, zrow0)) {
    if (tid == 0) {
      *flag = 0;
      atomicAdd(&stat[0], 1);
      if (ti == MT - 1 && tj == 1 && z == 0) stat[1] = 1;
    }
    return;
  }
  const int i = ti * T + tid, j0 = tj * T, jn = min(N, j0 + T), lgk = emul_ceil_log2(K);
  const unsigned long long* az = amax + (size_t)z * as;
  const unsigned long long ri = i < M ? az[i] : 0ull;
  const double* C = A.p[z] + offC + i;
  bool live = false;
  for (int jc = j0; jc < jn && !live; jc += SCR_COLS) {
    double cv[SCR_COLS];
    bool on[SCR_COLS];
#pragma unroll
    for (int q = 0; q < SCR_COLS; ++q) {
      const int j = jc + q;
      on[q] = j < jn && i >= j && i < M;
      cv[q] = on[q] ? C[(size_t)j * ldc] : 0.0;
    }
    bool lv = false;
#pragma unroll
    for (int q = 0; q < SCR_COLS; ++q)
      if (on[q]) lv |= !emul_neg_at(emul_neg_bound(lgk, ri, az[jc + q]), cv[q]);      // j < N <= M: the row maximum of column j's panel row exists
    live = __syncthreads_or(lv ? 1 : 0) != 0;
  }
  if (tid == 0) {
    *flag = live ? 1 : 0;
    if (!live) atomicAdd(&stat[0], 1);
    if (ti == MT - 1 && tj == 1 && z == 0) stat[1] = 1;
  }
}
// The live id list (lmm_emul.h): one workgroup per matrix of the group, no workgroup reads what another writes.  Workgroup z counts
// the live tiles of the matrices before it and its own (ballots, tile-list order), then walks its tiles again and stores, for the
// r-th live one, its nmod ids at emul_live_slot -- consecutive r in consecutive lanes.  The last workgroup stores the two counts.
__global__ __launch_bounds__(256) void emul_compact_kernel(const unsigned char* __restrict__ flags, const int2* __restrict__ tiles, int ntiles, int tm, int tn, int nmod,
                                                           int* __restrict__ list, int* __restrict__ count) {
  __shared__ int part[2][4], woff[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, z = blockIdx.x;
  auto flag = [&](int zz, int k) {
    const int2 t = tiles[k];
    return flags[emul_flag_at(tm, tn, zz, t.x, t.y)] != 0;
  };
  int nb = 0, nl = 0;      // wave-uniform: live tiles this wave saw in the matrices before z, and in z
  for (int q0 = 0; q0 < z * ntiles; q0 += 256) {
    const int q = q0 + tid;
    nb += __popcll(__ballot(q < z * ntiles && flag(q / ntiles, q % ntiles)));
  }
  for (int k0 = 0; k0 < ntiles; k0 += 256) nl += __popcll(__ballot(k0 + tid < ntiles && flag(z, k0 + tid)));
  if (lane == 0) { part[0][w] = nb; part[1][w] = nl; }
  __syncthreads();
  const int before = part[0][0] + part[0][1] + part[0][2] + part[0][3], lc = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  int run = 0;      // live tiles of z before this chunk
  for (int k0 = 0, it = 0; k0 < ntiles; k0 += 256, ++it) {
    const int k = k0 + tid;
    const bool f = k < ntiles && flag(z, k);
    const unsigned long long bal = __ballot(f);
    if (lane == 0) woff[it & 1][w] = __popcll(bal);
    __syncthreads();      // woff[it & 1] is next written two chunks on, with a barrier in between
    int r = run + __popcll(bal & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v) r += woff[it & 1][v];
    if (f)
      for (int t = 0; t < nmod; ++t) list[emul_live_slot(nmod, before, lc, t, r)] = (z * nmod + t) * ntiles + k;
    run += woff[it & 1][0] + woff[it & 1][1] + woff[it & 1][2] + woff[it & 1][3];
  }
  if (z == (int)gridDim.x - 1 && tid == 0) { count[0] = nmod * (before + lc); count[1] = before + lc; }
}

__device__ __forceinline__ void glds16(const int8_t* src, int8_t* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// 4 x 4 transpose of w[0..3] over the lanes c, c + 16, c + 32, c + 48 (the four 16-lane rows of a wave), for every c: afterwards w[k]
// of row g is what w[g] of row k was.  Two rounds of 2 x 2 block swaps: v_permlane32_swap_b32 exchanges rows 2, 3 of its first operand
// with rows 0, 1 of its second, v_permlane16_swap_b32 the odd rows of the first with the even rows of the second.  All 64 lanes
// must be active.
__device__ __forceinline__ void emul_transpose4(unsigned (&w)[4]) {
  typedef unsigned v2u __attribute__((ext_vector_type(2)));
  v2u s = __builtin_amdgcn_permlane32_swap(w[0], w[2], false, false);
  w[0] = s[0]; w[2] = s[1];
  s = __builtin_amdgcn_permlane32_swap(w[1], w[3], false, false);
  w[1] = s[0]; w[3] = s[1];
  s = __builtin_amdgcn_permlane16_swap(w[0], w[1], false, false);
  w[0] = s[0]; w[1] = s[1];
  s = __builtin_amdgcn_permlane16_swap(w[2], w[3], false, false);
  w[2] = s[0]; w[3] = s[1];
}

// One batch item = one (matrix, modulus): U[item][j][i] = (sum_k R[item][i][k] R[item][j][k]) mod p, i contiguous.
//   workgroup tile 256 x 256 x 128, 8 waves as 2 (M) x 4 (N), v_mfma_i32_16x16x64_i8 (wave tile 128 x 64 = 8 x 4 accumulators);
//   two LDS stages of 64 KiB filled by global_load_lds_dwordx4 (stage s + 1 in flight while stage s is multiplied);
//   LDS rows are 128 B; the 16-B chunk index is XORed with (row >> 1) & 7 on the SOURCE address and on the fragment read, so every
//   ds_read_b128 lane group hits 16 distinct 16-B slots of the 256-B bank row.
// Both operands are fragment-loaded the same way (lane l: row l & 15, bytes 16 (l >> 4) .. + 15 of the 64-deep k range), so the k
// order inside an MFMA is the same for A and B whatever the hardware's k map is.  Mp, Np multiples of 256, K of 128: no edges.
//
// Persistent: the grid is min(work ids, CUs) workgroups (emul_set_gemm_workgroups caps it), a work id = an (item, tile) pair in the
// order item-major, tile list inside.  Blocks b and b + 8 share an XCD: XCD b & 7 owns a contiguous range of ids and its w workgroups
// walk it from (b >> 3) with stride w, so at any moment the workgroups of an XCD sit on w consecutive ids, one supertile.  The walk
// is static: no workgroup waits for, or reads anything written by, another one.
//
// The K steps of the tiles a workgroup walks form ONE stream of stages s = 0, 1, 2, ..; stage s lives in buffer s & 1 (not kt & 1:
// nk may be odd).  A buffer is two halves of 32 KiB, the A tile and the B tile of the stage, which are restaged separately.  A staging
// cursor (tile base pointers, k offset) runs two stages ahead of the MFMAs and steps into the next work id when it has issued a
// tile's last K step, so the last two K steps of a tile stage the first two of the next one (with nk = 1 the cursor is two TILES
// ahead), and between the last MFMA of a tile and the first of the next only the epilogue stands, with the next tile's loads and
// its first fragment reads issued above it.
//
// One K step is four phases of 16 MFMAs, (ks, mh) = the 64-byte half of the k range x the upper / lower 4 of the wave's 8 row
// fragments.  The fragments of a phase are read into registers in the MIDDLE of the phase before it, between its two groups of 8
// MFMAs, so they are 8 MFMAs old when the wait before their first use comes (the compiler waits with lgkmcnt(0) there, so reads
// issued right before that wait would be waited for too).  sched_barrier(0) pins that order: left alone, the scheduler sinks the
// reads down to their uses.  A wave's 8 pieces of a stage (global_load_lds_dwordx4, 8 rows x 128 B each: whole 128-byte lines) are
// issued one after each group of 4 MFMAs, never as a burst in front of them.  A K step has two barriers, both s_barrier with a
// hand-written s_waitcnt (__syncthreads() would wait for vmcnt(0)): X after phase 2, Y after phase 3.
//
//   phase of stage s | MFMAs use (registers)        | ds_reads issued (buffer)                 | global_load_lds issued
//   1 (ks 0, mh 0)   | a[0..3], b[0..3]   of s      | a[4..7] ks 0 of s  (s & 1)               |
//   2 (ks 0, mh 1)   | a[4..7], b[0..3]   of s      | a[0..3], b[0..3] ks 1 of s  (s & 1): the LAST read of the B half of buffer s & 1
//   -- X: s_waitcnt lgkmcnt(0); s_barrier: every wave holds all its B fragments of stage s in registers --
//   3 (ks 1, mh 0)   | a[0..3]', b[0..3]' of s      | a[4..7] ks 1 of s  (s & 1): the LAST read | B tile of stage s + 2 into the B half of
//                                                     of the A half of buffer s & 1              buffer s & 1 (4 pieces)
//   -- Y: s_waitcnt lgkmcnt(0) vmcnt(4); s_barrier: every wave holds all its fragments of stage s in registers, and every wave's
//      loads of stage s + 1 have landed in buffer (s + 1) & 1; the 4 pieces of phase 3 may still be in flight --
//   4 (ks 1, mh 1)   | a[4..7]', b[0..3]' of s      | a[0..3], b[0..3] ks 0 of s + 1 ((s+1)&1) | A tile of stage s + 2 into the A half of
//                                                                                                buffer s & 1 (4 pieces)
//   -- after the last stage of a tile: the epilogue of that tile (registers and global stores only) --
//
//   read after write: buffer (s + 1) & 1 is first read in phase 4 of stage s, after Y of stage s.  A wave issues its loads in the
//   order B(s + 1) [phase 3 of s - 1], A(s + 1) [phase 4 of s - 1], B(s + 2) [phase 3 of s] and they retire in that order, so
//   at most 4 outstanding at Y means that its pieces of stage s + 1 have landed, and the barrier makes that true of all eight waves
//   before any of them reads.  The pieces in flight across Y go to buffer s & 1, which nobody reads before Y of stage s + 1.
//   write after read: the B half of buffer s & 1 is restaged in phase 3 of stage s, after X, which every wave reaches only with its
//   last reads of that half (phase 2) complete; the A half in phase 4, after Y, which every wave reaches only with its last reads of
//   that half (phase 3) complete.  Neither argument looks at which tile a stage belongs to: stages s, s + 1, s + 2 may lie in one,
//   two or three tiles, and the epilogue touches no LDS and stands after phase 4 of a stage and before phase 1 of the next, where
//   the schedule has no LDS ordering to keep.
//   The count: when the cursor has run out (the last two stages of a walk) phase 3 issues nothing and Y waits for vmcnt(0), a
//   uniform branch; vmcnt(4) there would not wait for the stage about to be read.  The epilogue's 8 stores per lane count in vmcnt
//   too and nothing here relies on how stores retire relative to loads: the first Y after an epilogue waits for vmcnt(0), once per
//   tile.  A load is 3 (A) or 4 (B) phases old when it is waited for, and Y never empties the queue inside a tile.
//   The prologue (once per workgroup) stages 0, waits, and stages 1 if the walk has a second stage at all.
//
// Zero skip: a tile's K steps are not all K / 128 blocks but the blocks that are live in both of its operands (the convert's masks,
// emul_live_stages in lmm_emul.h), in increasing k: a block of 256 rows x 128 k whose truncated integers are all zero adds exactly
// zero to every accumulator.  The cursor's k offset is the next set bit of its tile's list and the MFMA loop runs popcount(list)
// times, both from the same helper on the same two mask words, which are loaded with the tile coordinates, one tile ahead.  Nothing
// above asks which k a stage holds or how many stages a tile has (>= 1 is kept: an empty list becomes block 0), so the phase table, the
// barriers and the counts stand as they are.  All-ones masks (lmm_dev_set_emul_zero_skip(0)) give the full walk.
//
// Screen: the walk is not over all (item, tile) pairs but over the live id list (emul_compact_kernel): nlive[0] entries, read from
// device memory at entry -- the XCD ranges and cnt come from it, and a workgroup whose range is empty returns -- and a position of
// the walk maps to its work id through live[], one scalar load more where the tile coordinates are loaded, still one tile ahead.
// The grid is sized by the host's upper bound, all ids.  A tile that is not in the list is never staged, multiplied or stored: its
// part of U keeps whatever it held.  The K loop does not know: it sees tiles, as before.
__global__ __launch_bounds__(512, 2) void emul_gemm_kernel(const int8_t* __restrict__ R, int8_t* __restrict__ U, const int2* __restrict__ tiles, int ntiles,
                                                           const int* __restrict__ live, const int* __restrict__ nlive, int Mp, int Np, int K, EmulConst c,
                                                           const unsigned long long* __restrict__ masks) {
  __shared__ __attribute__((aligned(1024))) int8_t lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // the walk of this workgroup: ids first, first + step, .. (cnt of them) of its XCD's range; fewer than 8 workgroups split the ids
  // among themselves
  const int nwg = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int step = emul_range_wgs(nwg, xcd);
  const int nids = nlive[0];      // entries of the live id list: the walk is over list positions, live[position] is the work id
  const EmulRange rg = emul_xcd_range(nids, nwg, xcd);
  const int first = rg.start + slot, span = rg.len - slot;
  const int cnt = span > 0 ? (span + step - 1) / step : 0;
  if (cnt == 0) return;
  // source offsets of a lane's four 16-byte loads of one operand, from the tile's first row at k = 0
  unsigned roff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = wid * 32 + q * 8 + (lane >> 3), chunk = (lane & 7) ^ ((row >> 1) & 7);
    roff[q] = (unsigned)row * (unsigned)K + chunk * 16;
  }
  // the staging cursor: operand panels of the cn-th work id of the walk, next k offset ck; (pitem, pt) is the (cn + 1)-th work id,
  // loaded one tile ahead so that stepping into it waits for no load
  // The stages of a tile are the live K blocks of both its operands (emul_live_stages, lmm_emul.h): cm holds the ones the cursor has
  // not issued yet, ck is the first of them; pm is the list of the (cn + 1)-th work id, loaded with its coordinates.
  const int8_t* cA = nullptr;
  const int8_t* cB = nullptr;
  int cn = 0, ck = 0, pitem = 0;
  int2 pt = make_int2(0, 0);
  EmulMask cm{0, 0}, pm{0, 0};
  const int tr = Mp / TILE, nkb = K / BK;
  auto live_of = [&](int item, int2 t) {
    const unsigned long long* mz = masks + (size_t)(item / c.nmod) * tr * LMM_EMUL_MASK_WORDS;
    const EmulMask a{mz[t.x * LMM_EMUL_MASK_WORDS], mz[t.x * LMM_EMUL_MASK_WORDS + 1]}, b{mz[t.y * LMM_EMUL_MASK_WORDS], mz[t.y * LMM_EMUL_MASK_WORDS + 1]};
    return emul_live_stages(a, b, nkb);
  };
  auto cursor_peek = [&](int pos) {
    const int idn = live[pos];
    pitem = idn / ntiles;
    pt = tiles[idn - pitem * ntiles];
    pm = live_of(pitem, pt);
  };
  auto cursor_tile = [&]() {
    const int8_t* Rb = R + (size_t)pitem * Mp * K;
    cA = Rb + (size_t)pt.x * TILE * K;
    cB = Rb + (size_t)pt.y * TILE * K;
    cm = pm;
    ck = emul_mask_first(cm) * BK;
    if (cn + 1 < cnt) cursor_peek(first + (cn + 1) * step);
  };
  // piece q (0..3: A, 4..7: B) of the cursor's stage into buffer buf; the cursor moves on after piece 3, the last one issued
  auto piece = [&](int buf, int q) {      // cn < cnt
    int8_t* base = lds + buf * STAGE_BYTES + wid * 4096;
    if (q < 4) glds16(cA + ck + roff[q], base + q * 1024);
    else glds16(cB + ck + roff[q - 4], base + TILE * BK + (q - 4) * 1024);
    if (q == 3) {
      cm = emul_mask_pop(cm);
      if (emul_mask_empty(cm)) {
        ++cn;
        if (cn < cnt) cursor_tile();
      } else ck = emul_mask_first(cm) * BK;
    }
  };
  auto stage_next = [&](int buf) {      // cn < cnt: a whole stage at once (the prologue)
#pragma unroll
    for (int q = 4; q < 8; ++q) piece(buf, q);
#pragma unroll
    for (int q = 0; q < 4; ++q) piece(buf, q);
  };
  const int frow = lane & 15, fk = lane >> 4;
  // byte offset of a fragment in its stage: (row 128) + ((ks 4 + fk) ^ (row >> 1) & 7) 16 with row = 16 m + frow (+ the wave's first
  // row, a multiple of 64): the swizzle is (frow >> 1), and ks = 1 flips bit 6 of the offset
  const int offA = (wr * 128 + frow) * BK + ((fk ^ (frow >> 1)) << 4), offB = TILE * BK + (wc * 64 + frow) * BK + ((fk ^ (frow >> 1)) << 4);
  auto frag = [&](const int8_t* st, int off, int ks, int f) { return *reinterpret_cast<const v4i*>(st + (off ^ (ks << 6)) + f * 16 * BK); };
  v4i acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (v4i){0, 0, 0, 0};
  cursor_peek(first);
  cursor_tile();
  stage_next(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (cn < cnt) stage_next(1);
  v4i alo[4], ahi[4], b[4], alo1[4], ahi1[4], b1[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) { alo[f] = frag(lds, offA, 0, f); b[f] = frag(lds, offB, 0, f); }
  // 8 MFMAs: row fragments 2 h, 2 h + 1 of A4 (accumulator rows M0 + 2 h ..) x the 4 column fragments
#define EMUL_MMA8(A4, B4, M0, h)                                                                                                   \
  _Pragma("unroll") for (int m = 2 * (h); m < 2 * (h) + 2; ++m)                                                                    \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + m][n], 0, 0, 0)
  // 4 MFMAs: row fragment m of A4 (accumulator row M0 + m) x the 4 column fragments
#define EMUL_MMA4(A4, B4, M0, m)                                                                                                   \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + (m)][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + (m)][n], 0, 0, 0)
#define EMUL_PIN() __builtin_amdgcn_sched_barrier(0)
  int par = 0;      // s & 1
  bool stored = false;      // an epilogue's stores have been issued since the last wait for vmcnt
  // the MFMA side: coordinates and stage count of the next work id, loaded one tile ahead like the cursor's
  int nid = live[first];
  int nitem = nid / ntiles;
  int2 nt = tiles[nid - nitem * ntiles];
  int nnk = emul_mask_count(live_of(nitem, nt));
  for (int n = 0, pos = first; n < cnt; ++n, pos += step) {
    // what this work id's K loop and epilogue need
    const int item = nitem, nk = nnk;
    const int2 t = nt;
    const int p = c.p[item % c.nmod];
    if (n + 1 < cnt) {
      nid = live[pos + step];
      nitem = nid / ntiles;
      nt = tiles[nid - nitem * ntiles];
      nnk = emul_mask_count(live_of(nitem, nt));
    }
    for (int kt = 0; kt < nk; ++kt, par ^= 1) {
      const int8_t* cur = lds + par * STAGE_BYTES;
      const int8_t* nxt = lds + (par ^ 1) * STAGE_BYTES;
      EMUL_MMA8(alo, b, 0, 0); EMUL_PIN();      // phase 1
#pragma unroll
      for (int f = 0; f < 4; ++f) ahi[f] = frag(cur, offA, 0, 4 + f);
      EMUL_PIN(); EMUL_MMA8(alo, b, 0, 1); EMUL_PIN();
      EMUL_MMA8(ahi, b, 4, 0); EMUL_PIN();      // phase 2
#pragma unroll
      for (int f = 0; f < 4; ++f) { alo1[f] = frag(cur, offA, 1, f); b1[f] = frag(cur, offB, 1, f); }
      EMUL_PIN(); EMUL_MMA8(ahi, b, 4, 1); EMUL_PIN();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // X
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const bool more = cn < cnt;      // stage s + 2 exists
      EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 0); EMUL_PIN();      // phase 3
      if (more) piece(par, 4);
      EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 1); EMUL_PIN();
      if (more) piece(par, 5);
#pragma unroll
      for (int f = 0; f < 4; ++f) ahi1[f] = frag(cur, offA, 1, 4 + f);
      EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 2); EMUL_PIN();
      if (more) piece(par, 6);
      EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 3); EMUL_PIN();
      if (more) piece(par, 7);
      if (more && !stored) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");      // Y
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      stored = false;
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 0); EMUL_PIN();      // phase 4
      if (more) piece(par, 0);
      EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 1); EMUL_PIN();
      if (more) piece(par, 1);
      if (kt + 1 < nk || n + 1 < cnt) {
#pragma unroll
        for (int f = 0; f < 4; ++f) { alo[f] = frag(nxt, offA, 0, f); b[f] = frag(nxt, offB, 0, f); }
      }
      EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 2); EMUL_PIN();
      if (more) piece(par, 2);
      EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 3); EMUL_PIN();
      if (more) piece(par, 3);
      EMUL_PIN();
    }
    // epilogue of this work id: reduce mod p (emul_acc_residue: |acc| <= K 128^2 <= 2^28) and pack the 4 consecutive rows a lane holds of
    // a 16 x 16 block into one dword.  C/D map of 16x16: column = lane & 15, rows = 4 (lane >> 4) + e, so the dword of row fragment m
    // in lane (c, g) is rows 16 m + 4 g .. + 3 of column c, and storing it as it is makes a wave store 16 pieces of 16 bytes in 16
    // lines (the columns of U are Mp bytes apart).  Instead the four row groups of a column exchange the dwords of row fragments
    // 4 q .. 4 q + 3 (emul_transpose4: registers only), after which lane (c, g) holds rows 16 (4 q + g) .. + 15 of its column: one
    // 16-byte store per lane, 16 columns x 64 contiguous bytes per wave store, 8 stores per lane and tile instead of 32.  The
    // accumulators are cleared for the next tile.
    const int cf = emul_fold_const(p);
    const float pf = (float)p, rp = 1.0f / pf;
    int8_t* Ub = U + (size_t)item * Np * Mp;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[k] = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[k] |= emul_acc_residue(acc[4 * q + k][nn][e], cf, pf, rp) << (8 * e);
          acc[4 * q + k][nn] = (v4i){0, 0, 0, 0};
        }
        emul_transpose4(w);
        const size_t j = (size_t)t.y * TILE + wc * 64 + nn * 16 + frow;
        const int i = t.x * TILE + wr * 128 + (4 * q + fk) * 16;
        *reinterpret_cast<v4u*>(Ub + j * Mp + i) = (v4u){w[0], w[1], w[2], w[3]};
      }
    stored = true;
  }
#undef EMUL_MMA8
#undef EMUL_MMA4
#undef EMUL_PIN
}

// 4 consecutive rows x 1 column per thread, NMOD moduli: 16 dword loads of residues (coalesced along i) and the thread's entries of C,
// the row scales and exponents, all issued before any of them is used (one memory latency per thread); CRT; C for i >= j written back.
// The sums of emul_crt run modulus-outer over the thread's 4 outputs (each output sees the same operations in the same order), so a
// CRT weight is a scalar operand that is dead after 4 FMAs: held for all 16 moduli at once, the 96 dwords of weights do not fit the
// scalar registers.
// A wave covers 256 consecutive rows of one column, which lie in ONE tile: it reads that tile's flag first (the screen's) and returns
// for a dead tile, having loaded nothing else.  The GEMM never wrote U there, so the flag is the only guard against its stale bytes.
template <int NMOD>
__global__ __launch_bounds__(256) void emul_combine_kernel(BatchPtr A, int g0, size_t offC, int ldc, int M, int N, int Mp, int Np, EmulConst c,
                                                           const int8_t* __restrict__ U, const double* __restrict__ sc, const int* __restrict__ ex,
                                                           const unsigned char* __restrict__ flags) {
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4, j = blockIdx.y, z = blockIdx.z;
  if (i0 + 3 < j || i0 >= M) return;
  if (flags[emul_flag_at(Mp / TILE, Np / TILE, z, i0 / TILE, j / TILE)] == 0) return;
  unsigned w[NMOD];
#pragma unroll
  for (int t = 0; t < NMOD; ++t) w[t] = *reinterpret_cast<const unsigned*>(U + (((size_t)z * NMOD + t) * Np + j) * Mp + i0);
  const double scj = sc[(size_t)z * Mp + j];
  const int exj = ex[(size_t)z * Mp + j];
  double* C = A.p[g0 + z] + offC + (size_t)j * ldc;
  double cv[4], sci[4];
  int exi[4];
  bool on[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {      // i0 + 3 < Mp: the scales and exponents of the padding rows exist; C does not
    const int i = i0 + e;
    on[e] = i >= j && i < M;
    sci[e] = sc[(size_t)z * Mp + i];
    exi[e] = ex[(size_t)z * Mp + i];
    cv[e] = on[e] ? C[i] : 0.0;
  }
  double S1[4] = {0.0, 0.0, 0.0, 0.0}, S2[4] = {0.0, 0.0, 0.0, 0.0}, S3[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < NMOD; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) emul_crt_term((int)(int8_t)(w[t] >> (8 * e)), t, c, S1[e], S2[e], S3[e]);
  // all twelve sums exist here: without this the compiler sinks each output's sums into its branch below, output-outer again
#pragma unroll
  for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(S1[e]), "+v"(S2[e]), "+v"(S3[e]));
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!on[e]) continue;
    const double X = emul_crt_finish(S1[e], S2[e], S3[e], c);
    C[i0 + e] = cv[e] - ldexp(X * sci[e] * scj, exi[e] + exj);
  }
}
template <int NMOD>
void launch_combine(int nmod, dim3 grid, hipStream_t st, const BatchPtr& C, int g0, size_t offC, int ldc, int M, int N, int Mp, int Np, const EmulConst& c,
                    const int8_t* U, const double* sc, const int* ex, const unsigned char* flags) {
  if constexpr (NMOD > LMM_EMUL_MINMOD) {
    if (nmod != NMOD) return launch_combine<NMOD - 1>(nmod, grid, st, C, g0, offC, ldc, M, N, Mp, Np, c, U, sc, ex, flags);
  }
  emul_combine_kernel<NMOD><<<grid, 256, 0, st>>>(C, g0, offC, ldc, M, N, Mp, Np, c, U, sc, ex, flags);
}

int g_emul_gemm_wgs = 0;      // emul_set_gemm_workgroups: 0 = one workgroup per CU
int g_emul_zero_skip = -1;    // emul_set_zero_skip: -1 = LMM_EMUL_ZERO_SKIP (read once; default on)
int g_emul_poison = 0;        // emul_set_scratch_poison (tests): the residue scratch of a group is filled with a non-zero byte before its convert
int g_emul_screen = -1;       // emul_set_screen: -1 = LMM_EMUL_SCREEN (read once; default on)

bool emul_zero_skip_on() {
  if (g_emul_zero_skip < 0) {
    const char* e = getenv("LMM_EMUL_ZERO_SKIP");
    g_emul_zero_skip = (e && e[0] == '0') ? 0 : 1;
  }
  return g_emul_zero_skip != 0;
}

bool emul_screen_on() {
  if (g_emul_screen < 0) {
    const char* e = getenv("LMM_EMUL_SCREEN");
    g_emul_screen = (e && e[0] == '0') ? 0 : 1;
  }
  return g_emul_screen != 0;
}

}  // namespace

void emul_set_screen(int on) { g_emul_screen = on < 0 ? -1 : (on ? 1 : 0); }
void emul_set_gemm_workgroups(int wgs) { g_emul_gemm_wgs = wgs; }
void emul_set_zero_skip(int on) { g_emul_zero_skip = on < 0 ? -1 : (on ? 1 : 0); }
void emul_set_scratch_poison(int on) { g_emul_poison = on ? 1 : 0; }

hipError_t launch_f64_screen(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& P, size_t offP, int ldp, int M, int N, int K, int strip, int nb,
                             const EmulAmaxKeep& keep, unsigned char* flags, int* stat, const int* vote, hipStream_t st, const ZeroExt& zx, int zrow0) {
  const int Mn = f64_screen_rows(M, strip);
  const int MT = (Mn + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE, NT = (N + LMM_F64_SCREEN_TILE - 1) / LMM_F64_SCREEN_TILE;
  if (nb <= 0 || MT < 2 || NT < 2 || N > Mn || (K % BK) != 0 || (keep.scan0 % BK) != 0) return hipErrorInvalidValue;
  EmulBlockMax bm{};
  if (keep.bmax != nullptr) bm = EmulBlockMax{keep.bmax + (size_t)keep.cb0 * keep.ld + keep.row0, (size_t)keep.ncb * keep.ld, (size_t)keep.ld};
  emul_amax_fold_kernel<<<dim3((M + 255) / 256, nb), 256, 0, st>>>(keep, M);      // every row's first write: no memset
  if (keep.scan0 < K)
    emul_rowmax_kernel<<<dim3((M + 255) / 256, (K - keep.scan0) / BK, nb), 256, 0, st>>>(P, 0, offP, ldp, M, keep.ld, keep.scan0, keep.out + keep.row0, bm, vote);
  f64_screen_kernel<<<dim3(MT, NT - 1, nb), LMM_F64_SCREEN_TILE, 0, st>>>(C, offC, ldc, Mn, N, K, keep.out + keep.row0, keep.ld, MT, NT, flags, stat, vote, zx.p, zx.ld, zrow0);
  return hipGetLastError();
}

// C_m (M x N at C.p[m] + offC, ldc) -= P_m P_m[0:N]' for the panels P_m (M x K at P.p[m] + offP, ldp), m < nb, lower trapezoid
// (i >= j) only, in groups of G matrices through `scratch` (emul_scratch_bytes(M, N, K, G, nmod) bytes).  Returns the first HIP
// error of its host-side calls (nothing is launched after one).  keep: the row maxima and the block maxima go to arrays of the
// caller's, for all nb matrices before the first group, and start from what earlier updates found (EmulAmaxKeep, lmm_internal.h);
// aux is then emul_aux(M, G, K).total bytes.  Without keep the block maxima of a group live in aux too: emul_aux(M, G, K).total_bmax
// bytes.  aux holds the live K blocks of a group's panels and its dead pieces (lmm_emul.h): written in full by emul_live_kernel
// before each convert, or, with the zero skip switched off, the masks set to ones on the stream and no bitmap.  The residues R are
// shared by the groups and the updates that go through one scratch block and a dead block is never written, so it holds whatever
// was there: R is read through emul_live_stages only.  screen: emul_screen_layout(M, N, G, nmod).total bytes for a group's tile
// flags, its live id list and the two counts (lmm_emul.h), written in full by every group: by emul_screen_kernel once the row maxima
// exist, or, with the screen switched off, the flags set to ones on the stream; emul_compact_kernel runs either way, and the list is
// then the identity.  U is written for live tiles only and holds stale bytes elsewhere: U is read behind the flags only.
hipError_t launch_emul_update(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& P, size_t offP, int ldp, int M, int N, int K, int nb,
                              int G, int nmod, void* scratch, void* aux, void* screen, hipStream_t st, const EmulAmaxKeep* keep, const ZeroExt& zx, int zrow0) {
  static EmulConst consts[LMM_EMUL_MAXMOD + 1];
  if (consts[nmod].nmod != nmod) consts[nmod] = emul_make_const(nmod);
  const EmulConst& c = consts[nmod];
  const int bits = emul_bits(nmod, K);
  const EmulLayout L = emul_layout(M, N, K, G, nmod);
  const int tm = L.Mp / TILE, tn = L.Np / TILE, ntiles = emul_tile_list(tm, tn, nullptr);
  hipError_t err = hipSuccess;
  const int2* tiles = emul_tiles(L.Mp / TILE, L.Np / TILE, &err);
  if (tiles == nullptr) return err;
  char* s = static_cast<char*>(scratch);
  int8_t* R = reinterpret_cast<int8_t*>(s + L.R);
  int8_t* U = reinterpret_cast<int8_t*>(s + L.U);
  unsigned long long* amax = reinterpret_cast<unsigned long long*>(s + L.amax);
  double* sc = reinterpret_cast<double*>(s + L.sc);
  int* ex = reinterpret_cast<int*>(s + L.ex);
  const bool skip = emul_zero_skip_on(), screened = emul_screen_on();
  const int wgs = g_emul_gemm_wgs > 0 ? g_emul_gemm_wgs : device_cus();      // one 128-KiB workgroup fits on a CU
  EmulBlockMax bm{};
  if (keep) {      // every row of every matrix gets its first write from the fold: no memset
    bm = EmulBlockMax{keep->bmax + (size_t)keep->cb0 * keep->ld + keep->row0, (size_t)keep->ncb * keep->ld, (size_t)keep->ld};
    emul_amax_fold_kernel<<<dim3((M + 255) / 256, nb), 256, 0, st>>>(*keep, M);
    if (keep->scan0 < K)
      emul_rowmax_kernel<<<dim3((M + 255) / 256, (K - keep->scan0) / BK, nb), 256, 0, st>>>(P, 0, offP, ldp, M, keep->ld, keep->scan0, keep->out + keep->row0, bm, nullptr);
  }
  for (int g0 = 0; g0 < nb; g0 += G) {
    const int gc = std::min(G, nb - g0);
    const EmulAux X = emul_aux(M, gc, K);
    const unsigned long long* am = amax;
    int as = L.Mp;
    EmulBlockMax gbm{reinterpret_cast<unsigned long long*>(static_cast<char*>(aux) + X.bmax), (size_t)(K / BK) * M, (size_t)M};
    if (keep) { am = keep->out + (size_t)g0 * keep->ld + keep->row0; as = keep->ld; gbm = bm; gbm.p += (size_t)g0 * bm.zs; }
    else {
      err = hipMemsetAsync(amax, 0, (size_t)gc * L.Mp * 8, st);      // stale row maxima would give wrong scales: stop here
      if (err != hipSuccess) return err;
      emul_rowmax_kernel<<<dim3((M + 255) / 256, K / BK, gc), 256, 0, st>>>(P, g0, offP, ldp, M, L.Mp, 0, amax, gbm, nullptr);
    }
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(static_cast<char*>(aux) + X.masks);
    unsigned short* dead = skip ? reinterpret_cast<unsigned short*>(static_cast<char*>(aux) + X.pieces) : nullptr;
    if (skip) emul_live_kernel<<<dim3(L.Mp / TILE, gc), 256, 0, st>>>(M, L.Mp, K, bits, am, as, gbm, masks, dead);
    else {
      err = hipMemsetAsync(masks, 0xFF, emul_mask_bytes(M, gc), st);
      if (err != hipSuccess) return err;
    }
    if (g_emul_poison) {
      err = hipMemsetAsync(R, 0x5A, (size_t)gc * nmod * L.Mp * K, st);
      if (err == hipSuccess) err = hipMemsetAsync(U, 0x5A, (size_t)gc * nmod * L.Np * L.Mp, st);
      if (err != hipSuccess) return err;
    }
    const EmulScreen S = emul_screen_layout(M, N, gc, nmod);
    unsigned char* flags = static_cast<unsigned char*>(screen) + S.flags;
    int* nlive = reinterpret_cast<int*>(static_cast<char*>(screen) + S.count);
    int* live = reinterpret_cast<int*>(static_cast<char*>(screen) + S.list);
    if (screened) emul_screen_kernel<<<dim3(ntiles, gc), 256, 0, st>>>(C, g0, offC, ldc, M, N, K, am, as, tiles, tm, tn, flags, zx.p, zx.ld, zrow0, zx.stat);
    else {
      err = hipMemsetAsync(flags, 1, (size_t)gc * tm * tn, st);
      if (err != hipSuccess) return err;
    }
    emul_compact_kernel<<<gc, 256, 0, st>>>(flags, tiles, ntiles, tm, tn, nmod, live, nlive);
    launch_convert<LMM_EMUL_MAXMOD>(nmod, dim3(L.Mp / TILE * CV_SPLIT, K / CV_K, gc), st, P, g0, offP, ldp, M, L.Mp, K, bits, am, as, R, sc, ex, masks, dead);
    const int nids = ntiles * gc * nmod;
    emul_gemm_kernel<<<std::min(nids, wgs), 512, 0, st>>>(R, U, tiles, ntiles, live, nlive, L.Mp, L.Np, K, c, masks);
    launch_combine<LMM_EMUL_MAXMOD>(nmod, dim3((M + 1023) / 1024, N, gc), st, C, g0, offC, ldc, M, N, L.Mp, L.Np, c, U, sc, ex, flags);
  }
  return hipSuccess;
}
