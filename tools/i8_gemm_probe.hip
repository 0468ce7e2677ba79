// Go/no-go probe for the int8 modular emulation of the large f64 Cholesky updates: the sustained rate of a
// batched int8 SYRK-shaped GEMM on gfx950 at the C2 level shapes, with the mod-p epilogue that writes one byte per output.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/i8_gemm_probe.hip -o tools/i8_gemm_probe && tools/i8_gemm_probe [nmat]
// One batch item is one (matrix, modulus) pair: operand R[M][K] int8, K-contiguous; output U[N][M] bytes (i contiguous, as the
// column-major C of the update wants it), U[j][i] = (sum_k R[i][k] R[j][k]) mod p in the symmetric range.  Only 256 x 256 tiles
// of the lower trapezoid (tile row >= tile column) are computed.  Shapes must be multiples of the tile (M, N % 256, K % 128).
//   workgroup tile 256 x 256 x 128, 8 waves as 2 (M) x 4 (N), v_mfma_i32_32x32x32_i8 or v_mfma_i32_16x16x64_i8, int32 accumulators;
//   two LDS stages of 64 KiB filled by global_load_lds_dwordx4 (tile t+1 is in flight while tile t is multiplied);
//   LDS rows are 128 B; the 16-B chunk index is XORed with (row >> 1) & 7 on the SOURCE address and on the fragment read,
//   which makes every ds_read_b128 lane group hit 16 distinct 16-B slots of the 256-B bank row.
// Both operands are fragment-loaded the same way (lane l: row l & 31 or l & 15, 16 consecutive k), so the k order inside an
// MFMA is the same permutation for A and B whatever the hardware's k map is; the row/column map is checked with exact
// asymmetric integer data (full check at a small shape, sampled check at every timed shape).
// NOTE: i8_syrk_mod_kernel_ps here is the library's emul_gemm_kernel as it was BEFORE the zero skip: every tile walks
// all K / 128 blocks, on dense random operands.  It still speaks for the cost of a K step and for the fixed cost of a tile, which the
// skip leaves alone; it no longer speaks for the library's time at a level, which depends on how many blocks of its panels are live.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

constexpr int TILE = 256, BK = 128, NMOD = 16;
constexpr int STAGE_BYTES = 2 * TILE * BK;  // A tile + B tile
struct Moduli { int p[NMOD]; };
static const Moduli kModuli = {{256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193}};

__device__ __forceinline__ int mod_sym(int x, int p, float rp, int lo) {
  // |x| <= 2^27: the float quotient is off by less than 0.3, so one correction each way lands in [lo, lo + p - 1]
  const int q = __float2int_rn((float)x * rp);
  int r = x - q * p;
  r += (r < lo) ? p : 0;
  r -= (r > lo + p - 1) ? p : 0;
  return r;
}

__device__ __forceinline__ void glds16(const int8_t* src, int8_t* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// SHAPE 32: v_mfma_i32_32x32x32_i8 (wave tile 128 x 64 = 4 x 2 accumulators of 16); SHAPE 16: v_mfma_i32_16x16x64_i8 (8 x 4 of 4)
template <int SHAPE, bool STAMP>
__global__ __launch_bounds__(512, 2) void i8_syrk_mod_kernel(const int8_t* __restrict__ R, int8_t* __restrict__ U, const int2* __restrict__ tiles, int ntiles,
                                                             int M, int N, int K, Moduli mod, unsigned long long* __restrict__ stamps) {
  __shared__ __attribute__((aligned(1024))) int8_t lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // blocks b and b + 8 share an XCD: give each XCD a contiguous range of work ids, so that its 32 resident blocks are one supertile
  const int nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
  const int batch = wg / ntiles;
  const int2 t = tiles[wg - batch * ntiles];
  const int8_t* Rb = R + (size_t)batch * M * K;
  const int8_t* srcA[4];
  const int8_t* srcB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = wid * 32 + q * 8 + (lane >> 3), chunk = (lane & 7) ^ ((row >> 1) & 7);
    srcA[q] = Rb + ((size_t)t.x * TILE + row) * K + chunk * 16;
    srcB[q] = Rb + ((size_t)t.y * TILE + row) * K + chunk * 16;
  }
  auto stage = [&](int buf, int k0) {
    int8_t* base = lds + buf * STAGE_BYTES + wid * 4096;
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(srcA[q] + k0, base + q * 1024);
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(srcB[q] + k0, base + TILE * BK + q * 1024);
  };
  constexpr int MR = SHAPE == 32 ? 4 : 8, NR = SHAPE == 32 ? 2 : 4, KS = SHAPE == 32 ? 4 : 2, NACC = SHAPE == 32 ? 16 : 4;
  typedef int acc_t __attribute__((ext_vector_type(NACC)));
  acc_t acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int e = 0; e < NACC; ++e) acc[m][n][e] = 0;
  unsigned long long t0 = 0, r0 = 0;
  if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int nk = K / BK;
  const int frow = lane & (SHAPE - 1), fk = lane / SHAPE;  // fragment row and 16-B k-chunk within one MFMA's k range
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) stage((kt + 1) & 1, (kt + 1) * BK);
    const int8_t* la = lds + (kt & 1) * STAGE_BYTES;
    const int8_t* lb = la + TILE * BK;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int chunk = ks * (8 / KS) + fk;
      v4i a[MR], b[NR];
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const int row = wr * 128 + m * SHAPE + frow;
        a[m] = *reinterpret_cast<const v4i*>(la + row * BK + ((chunk ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        const int row = wc * 64 + n * SHAPE + frow;
        b[n] = *reinterpret_cast<const v4i*>(lb + row * BK + ((chunk ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n) {
          if constexpr (SHAPE == 32) acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], b[n], acc[m][n], 0, 0, 0);
          else acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (STAMP) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) { stamps[2 * (size_t)blockIdx.x] = t1 - t0; stamps[2 * (size_t)blockIdx.x + 1] = r1 - r0; }
  }
  // epilogue: reduce mod p, pack the 4 consecutive rows (i) a lane holds per register group into one dword of U[j][i]
  const int p = mod.p[batch % NMOD], lo = -(p / 2);
  const float rp = 1.0f / (float)p;
  int8_t* Ub = U + (size_t)batch * N * M;
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const size_t j = (size_t)t.y * TILE + wc * 64 + n * SHAPE + frow;
#pragma unroll
      for (int g = 0; g < NACC / 4; ++g) {
        // C/D map: 32x32: row = 8 g + 4 (lane >> 5) + e; 16x16: row = 4 (lane >> 4) + e
        const int i = t.x * TILE + wr * 128 + m * SHAPE + (SHAPE == 32 ? 8 * g + 4 * fk : 4 * fk);
        unsigned w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w |= (unsigned)(mod_sym(acc[m][n][4 * g + e], p, rp, lo) & 0xFF) << (8 * e);
        *reinterpret_cast<unsigned*>(Ub + j * M + i) = w;
      }
    }
}

__device__ __forceinline__ int mod_sym24(int x, int p, float rp, int lo) {
  const int q = __float2int_rn((float)x * rp);
  int r = x - __mul24(q, p);
  r += (r < lo) ? p : 0;
  r -= (r > lo + p - 1) ? p : 0;
  return r;
}

// The library's emul_gemm_kernel (lmm_kernels_i8.hip), 16x16x64 form, as it stood before the persistent kernel below: one workgroup
// per tile; i8_syrk_mod_kernel<16> above is the kernel it replaced.
// The K loop: one K step is four phases of 16 MFMAs, (ks, mh) = the 64-byte half of the k range x the upper / lower 4 of the wave's 8
// row fragments.  The fragments of a phase are read into registers in the MIDDLE of the phase before it, between its two groups of 8
// MFMAs, so they are 8 MFMAs old when the wait before their first use comes (the compiler waits with lgkmcnt(0) there, so reads
// issued right before that wait would be waited for too).  sched_barrier(0) pins that order: left alone, the scheduler sinks the
// reads down to their uses.  The one barrier of a K step stands between phases 3 and 4.  Stage t lives in buffer t & 1.
//
//   phase of step t | MFMAs use (registers)        | ds_reads issued (buffer)                 | global_load_lds issued
//   1 (ks 0, mh 0)  | a[0..3], b[0..3]   of t      | a[4..7] ks 0 of t  (t & 1)               |
//   2 (ks 0, mh 1)  | a[4..7], b[0..3]   of t      | a[0..3], b[0..3] ks 1 of t  (t & 1)      |
//   3 (ks 1, mh 0)  | a[0..3]', b[0..3]' of t      | a[4..7] ks 1 of t  (t & 1): the LAST read of buffer t & 1
//   -- s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier: every wave holds all its fragments of stage t in registers, and every wave's
//      loads of stage t + 1 (issued one whole K step earlier, at this point of step t - 1) have landed in buffer (t + 1) & 1 --
//   4 (ks 1, mh 1)  | a[4..7]', b[0..3]' of t      | a[0..3], b[0..3] ks 0 of t + 1 ((t+1)&1) | stage t + 2 into buffer t & 1
//
//   read after write: buffer (t + 1) & 1 is first read in phase 4 of step t, after the wait-plus-barrier that retires stage t + 1.
//   write after read: buffer t & 1 is restaged in phase 4 of step t, after the barrier every wave reaches only with its last reads
//   of that buffer (phase 3) complete.  One stage is in flight at a time, so the wait is vmcnt(0); it waits for loads that are one
//   K step (64 MFMAs per wave) old.  nk = 1 and 2: the prologue stages tiles 0 and 1, the loop stages t + 2 < nk only.
template <bool STAMP>
__global__ __launch_bounds__(512, 2) void i8_syrk_mod_kernel_pf(const int8_t* __restrict__ R, int8_t* __restrict__ U, const int2* __restrict__ tiles, int ntiles,
                                                                int Mp, int Np, int K, Moduli mod, unsigned long long* __restrict__ stamps) {
  __shared__ __attribute__((aligned(1024))) int8_t lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // blocks b and b + 8 share an XCD: give each XCD a contiguous range of work ids, so that its 32 resident blocks are one supertile
  const int nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
  const int item = wg / ntiles;
  const int2 t = tiles[wg - item * ntiles];
  const int8_t* Rb = R + (size_t)item * Mp * K;
  const int8_t* srcA[4];
  const int8_t* srcB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = wid * 32 + q * 8 + (lane >> 3), chunk = (lane & 7) ^ ((row >> 1) & 7);
    srcA[q] = Rb + ((size_t)t.x * TILE + row) * K + chunk * 16;
    srcB[q] = Rb + ((size_t)t.y * TILE + row) * K + chunk * 16;
  }
  auto stage = [&](int buf, int k0) {
    int8_t* base = lds + buf * STAGE_BYTES + wid * 4096;
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(srcA[q] + k0, base + q * 1024);
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(srcB[q] + k0, base + TILE * BK + q * 1024);
  };
  const int nk = K / BK, frow = lane & 15, fk = lane >> 4;
  // byte offset of a fragment in its stage: (row 128) + ((ks 4 + fk) ^ (row >> 1) & 7) 16 with row = 16 m + frow (+ the wave's first
  // row, a multiple of 64): the swizzle is (frow >> 1), and ks = 1 flips bit 6 of the offset
  const int offA = (wr * 128 + frow) * BK + ((fk ^ (frow >> 1)) << 4), offB = TILE * BK + (wc * 64 + frow) * BK + ((fk ^ (frow >> 1)) << 4);
  auto frag = [&](const int8_t* st, int off, int ks, int f) { return *reinterpret_cast<const v4i*>(st + (off ^ (ks << 6)) + f * 16 * BK); };
  v4i acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (v4i){0, 0, 0, 0};
  unsigned long long t0 = 0, r0 = 0;
  if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nk > 1) stage(1, BK);
  v4i alo[4], ahi[4], b[4], alo1[4], ahi1[4], b1[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) { alo[f] = frag(lds, offA, 0, f); b[f] = frag(lds, offB, 0, f); }
  // 8 MFMAs: row fragments 2 h, 2 h + 1 of A4 (accumulator rows M0 + 2 h ..) x the 4 column fragments
#define EMUL_MMA8(A4, B4, M0, h)                                                                                                   \
  _Pragma("unroll") for (int m = 2 * (h); m < 2 * (h) + 2; ++m)                                                                    \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + m][n], 0, 0, 0)
#define EMUL_PIN() __builtin_amdgcn_sched_barrier(0)
  for (int kt = 0; kt < nk; ++kt) {
    const int8_t* cur = lds + (kt & 1) * STAGE_BYTES;
    const int8_t* nxt = lds + ((kt + 1) & 1) * STAGE_BYTES;
    EMUL_MMA8(alo, b, 0, 0); EMUL_PIN();      // phase 1
#pragma unroll
    for (int f = 0; f < 4; ++f) ahi[f] = frag(cur, offA, 0, 4 + f);
    EMUL_PIN(); EMUL_MMA8(alo, b, 0, 1); EMUL_PIN();
    EMUL_MMA8(ahi, b, 4, 0); EMUL_PIN();      // phase 2
#pragma unroll
    for (int f = 0; f < 4; ++f) { alo1[f] = frag(cur, offA, 1, f); b1[f] = frag(cur, offB, 1, f); }
    EMUL_PIN(); EMUL_MMA8(ahi, b, 4, 1); EMUL_PIN();
    EMUL_MMA8(alo1, b1, 0, 0); EMUL_PIN();    // phase 3
#pragma unroll
    for (int f = 0; f < 4; ++f) ahi1[f] = frag(cur, offA, 1, 4 + f);
    EMUL_PIN(); EMUL_MMA8(alo1, b1, 0, 1); EMUL_PIN();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 2 < nk) stage(kt & 1, (kt + 2) * BK);
    EMUL_PIN(); EMUL_MMA8(ahi1, b1, 4, 0); EMUL_PIN();      // phase 4
    if (kt + 1 < nk) {
#pragma unroll
      for (int f = 0; f < 4; ++f) { alo[f] = frag(nxt, offA, 0, f); b[f] = frag(nxt, offB, 0, f); }
    }
    EMUL_PIN(); EMUL_MMA8(ahi1, b1, 4, 1); EMUL_PIN();
  }
#undef EMUL_MMA8
#undef EMUL_PIN
  if (STAMP) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) { stamps[2 * (size_t)blockIdx.x] = t1 - t0; stamps[2 * (size_t)blockIdx.x + 1] = r1 - r0; }
  }
  // epilogue: reduce mod p with the 24-bit multiply (|q| < 2^23), pack the 4 consecutive rows a lane holds into one dword of U[j][i]
  const int p = mod.p[item % NMOD], lo = -(p / 2);
  const float rp = 1.0f / (float)p;
  int8_t* Ub = U + (size_t)item * Np * Mp;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const size_t j = (size_t)t.y * TILE + wc * 64 + n * 16 + frow;      // C/D map of 16x16: column = lane & 15, row = 4 (lane >> 4) + e
      const int i = t.x * TILE + wr * 128 + m * 16 + 4 * fk;
      unsigned w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) w |= (unsigned)(mod_sym24(acc[m][n][e], p, rp, lo) & 0xFF) << (8 * e);
      *reinterpret_cast<unsigned*>(Ub + j * Mp + i) = w;
    }
}

// The library's epilogue reduction (lmm_emul.h, emul_acc_residue): x = hi 2^16 + lo is folded to y = hi (2^16 mod p) + lo, |y| < 2^19.2,
// where rint(y fl(1 / p)) is the nearest integer to y / p, so y - q p is the symmetric residue with no correction; the float steps run
// on 1.5 2^23 + y, whose bit pattern's low byte ends as the residue's.
__device__ __forceinline__ int fold_const(int p) { const int r = 65536 % p; return r > p / 2 ? r - p : r; }
__device__ __forceinline__ unsigned acc_residue(int x, int c, float pf, float rp) {
  const float ym = __uint_as_float((unsigned)(__mul24(x >> 16, c) + (int)(((unsigned)x & 0xFFFFu) | 0x4B400000u)));
  const float q = rintf((ym - 12582912.0f) * rp);
  return __float_as_uint(fmaf(-q, pf, ym)) & 0xFFu;
}

// 4 x 4 transpose of w[0..3] over the lanes c, c + 16, c + 32, c + 48, for every c (the library's emul_transpose4): afterwards w[k] of
// row g is what w[g] of row k was.  v_permlane32_swap_b32 exchanges rows 2, 3 of its first operand with rows 0, 1 of its second,
// v_permlane16_swap_b32 the odd rows of the first with the even rows of the second.
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void transpose4(unsigned (&w)[4]) {
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

// The library's emul_gemm_kernel (lmm_kernels_i8.hip): i8_syrk_mod_kernel_pf above with a persistent grid, the K steps of
// consecutive tiles as one stream of stages, and the fold reduction in the epilogue (EPI 3: with 16-byte stores, the library's; EPI 0:
// with dword stores, the library's before); i8_syrk_mod_kernel_pf stays as the baseline.
// ABL picks the K loop.  0: the loop the library had before the half-stage staging, described below.  1 .. 4 are its ablation legs,
// which differ from it by one thing each, compute wrong products on purpose and are timed only: 1 (a) no global_load_lds after the
// prologue (the LDS keeps stages 0 and 1), 2 (b) no fragment reads after the prologue, 3 (c) no wait and no barrier, 4 (d) every
// tile of an item on operand panels 0 and 1 (L2-resident).  5 (e): the 8 pieces of a stage issued 2 at a time after the first and
// third group of 4 MFMAs of phase 4 and of the next step's phase 1, still waited for with vmcnt(0).  6 (f): THE LIBRARY'S LOOP NOW:
// the B half of buffer s & 1 restaged in phase 3 behind a second barrier after phase 2, the A half in phase 4, one piece after each
// group of 4 MFMAs, the wait between phases 3 and 4 vmcnt(4) (vmcnt(0) when phase 3 issued nothing and after an epilogue); the
// phase table and the ordering argument of that loop are in lmm_kernels_i8.hip.
// Persistent: the grid is min(work ids, CUs) workgroups (launch_ps takes the cap), a work id = an (item, tile) pair in the
// order item-major, tile list inside.  Blocks b and b + 8 share an XCD: XCD b & 7 owns a contiguous range of ids and its w workgroups
// walk it from (b >> 3) with stride w, so at any moment the workgroups of an XCD sit on w consecutive ids, one supertile.  The walk
// is static: no workgroup waits for, or reads anything written by, another one.
//
// The K steps of the tiles a workgroup walks form ONE stream of stages s = 0, 1, 2, ..; stage s lives in buffer s & 1 (not kt & 1:
// nk may be odd).  A staging cursor (tile base pointers, k offset) runs two stages ahead of the MFMAs and steps into the next work
// id when it has issued a tile's last K step, so the last two K steps of a tile stage the first two of the next one (with nk = 1
// the cursor is two TILES ahead), and between the last MFMA of a tile and the first of the next only the epilogue stands, with the
// next tile's loads and its first fragment reads issued above it.
//
// One K step is four phases of 16 MFMAs, (ks, mh) = the 64-byte half of the k range x the upper / lower 4 of the wave's 8 row
// fragments.  The fragments of a phase are read into registers in the MIDDLE of the phase before it, between its two groups of 8
// MFMAs, so they are 8 MFMAs old when the wait before their first use comes (the compiler waits with lgkmcnt(0) there, so reads
// issued right before that wait would be waited for too).  sched_barrier(0) pins that order: left alone, the scheduler sinks the
// reads down to their uses.  The one barrier of a K step stands between phases 3 and 4.
//
//   phase of stage s | MFMAs use (registers)        | ds_reads issued (buffer)                 | global_load_lds issued
//   1 (ks 0, mh 0)   | a[0..3], b[0..3]   of s      | a[4..7] ks 0 of s  (s & 1)               |
//   2 (ks 0, mh 1)   | a[4..7], b[0..3]   of s      | a[0..3], b[0..3] ks 1 of s  (s & 1)      |
//   3 (ks 1, mh 0)   | a[0..3]', b[0..3]' of s      | a[4..7] ks 1 of s  (s & 1): the LAST read of buffer s & 1
//   -- s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier: every wave holds all its fragments of stage s in registers, and every wave's
//      loads of stage s + 1 (issued one whole K step earlier, at this point of stage s - 1) have landed in buffer (s + 1) & 1 --
//   4 (ks 1, mh 1)   | a[4..7]', b[0..3]' of s      | a[0..3], b[0..3] ks 0 of s + 1 ((s+1)&1) | stage s + 2 into buffer s & 1
//   -- after the last stage of a tile: the epilogue of that tile (registers and global stores only) --
//
//   read after write: buffer (s + 1) & 1 is first read in phase 4 of stage s, after the wait-plus-barrier that retires stage s + 1.
//   write after read: buffer s & 1 is restaged in phase 4 of stage s, after the barrier every wave reaches only with its last reads
//   of that buffer (phase 3) complete.  Neither argument looks at which tile a stage belongs to: stages s, s + 1, s + 2 may lie in
//   one, two or three tiles, and the epilogue touches no LDS and stands after phase 4 of a stage and before phase 1 of the next,
//   where the schedule has no LDS ordering to keep.  One stage is in flight at a time, so the wait is vmcnt(0); it waits for loads
//   that are one K step (64 MFMAs per wave) old, and after a tile boundary also for the epilogue's 32 stores per lane, as old.
//   The prologue (once per workgroup) stages 0, waits, and stages 1 if the walk has a second stage at all.
template <bool STAMP, int EPI, int ABL = 0>
__global__ __launch_bounds__(512, 2) void i8_syrk_mod_kernel_ps(const int8_t* __restrict__ R, int8_t* __restrict__ U, const int2* __restrict__ tiles, int ntiles,
                                                                int nids, int Mp, int Np, int K, Moduli mod, unsigned long long* __restrict__ stamps) {
  __shared__ __attribute__((aligned(1024))) int8_t lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // the walk of this workgroup: ids first, first + step, .. (cnt of them) of its XCD's range; fewer than 8 workgroups split the ids
  // among themselves
  const int nwg = gridDim.x, parts = nwg < 8 ? nwg : 8, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int step = (nwg >> 3) + (xcd < (nwg & 7) ? 1 : 0);
  const int qi = nids / parts, ri = nids - qi * parts;
  const int first = xcd * qi + (xcd < ri ? xcd : ri) + slot, span = qi + (xcd < ri ? 1 : 0) - slot;
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
  const int8_t* cA = nullptr;
  const int8_t* cB = nullptr;
  int cn = 0, ck = 0, pitem = 0;
  int2 pt = make_int2(0, 0);
  auto cursor_peek = [&](int idn) {
    pitem = idn / ntiles;
    pt = tiles[idn - pitem * ntiles];
  };
  auto cursor_tile = [&]() {
    const int8_t* Rb = R + (size_t)pitem * Mp * K;
    cA = Rb + (size_t)(ABL == 4 ? 0 : pt.x) * TILE * K;
    cB = Rb + (size_t)(ABL == 4 ? 1 : pt.y) * TILE * K;
    if (cn + 1 < cnt) cursor_peek(first + (cn + 1) * step);
  };
  auto cursor_step = [&]() {
    ck += BK;
    if (ck == K) {
      ck = 0; ++cn;
      if (cn < cnt) cursor_tile();
    }
  };
  // pieces q0, q0 + 1 of the cursor's stage (0..3: A, 4..7: B) into buffer buf
  auto pieces2 = [&](int buf, int q0) {
    int8_t* base = lds + buf * STAGE_BYTES + wid * 4096;
#pragma unroll
    for (int q = q0; q < q0 + 2; ++q) {
      if (q < 4) glds16(cA + ck + roff[q], base + q * 1024);
      else glds16(cB + ck + roff[q - 4], base + TILE * BK + (q - 4) * 1024);
    }
  };
  auto piece1 = [&](int buf, int q) {
    int8_t* base = lds + buf * STAGE_BYTES + wid * 4096;
    if (q < 4) glds16(cA + ck + roff[q], base + q * 1024);
    else glds16(cB + ck + roff[q - 4], base + TILE * BK + (q - 4) * 1024);
  };
  auto stage_next = [&](int buf, bool load) {      // cn < cnt
    if (load) {
#pragma unroll
      for (int q0 = 0; q0 < 8; q0 += 2) pieces2(buf, q0);
    }
    cursor_step();
  };
  const int nk = K / BK, frow = lane & 15, fk = lane >> 4;
  // byte offset of a fragment in its stage: (row 128) + ((ks 4 + fk) ^ (row >> 1) & 7) 16 with row = 16 m + frow (+ the wave's first
  // row, a multiple of 64): the swizzle is (frow >> 1), and ks = 1 flips bit 6 of the offset
  const int offA = (wr * 128 + frow) * BK + ((fk ^ (frow >> 1)) << 4), offB = TILE * BK + (wc * 64 + frow) * BK + ((fk ^ (frow >> 1)) << 4);
  auto frag = [&](const int8_t* st, int off, int ks, int f) { return *reinterpret_cast<const v4i*>(st + (off ^ (ks << 6)) + f * 16 * BK); };
  v4i acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (v4i){0, 0, 0, 0};
  unsigned long long t0 = 0, r0 = 0;
  if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  cursor_peek(first);
  cursor_tile();
  stage_next(0, true);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (cn < cnt) stage_next(1, true);
  v4i alo[4], ahi[4], b[4], alo1[4], ahi1[4], b1[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) { alo[f] = frag(lds, offA, 0, f); b[f] = frag(lds, offB, 0, f); }
  if (ABL == 2) {      // every fragment register is read once, here, from stage 0
#pragma unroll
    for (int f = 0; f < 4; ++f) { ahi[f] = frag(lds, offA, 0, 4 + f); alo1[f] = frag(lds, offA, 1, f); b1[f] = frag(lds, offB, 1, f); ahi1[f] = frag(lds, offA, 1, 4 + f); }
  }
  bool stored = false;    // ABL 6: an epilogue's stores have been issued since the last wait
  bool pend = false;      // ABL 5: the B pieces of the cursor's stage are still to be issued, in phase 1 of the next K step
  // 8 MFMAs: row fragments 2 h, 2 h + 1 of A4 (accumulator rows M0 + 2 h ..) x the 4 column fragments
#define EMUL_MMA8(A4, B4, M0, h)                                                                                                   \
  _Pragma("unroll") for (int m = 2 * (h); m < 2 * (h) + 2; ++m)                                                                    \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + m][n], 0, 0, 0)
#define EMUL_MMA4(A4, B4, M0, m)                                                                                                   \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + (m)][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + (m)][n], 0, 0, 0)
#define EMUL_PIN() __builtin_amdgcn_sched_barrier(0)
  int par = 0;      // s & 1
  for (int n = 0, id = first; n < cnt; ++n, id += step) {
    // what the epilogue of this work id needs, loaded above its K loop
    const int item = id / ntiles;
    const int2 t = tiles[id - item * ntiles];
    const int p = mod.p[item % NMOD];
    for (int kt = 0; kt < nk; ++kt, par ^= 1) {
      const int8_t* cur = lds + par * STAGE_BYTES;
      const int8_t* nxt = lds + (par ^ 1) * STAGE_BYTES;
      if (ABL == 6) {      // the split ring: the B half of a buffer is free after phase 2, the A half after phase 3
        EMUL_MMA8(alo, b, 0, 0); EMUL_PIN();      // phase 1
#pragma unroll
        for (int f = 0; f < 4; ++f) ahi[f] = frag(cur, offA, 0, 4 + f);
        EMUL_PIN(); EMUL_MMA8(alo, b, 0, 1); EMUL_PIN();
        EMUL_MMA8(ahi, b, 4, 0); EMUL_PIN();      // phase 2
#pragma unroll
        for (int f = 0; f < 4; ++f) { alo1[f] = frag(cur, offA, 1, f); b1[f] = frag(cur, offB, 1, f); }      // b1: the LAST read of the B half
        EMUL_PIN(); EMUL_MMA8(ahi, b, 4, 1); EMUL_PIN();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        pend = cn < cnt;      // stage s + 2 exists: its B half goes into this buffer now, its A half in phase 4
        EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 0); EMUL_PIN();      // phase 3
        if (pend) piece1(par, 4);
        EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 1); EMUL_PIN();
        if (pend) piece1(par, 5);
#pragma unroll
        for (int f = 0; f < 4; ++f) ahi1[f] = frag(cur, offA, 1, 4 + f);      // the LAST read of the A half
        EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 2); EMUL_PIN();
        if (pend) piece1(par, 6);
        EMUL_PIN(); EMUL_MMA4(alo1, b1, 0, 3); EMUL_PIN();
        if (pend) piece1(par, 7);
        // stage s + 1 (8 pieces) has to have landed; only the 4 pieces just issued are younger.  After an epilogue its stores count too.
        if (pend && !stored) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        stored = false;
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 0); EMUL_PIN();      // phase 4
        if (pend) piece1(par, 0);
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 1); EMUL_PIN();
        if (pend) piece1(par, 1);
        if (kt + 1 < nk || n + 1 < cnt) {
#pragma unroll
          for (int f = 0; f < 4; ++f) { alo[f] = frag(nxt, offA, 0, f); b[f] = frag(nxt, offB, 0, f); }
        }
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 2); EMUL_PIN();
        if (pend) piece1(par, 2);
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 3); EMUL_PIN();
        if (pend) { piece1(par, 3); cursor_step(); }
        EMUL_PIN();
        continue;
      }
      if (ABL == 5) {      // phase 1 with the second half of the stage begun in phase 4 of the step before (buffer par ^ 1)
        EMUL_MMA4(alo, b, 0, 0); EMUL_PIN();
        if (pend) pieces2(par ^ 1, 4);
        EMUL_PIN(); EMUL_MMA4(alo, b, 0, 1); EMUL_PIN();
      } else {
        EMUL_MMA8(alo, b, 0, 0); EMUL_PIN();      // phase 1
      }
      if (ABL != 2) {
#pragma unroll
        for (int f = 0; f < 4; ++f) ahi[f] = frag(cur, offA, 0, 4 + f);
      }
      if (ABL == 5) {
        EMUL_PIN(); EMUL_MMA4(alo, b, 0, 2); EMUL_PIN();
        if (pend) { pieces2(par ^ 1, 6); cursor_step(); pend = false; }
        EMUL_PIN(); EMUL_MMA4(alo, b, 0, 3); EMUL_PIN();
      } else {
        EMUL_PIN(); EMUL_MMA8(alo, b, 0, 1); EMUL_PIN();
      }
      EMUL_MMA8(ahi, b, 4, 0); EMUL_PIN();      // phase 2
      if (ABL != 2) {
#pragma unroll
        for (int f = 0; f < 4; ++f) { alo1[f] = frag(cur, offA, 1, f); b1[f] = frag(cur, offB, 1, f); }
      }
      EMUL_PIN(); EMUL_MMA8(ahi, b, 4, 1); EMUL_PIN();
      EMUL_MMA8(alo1, b1, 0, 0); EMUL_PIN();    // phase 3
      if (ABL != 2) {
#pragma unroll
        for (int f = 0; f < 4; ++f) ahi1[f] = frag(cur, offA, 1, 4 + f);
      }
      EMUL_PIN(); EMUL_MMA8(alo1, b1, 0, 1); EMUL_PIN();
      if (ABL != 3) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      if (ABL == 5) {      // phase 4 with the first half of stage s + 2: 2 pieces after the first and the third group of 4 MFMAs
        pend = cn < cnt;
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 0); EMUL_PIN();
        if (pend) pieces2(par, 0);
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 1); EMUL_PIN();
      } else {
        if (cn < cnt) stage_next(par, ABL != 1);
        EMUL_PIN(); EMUL_MMA8(ahi1, b1, 4, 0); EMUL_PIN();      // phase 4
      }
      if (ABL != 2 && (kt + 1 < nk || n + 1 < cnt)) {
#pragma unroll
        for (int f = 0; f < 4; ++f) { alo[f] = frag(nxt, offA, 0, f); b[f] = frag(nxt, offB, 0, f); }
      }
      if (ABL == 5) {
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 2); EMUL_PIN();
        if (pend) pieces2(par, 2);
        EMUL_PIN(); EMUL_MMA4(ahi1, b1, 4, 3); EMUL_PIN();
      } else {
        EMUL_PIN(); EMUL_MMA8(ahi1, b1, 4, 1); EMUL_PIN();
      }
    }
    // epilogue of work id `id`: reduce mod p (|acc| <= K 128^2 <= 2^28), pack the 4 consecutive rows a lane holds into one dword of
    // U[j][i], and clear the accumulators for the next tile.  EPI 0: the fold reduction with one dword store per 16 x 16 block (the
    // library's before the 16-byte stores), 1: the low byte as it is (wrong but for p = 256: the floor of any epilogue), 2: the
    // two-correction reduction of the kernel before, 3: the fold reduction, the dwords of four row fragments transposed over the four
    // row groups of a column (transpose4) and stored as one 16-byte piece per lane (the library's)
    const int cf = fold_const(p), lo = -(p / 2);
    const float pf = (float)p, rp = 1.0f / pf;
    int8_t* Ub = U + (size_t)item * Np * Mp;
    if (EPI == 3) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          unsigned w[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            w[k] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[k] |= acc_residue(acc[4 * q + k][nn][e], cf, pf, rp) << (8 * e);
            acc[4 * q + k][nn] = (v4i){0, 0, 0, 0};
          }
          transpose4(w);
          const size_t j = (size_t)t.y * TILE + wc * 64 + nn * 16 + frow;
          const int i = t.x * TILE + wr * 128 + (4 * q + fk) * 16;
          *reinterpret_cast<v4u*>(Ub + j * Mp + i) = (v4u){w[0], w[1], w[2], w[3]};
        }
    } else {
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          const size_t j = (size_t)t.y * TILE + wc * 64 + nn * 16 + frow;      // C/D map of 16x16: column = lane & 15, row = 4 (lane >> 4) + e
          const int i = t.x * TILE + wr * 128 + m * 16 + 4 * fk;
          unsigned w = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = acc[m][nn][e];
            w |= (EPI == 0 ? acc_residue(x, cf, pf, rp) : EPI == 1 ? (unsigned)x & 0xFFu : (unsigned)(mod_sym24(x, p, rp, lo) & 0xFF)) << (8 * e);
          }
          *reinterpret_cast<unsigned*>(Ub + j * Mp + i) = w;
          acc[m][nn] = (v4i){0, 0, 0, 0};
        }
    }
    stored = true;
  }
#undef EMUL_MMA8
#undef EMUL_MMA4
#undef EMUL_PIN
  if (ABL == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no wave ends with a load into LDS in flight
  if (STAMP) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) { stamps[2 * (size_t)blockIdx.x] = t1 - t0; stamps[2 * (size_t)blockIdx.x + 1] = r1 - r0; }
  }
}


constexpr int HK = 64, HALF_BYTES = 2 * TILE * HK;      // a half-stage: 64 bytes of k of the A tile + of the B tile

// MEASURED AND NOT KEPT: the persistent walk and the epilogue of i8_syrk_mod_kernel_ps<.., 3> above, with the K loop
// staged in half-stages of 64 bytes of k through a ring of four LDS slots and waited for with counted vmcnt.  Exact, and slower than
// the loop it was to replace: its pieces are 16 rows x 64 B, half a 128-byte line per row.  SWZ false: the same kernel without the
// chunk XOR on either side (the same bytes out; it is there to time the bank conflicts the XOR removes).
//   workgroup tile 256 x 256 x 128, 8 waves as 2 (M) x 4 (N), v_mfma_i32_16x16x64_i8 (wave tile 128 x 64 = 8 x 4 accumulators);
//   the 128 KiB of LDS are a ring of four 32-KiB slots; a slot holds one HALF-STAGE: 64 bytes of k of the A tile (256 rows x 64 B)
//   and of the B tile, filled by global_load_lds_dwordx4 in pieces of 16 rows x 64 B (each wave 2 of A and 2 of B per half-stage);
//   LDS rows are 64 B, four to a 256-B bank row; the 16-B chunk c of row r is stored at chunk c ^ ((0 - (r >> 2)) & 3), the XOR put
//   on the SOURCE address of the piece and on the fragment read, so every ds_read_b128 lane group hits 16 distinct 16-B slots.
// Both operands are fragment-loaded the same way (lane l: row l & 15, bytes 16 (l >> 4) .. + 15 of the 64-deep k range), so the k
// order inside an MFMA is the same for A and B whatever the hardware's k map is.  Mp, Np multiples of 256, K of 128: no edges.
//
// Persistent: the grid is min(work ids, CUs) workgroups (launch_hs takes the cap), a work id = an (item, tile) pair in the
// order item-major, tile list inside.  Blocks b and b + 8 share an XCD: XCD b & 7 owns a contiguous range of ids and its w workgroups
// walk it from (b >> 3) with stride w, so at any moment the workgroups of an XCD sit on w consecutive ids, one supertile.  The walk
// is static: no workgroup waits for, or reads anything written by, another one.
//
// The half-stages of the tiles a workgroup walks form ONE stream h = 0, 1, 2, .. (two per K step of 128, 2 nk per tile); half-stage h
// lives in slot h & 3.  A staging cursor (tile base pointers, k offset) runs four half-stages ahead of the MFMAs and steps into the
// next work id when it has issued a tile's last half-stage (with nk = 1 the cursor is two TILES ahead), so between the last MFMA
// of a tile and the first of the next only the epilogue stands, with the next tile's loads and first fragment reads issued above it.
//
// A half-stage is two phases of 16 MFMAs (mh = the upper / lower 4 of the wave's 8 row fragments).  The fragments of a phase are read
// into registers in the MIDDLE of the phase before it, between its two groups of 8 MFMAs, so they are 8 MFMAs old when the wait before
// their first use comes.  sched_barrier(0) pins that order: left alone, the scheduler sinks the reads down to their uses.  The loop
// body is one K step = half-stages h (even) and h + 1, which alternate between two sets of fragment registers.
//
//   phase of half-stage h | MFMAs use (registers)   | ds_reads issued (slot)                  | global_load_lds issued
//   1 (mh 0)              | a[0..3], b[0..3] of h   | a[4..7] of h (h & 3): the LAST read of slot h & 3
//   -- s_waitcnt lgkmcnt(0) vmcnt(n); s_barrier: every wave holds all its fragments of h in registers, and every wave's pieces of
//      h + 1 have landed in slot (h + 1) & 3.  n = 8: the wave's pieces of h + 2 and h + 3, issued after those of h + 1, may still
//      be in flight; less at the tail of the walk, 0 right after an epilogue (see below) --
//   2 (mh 1)              | a[4..7], b[0..3] of h   | a[0..3], b[0..3] of h + 1 ((h + 1) & 3) | h + 4 into slot h & 3: one piece
//                                                                                               after each group of 4 MFMAs
//   -- after the last half-stage of a tile: the epilogue of that tile (registers and global stores only) --
//
//   read after write: slot (h + 1) & 3 is first read in phase 2 of h, after the wait-plus-barrier of h: each wave has waited for its
//   own pieces of h + 1 (a wave's loads retire in the order it issued them, so at most 8 outstanding means h + 1 and everything
//   older have landed), and the barrier makes that true of all eight waves before any of them reads.
//   write after read: slot h & 3 is restaged with h + 4 in phase 2 of h, after the barrier of h, which every wave reaches only with
//   its last reads of that slot (phase 1 of h) complete (lgkmcnt(0)).  The pieces of h + 4 are waited for three half-stages
//   (96 MFMAs per wave) later, at the barrier of h + 3.
//   Neither argument looks at which tile a half-stage belongs to: h .. h + 4 may lie in one to three tiles (five with nk = 1), and
//   the epilogue touches no LDS and stands after phase 2 of a half-stage and before phase 1 of the next, where the schedule has no
//   LDS ordering to keep.
//   The count: `issued` half-stages have been issued when the wait of h comes, so issued - h - 2 of them are younger than h + 1,
//   4 loads each.  That is 2 in the steady state and 1, 0, 0 for the last three half-stages of the walk, when the cursor has run
//   out: vmcnt(8) there would not wait for the half-stage about to be read.  The epilogue's 8 stores per lane count in vmcnt too
//   and nothing here relies on how stores retire relative to loads: the first wait after an epilogue is vmcnt(0), once per tile.
//   The prologue (once per workgroup) issues up to four half-stages and waits for the first with the same count.
template <bool STAMP, bool SWZ>
__global__ __launch_bounds__(512, 2) void i8_syrk_mod_kernel_hs(const int8_t* __restrict__ R, int8_t* __restrict__ U, const int2* __restrict__ tiles, int ntiles,
                                                                int nids, int Mp, int Np, int K, Moduli mod, unsigned long long* __restrict__ stamps) {
  __shared__ __attribute__((aligned(1024))) int8_t lds[4 * HALF_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // the walk of this workgroup: ids first, first + step, .. (cnt of them) of its XCD's range; fewer than 8 workgroups split the ids
  // among themselves
  const int nwg = gridDim.x, parts = nwg < 8 ? nwg : 8, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int step = (nwg >> 3) + (xcd < (nwg & 7) ? 1 : 0);
  const int qi = nids / parts, ri = nids - qi * parts;
  const int first = xcd * qi + (xcd < ri ? xcd : ri) + slot, span = qi + (xcd < ri ? 1 : 0) - slot;
  const int cnt = span > 0 ? (span + step - 1) / step : 0;
  if (cnt == 0) return;
  // source offsets of a lane's two 16-byte loads of one operand, from the tile's first row at k = 0: lane l of a piece lands at
  // row l >> 2, chunk slot l & 3 and fetches the source chunk that the swizzle stores there
  unsigned roff[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = wid * 32 + q * 16 + (lane >> 2), chunk = (lane & 3) ^ (SWZ ? (0 - (row >> 2)) & 3 : 0);
    roff[q] = (unsigned)row * (unsigned)K + chunk * 16;
  }
  // the staging cursor: operand panels of the cn-th work id of the walk, next k offset ck; (pitem, pt) is the (cn + 1)-th work id,
  // loaded one tile ahead so that stepping into it waits for no load
  const int8_t* cA = nullptr;
  const int8_t* cB = nullptr;
  int cn = 0, ck = 0, pitem = 0;
  int2 pt = make_int2(0, 0);
  auto cursor_peek = [&](int idn) {
    pitem = idn / ntiles;
    pt = tiles[idn - pitem * ntiles];
  };
  auto cursor_tile = [&]() {
    const int8_t* Rb = R + (size_t)pitem * Mp * K;
    cA = Rb + (size_t)pt.x * TILE * K;
    cB = Rb + (size_t)pt.y * TILE * K;
    if (cn + 1 < cnt) cursor_peek(first + (cn + 1) * step);
  };
  int issued = 0, h = 0;      // half-stages issued so far; the half-stage the MFMAs are in
  // piece i (0, 1: A; 2, 3: B) of the cursor's half-stage into slot sl; the cursor moves on with the last one
  auto piece = [&](int sl, int i) {      // cn < cnt
    int8_t* base = lds + sl * HALF_BYTES + wid * 2048;
    if (i < 2) glds16(cA + ck + roff[i], base + i * 1024);
    else glds16(cB + ck + roff[i - 2], base + TILE * HK + (i - 2) * 1024);
    if (i == 3) {
      ck += HK; ++issued;
      if (ck == K) {
        ck = 0; ++cn;
        if (cn < cnt) cursor_tile();
      }
    }
  };
  bool stored = false;      // an epilogue's stores have been issued since the last wait
  // the wait-plus-barrier of half-stage h (see above); all branches are uniform
  auto retire = [&]() {
    const int younger = stored ? 0 : issued - h - 2;
    if (younger >= 3) asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stored = false; ++h;
  };
  const int nk = K / BK, frow = lane & 15, fk = lane >> 4;
  // byte offset of a fragment in its slot: (row 64) + ((fk ^ (0 - (row >> 2)) & 3) 16) with row = 16 m + frow (+ the wave's first
  // row, a multiple of 64): the swizzle is that of frow
  const int fsw = (fk ^ (SWZ ? (0 - (frow >> 2)) & 3 : 0)) << 4;
  const int offA = (wr * 128 + frow) * HK + fsw, offB = TILE * HK + (wc * 64 + frow) * HK + fsw;
  auto frag = [&](const int8_t* st, int off, int f) { return *reinterpret_cast<const v4i*>(st + off + f * 16 * HK); };
  v4i acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (v4i){0, 0, 0, 0};
  unsigned long long t0 = 0, r0 = 0;
  if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  cursor_peek(first);
  cursor_tile();
#pragma unroll
  for (int sl = 0; sl < 4; ++sl)
    if (cn < cnt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) piece(sl, i);
    }
  h = -1;      // the wait for half-stage 0 is that of a half-stage -1
  retire();
  v4i alo[4], ahi[4], b[4], alo1[4], ahi1[4], b1[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) { alo[f] = frag(lds, offA, f); b[f] = frag(lds, offB, f); }
  // 4 MFMAs: row fragment m of A4 (accumulator row M0 + m) x the 4 column fragments
#define EMUL_MMA4(A4, B4, M0, m)                                                                                                   \
  _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[(M0) + (m)][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A4[m], B4[n], acc[(M0) + (m)][n], 0, 0, 0)
#define EMUL_PIN() __builtin_amdgcn_sched_barrier(0)
  // phase 1 of a half-stage held in (ALO, B): its a[4..7] are read from slot SL into AHI, then the wait-plus-barrier
#define EMUL_PHASE1(ALO, AHI, B, SL)                                                                                               \
  EMUL_MMA4(ALO, B, 0, 0); EMUL_MMA4(ALO, B, 0, 1); EMUL_PIN();                                                                    \
  _Pragma("unroll") for (int f = 0; f < 4; ++f) AHI[f] = frag(lds + (SL) * HALF_BYTES, offA, 4 + f);                               \
  EMUL_PIN(); EMUL_MMA4(ALO, B, 0, 2); EMUL_MMA4(ALO, B, 0, 3); EMUL_PIN();                                                        \
  retire(); EMUL_PIN()
  // phase 2 of the half-stage in slot SL, held in (AHI, B): the cursor's half-stage goes into SL, one piece after each group of 4
  // MFMAs, and if MORE the first fragments of the next half-stage are read from slot SN into (ALO, BN)
#define EMUL_PHASE2(AHI, B, SL, ALO, BN, SN, MORE)                                                                                 \
  {                                                                                                                                \
    const bool st = cn < cnt;                                                                                                      \
    EMUL_MMA4(AHI, B, 4, 0); EMUL_PIN();                                                                                           \
    if (st) piece(SL, 0);                                                                                                          \
    EMUL_PIN(); EMUL_MMA4(AHI, B, 4, 1); EMUL_PIN();                                                                               \
    if (st) piece(SL, 1);                                                                                                          \
    if (MORE) {                                                                                                                    \
      _Pragma("unroll") for (int f = 0; f < 4; ++f) { ALO[f] = frag(lds + (SN) * HALF_BYTES, offA, f); BN[f] = frag(lds + (SN) * HALF_BYTES, offB, f); } \
    }                                                                                                                              \
    EMUL_PIN(); EMUL_MMA4(AHI, B, 4, 2); EMUL_PIN();                                                                               \
    if (st) piece(SL, 2);                                                                                                          \
    EMUL_PIN(); EMUL_MMA4(AHI, B, 4, 3); EMUL_PIN();                                                                               \
    if (st) piece(SL, 3);                                                                                                          \
    EMUL_PIN();                                                                                                                    \
  }
  int par = 0;      // (h >> 1) & 1 at the top of a K step: its half-stages live in slots 2 par and 2 par + 1
  for (int n = 0, id = first; n < cnt; ++n, id += step) {
    // what the epilogue of this work id needs, loaded above its K loop
    const int item = id / ntiles;
    const int2 t = tiles[id - item * ntiles];
    const int p = mod.p[item % NMOD];
    for (int kt = 0; kt < nk; ++kt, par ^= 1) {
      const int s0 = 2 * par, s1 = s0 + 1, s2 = s0 ^ 2;
      EMUL_PHASE1(alo, ahi, b, s0);
      EMUL_PHASE2(ahi, b, s0, alo1, b1, s1, true);
      EMUL_PHASE1(alo1, ahi1, b1, s1);
      EMUL_PHASE2(ahi1, b1, s1, alo, b, s2, kt + 1 < nk || n + 1 < cnt);
    }
    // epilogue of work id `id`: that of i8_syrk_mod_kernel_ps<.., 3>; the accumulators are cleared for the next tile
    const int cf = fold_const(p);
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
          for (int e = 0; e < 4; ++e) w[k] |= acc_residue(acc[4 * q + k][nn][e], cf, pf, rp) << (8 * e);
          acc[4 * q + k][nn] = (v4i){0, 0, 0, 0};
        }
        transpose4(w);
        const size_t j = (size_t)t.y * TILE + wc * 64 + nn * 16 + frow;
        const int i = t.x * TILE + wr * 128 + (4 * q + fk) * 16;
        *reinterpret_cast<v4u*>(Ub + j * Mp + i) = (v4u){w[0], w[1], w[2], w[3]};
      }
    stored = true;
  }
#undef EMUL_MMA4
#undef EMUL_PIN
#undef EMUL_PHASE1
#undef EMUL_PHASE2
  if (STAMP) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) { stamps[2 * (size_t)blockIdx.x] = t1 - t0; stamps[2 * (size_t)blockIdx.x + 1] = r1 - r0; }
  }
}


// bare issue rate: operands in registers, 4 independent accumulators, no memory traffic
__global__ __launch_bounds__(256) void mfma_i8_bare(int* out, unsigned long long* stamps, int iters) {
  v16i acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0;
  unsigned h = (blockIdx.x * 256u + threadIdx.x + 1u) * 2654435761u;
  v4i a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) { h = h * 1664525u + 1013904223u; a[e] = (int)h; h = h * 1664525u + 1013904223u; b[e] = (int)h; }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q & 3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[q & 3], 0, 0, 0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  int s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[q][e];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0) {
    stamps[(blockIdx.x * 4 + (threadIdx.x >> 6)) * 2] = t1 - t0;
    stamps[(blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + 1] = r1 - r0;
  }
}

__global__ void fill_rand_i8(int8_t* p, size_t n, unsigned seed) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull + seed; z ^= z >> 29; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 32;
    p[i] = (int8_t)(z & 0xFF);
  }
}

// lower-trapezoid tiles in supertiles of 8 tile rows x 4 tile columns: 32 consecutive tiles share at most 12 operand panels
static std::vector<int2> tile_list(int M, int N) {
  std::vector<int2> v;
  const int tm = M / TILE, tn = N / TILE;
  for (int I = 0; I < tm; I += 8)
    for (int J = 0; J < tn; J += 4)
      for (int i = I; i < std::min(I + 8, tm); ++i)
        for (int j = J; j < std::min(J + 4, tn); ++j)
          if (j <= i) v.push_back(make_int2(i, j));
  return v;
}

static int mod_sym_host(long long x, int p) {
  const int lo = -(p / 2);
  long long r = x % p;
  if (r < lo) r += p;
  if (r > lo + p - 1) r -= p;
  return (int)r;
}

template <int SHAPE, bool STAMP>
static void launch(const int8_t* R, int8_t* U, const int2* tiles, int ntiles, int M, int N, int K, int batch, unsigned long long* stamps) {
  if constexpr (SHAPE == 0) i8_syrk_mod_kernel_pf<STAMP><<<ntiles * batch, 512>>>(R, U, tiles, ntiles, M, N, K, kModuli, stamps);      // SHAPE 0: the register-prefetch kernel
  else i8_syrk_mod_kernel<SHAPE, STAMP><<<ntiles * batch, 512>>>(R, U, tiles, ntiles, M, N, K, kModuli, stamps);
}

// the persistent kernel on at most `wgs` workgroups (0: one per CU)
static int g_cus = 256;
template <bool STAMP, int EPI>
static void launch_ps(const int8_t* R, int8_t* U, const int2* tiles, int ntiles, int M, int N, int K, int batch, int wgs, unsigned long long* stamps) {
  const int nids = ntiles * batch;
  i8_syrk_mod_kernel_ps<STAMP, EPI><<<std::min(nids, wgs > 0 ? wgs : g_cus), 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps);
}

// variant v of the K loop on at most `wgs` workgroups (0: one per CU).  0: the loop the library had before the half-stage ring
// (i8_syrk_mod_kernel_ps<.., 3, 0>); 1 .. 5: its legs (a) .. (e) (ABL 1 .. 5 of that kernel); 6: the ring of four 64-byte-deep slots
// (i8_syrk_mod_kernel_hs: built first, slower, not the library's); 7: that ring without the LDS swizzle; 8: (f), the library's loop
// (ABL 6).  1 .. 4 compute wrong products on purpose: they are timed only.
constexpr int NVAR = 9;
static const char* kVarNames[NVAR] = {"shipped before (full-stage burst)", "(a) no global_load_lds", "(b) no fragment reads", "(c) no wait, no barrier",
                                      "(d) operands L2-resident", "(e) pieces spread, vmcnt(0)", "ring of four 64-B slots (rejected)", "ring of four 64-B slots, no swizzle", "(f) halves restaged apart (library)"};
template <bool STAMP>
static void launch_var(int v, const int8_t* R, int8_t* U, const int2* tiles, int ntiles, int M, int N, int K, int batch, int wgs, unsigned long long* stamps) {
  const int nids = ntiles * batch, g = std::min(nids, wgs > 0 ? wgs : g_cus);
  switch (v) {
    case 0: i8_syrk_mod_kernel_ps<STAMP, 3, 0><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 1: i8_syrk_mod_kernel_ps<STAMP, 3, 1><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 2: i8_syrk_mod_kernel_ps<STAMP, 3, 2><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 3: i8_syrk_mod_kernel_ps<STAMP, 3, 3><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 4: i8_syrk_mod_kernel_ps<STAMP, 3, 4><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 5: i8_syrk_mod_kernel_ps<STAMP, 3, 5><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 6: i8_syrk_mod_kernel_hs<STAMP, true><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    case 7: i8_syrk_mod_kernel_hs<STAMP, false><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps); break;
    default: i8_syrk_mod_kernel_ps<STAMP, 3, 6><<<g, 512>>>(R, U, tiles, ntiles, nids, M, N, K, kModuli, stamps);
  }
}

// exact check of U against a host integer product; every == true checks every computed tile and that nothing else was written
static long check(const int8_t* dR, const int8_t* dU, int M, int N, int K, int batch, bool every, const char* what) {
  std::vector<int8_t> hR((size_t)M * K), hU((size_t)N * M);
  long bad = 0, checked = 0;
  for (int b = 0; b < batch; b += every ? 1 : 5) {
    CHECK(hipMemcpy(hR.data(), dR + (size_t)b * M * K, hR.size(), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hU.data(), dU + (size_t)b * N * M, hU.size(), hipMemcpyDeviceToHost));
    const int p = kModuli.p[b % NMOD];
    unsigned long long z = 12345 + b;
    const long n = every ? (long)N * M : 4096;
    for (long s = 0; s < n; ++s) {
      int i, j;
      if (every) { j = (int)(s / M); i = (int)(s % M); }
      else {
        z = z * 6364136223846793005ull + 1442695040888963407ull; i = (int)((z >> 33) % M);
        z = z * 6364136223846793005ull + 1442695040888963407ull; j = (int)((z >> 33) % N);
      }
      const bool computed = i / TILE >= j / TILE;
      if (!computed) { if (every && hU[(size_t)j * M + i] != 0x5A) ++bad; continue; }
      long long d = 0;
      for (int k = 0; k < K; ++k) d += (long long)hR[(size_t)i * K + k] * hR[(size_t)j * K + k];
      ++checked;
      if (hU[(size_t)j * M + i] != (int8_t)mod_sym_host(d, p)) {
        if (bad < 5) printf("  MISMATCH %s b=%d i=%d j=%d got %d want %d\n", what, b, i, j, hU[(size_t)j * M + i], mod_sym_host(d, p));
        ++bad;
      }
    }
  }
  printf("check %-28s M=%5d N=%5d K=%5d: %ld entries compared exactly, %ld wrong\n", what, M, N, K, checked, bad);
  return bad;
}

int main(int argc, char** argv) {
  const int nmat = argc > 1 ? atoi(argv[1]) : 1;
  const bool brief = argc > 2;      // any second argument: the exact checks and one round of the older kernels only
  const bool looponly = argc > 2 && !strcmp(argv[2], "loop");      // "loop": the exact checks and the timing of the K loop's variants (section 4) only
  const int batch = NMOD * nmat;
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  long bad = 0;
  { int dev = 0; CHECK(hipGetDevice(&dev)); CHECK(hipDeviceGetAttribute(&g_cus, hipDeviceAttributeMultiprocessorCount, dev)); }

  if (!brief) {  // 1. bare v_mfma_i32_32x32x32_i8 issue rate and the clock held
    int* out; unsigned long long* st;
    for (int blocks : {256, 512}) {
      const int iters = 200000;
      CHECK(hipMalloc(&out, blocks * 256 * 4)); CHECK(hipMalloc(&st, blocks * 8 * 8));
      mfma_i8_bare<<<blocks, 256>>>(out, st, iters / 10);
      CHECK(hipDeviceSynchronize());
      hipEventRecord(e0);
      mfma_i8_bare<<<blocks, 256>>>(out, st, iters);
      hipEventRecord(e1); CHECK(hipEventSynchronize(e1));
      float ms; hipEventElapsedTime(&ms, e0, e1);
      std::vector<unsigned long long> h(blocks * 8);
      CHECK(hipMemcpy(h.data(), st, blocks * 8 * 8, hipMemcpyDeviceToHost));
      std::vector<double> clk, cyc;
      for (int w = 0; w < blocks * 4; ++w) { clk.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 100.0); cyc.push_back((double)h[2 * w] / iters / 8); }
      std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
      printf("bare v_mfma_i32_32x32x32_i8, %d wave(s)/SIMD: %.3f ms  %.0f TOPS  %.1f wave cycles per MFMA  clock %.0f MHz\n", blocks / 256, ms,
             blocks * 4.0 * iters * 8 * 65536.0 / ms / 1e9, cyc[cyc.size() / 2], clk[clk.size() / 2]);
      CHECK(hipFree(out)); CHECK(hipFree(st));
    }
    fflush(stdout);
  }

  {  // 2. full exact check at a small shape: two tile rows, one tile column, three K tiles, every modulus
    const int M = 512, N = 256, K = 384;
    int8_t *R, *U; int2* dt;
    CHECK(hipMalloc(&R, (size_t)NMOD * M * K)); CHECK(hipMalloc(&U, (size_t)NMOD * N * M));
    fill_rand_i8<<<512, 256>>>(R, (size_t)NMOD * M * K, 7u);
    std::vector<int2> tl = tile_list(M, N);
    CHECK(hipMalloc(&dt, tl.size() * sizeof(int2))); CHECK(hipMemcpy(dt, tl.data(), tl.size() * sizeof(int2), hipMemcpyHostToDevice));
    CHECK(hipMemset(U, 0x5A, (size_t)NMOD * N * M));
    launch<32, false>(R, U, dt, (int)tl.size(), M, N, K, NMOD, nullptr);
    CHECK(hipDeviceSynchronize());
    bad += check(R, U, M, N, K, NMOD, true, "32x32x32 full");
    CHECK(hipMemset(U, 0x5A, (size_t)NMOD * N * M));
    launch<16, false>(R, U, dt, (int)tl.size(), M, N, K, NMOD, nullptr);
    CHECK(hipDeviceSynchronize());
    bad += check(R, U, M, N, K, NMOD, true, "16x16x64 full");
    if (!looponly)
    for (int Kp : {128, 256, 384, 512}) {      // the register-prefetch kernel: K loops shorter than its pipeline, odd and even counts (R holds 512 x 384 x 16 bytes: the same rows, read with K = Kp, for Kp <= 384; 512 fits as M K NMOD = 512 * 512 * 12)
      const int nb = Kp <= K ? NMOD : 12;
      CHECK(hipMemset(U, 0x5A, (size_t)NMOD * N * M));
      launch<0, false>(R, U, dt, (int)tl.size(), M, N, Kp, nb, nullptr);
      CHECK(hipDeviceSynchronize());
      bad += check(R, U, M, N, Kp, nb, true, "16x16x64 prefetch full");
    }
    if (!looponly)
    for (int Kp : {128, 256, 384, 512})      // the persistent kernel: one, two, five workgroups walk the 3 tiles x 16 (12) moduli, and the default grid
      for (int wgs : {1, 2, 5, 0}) {
        const int nb = Kp <= K ? NMOD : 12;
        CHECK(hipMemset(U, 0x5A, (size_t)NMOD * N * M));
        launch_ps<false, 0>(R, U, dt, (int)tl.size(), M, N, Kp, nb, wgs, nullptr);
        CHECK(hipDeviceSynchronize());
        char what[64]; snprintf(what, sizeof what, "persistent full, %d wgs", wgs);
        bad += check(R, U, M, N, Kp, nb, true, what);
        launch_ps<false, 2>(R, U, dt, (int)tl.size(), M, N, Kp, nb, wgs, nullptr);      // the old reduction gives the same bytes
        CHECK(hipDeviceSynchronize());
        bad += check(R, U, M, N, Kp, nb, true, "persistent, old epilogue");
        CHECK(hipMemset(U, 0x5A, (size_t)NMOD * N * M));
        launch_ps<false, 3>(R, U, dt, (int)tl.size(), M, N, Kp, nb, wgs, nullptr);      // ... and so do the 16-byte stores
        CHECK(hipDeviceSynchronize());
        bad += check(R, U, M, N, Kp, nb, true, "persistent, 16-byte stores");
      }
    // the K loop's variants that compute the product (kVarNames 5 .. 8): K / 128 = 1 .. 5 and 9 (the ring wraps at every phase; odd
    // counts; one K step per tile, where the cursor runs two tiles ahead), one to seven workgroups and the default grid.  The loop
    // before (variant 0) on the default grid is checked against the host once per K; its bytes, canaries included, are the reference
    // of every other launch.
    for (int Kp : {128, 256, 384, 512, 640, 1152}) {
      const int nb = std::min(NMOD, NMOD * K / Kp);      // R holds 512 x 384 x 16 bytes: the same bytes read as nb matrices of 512 x Kp
      const size_t ub = (size_t)nb * N * M;
      std::vector<int8_t> ref(ub), got(ub);
      CHECK(hipMemset(U, 0x5A, ub));
      launch_var<false>(0, R, U, dt, (int)tl.size(), M, N, Kp, nb, 0, nullptr);
      CHECK(hipDeviceSynchronize());
      bad += check(R, U, M, N, Kp, nb, true, "loop before, full");
      CHECK(hipMemcpy(ref.data(), U, ub, hipMemcpyDeviceToHost));
      for (int v : {5, 6, 7, 8})
        for (int wgs : {1, 2, 3, 5, 7, 0}) {
          CHECK(hipMemset(U, 0x5A, ub));
          launch_var<false>(v, R, U, dt, (int)tl.size(), M, N, Kp, nb, wgs, nullptr);
          CHECK(hipDeviceSynchronize());
          CHECK(hipMemcpy(got.data(), U, ub, hipMemcpyDeviceToHost));
          long diff = 0;
          for (size_t i = 0; i < ub; ++i) diff += got[i] != ref[i];
          if (diff) printf("  MISMATCH %s, K=%d, %d wgs: %ld bytes differ from the loop before\n", kVarNames[v], Kp, wgs, diff);
          bad += diff;
        }
      printf("check K=%4d: variants (e), (f), half-stage ring, ring without swizzle on 1, 2, 3, 5, 7 workgroups and the default grid: %s\n", Kp, bad ? "WRONG" : "same bytes");
    }
    CHECK(hipFree(R)); CHECK(hipFree(U)); CHECK(hipFree(dt));
    fflush(stdout);
    if (bad) { printf("operand or output map wrong: not timing\n"); return 1; }
  }

  // 3. the C2 level shapes
  struct Shape { int M, N, K; };
  const Shape shapes[] = {{8192, 8192, 8192}, {12288, 4096, 4096}, {14336, 2048, 2048}, {15360, 1024, 1024}};
  for (const Shape& s : shapes) {
    int8_t *R, *U; int2* dt; unsigned long long* st;
    const size_t rb = (size_t)batch * s.M * s.K, ub = (size_t)batch * s.N * s.M;
    CHECK(hipMalloc(&R, rb)); CHECK(hipMalloc(&U, ub));
    fill_rand_i8<<<4096, 256>>>(R, rb, 100u + s.K);
    CHECK(hipMemset(U, 0x5A, ub));
    std::vector<int2> tl = tile_list(s.M, s.N);
    const int nt = (int)tl.size();
    CHECK(hipMalloc(&dt, tl.size() * sizeof(int2))); CHECK(hipMemcpy(dt, tl.data(), tl.size() * sizeof(int2), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&st, (size_t)nt * batch * 16));
    const double outs = (double)s.N * (s.N + 1) / 2 + (double)(s.M - s.N) * s.N;
    const double useful = 2.0 * s.K * outs * batch, issued = 2.0 * s.K * (double)TILE * TILE * nt * batch;
    const int reps = (int)std::max(4.0, 0.15 / (issued / 2.0e15));  // about 150 ms per window at 2 POPS
    if (!looponly) {
    std::vector<float> t32, t16, tpf;
    for (int round = 0; round < (brief ? 1 : 3); ++round)
      for (int v = 0; v < 3; ++v) {
        auto go = [&]() {
          if (v == 0) launch<32, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
          else if (v == 1) launch<16, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
          else launch<0, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
        };
        go();
        hipEventRecord(e0);
        for (int r = 0; r < reps; ++r) go();
        hipEventRecord(e1); CHECK(hipEventSynchronize(e1));
        float ms; hipEventElapsedTime(&ms, e0, e1);
        (v == 0 ? t32 : v == 1 ? t16 : tpf).push_back(ms / reps);
      }
    double clk[3];
    for (int v = 0; v < 3; ++v) {  // diagnostic build with stamps, after the timed windows (the chip is warm)
      for (int r = 0; r < 3; ++r) { if (v == 0) launch<32, true>(R, U, dt, nt, s.M, s.N, s.K, batch, st); else if (v == 1) launch<16, true>(R, U, dt, nt, s.M, s.N, s.K, batch, st); else launch<0, true>(R, U, dt, nt, s.M, s.N, s.K, batch, st); }
      CHECK(hipDeviceSynchronize());
      std::vector<unsigned long long> h((size_t)nt * batch * 2);
      CHECK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
      std::vector<double> c;
      for (size_t w = 0; w < h.size() / 2; ++w) c.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 100.0);
      std::sort(c.begin(), c.end());
      clk[v] = c[c.size() / 2];
    }
    if (brief) for (std::vector<float>* tvp : {&t32, &t16, &tpf}) tvp->resize(2, (*tvp)[0]);
    std::sort(t32.begin(), t32.end()); std::sort(t16.begin(), t16.end()); std::sort(tpf.begin(), tpf.end());
    printf("i8 syrk M=%5d N=%5d K=%5d batch=%d (%d tiles, %d reps) | 32x32x32: min %.3f med %.3f ms, %.0f TOPS useful (%.0f issued), clock %.0f MHz"
           " | 16x16x64: min %.3f med %.3f ms, %.0f TOPS useful (%.0f issued), clock %.0f MHz\n",
           s.M, s.N, s.K, batch, nt, reps, t32[0], t32[1], useful / t32[0] / 1e9, issued / t32[0] / 1e9, clk[0], t16[0], t16[1], useful / t16[0] / 1e9,
           issued / t16[0] / 1e9, clk[1]);
    printf("                                                  | 16x16x64 prefetch (the library's kernel): min %.3f med %.3f ms, %.0f TOPS useful (%.0f issued), clock %.0f MHz"
           " | baseline 16x16x64 / prefetch: medians %.3f\n", tpf[0], tpf[1], useful / tpf[0] / 1e9, issued / tpf[0] / 1e9, clk[2], t16[1] / tpf[1]);
    {  // the persistent kernel and the split of the per-tile fixed cost: grid (one workgroup per tile / per CU) x epilogue (fold
       // reduction / low byte only / the prefetch kernel's), interleaved with the prefetch kernel in every round
      const char* names[8] = {"prefetch (before)", "per tile, fold", "per tile, low byte", "persistent, old epilogue", "persistent, fold, dword stores (before)",
                              "persistent, low byte", "prefetch (before), again", "persistent, fold, 16-byte stores (library)"};
      std::vector<float> tv[8];
      const int nids = nt * batch;
      for (int round = 0; round < 3; ++round)
        for (int v = 0; v < 8; ++v) {
          auto go = [&]() {
            switch (v) {
              case 7: launch_ps<false, 3>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr); break;
              case 1: launch_ps<false, 0>(R, U, dt, nt, s.M, s.N, s.K, batch, nids, nullptr); break;
              case 2: launch_ps<false, 1>(R, U, dt, nt, s.M, s.N, s.K, batch, nids, nullptr); break;
              case 3: launch_ps<false, 2>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr); break;
              case 4: launch_ps<false, 0>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr); break;
              case 5: launch_ps<false, 1>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr); break;
              default: launch<0, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
            }
          };
          go();
          hipEventRecord(e0);
          for (int r = 0; r < reps; ++r) go();
          hipEventRecord(e1); CHECK(hipEventSynchronize(e1));
          float ms; hipEventElapsedTime(&ms, e0, e1);
          tv[v].push_back(ms / reps);
        }
      for (int r = 0; r < 3; ++r) launch_ps<true, 0>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, st);
      CHECK(hipDeviceSynchronize());
      const int g = std::min(nids, g_cus);
      std::vector<unsigned long long> h((size_t)g * 2);
      CHECK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
      std::vector<double> cl;
      for (int w = 0; w < g; ++w) cl.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 100.0);
      std::sort(cl.begin(), cl.end());
      const double tiles_per_cu = (double)nids / g_cus;
      for (int v = 0; v < 8; ++v) {
        std::sort(tv[v].begin(), tv[v].end());
        printf("    %-42s min %.3f med %.3f max %.3f ms, %.0f TOPS useful, %.2f us per tile and CU\n", names[v], tv[v][0], tv[v][1], tv[v][2], useful / tv[v][1] / 1e9,
               tv[v][1] * 1e3 / tiles_per_cu);
      }
      printf("    persistent kernel's clock %.0f MHz; before / persistent medians %.3f; dword / 16-byte stores medians %.3f\n", cl[cl.size() / 2], tv[0][1] / tv[7][1],
             tv[4][1] / tv[7][1]);
      CHECK(hipMemset(U, 0x5A, ub));
      launch_ps<false, 3>(R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr);
      CHECK(hipDeviceSynchronize());
      bad += check(R, U, s.M, s.N, s.K, batch, false, "persistent sampled");
    }
    launch<32, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
    CHECK(hipDeviceSynchronize());
    bad += check(R, U, s.M, s.N, s.K, batch, false, "32x32x32 sampled");
    CHECK(hipMemset(U, 0x5A, ub));
    launch<0, false>(R, U, dt, nt, s.M, s.N, s.K, batch, nullptr);
    CHECK(hipDeviceSynchronize());
    bad += check(R, U, s.M, s.N, s.K, batch, false, "16x16x64 prefetch sampled");
    }
    {  // 4. the K loop: the loop before, its ablation legs, and the half-stage ring, interleaved in every round; the clock of each
      std::vector<float> tv[NVAR];
      const int nids = nt * batch, g = std::min(nids, g_cus);
      const double tiles_per_cu = (double)nids / g_cus;
      for (int round = 0; round < 3; ++round)
        for (int v = 0; v < NVAR; ++v) {
          launch_var<false>(v, R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr);
          hipEventRecord(e0);
          for (int r = 0; r < reps; ++r) launch_var<false>(v, R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr);
          hipEventRecord(e1); CHECK(hipEventSynchronize(e1));
          float ms; hipEventElapsedTime(&ms, e0, e1);
          tv[v].push_back(ms / reps);
        }
      printf("  K loop variants, M=%5d N=%5d K=%5d, %.2f tiles per CU: us per tile and CU, median (min - max) of 3 windows of %d launches; clock\n", s.M, s.N, s.K, tiles_per_cu, reps);
      for (int v = 0; v < NVAR; ++v) {
        for (int r = 0; r < 3; ++r) launch_var<true>(v, R, U, dt, nt, s.M, s.N, s.K, batch, 0, st);
        CHECK(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)g * 2);
        CHECK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
        std::vector<double> cl;
        for (int w = 0; w < g; ++w) cl.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 100.0);
        std::sort(cl.begin(), cl.end());
        std::sort(tv[v].begin(), tv[v].end());
        const double u = 1e3 / tiles_per_cu;
        printf("    %-36s %8.2f (%8.2f - %8.2f) us   %.3f ms   clock %.0f MHz\n", kVarNames[v], tv[v][1] * u, tv[v][0] * u, tv[v][2] * u, tv[v][1], cl[cl.size() / 2]);
      }
      for (int v : {5, 6, 8}) {
        CHECK(hipMemset(U, 0x5A, ub));
        launch_var<false>(v, R, U, dt, nt, s.M, s.N, s.K, batch, 0, nullptr);
        CHECK(hipDeviceSynchronize());
        bad += check(R, U, s.M, s.N, s.K, batch, false, v == 5 ? "(e) sampled" : v == 6 ? "ring of four slots sampled" : "(f) sampled");
      }
    }
    fflush(stdout);
    CHECK(hipFree(R)); CHECK(hipFree(U)); CHECK(hipFree(dt)); CHECK(hipFree(st));
  }
  printf(bad ? "FAILED: %ld wrong entries\n" : "all checks exact (%ld wrong)\n", bad);
  return bad ? 1 : 0;
}
