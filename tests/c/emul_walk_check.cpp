// Stand-alone host check of two index helpers of csrc/lmm_emul.h (no HIP, no GPU):
//   the GEMM's work-id ranges (emul_xcd_range, emul_range_parts, emul_range_wgs): for nids = 1 .. 5000 work ids and 1 .. 300
//   workgroups the ranges are non-negative, follow one another and tile [0, nids) exactly, differ by at most one id, every range has a
//   workgroup, the workgroups of all ranges add up to the grid, and the static walk (first = start + slot, stride = the range's
//   workgroups) visits every id exactly once;
//   the unwritten-piece bitmap (emul_piece_block, emul_piece_word, emul_piece_shift, emul_piece_bytes, emul_aux): for M = 1 .. 16448
//   rows, every (matrix, tile row, K block) gets 16 bits of its own, the last word lies inside emul_piece_bytes, the bitmap starts
//   where the masks end, and both fit emul_aux(..).total, a multiple of 8.
// tests/test_emul_walk_host.py builds and runs it plainly; meant to be built with the sanitizers too:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/emul_walk_check.cpp -o tests/c/emul_walk_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lmm_emul.h"

static int failures = 0;
static long long checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (++failures < 20) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_ranges(int nids, int nwg, bool walk) {
  const int parts = emul_range_parts(nwg);
  CHECK(parts >= 1 && parts <= 8 && parts <= nwg, "nids %d nwg %d parts %d", nids, nwg, parts);
  int next = 0, wgs = 0, lo = nids, hi = 0;
  for (int x = 0; x < parts; ++x) {
    const EmulRange r = emul_xcd_range(nids, nwg, x);
    CHECK(r.start == next && r.len >= 0, "nids %d nwg %d x %d start %d len %d next %d", nids, nwg, x, r.start, r.len, next);
    next = r.start + r.len;
    lo = r.len < lo ? r.len : lo; hi = r.len > hi ? r.len : hi;
    const int w = emul_range_wgs(nwg, x);
    CHECK(w >= 1, "nids %d nwg %d x %d wgs %d", nids, nwg, x, w);
    wgs += w;
  }
  CHECK(next == nids, "nids %d nwg %d covered %d", nids, nwg, next);
  CHECK(hi - lo <= 1, "nids %d nwg %d lengths %d .. %d", nids, nwg, lo, hi);
  CHECK(wgs == nwg, "nids %d nwg %d workgroups %d", nids, nwg, wgs);
  if (!walk) return;
  std::vector<unsigned char> seen(nids, 0);
  for (int b = 0; b < nwg; ++b) {      // the kernel's walk of workgroup b
    const int x = b & 7, slot = b >> 3, step = emul_range_wgs(nwg, x);
    const EmulRange r = emul_xcd_range(nids, nwg, x);
    for (int id = r.start + slot; id < r.start + r.len; id += step) {
      CHECK(id >= 0 && id < nids, "nids %d nwg %d b %d id %d", nids, nwg, b, id);
      if (id >= 0 && id < nids) ++seen[id];
    }
  }
  int once = 0;
  for (int id = 0; id < nids; ++id) once += seen[id] == 1;
  CHECK(once == nids, "nids %d nwg %d: %d ids visited exactly once", nids, nwg, once);
}

static void check_bitmap(int M, int G, int K) {
  const int tr = (M + LMM_EMUL_TILE - 1) / LMM_EMUL_TILE, nkb = K / 128;
  const size_t bytes = emul_piece_bytes(M, G, K);
  const EmulAux a = emul_aux(M, G, K);
  CHECK(bytes % 4 == 0, "M %d G %d K %d bytes %zu", M, G, K, bytes);
  CHECK(a.masks == 0 && a.pieces == emul_mask_bytes(M, G) && a.pieces % 8 == 0, "M %d G %d K %d pieces at %zu", M, G, K, a.pieces);
  CHECK(a.total % 8 == 0 && a.total >= a.pieces + bytes && a.total < a.pieces + bytes + 8, "M %d G %d K %d total %zu", M, G, K, a.total);
  // first, last and the corners in between: block numbers are dense, so these bound every word
  const int zs[2] = {0, G - 1}, ts[2] = {0, tr - 1}, ks[2] = {0, nkb - 1};
  for (int z : zs) for (int t : ts) for (int k : ks) {
    const size_t b = emul_piece_block(tr, nkb, z, t, k), w = emul_piece_word(b);
    const unsigned s = emul_piece_shift(b);
    CHECK(b < (size_t)G * tr * nkb, "M %d G %d K %d block %zu", M, G, K, b);
    CHECK(4 * w + 4 <= bytes, "M %d G %d K %d word %zu of %zu bytes", M, G, K, w, bytes);
    CHECK((s == 0 || s == 16) && s + LMM_EMUL_PIECES <= 32, "shift %u", s);
  }
  CHECK(emul_piece_block(tr, nkb, G - 1, tr - 1, nkb - 1) + 1 == (size_t)G * tr * nkb, "M %d G %d K %d last block", M, G, K);
}

int main() {
  for (int nids = 1; nids <= 5000; ++nids)
    for (int nwg = 1; nwg <= 300; ++nwg) check_ranges(nids, nwg, nids <= 300 || nids % 97 == 0);
  // every (block) -> (word, shift) pair is its own 16 bits: dense numbering, exhaustively for a small shape
  {
    const int G = 3, tr = 5, nkb = 7;
    std::vector<unsigned> words(emul_piece_bytes(tr * LMM_EMUL_TILE, G, nkb * 128) / 4, 0u);
    for (int z = 0; z < G; ++z) for (int t = 0; t < tr; ++t) for (int k = 0; k < nkb; ++k) {
      const size_t b = emul_piece_block(tr, nkb, z, t, k);
      CHECK(emul_piece_word(b) < words.size(), "block %zu", b);
      if (emul_piece_word(b) >= words.size()) continue;
      unsigned& w = words[emul_piece_word(b)];
      const unsigned field = 0xFFFFu << emul_piece_shift(b);
      CHECK((w & field) == 0u, "block %zu shares bits", b);
      w |= field;
    }
  }
  for (int M = 1; M <= 16448; ++M)
    for (int G : {1, 2, 5, 16, 32})
      for (int K : {128, 256, 640, 8192, 8320, 16384}) check_bitmap(M, G, K);
  printf("%lld checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
