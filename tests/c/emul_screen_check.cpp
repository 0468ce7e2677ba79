// Stand-alone host check of the screen's index arithmetic in csrc/lmm_emul.h (no HIP, no GPU):
//   the live id list (emul_tile_list, emul_flag_at, emul_live_slot, emul_compact_host -- the arithmetic of emul_compact_kernel): for
//   several trapezoids, group sizes and modulus counts and the flag patterns all dead, all live, alternating, first only, last only,
//   one matrix dead among live ones and pseudo-random, the list is exactly the increasing sequence of the live work ids (item-major,
//   the tile list inside), the count is its length, nothing is written beyond it, and the identity comes out of all-live flags;
//   the layout of the screen's block (emul_screen_layout): flags, counts and list do not overlap and the list holds every id;
//   the GEMM's ranges over a list of `count` entries (emul_xcd_range, emul_range_wgs): for count = 0 .. 5000 and 1 .. 300 workgroups
//   the ranges tile [0, count) and the kernel's walk visits every position exactly once -- count = 0, which the screen makes
//   possible, gives every workgroup an empty walk.
// tests/test_emul_screen_host.py builds and runs it plainly; meant to be built with the sanitizers too:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/emul_screen_check.cpp -o tests/c/emul_screen_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lmm_emul.h"

static int failures = 0;
static long long checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (++failures < 20) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_compaction(int tm, int tn, int gc, int nmod, int pattern) {
  const int ntiles = emul_tile_list(tm, tn, nullptr);
  std::vector<int> xy(2 * (size_t)ntiles);
  CHECK(emul_tile_list(tm, tn, xy.data()) == ntiles, "tm %d tn %d", tm, tn);
  int expect = 0;
  for (int i = 0; i < tm; ++i) expect += i + 1 < tn ? i + 1 : tn;
  CHECK(ntiles == expect, "tm %d tn %d: %d tiles, %d in the trapezoid", tm, tn, ntiles, expect);
  // every tile of the trapezoid once
  std::vector<unsigned char> seen((size_t)tm * tn, 0);
  for (int k = 0; k < ntiles; ++k) {
    const int i = xy[2 * k], j = xy[2 * k + 1];
    CHECK(i >= 0 && i < tm && j >= 0 && j < tn && j <= i, "tile %d = (%d, %d)", k, i, j);
    if (i >= 0 && i < tm && j >= 0 && j < tn) { CHECK(seen[(size_t)i * tn + j] == 0, "tile (%d, %d) twice", i, j); seen[(size_t)i * tn + j] = 1; }
  }
  // flags in the screen's layout; the bytes above the diagonal hold a value the compaction must not read as a flag of the list
  std::vector<unsigned char> flags((size_t)gc * tm * tn, 0x77);
  unsigned lcg = 12345u + 977u * pattern + 31u * tm + 7u * tn;
  for (int z = 0; z < gc; ++z)
    for (int k = 0; k < ntiles; ++k) {
      bool on = false;
      switch (pattern) {
        case 0: on = false; break;
        case 1: on = true; break;
        case 2: on = ((z * ntiles + k) & 1) != 0; break;
        case 3: on = z == 0 && k == 0; break;
        case 4: on = z == gc - 1 && k == ntiles - 1; break;
        case 5: on = z != gc / 2; break;
        default: lcg = lcg * 1664525u + 1013904223u; on = (lcg >> 24) % 5 == 0; break;
      }
      const size_t at = emul_flag_at(tm, tn, z, xy[2 * k], xy[2 * k + 1]);
      CHECK(at < flags.size(), "flag (%d, %d, %d) at %zu of %zu", z, xy[2 * k], xy[2 * k + 1], at, flags.size());
      if (at < flags.size()) flags[at] = on ? (unsigned char)(1 + (k & 1) * 200) : 0;      // any non-zero byte is live
    }
  const int nids = gc * nmod * ntiles;
  std::vector<int> want;
  for (int id = 0; id < nids; ++id) {
    const int item = id / ntiles, k = id - item * ntiles, z = item / nmod;
    if (flags[emul_flag_at(tm, tn, z, xy[2 * k], xy[2 * k + 1])] != 0) want.push_back(id);
  }
  std::vector<int> list((size_t)nids + 1, -7);
  const int count = emul_compact_host(flags.data(), xy.data(), ntiles, tm, tn, gc, nmod, list.data());
  CHECK(count == (int)want.size(), "tm %d tn %d gc %d nmod %d pattern %d: count %d, %zu live ids", tm, tn, gc, nmod, pattern, count, want.size());
  if (count == (int)want.size()) {
    int same = 0;
    for (int q = 0; q < count; ++q) same += list[q] == want[q];
    CHECK(same == count, "tm %d tn %d gc %d nmod %d pattern %d: %d of %d entries in place", tm, tn, gc, nmod, pattern, same, count);
  }
  for (size_t q = (size_t)(count < 0 ? 0 : count); q < list.size(); ++q) CHECK(list[q] == -7, "entry %zu written beyond the count %d", q, count);
  if (pattern == 1) {
    CHECK(count == nids, "all live: %d of %d", count, nids);
    for (int q = 0; q < count && q < nids; ++q) CHECK(list[q] == q, "all live: entry %d = %d", q, list[q]);
  }
  if (pattern == 0) CHECK(count == 0, "all dead: %d", count);
  const EmulScreen S = emul_screen_layout(tm * LMM_EMUL_TILE - 3, tn * LMM_EMUL_TILE - 200, gc, nmod);
  CHECK(S.ntiles == ntiles, "layout: %d tiles, %d", S.ntiles, ntiles);
  CHECK(S.flags == 0 && S.count >= flags.size() && S.count % 8 == 0 && S.list >= S.count + 8 && S.list % 4 == 0, "layout: flags %zu count %zu list %zu", S.flags, S.count, S.list);
  CHECK(S.total >= S.list + 4 * (size_t)nids && S.total % 8 == 0, "layout: total %zu for %d ids from %zu", S.total, nids, S.list);
}

static void check_ranges(int count, int nwg) {
  const int parts = emul_range_parts(nwg);
  int next = 0;
  for (int x = 0; x < parts; ++x) {
    const EmulRange r = emul_xcd_range(count, nwg, x);
    CHECK(r.start == next && r.len >= 0, "count %d nwg %d x %d start %d len %d next %d", count, nwg, x, r.start, r.len, next);
    next = r.start + r.len;
  }
  CHECK(next == count, "count %d nwg %d covered %d", count, nwg, next);
  if (count > 300 && count % 89 != 0) return;
  std::vector<unsigned char> seen((size_t)count + 1, 0);
  for (int b = 0; b < nwg; ++b) {      // the kernel's walk of workgroup b: cnt positions from first with stride step
    const int x = b & 7, slot = b >> 3, step = emul_range_wgs(nwg, x);
    const EmulRange r = emul_xcd_range(count, nwg, x);
    const int first = r.start + slot, span = r.len - slot, cnt = span > 0 ? (span + step - 1) / step : 0;
    if (count == 0) CHECK(cnt == 0, "nwg %d b %d walks %d positions of an empty list", nwg, b, cnt);
    for (int n = 0; n < cnt; ++n) {
      const int pos = first + n * step;
      CHECK(pos >= 0 && pos < count, "count %d nwg %d b %d position %d", count, nwg, b, pos);
      if (pos >= 0 && pos < count) ++seen[pos];
    }
  }
  int once = 0;
  for (int q = 0; q < count; ++q) once += seen[q] == 1;
  CHECK(once == count, "count %d nwg %d: %d positions visited exactly once", count, nwg, once);
}

int main() {
  const int shapes[][2] = {{1, 1}, {2, 1}, {3, 3}, {4, 2}, {4, 3}, {9, 4}, {9, 5}, {17, 9}, {34, 33}, {57, 8}};
  for (const auto& s : shapes)
    for (int gc : {1, 2, 3, 5})
      for (int nmod : {8, 13, 16})
        for (int pattern = 0; pattern < 9; ++pattern) check_compaction(s[0], s[1], gc, nmod, pattern);
  for (int count = 0; count <= 5000; ++count)
    for (int nwg = 1; nwg <= 300; ++nwg) check_ranges(count, nwg);
  printf("%lld checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
