// Stand-alone host check of the live-mask helpers of csrc/lmm_emul.h (no HIP, no GPU): the stage list of a GEMM tile of the int8
// emulation, as the kernel's staging cursor walks it (emul_mask_first / emul_mask_pop) and as its MFMA loop counts it
// (emul_mask_count), against a bit-by-bit reference, for masks with bits in word 0 only, word 1 only, both, none, all and one bit, at
// every depth nk = K / 128 from 1 to 128.  The list must be increasing, stay below nk, have the counted length, hold exactly the bits
// set in both operands, and be block 0 alone when they share none.  tests/test_emul_mask_host.py builds and runs it plainly; meant to
// be built with the sanitizers too:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/emul_mask_check.cpp -o tests/c/emul_mask_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lmm_emul.h"

static int failures = 0;
static long long lists = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s (a %016llx %016llx b %016llx %016llx nk %d)\n", __FILE__, __LINE__, #c, a.w1, a.w0, b.w1, b.w0, nk); } } while (0)

static bool bit(EmulMask m, int k) { return ((k < 64 ? m.w0 >> k : m.w1 >> (k - 64)) & 1ull) != 0; }

static void check(EmulMask a, EmulMask b, int nk) {
  std::vector<int> want;
  for (int k = 0; k < nk; ++k) if (bit(a, k) && bit(b, k)) want.push_back(k);
  if (want.empty()) want.push_back(0);
  EmulMask m = emul_live_stages(a, b, nk);
  const int count = emul_mask_count(m);
  std::vector<int> got;
  while (!emul_mask_empty(m) && got.size() <= 128) { got.push_back(emul_mask_first(m)); m = emul_mask_pop(m); }
  CHECK(count == (int)want.size());
  CHECK(got == want);
  for (size_t i = 0; i < got.size(); ++i) CHECK(got[i] >= 0 && got[i] < nk && (i == 0 || got[i] > got[i - 1]));
  ++lists;
}

int main() {
  const unsigned long long ones = ~0ull;
  std::vector<EmulMask> masks = {{0, 0}, {ones, ones}, {ones, 0}, {0, ones}, {1, 0}, {0, 1}, {1ull << 63, 0}, {0, 1ull << 63}, {1ull << 63, 1},
                                 {0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull}, {0xAAAAAAAAAAAAAAAAull, 0x5555555555555555ull},
                                 {0xF0, 0}, {0, 0x1F}, {0xF000000000000000ull, 0xF}, {0x8000000000000001ull, 0x8000000000000001ull}};
  for (int k = 0; k < 128; ++k) masks.push_back(k < 64 ? EmulMask{1ull << k, 0} : EmulMask{0, 1ull << (k - 64)});      // one bit
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 64; ++i) {      // xorshift words, thinned so that intersections are often small or empty
    unsigned long long w[4];
    for (auto& x : w) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; x = s; }
    masks.push_back(EmulMask{w[0] & w[1], w[2] & w[3]});
  }
  for (const EmulMask& a : masks)
    for (const EmulMask& b : masks)
      for (int nk : {1, 2, 3, 5, 9, 16, 32, 63, 64, 65, 66, 127, 128}) check(a, b, nk);
  for (int nk = 1; nk <= 128; ++nk) { check({ones, ones}, {ones, ones}, nk); check({0, 0}, {ones, ones}, nk); check({0, ones}, {ones, ones}, nk); }
  printf("%lld stage lists, %d failures\n", lists, failures);
  return failures ? 1 : 0;
}
