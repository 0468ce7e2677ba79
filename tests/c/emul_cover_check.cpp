// Stand-alone host check of emul_amax_cover (csrc/lmm_potrf_plan.h; no HIP, no GPU): for a grid of shapes -- powers of two and widths
// whose halves are uneven -- and switch settings that emulate from K = 128, 256, 2048 or by the shape rule, with and without the
// region kernel as base case, every emulated update's kept ranges plus its scanned range tile its panel's columns [j0, j0 + h)
// exactly, in order; every kept array comes from an EARLIER emulated step whose panel lies inside this one's and whose rows begin at
// or before this update's first row j0 + h (so it holds every row the update needs); with reuse off nothing is covered; and the
// documented chains of C2's levels come out.  tests/test_emul_cover_host.py builds and runs it plainly; meant to be built with the
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/emul_cover_check.cpp -o tests/c/emul_cover_check
#include <cstdio>
#include <cstdlib>
#include "lmm_potrf_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s (NR %d NC %d nb %d step %d)\n", __FILE__, __LINE__, #c, NR, NC, nb, si); } } while (0)

int main() {
  const int shapes[][2] = {{16448, 16384}, {8256, 8192}, {4160, 4096}, {2112, 2048}, {2368, 2304}, {1216, 1152}, {1088, 1024}, {1024, 1024}, {1280, 1216},
                           {1408, 1408}, {704, 640}, {448, 384}, {320, 256}, {192, 192}, {5184, 5120}, {3392, 3328}};
  std::vector<FactorSwitches> settings(6);
  settings[1].emul_on = 1; settings[1].emul_mink = 128; settings[1].region = 0;
  settings[2].emul_on = 1; settings[2].emul_mink = 256;
  settings[3].emul_on = 1; settings[3].emul_mink = 128; settings[3].region_all = LMM_REGION_NEVER;
  settings[4].rule_always = 512; settings[4].rule_shape = 256; settings[4].rule_outs = 2.0e5; settings[4].region = 0;
  settings[5].emul_on = 1; settings[5].emul_mink = 384; settings[5].region = 0;
  long long updates = 0, covered = 0, longest = 0;
  for (const FactorSwitches& sw : settings)
    for (const auto& sh : shapes)
      for (int nb : {1, 5, 16}) {
        const int NR = sh[0], NC = sh[1];
        const PotrfPlan P = plan_potrf(NR, NC, nb, -1, 1, 256, false, false, true, true, sw);
        for (int si = 0; si < (int)P.steps.size(); ++si) {
          const PotrfStep& s = P.steps[si];
          if (s.kind != POTRF_EMUL_UPDATE_LEAF) continue;
          const EmulCover off = emul_amax_cover(P.steps, si, false);
          CHECK(off.n == 0 && off.scan0 == s.j0);
          const EmulCover c = emul_amax_cover(P.steps, si, true);
          CHECK(c.n >= 0 && c.n <= LMM_EMUL_COVER_MAX);
          int at = s.j0;
          for (int q = 0; q < c.n; ++q) {
            CHECK(c.step[q] >= 0 && c.step[q] < si);
            const PotrfStep& e = P.steps[c.step[q]];
            CHECK(e.kind == POTRF_EMUL_UPDATE_LEAF);
            CHECK(e.j0 == at);                                   // the kept ranges follow each other from j0
            CHECK(e.j0 + e.h <= s.j0 + s.h);                     // inside this panel, and its rows begin at or before row j0 + h
            CHECK(e.j0 + e.h + e.M == NR && s.j0 + s.h + s.M == NR);      // both reach the last row
            at += e.h;
          }
          CHECK(at == c.scan0 && c.scan0 <= s.j0 + s.h);         // kept ranges + [scan0, j0 + h) = [j0, j0 + h)
          // nothing usable is left out: no earlier emulated panel begins at scan0 inside this one (unless the list is full)
          if (c.n < LMM_EMUL_COVER_MAX)
            for (int t = 0; t < si; ++t) CHECK(!(P.steps[t].kind == POTRF_EMUL_UPDATE_LEAF && P.steps[t].j0 == c.scan0 && P.steps[t].j0 + P.steps[t].h <= s.j0 + s.h && c.scan0 < s.j0 + s.h));
          ++updates; covered += c.n > 0; longest = std::max<long long>(longest, c.n);
        }
      }
  {   // C2: of the K = 8192 panel only [6144, 8192) is scanned, of each K = 4096 panel the second half, the K = 2048 panels whole
    const int NR = 16448, NC = 16384, nb = 16;
    const PotrfPlan P = plan_potrf(NR, NC, nb, -1, 2, 256, false, false, true, true, FactorSwitches{});
    int seen = 0;
    for (int si = 0; si < (int)P.steps.size(); ++si) {
      const PotrfStep& s = P.steps[si];
      if (s.kind != POTRF_EMUL_UPDATE_LEAF) continue;
      const EmulCover c = emul_amax_cover(P.steps, si, true);
      if (s.h == 8192) { CHECK(c.n == 2 && c.scan0 == 6144); ++seen; }
      if (s.h == 4096) { CHECK(c.n == 1 && c.scan0 == s.j0 + 2048); ++seen; }
      if (s.h == 2048) { CHECK(c.n == 0 && c.scan0 == s.j0); ++seen; }
    }
    const int si = -1;      // (CHECK names a step)
    CHECK(seen == 6);       // one K = 8192, two K = 4096, three K = 2048 updates are emulated
  }
  printf("%lld emulated updates, %lld with kept maxima, longest chain %lld, %d failures\n", updates, covered, longest, failures);
  return failures ? 1 : 0;
}
