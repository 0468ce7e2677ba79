// Stand-alone host check of the f64 update launches' screen (csrc/lmm_potrf_plan.h; no HIP, no GPU):
//   1. the flag bytes: over a grid of launch shapes, with and without a ragged last 64 rows, the rest tiles (1 <= tj <= ti < MT) of
//      every matrix get distinct bytes inside f64_screen_flag_bytes, as many as f64_screen_rest_tiles counts, and the node launch's
//      own tile count (rows without the strip) is the MT the index uses;
//   2. which steps the plan marks: f64 update + leaf steps with K >= min_k and more than one tile column -- and, while no explicit
//      threshold switches the size rule off, more work items than one round of the device -- nothing else, nothing when the switch is off;
//   3. emul_amax_cover over step lists that mix emulated and screened f64 steps: with f64_too every kept range comes from an EARLIER
//      scanning step (emulated, or f64 and screened) whose panel lies inside this one's and begins where the previous range ended;
//      kept ranges + the scanned range tile the panel; nothing usable is left out; without f64_too no f64 step is ever taken and
//      the chains are the emulation's own; with reuse off nothing is covered; and C2's chains come out as documented.
// tests/test_f64_screen_rule_host.py builds and runs it plainly; meant to be built with the sanitizers as well:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/f64_screen_check.cpp -o tests/c/f64_screen_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lmm_potrf_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s (NR %d NC %d nb %d step %d)\n", __FILE__, __LINE__, #c, NR, NC, nb, si); } } while (0)

static void check_flags() {
  const int NR = 0, NC = 0, si = -1;
  long long shapes = 0;
  for (int M : {256, 320, 704, 512, 1088, 2112, 7232})
    for (int N : {192, 256, 384, 512, 1024, 2048})
      for (int strip : {POTRF_STRIP_NONE, POTRF_STRIP_IN_LAUNCH, POTRF_STRIP_SEPARATE})
        for (int nb : {1, 3, 16}) {
          const int Mn = f64_screen_rows(M, strip);
          if (N > Mn || (strip != POTRF_STRIP_NONE && (M % 128) != 64)) continue;
          CHECK(Mn == (strip == POTRF_STRIP_NONE ? M : M - 64));
          const int MT = (Mn + 127) / 128, NT = (N + 127) / 128;
          const size_t bytes = f64_screen_flag_bytes(M, N, strip, nb);
          CHECK(bytes % 8 == 0 && bytes >= (size_t)nb * MT * NT && bytes < (size_t)nb * MT * NT + 8);
          std::vector<unsigned char> hit(bytes, 0);
          long long rest = 0;
          for (int z = 0; z < nb; ++z)
            for (int tj = 1; tj < NT; ++tj)
              for (int ti = tj; ti < MT; ++ti) {
                const size_t at = f64_screen_flag_at(MT, NT, z, ti, tj);
                CHECK(at < bytes);
                if (at < bytes) { CHECK(hit[at] == 0); hit[at] = 1; }
                ++rest;
              }
          CHECK(rest == (long long)nb * f64_screen_rest_tiles(MT, NT));
          for (int z = 0; z < nb; ++z)      // column 0 is never among them
            for (int ti = 0; ti < MT; ++ti) CHECK(hit[f64_screen_flag_at(MT, NT, z, ti, 0)] == 0);
          ++shapes;
        }
  printf("%lld flag layouts\n", shapes);
}

int main() {
  check_flags();
  const int shapes[][2] = {{16448, 16384}, {8256, 8192}, {4160, 4096}, {2112, 2048}, {2368, 2304}, {1216, 1152}, {1152, 1152}, {1088, 1024}, {1280, 1216},
                           {1408, 1408}, {704, 640}, {448, 384}, {320, 256}, {192, 192}, {5184, 5120}, {3392, 3328}};
  std::vector<FactorSwitches> settings(7);
  for (int q : {1, 2, 3, 6}) settings[q].f64_screen_rounds = 0;      // an explicit threshold: no size rule
  settings[1].region = 0; settings[1].f64_screen_mink = 128; settings[1].emul_on = 0;                 // f64 scanning steps only
  settings[2].region = 0; settings[2].f64_screen_mink = 128; settings[2].emul_on = 1; settings[2].emul_mink = 512;      // f64 below, emulated above
  settings[3].region_all = LMM_REGION_NEVER; settings[3].f64_screen_mink = 256; settings[3].emul_on = 1; settings[3].emul_mink = 1024;
  settings[4].f64_screen = 0;
  settings[5].f64_screen_mink = 1024;
  settings[6].region = 0; settings[6].f64_screen_mink = 256; settings[6].rule_always = 2048; settings[6].rule_shape = 512; settings[6].rule_outs = 2.0e5;
  long long updates = 0, covered = 0, longest = 0, from_f64 = 0, marked = 0;
  for (const FactorSwitches& sw : settings)
    for (const auto& sh : shapes)
      for (int nb : {1, 5, 16}) {
        const int NR = sh[0], NC = sh[1];
        const PotrfPlan P = plan_potrf(NR, NC, nb, -1, 1, 256, false, false, true, true, sw);
        for (int si = 0; si < (int)P.steps.size(); ++si) {
          const PotrfStep& s = P.steps[si];
          // 2. the marks
          bool want = s.kind == POTRF_UPDATE_LEAF && sw.f64_screen != 0 && s.h >= sw.f64_screen_mink && s.N > 128 && (s.h % 128) == 0;
          if (want && sw.f64_screen_rounds > 0) {      // the size rule: more work items than `rounds` rounds of two workgroups on each of the 256 CUs
            const int MT = (f64_screen_rows(s.M, s.strip) + 127) / 128, NT = (s.N + 127) / 128;
            want = (long long)nb * (MT + f64_screen_rest_tiles(MT, NT)) > 512LL * sw.f64_screen_rounds;
            CHECK(want == f64_screen_pays(s.M, s.N, s.strip, nb, 256, sw));
          }
          CHECK(s.screened == want);
          if (s.screened) { CHECK(s.N <= f64_screen_rows(s.M, s.strip) && s.j0 + s.h + s.M == NR && (s.j0 % 128) == 0); ++marked; }
          // 3. the cover
          if (!emul_step_scans(s, true)) continue;
          const EmulCover off = emul_amax_cover(P.steps, si, false, true);
          CHECK(off.n == 0 && off.scan0 == s.j0);
          for (int f64_too = 0; f64_too < 2; ++f64_too) {
            const EmulCover c = emul_amax_cover(P.steps, si, true, f64_too != 0);
            CHECK(c.n >= 0 && c.n <= LMM_EMUL_COVER_MAX);
            int at = s.j0;
            for (int q = 0; q < c.n; ++q) {
              CHECK(c.step[q] >= 0 && c.step[q] < si);
              const PotrfStep& e = P.steps[c.step[q]];
              CHECK(emul_step_scans(e, f64_too != 0));
              if (!f64_too) CHECK(e.kind == POTRF_EMUL_UPDATE_LEAF);
              CHECK(e.j0 == at);
              CHECK(e.j0 + e.h <= s.j0 + s.h);
              CHECK(e.j0 + e.h + e.M == NR && s.j0 + s.h + s.M == NR);
              if (f64_too && e.kind == POTRF_UPDATE_LEAF) ++from_f64;
              at += e.h;
            }
            CHECK(at == c.scan0 && c.scan0 <= s.j0 + s.h);
            if (c.n < LMM_EMUL_COVER_MAX)
              for (int t = 0; t < si; ++t)
                CHECK(!(emul_step_scans(P.steps[t], f64_too != 0) && P.steps[t].j0 == c.scan0 && P.steps[t].j0 + P.steps[t].h <= s.j0 + s.h && c.scan0 < s.j0 + s.h));
            if (f64_too) { ++updates; covered += c.n > 0; longest = std::max<long long>(longest, c.n); }
          }
          // the default argument is "emulated steps only"
          const EmulCover d = emul_amax_cover(P.steps, si, true), d0 = emul_amax_cover(P.steps, si, true, false);
          CHECK(d.n == d0.n && d.scan0 == d0.scan0);
        }
      }
  {   // C2 (two batches in flight, 512-column region launches): the K = 512 steps scan their panels whole; a K = 1024 step takes the
      // first half of its panel from the K = 512 step before it; the f64 K = 2048 step [12288, 14336) takes 1024 + 512 columns; the
      // emulated K = 8192 step could take 4096 + 2048 + 1024 + 512 columns once f64 steps count
    const int NR = 16448, NC = 16384, nb = 16;
    const PotrfPlan P = plan_potrf(NR, NC, nb, -1, 2, 256, false, false, true, true, FactorSwitches{});
    int seen = 0;
    for (int si = 0; si < (int)P.steps.size(); ++si) {
      const PotrfStep& s = P.steps[si];
      if (!emul_step_scans(s, true)) continue;
      const EmulCover c = emul_amax_cover(P.steps, si, true, true);
      if (s.kind == POTRF_UPDATE_LEAF && s.h == 512) { CHECK(c.n == 0 && c.scan0 == s.j0); ++seen; }
      if (s.kind == POTRF_UPDATE_LEAF && s.h == 1024) { CHECK(c.n == 1 && c.scan0 == s.j0 + 512 && P.steps[c.step[0]].h == 512); ++seen; }
      if (s.kind == POTRF_UPDATE_LEAF && s.h == 2048) { CHECK(s.j0 == 12288 && c.n == 2 && c.scan0 == s.j0 + 1536); ++seen; }
      if (s.kind == POTRF_EMUL_UPDATE_LEAF && s.h == 8192) {
        CHECK(c.n == 4 && c.scan0 == 7680);
        const EmulCover e = emul_amax_cover(P.steps, si, true, false);
        CHECK(e.n == 2 && e.scan0 == 6144);
        ++seen;
      }
    }
    const int si = -1;
    CHECK(seen == 15 + 8 + 1 + 1);      // the last K = 512 update (576 x 512: 224 work items) fits the device in one round and is not screened
  }
  printf("%lld scanning updates, %lld with kept maxima, %lld ranges from f64 steps, longest chain %lld, %lld steps marked, %d failures\n", updates, covered, from_f64,
         longest, marked, failures);
  if (from_f64 == 0 || marked == 0) { fprintf(stderr, "no f64 step was ever marked or taken: the check is vacuous\n"); return 1; }
  return failures ? 1 : 0;
}
