// Stand-alone host check of the scratch list, the per-step wiring and the extent invariants that plan_potrf's finishing pass puts into
// a plan (csrc/lmm_potrf_plan.h; no HIP, no GPU).  Everything is recomputed here from the step list alone, with the formulas the
// executor used while it still sized its scratch itself (in doubles, as it asked the allocator for them), and compared with the plan:
// over the grid of tests/c/potrf_plan_check.cpp, the EMUL_SHAPES of tests/test_potrf_plan_host.py and the factor shapes of the C2 and
// C3 workloads (bench.py WORKLOADS: n = 16384 in 16-latent batches, two in flight; n = 8192 in 8-latent batches, four in flight; one
// 64-row block of riders each), for nb in {1, 3, 4, 16, 32}, under the default switches, emulation from K = 256, the f64 screen from
// K = 256 with and without its vote, kept maxima not reused, and zero extents present or absent.  Then batch_plan's per-stream term,
// and for each of the seven invariants one plan that violates exactly that one.  tests/test_potrf_plan_host.py builds and runs it
// plainly; meant to be built with the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/potrf_scratch_check.cpp -o tests/c/potrf_scratch_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "lmm_potrf_plan.h"

static int failures = 0;
static int NR, NC, nb, si;      // what CHECK names
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s (NR %d NC %d nb %d step %d)\n", __FILE__, __LINE__, #c, NR, NC, nb, si); } } while (0)

static bool same_cover(const EmulCover& a, const EmulCover& b) { return a.n == b.n && a.scan0 == b.scan0 && memcmp(a.step, b.step, sizeof(a.step)) == 0; }

// One plan against the executor's former arithmetic
static void check_plan(const PotrfPlan& P, const FactorSwitches& sw, bool f32, bool zext, bool counters) {
  const size_t n = P.steps.size();
  size_t scr_bytes = 0, emul_screen_bytes = 0;
  int scr_vote = -1, kmax = 128, emul_ncb = 0, kept = 0;
  for (size_t i = 0; i < n; ++i) {
    const PotrfStep& s = P.steps[i];
    if (s.kind == POTRF_EMUL_UPDATE_LEAF || (s.kind == POTRF_UPDATE_LEAF && s.screened)) ++kept;
    if (s.kind == POTRF_UPDATE_LEAF && s.screened) {
      const int rows = s.strip != POTRF_STRIP_NONE ? s.M - 64 : s.M, MT = (rows + 127) / 128, NT = (s.N + 127) / 128;
      scr_bytes = std::max(scr_bytes, ((size_t)nb * MT * NT + 7) & ~size_t(7));
      if (scr_vote < 0 && NT >= 4) scr_vote = (int)i;
    }
    if (s.kind == POTRF_EMUL_UPDATE_LEAF) {
      kmax = std::max(kmax, s.h); emul_ncb = std::max(emul_ncb, (s.j0 + s.h) / 128);
      emul_screen_bytes = std::max(emul_screen_bytes, emul_screen_layout(s.M, s.N, std::min(s.group, nb), P.emul_nmod).total);
    }
  }
  si = -1;
  // the arrays, in the doubles the executor asked for
  CHECK(P.amax_arrays == kept && P.amax_bytes % 8 == 0 && P.amax_bytes / 8 == (size_t)nb * NR);
  CHECK(P.f64_flag_bytes == scr_bytes && scr_bytes % 8 == 0);
  CHECK(P.f64_stat_bytes % 8 == 0 && P.f64_stat_bytes / 8 == (scr_bytes > 0 ? n : 0));              // two ints per step
  CHECK(P.vote_step == scr_vote);
  if (P.emul_bytes > 0) {
    CHECK(P.emul_kmax == kmax && P.emul_aux_bytes % 8 == 0 && P.emul_aux_bytes / 8 == emul_aux(NR, nb, kmax).total / 8);
    CHECK(P.emul_screen_bytes % 8 == 0 && P.emul_screen_bytes / 8 == emul_screen_bytes / 8);
    CHECK(P.emul_ncb == emul_ncb && P.emul_bmax_bytes == (size_t)nb * emul_ncb * NR * 8 && emul_ncb <= NC / 128);
  } else CHECK(P.emul_kmax == 0 && P.emul_ncb == 0 && P.emul_aux_bytes == 0 && P.emul_screen_bytes == 0 && P.emul_bmax_bytes == 0 && emul_ncb == 0);
  const bool takes = zext && !f32 && sw.zero_extents;
  CHECK(P.zext == takes && P.zext_bytes % 8 == 0 && P.zext_bytes / 8 == (takes ? ((size_t)(NR / 64 + 4) * nb + 1) / 2 : 0));
  CHECK(P.zext_stat_bytes % 8 == 0 && P.zext_stat_bytes / 8 == (takes && counters ? (n + 1) / 2 : 0));       // one int per step
  // the steps' wiring
  for (si = 0; si < (int)n; ++si) {
    const PotrfStep& s = P.steps[si];
    const bool screened = s.kind == POTRF_UPDATE_LEAF && s.screened, emulated = s.kind == POTRF_EMUL_UPDATE_LEAF;
    CHECK(s.keeps_amax == (screened || emulated));
    // an emulated step's cover never takes from f64 steps' arrays, a screened f64 step's does
    if (screened || emulated) CHECK(same_cover(s.cover, emul_amax_cover(P.steps, si, sw.emul_amax_reuse != 0, screened)));
    else CHECK(s.cover.n == 0);
    if (!sw.emul_amax_reuse && (screened || emulated)) CHECK(s.cover.n == 0 && s.cover.scan0 == s.j0);
    for (int q = 0; q < s.cover.n; ++q) CHECK(s.cover.step[q] < si && P.steps[s.cover.step[q]].keeps_amax);
    if (screened) {
      const int rows = s.strip != POTRF_STRIP_NONE ? s.M - 64 : s.M, MT = (rows + 127) / 128, NT = (s.N + 127) / 128;
      CHECK(s.flag_bytes == (((size_t)nb * MT * NT + 7) & ~size_t(7)));
      CHECK(s.vote_from == ((sw.f64_screen_vote && scr_vote >= 0 && si > scr_vote) ? scr_vote : -1));
    } else CHECK(s.flag_bytes == 0 && s.vote_from == -1);
    if (emulated) CHECK(s.screen_bytes == emul_screen_layout(s.M, s.N, std::min(s.group, nb), P.emul_nmod).total && s.screen_bytes % 8 == 0);
    else CHECK(s.screen_bytes == 0);
  }
  si = -1;
  const PotrfViolation v = plan_potrf_check(P, NR);
  CHECK(!v && v.which == POTRF_INV_NONE && v.step == -1);
}

// A copy of `base` with one field edited violates `which` at step `at`, and the check says so
template <class F>
static void must_fail(const PotrfPlan& base, int which, int at, F edit) {
  PotrfPlan P = base;
  edit(P, P.steps[at]);
  const PotrfViolation v = plan_potrf_check(P, NR);
  si = at;
  CHECK(v && v.which == which && v.step == at);
  CHECK(potrf_invariant_text(v.which)[0] != 0);
  if (!(v && v.which == which && v.step == at)) fprintf(stderr, "  wanted invariant %d at step %d, got %d at step %d (%lld against %lld)\n", which, at, v.which, v.step, v.needs, v.has);
}

int main() {
  const int shapes[][2] = {{16448, 16384}, {8256, 8192}, {4160, 4096}, {2112, 2048}, {2368, 2304}, {1216, 1152}, {2304, 2304}, {320, 256}, {1088, 1024}, {1280, 1216}, {192, 192}};
  std::vector<FactorSwitches> settings(8);
  settings[1].emul_on = 1; settings[1].emul_mink = 256;
  settings[2].f64_screen = 1; settings[2].f64_screen_mink = 256; settings[2].f64_screen_rounds = 0; settings[2].f64_screen_vote = 1;
  settings[3] = settings[2]; settings[3].f64_screen_vote = 0;
  settings[4].emul_amax_reuse = 0;
  settings[5] = settings[1]; settings[5].emul_amax_reuse = 0;
  settings[6] = settings[2]; settings[6].emul_amax_reuse = 0;
  settings[7] = settings[2]; settings[7].zero_extents = 0;
  long long plans = 0, kept = 0, screened = 0, listeners = 0, emulated = 0;
  auto run = [&](const FactorSwitches& sw, int in_flight, bool f32, bool allowed, bool zext, bool counters) {
    const PotrfPlan P = plan_potrf(NR, NC, nb, NR > NC ? NC + 1 : -1, in_flight, 256, f32, false, true, allowed, sw, zext, counters);
    check_plan(P, sw, f32, zext, counters);
    ++plans; kept += P.amax_arrays;
    for (const PotrfStep& s : P.steps) { screened += s.flag_bytes > 0; listeners += s.vote_from >= 0; emulated += s.screen_bytes > 0; }
  };
  for (const FactorSwitches& sw : settings) {
    for (const auto& sh : shapes)
      for (int b : {1, 3, 4, 16, 32})
        for (int in_flight : {1, 2})
          for (int k = 0; k < 16; ++k) {
            NR = sh[0]; NC = sh[1]; nb = b;
            run(sw, in_flight, (k & 1) != 0, (k & 2) != 0, (k & 4) != 0, (k & 8) != 0);
          }
    // C2 and C3 as the benchmark runs them
    for (int k = 0; k < 4; ++k) {
      NR = 16448; NC = 16384; nb = 16; run(sw, 2, false, true, (k & 1) != 0, (k & 2) != 0);
      NR = 8256; NC = 8192; nb = 8; run(sw, 4, false, true, (k & 1) != 0, (k & 2) != 0);
    }
  }
  si = -1;
  CHECK(screened > 0 && listeners > 0 && emulated > 0);      // the grid reaches every kind of wiring

  // batch_plan's per-stream term: the emulation block at its cap + block maxima for all n / 128 column blocks of the square working
  // set of bytes_per_latent = 8 n^2 (with one 64-row block of riders), when the plan at that batch size emulates anything
  for (const FactorSwitches& sw : {settings[0], settings[1]})
    for (int n : {4096, 8192, 16384, 32768})
      for (int b : {1, 4, 16}) {
        NR = n + 64; NC = n; nb = b;
        const PotrfPlan P = plan_potrf_emul_view(NR, NC, nb, sw);
        const double want = P.emul_bytes > 0 ? 12e9 + (double)((size_t)nb * (NC / 128) * NR * 8) : 0.0;
        CHECK(emul_stream_budget(P, NR, NC, nb) == want);
        CHECK(n < 8192 || P.emul_bytes > 0);                 // K >= 4096 is always emulated: the term is not vacuous
        CHECK((double)P.emul_bytes <= 12e9 || P.emul_G == 1); // ... and the cap is the one the block was cut to
        CHECK((double)P.emul_bmax_bytes <= want);
      }

  {   // The check can fail: C2's plan has screened f64 steps and emulated ones
    NR = 16448; NC = 16384; nb = 16;
    const PotrfPlan P = plan_potrf(NR, NC, nb, NC + 1, 2, 256, false, false, true, true, FactorSwitches{}, true, false);
    int scr = -1, emu = -1, emu_last = -1;
    for (int i = 0; i < (int)P.steps.size(); ++i) {
      const PotrfStep& s = P.steps[i];
      if (scr < 0 && s.kind == POTRF_UPDATE_LEAF && s.screened) scr = i;
      if (emu < 0 && s.kind == POTRF_EMUL_UPDATE_LEAF) emu = i;
      if (s.kind == POTRF_EMUL_UPDATE_LEAF && (emu_last < 0 || s.j0 + s.h > P.steps[emu_last].j0 + P.steps[emu_last].h)) emu_last = i;
    }
    si = -1;
    CHECK(scr >= 0 && emu >= 0 && emu_last >= 0);
    if (scr >= 0 && emu >= 0 && emu_last >= 0) {
      must_fail(P, POTRF_INV_FLAG_BYTES, scr, [](PotrfPlan& Q, PotrfStep& s) { s.flag_bytes = Q.f64_flag_bytes + 8; });
      must_fail(P, POTRF_INV_ROWS, scr, [](PotrfPlan&, PotrfStep& s) { s.M += 128; });
      must_fail(P, POTRF_INV_ROWS, emu, [](PotrfPlan&, PotrfStep& s) { s.M += 256; });
      must_fail(P, POTRF_INV_SCREEN_COLS, scr, [](PotrfPlan&, PotrfStep& s) { s.N = f64_screen_rows(s.M, s.strip) + 128; });
      must_fail(P, POTRF_INV_EMUL_SCRATCH, emu, [](PotrfPlan& Q, PotrfStep& s) { s.scratch = Q.emul_bytes + 1; });
      must_fail(P, POTRF_INV_EMUL_SCREEN, emu, [](PotrfPlan& Q, PotrfStep& s) { s.screen_bytes = Q.emul_screen_bytes + 8; });
      must_fail(P, POTRF_INV_PANEL_BLOCKS, emu, [](PotrfPlan&, PotrfStep& s) { s.cover.scan0 += 64; });
      must_fail(P, POTRF_INV_PANEL_BLOCKS, emu, [](PotrfPlan&, PotrfStep& s) { s.h += 64; s.M -= 64; });      // the same last row, the same last block
      must_fail(P, POTRF_INV_PANEL_BLOCKS, emu, [](PotrfPlan&, PotrfStep& s) { s.j0 += 64; s.h -= 64; s.cover.scan0 += 64; });
      must_fail(P, POTRF_INV_BMAX_BLOCKS, emu_last, [](PotrfPlan& Q, PotrfStep& s) { Q.emul_ncb = (s.j0 + s.h) / 128 - 1; });
    }
  }
  printf("%lld plans, %lld kept arrays, %lld screened steps (%lld listen to a vote), %lld emulated steps, %d failures\n", plans, kept, screened, listeners, emulated, failures);
  return failures ? 1 : 0;
}
