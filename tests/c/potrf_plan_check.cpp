// Stand-alone host check of csrc/lmm_potrf_plan.h (no HIP, no GPU): builds the plan of every case of the grid of
// tests/test_potrf_plan_host.py under the switch settings of that test and checks what needs no model of the matrix -- every block
// column is covered once, emulated steps fit the block, and an odd leading dimension takes the 64-column path with no scratch (the
// one input of plan_potrf that lmm_dev_potrf_plan does not pass on).  tests/test_potrf_plan_host.py builds and runs it plainly; meant to be built with the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I linearmixingmodels.jl_amd/csrc tests/c/potrf_plan_check.cpp -o tests/c/potrf_plan_check
#include <cstdio>
#include <cstdlib>
#include "lmm_potrf_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s (NR %d NC %d nb %d)\n", __FILE__, __LINE__, #c, NR, NC, nb); } } while (0)

int main() {
  const int shapes[][2] = {{16448, 16384}, {8256, 8192}, {4160, 4096}, {2112, 2048}, {2368, 2304}, {1216, 1152}, {2304, 2304}, {320, 256}, {1088, 1024}, {1280, 1216}, {192, 192}};
  std::vector<FactorSwitches> settings(8);
  settings[1].panel128 = 0;
  settings[2].fuse_bulk = 0;
  settings[3].region_all = LMM_REGION_EVERYWHERE; settings[3].region = 512;
  settings[4].region_all = LMM_REGION_NEVER;
  settings[5].emul_on = 1; settings[5].emul_mink = 256;
  settings[6].rule_always = 512; settings[6].rule_shape = 256; settings[6].rule_outs = 2.0e5;
  settings[7].emul_on = 0; settings[7].region = 0;
  long long plans = 0, steps = 0;
  for (const FactorSwitches& sw : settings)
    for (const auto& sh : shapes)
      for (int nb : {1, 3, 16, 32})
        for (int in_flight : {1, 2, 4})
          for (int f32 = 0; f32 < 2; ++f32)
            for (int strict = 0; strict < 2; ++strict)
              for (int k = 0; k < 4; ++k) {
                const int allowed = k & 1, ld_odd = k >> 1;
                const int NR = sh[0], NC = sh[1];
                const PotrfPlan P = plan_potrf(NR, NC, nb, NR > NC ? NC + 1 : -1, in_flight, 256, f32 != 0, ld_odd != 0, strict != 0, allowed != 0, sw);
                if (ld_odd) {      // the panel kernels' 16-byte accesses need an even ld: the 64-column path, no region, no scratch, nothing emulated
                  CHECK(!P.panel128 && P.region_cols == 0 && P.w2_doubles == 0 && P.node_flag_ints == 0 && P.asst_doubles == 0 && P.emul_bytes == 0 && P.updates.empty());
                  for (const PotrfStep& s : P.steps) CHECK(s.kind == POTRF_DIAG64 || s.kind == POTRF_SOLVE64 || s.kind == POTRF_UPDATE);
                } else if (!f32 && sw.panel128 && NC >= 128) CHECK(P.panel128 && P.w2_doubles > 0);
                std::vector<int> factored(NC / 64, 0);
                for (const PotrfStep& s : P.steps) {
                  int c0 = -1, w = 0;
                  if (s.kind == POTRF_DIAG64) { c0 = s.j0; w = 64; }
                  if (s.kind == POTRF_LEAF128) { c0 = s.j0; w = 128; }
                  if (s.kind == POTRF_UPDATE_LEAF || s.kind == POTRF_EMUL_UPDATE_LEAF) { c0 = s.j0 + s.h; w = 128; }
                  if (s.kind == POTRF_REGION) { c0 = s.j0 + (s.first_done ? 128 : 0); w = s.N - (s.first_done ? 128 : 0); }
                  for (int c = c0; c >= 0 && c < c0 + w; c += 64) ++factored[c / 64];
                  if (s.kind == POTRF_UPDATE_LEAF || s.kind == POTRF_EMUL_UPDATE_LEAF) CHECK(s.update >= 0 && P.updates[s.update].M == s.M && P.updates[s.update].N == s.N && P.updates[s.update].K == s.h);
                  if (s.kind == POTRF_EMUL_UPDATE_LEAF) CHECK(allowed && s.group >= 1 && s.scratch > 0 && s.scratch <= P.emul_bytes);
                  CHECK(s.M > 0 && s.N > 0 && s.h > 0 && s.j0 + s.h <= NC && s.work > 0.0);
                }
                for (int f : factored) CHECK(f == 1);
                CHECK(allowed || P.emul_bytes == 0);
                ++plans; steps += (long long)P.steps.size();
              }
  printf("%lld plans, %lld steps, %d failures\n", plans, steps, failures);
  return failures ? 1 : 0;
}
