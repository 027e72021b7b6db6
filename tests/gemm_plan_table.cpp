// Prints the GEMM plan table (one JSON document) from wm_gemm_plan called directly: tests/test_gemm_plan_cpu.py builds this program
// from csrc/gemm_plan.cpp and csrc/wm_tuning.cpp alone, so nothing here may need the HIP runtime or the rest of the library.
#include "gemm_plan_cases.h"
#include "gemm_launch.h"

int main() {
  static const char* const fam[] = {"NT32", "NT16", "PP1", "PP2"};
  print_gemm_plan_header();
  bool first = true;
  for (int ncu : {256, 64})
    print_gemm_plan_cases(ncu, first, [&](const WmGemmArgs& a) {
      const GemmPlan p = wm_gemm_plan(a, ncu);
      if (wm_gemm_validate(a) != hipSuccess || p.err != hipSuccess) return GemmPlanRow{"-", 1};
      return GemmPlanRow{fam[p.family], 0, p.cfg, p.qi, p.ver, p.bands, p.grid, p.block, p.lds, p.fuses_ln ? 1 : 0, p.pf_c, p.group_bands};
    });
  printf("\n]}\n");
  return 0;
}
