// The GEMM's launch plan: which kernel family runs a WmGemmArgs, on which tile, with which grid.  wm_gemm_plan (gemm_plan.cpp) is the
// one place that decides; wm_launch_gemm, wm_gemm_fuses_ln and wm_launch_gemm_ln_fallback (gemm_launch.cpp) read the same plan, and each
// family's launcher (gemm_nt.hip, gemm_nt16.hip, gemm_pp.hip, gemm_pp2.hip) only picks the instantiation the plan names.
#pragma once
#include "wm_kernels.h"

enum GemmFamily {
  WM_GEMM_NT32,   // gemm_nt_kernel: lock-step, 32x32x16 MFMA, every epilogue but WM_EPI_CONV
  WM_GEMM_NT16,   // gemm_nt16_kernel: lock-step, 16x16x32 MFMA, backbone epilogues
  WM_GEMM_PP1,    // gemm_pp_kernel: ping-pong v1
  WM_GEMM_PP2,    // gemm_pp2_kernel: ping-pong v2 / v3, the only home of WM_EPI_CONV and of the fused LayerNorm
};

struct GemmPlan {
  hipError_t err;          // hipErrorInvalidValue: no kernel of the family takes this epilogue / tile id
  int family;              // GemmFamily
  int cfg;                 // tile id 0-6 (gemm_nt.hip lists them); 4 = 256 x 256 and 5 = 192 x 256 are the tiles of the other families
  int qi, ver;             // ping-pong kernels: QI (4 | 3 = tile rows / 64); gemm_pp2_kernel's VER (2 | 3)
#ifdef WM_GEMM_PP_DEBUG
  int dbg;                 // DBG of the timing-experiment instantiations (results are wrong), 0 = none
#endif
  int bands;               // row-band schedule of gemm_pp2_kernel (WmGemmArgs::sched_bands); 0 = full-height grid
  bool fuses_ln;           // the launch takes the fused-LayerNorm epilogue (WmGemmArgs::ln_out)
  int pf_c, group_bands;   // WmGemmArgs::pf_c, ::group_bands
  unsigned grid, block;    // launch geometry; grid = row bands (or row tiles) x column tiles
  size_t lds;              // dynamic LDS bytes
};

// host only, no HIP call.  wm_gemm_validate: the argument checks of wm_launch_gemm.  ncu: the device's CU count (wm_launch_gemm asks for it).
hipError_t wm_gemm_validate(const WmGemmArgs& a);
GemmPlan wm_gemm_plan(const WmGemmArgs& a, int ncu);

// one launcher per family: dtype / epilogue / tile -> instantiation, nothing else
hipError_t wm_gemm_launch_nt(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s);
hipError_t wm_gemm_launch_nt16(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s);
hipError_t wm_gemm_launch_pp(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s);
hipError_t wm_gemm_launch_pp2(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s);
hipError_t wm_gemm_launch_ln_fallback(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s);   // gemm_pp2.hip; a.sched_* filled

// one case of a family launcher's switch over a.epi: dtype x epilogue -> that file's launch_E<T, EPI>
#define WM_GEMM_EPI_CASE(epi_) case epi_: return a.dtype == WM_T_BF16 ? launch_E<WM_T_BF16, epi_>(a, p, s) : launch_E<WM_T_F16, epi_>(a, p, s);

// launch KERNEL with the plan's geometry (its dynamic LDS size is a constant of the instantiation: raised once)
template <auto KERNEL>
hipError_t wm_gemm_launch_kernel(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(p.grid), dim3(p.block), p.lds, s, a);
  return hipGetLastError();
}
