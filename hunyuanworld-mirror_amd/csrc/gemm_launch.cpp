// wm_launch_gemm and its two companions: validate, plan once (gemm_plan.cpp), hand the arguments and the plan to the family's launcher.
#include "gemm_launch.h"

static int wm_ncu() {   // the one place that asks the device
  static const int ncu = [] { hipDeviceProp_t pr; int d = 0; (void)hipGetDevice(&d); return hipGetDeviceProperties(&pr, d) == hipSuccess ? pr.multiProcessorCount : 256; }();
  return ncu;
}

bool wm_gemm_fuses_ln(const WmGemmArgs& a) { return wm_gemm_plan(a, wm_ncu()).fuses_ln; }

// the arguments as the kernels read them: the plan's schedule, the reciprocals of the QKV epilogue
static WmGemmArgs planned_args(const WmGemmArgs& a, const GemmPlan& p) {
  WmGemmArgs b = a;
  b.group_bands = p.group_bands;
  b.sched_bands = p.bands; b.sched_units = (a.M + 15) / 16;
  b.pf_c = p.pf_c;
  if (!p.fuses_ln) b.ln_out = nullptr;   // the kernel takes the fused epilogue iff ln_out is set
  if (a.epi == WM_EPI_QKV) {
    b.qkv.inv_tpv = 1.0f / (float)a.qkv.tokens_per_view;
    b.qkv.inv_gw = 1.0f / (float)a.qkv.grid_w;
  }
  return b;
}

hipError_t wm_launch_gemm_ln_fallback(const WmGemmArgs& a, hipStream_t s) {
  const GemmPlan p = wm_gemm_plan(a, wm_ncu());
  return p.fuses_ln ? wm_gemm_launch_ln_fallback(planned_args(a, p), p, s) : hipSuccess;
}

hipError_t wm_launch_gemm(const WmGemmArgs& a, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  if (wm_gemm_validate(a) != hipSuccess) return hipErrorInvalidValue;
  const GemmPlan p = wm_gemm_plan(a, wm_ncu());
  if (p.err != hipSuccess) return p.err;
  const WmGemmArgs b = planned_args(a, p);
  switch (p.family) {
    case WM_GEMM_NT32: return wm_gemm_launch_nt(b, p, s);
    case WM_GEMM_NT16: return wm_gemm_launch_nt16(b, p, s);
    case WM_GEMM_PP1: return wm_gemm_launch_pp(b, p, s);
    default: return wm_gemm_launch_pp2(b, p, s);
  }
}
