// The cases of the GEMM plan table (tests/golden/gemm_plan.json, tests/test_gemm_plan_cpu.py): shapes x tuning settings.
// No planner is called here: print_gemm_plan_cases sets each tuning, asks the caller for the plan of each case and prints the table.
#pragma once
#include "wm_kernels.h"

#include <stdio.h>
#include <string>
#include <utility>
#include <vector>

struct GemmPlanCase { std::string label; WmGemmArgs a; };
typedef std::vector<std::pair<int, int>> GemmPlanTuning;   // (WM_TUNE_* key, value)

inline std::vector<GemmPlanCase> gemm_plan_cases() {
  std::vector<GemmPlanCase> out;
  void* const ptr = (void*)64;   // a plan reads no memory: any non-null pointer
  auto base = [&](int epi, int dtype, int M, int N, int K) {
    WmGemmArgs a = {};
    a.A = ptr; a.W = ptr; a.C = ptr; a.bias = (const float*)ptr;
    a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N; a.dtype = dtype; a.epi = epi;
    if (epi == WM_EPI_RESID) a.gamma = (const float*)ptr;
    if (epi == WM_EPI_QKV) { a.qkv.H = N / 192; a.qkv.tokens_per_view = 1376; a.qkv.patch_start = 7; a.qkv.grid_w = 37; a.qkv.head_stride = M; }
    return a;
  };
  auto with_ln = [&](WmGemmArgs a) {
    a.ln_out = ptr; a.ln_ld = a.N; a.ln_w = a.ln_b = (const float*)ptr; a.ln_eps = 1e-5f;
    a.ln_stats = (float*)ptr; a.ln_sync = a.ln_fallback = (int*)ptr;
    return a;
  };
  auto add = [&](const std::string& label, const WmGemmArgs& a) { out.push_back({label, a}); };
  const char* dtn[2] = {"bf16", "f16"};
  // the four backbone GEMMs at 1, 2, 8 and 32 views of 518^2, both dtypes; the residual ones also with the LayerNorm pointers set
  for (int v : {1, 2, 8, 32})
    for (int dt = 0; dt < 2; ++dt) {
      const std::string s = " v" + std::to_string(v) + " " + dtn[dt];
      const int M = v * 1376;
      add("qkv" + s, base(WM_EPI_QKV, dt, M, 3072, 1024));
      add("proj" + s, base(WM_EPI_RESID, dt, M, 1024, 1024));
      add("proj+ln" + s, with_ln(base(WM_EPI_RESID, dt, M, 1024, 1024)));
      add("fc1" + s, base(WM_EPI_GELU_T16, dt, M, 4096, 1024));
      add("fc2" + s, base(WM_EPI_RESID, dt, M, 1024, 4096));
      add("fc2+ln" + s, with_ln(base(WM_EPI_RESID, dt, M, 1024, 4096)));
    }
  // the DPT heads' shared tap projection (split_n set), plain ROWMAP_ADD, CONVT
  for (int N : {768, 1536, 3072}) {
    WmGemmArgs a = base(WM_EPI_ROWMAP_ADD, 0, 10952, N, 2048);
    a.rows_per_group = 1369; a.out_group = 1369; a.split_n = 768; a.ldc = 768;
    for (int i = 0; i < N / 768; ++i) a.split_C[i] = ptr;
    add("tap-shared N" + std::to_string(N), a);
  }
  {
    WmGemmArgs a = base(WM_EPI_ROWMAP_ADD, 0, 10952, 768, 2048);
    a.rows_per_group = 1369; a.out_group = 1369;
    add("rowmap-add", a);
    WmGemmArgs c = base(WM_EPI_CONVT, 0, 10952, 4 * 4 * 256, 1024);
    c.ct_k = 4; c.ct_cout = 256; c.ct_gh = 37; c.ct_gw = 37;
    add("convt k4", c);
    c = base(WM_EPI_CONVT, 1, 1369, 2 * 2 * 512, 1024);
    c.ct_k = 2; c.ct_cout = 512; c.ct_gh = 37; c.ct_gw = 37;
    add("convt k2 f16", c);
  }
  // WM_EPI_CONV: the 3x3 form and the token-conv form
  for (int n : {1, 8}) {
    WmGemmArgs a = base(WM_EPI_CONV, 1, n * 74 * 74, 256, 9 * 256);
    a.cv_h = 74; a.cv_w = 74; a.cv_cin = 256; a.cv_zero = ptr;
    add("conv3x3 n" + std::to_string(n), a);
    for (int k : {4, 2}) {
      WmGemmArgs t = base(WM_EPI_CONV, 1, n * 37 * 37, k * k * 256, 4 * 1024);
      t.cv_h = 37; t.cv_w = 37; t.cv_cin = 1024; t.cv_zero = ptr; t.tc_k = k; t.ldc = 256; t.out16 = 1;
      add("tconv k" + std::to_string(k) + " n" + std::to_string(n), t);
    }
    // the tap GEMM of the 148^2 level
    add("tap n" + std::to_string(n), base(WM_EPI_T16, 1, n * 148 * 148, 1152, 256));
    add("tap f32 n" + std::to_string(n), base(WM_EPI_F32, 1, n * 148 * 148, 1152, 256));
  }
  // the shapes of test_gemm_epilogues and test_gemm_row_band_schedule_is_bit_identical, epilogues 0-3; M or N <= 128; a K the launch refuses
  const int shapes[][3] = {{256, 256, 128}, {1000, 384, 640}, {2752, 1024, 1024}, {77, 64, 64}, {1376, 4096, 1024}, {11008, 3072, 256},
                           {1376 * 3 + 5, 512, 256}, {200, 256, 128}, {128, 1024, 1024}, {1376, 128, 1024}, {129, 132, 64}, {256, 256, 96}};
  for (const auto& sh : shapes)
    for (int epi = WM_EPI_F32; epi <= WM_EPI_RESID; ++epi)
      add("op epi" + std::to_string(epi) + " " + std::to_string(sh[0]) + "x" + std::to_string(sh[1]) + "x" + std::to_string(sh[2]), base(epi, epi & 1, sh[0], sh[1], sh[2]));
  return out;
}

inline std::vector<std::pair<std::string, GemmPlanTuning>> gemm_plan_tunings() {
  std::vector<std::pair<std::string, GemmPlanTuning>> t;
  t.push_back({"default", {}});
  for (int v : {0, 2, 3, 4}) t.push_back({"gemm_pp=" + std::to_string(v), {{WM_TUNE_GEMM_PP, v}}});
  for (int v : {0, 2}) t.push_back({"gemm_pp=0,gemm_mfma16=" + std::to_string(v), {{WM_TUNE_GEMM_PP, 0}, {WM_TUNE_GEMM_MFMA16, v}}});
  for (int v = 0; v <= 6; ++v) t.push_back({"gemm_cfg=" + std::to_string(v), {{WM_TUNE_GEMM_CFG, v}}});
  // the schedule: off, forced counts (64 and 3 suit some shapes and not others), a count no shape can take
  for (int v : {0, 64, 3, 100000}) t.push_back({"gemm_sched=" + std::to_string(v), {{WM_TUNE_GEMM_SCHED, v}}});
  t.push_back({"ln_fuse=1", {{WM_TUNE_LN_FUSE, 1}}});
  t.push_back({"ln_fuse=1,gemm_cfg=5", {{WM_TUNE_LN_FUSE, 1}, {WM_TUNE_GEMM_CFG, 5}}});
  t.push_back({"ln_fuse=1,gemm_sched=0", {{WM_TUNE_LN_FUSE, 1}, {WM_TUNE_GEMM_SCHED, 0}}});
  t.push_back({"ln_fuse=1,gemm_pp=4", {{WM_TUNE_LN_FUSE, 1}, {WM_TUNE_GEMM_PP, 4}}});
  t.push_back({"resid_prefetch=1", {{WM_TUNE_RESID_PREFETCH, 1}}});
#ifdef WM_GEMM_PP_DEBUG   // the timing-experiment values of the stamps build (not part of the committed table)
  for (int v : {11, 12, 13, 14, 15, 16, 17, 100, 101, 103, 105, 106, 112, 115, 116}) t.push_back({"gemm_pp=" + std::to_string(v), {{WM_TUNE_GEMM_PP, v}}});
  t.push_back({"gemm_pp=14,gemm_cfg=5", {{WM_TUNE_GEMM_PP, 14}, {WM_TUNE_GEMM_CFG, 5}}});
  t.push_back({"gemm_pp=17,gemm_cfg=5", {{WM_TUNE_GEMM_PP, 17}, {WM_TUNE_GEMM_CFG, 5}}});
  t.push_back({"gemm_pp=12,gemm_cfg=5", {{WM_TUNE_GEMM_PP, 12}, {WM_TUNE_GEMM_CFG, 5}}});
  t.push_back({"gemm_pp=103,gemm_cfg=0", {{WM_TUNE_GEMM_PP, 103}, {WM_TUNE_GEMM_CFG, 0}}});
#endif
  return t;
}

// the plan of one (case, tuning, ncu); family: "NT32" | "NT16" | "PP1" | "PP2", or "-" with err = 1 (the launch is refused)
struct GemmPlanRow { const char* family; int err, cfg, qi, ver, bands; unsigned grid, block; size_t lds; int fuses_ln, pf_c, group_bands; };
inline void print_gemm_plan_header() {   // the tunings by index; the columns of a case line and of a plan inside it
  printf("{\"tunings\": [");
  const auto tunings = gemm_plan_tunings();
  for (const auto& t : tunings) printf("%s\"%s\"", &t == &tunings[0] ? "" : ", ", t.first.c_str());
  printf("],\n\"columns\": %s,\n\"rows\": [", "{\"case\": [\"case\", \"M\", \"N\", \"K\", \"dtype\", \"epi\", \"ncu\", \"plans\"],\n"
         " \"plan\": [\"err\", \"family\", \"cfg\", \"qi\", \"ver\", \"bands\", \"grid\", \"block\", \"lds\", \"fuses_ln\", \"pf_c\", \"group_bands\", \"tunings\"]}");
}

// Every case under every tuning: sets wm_tuning, calls row(args) -> GemmPlanRow, restores the table.  One line per (case, ncu); the
// tunings that give the same plan share one entry of the line (the table has one row per case and tuning: the reader expands it).
template <class F>
void print_gemm_plan_cases(int ncu, bool& first, F&& row) {
  const auto tunings = gemm_plan_tunings();
  for (const auto& c : gemm_plan_cases()) {
    std::vector<std::pair<std::string, std::string>> plans;   // (plan, its tunings)
    for (const auto& t : tunings) {
      for (const auto& kv : t.second) wm_tuning[kv.first] = kv.second;
      const GemmPlanRow r = row(c.a);
      for (const auto& kv : t.second) wm_tuning[kv.first] = -1;
      char buf[256];
      snprintf(buf, sizeof buf, "%d, \"%s\", %d, %d, %d, %d, %u, %u, %zu, %d, %d, %d", r.err, r.family, r.cfg, r.qi, r.ver, r.bands, r.grid, r.block, r.lds, r.fuses_ln,
               r.pf_c, r.group_bands);
      auto it = plans.begin();
      while (it != plans.end() && it->first != buf) ++it;
      const std::string ti = std::to_string(&t - &tunings[0]);   // a tuning is written as its index in the document's "tunings" list
      if (it == plans.end()) plans.push_back({buf, ti});
      else it->second += ", " + ti;
    }
    printf("%s\n[\"%s\", %d, %d, %d, %d, %d, %d, [", first ? "" : ",", c.label.c_str(), c.a.M, c.a.N, c.a.K, c.a.dtype, c.a.epi, ncu);
    for (size_t i = 0; i < plans.size(); ++i) printf("%s[%s, [%s]]", i ? ", " : "", plans[i].first.c_str(), plans[i].second.c_str());
    printf("]]");
    first = false;
  }
}
