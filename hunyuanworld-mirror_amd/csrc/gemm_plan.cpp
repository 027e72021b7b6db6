// The GEMM's launch plan (gemm_launch.h): argument checks, tile choice, kernel family, row-band schedule and launch geometry of
// wm_launch_gemm, decided once.  Host only: no HIP call, no kernel; the CU count is a parameter.
#include "wm_common.h"
#include "gemm_launch.h"

namespace {

int pick_cfg(const WmGemmArgs& a, int ncu) {
  const int forced = wm_tune(WM_TUNE_GEMM_CFG, -1);   // -1: choose below
  const bool conv = a.epi == WM_EPI_CONV;   // lives in the ping-pong v2 kernel only: tile 4 or 5 whatever the size
  if (forced >= 0 && (!conv || forced == 4 || forced == 5)) return forced;
  if (!conv && (a.M <= 128 || a.N <= 128)) return 0;
  // minimise (rounds over the CUs) x (tile area / relative tile efficiency): tile quantisation is the
  // first-order loss at M = 11008 (e.g. 516 tiles of 256^2 on 256 CUs = 3 rounds)
  struct Cand { int id, bm, bn, per_cu; float eff; };
  // relative tile efficiencies measured with tools/check_gemm_pp.py (rounds 1-2; git history) (cfg 4 = ping-pong v2, cfg 5 = ping-pong v1 at 192 x 256)
  static const Cand cands[] = {{4, 256, 256, 1, 1.00f}, {5, 192, 256, 1, 0.85f}, {1, 256, 128, 1, 0.70f}, {0, 128, 128, 2, 0.58f}};
  int best = 4;
  float best_cost = 1e30f;
  for (const Cand& c : cands) {
    if (conv && c.id != 4 && c.id != 5) continue;
    const long tiles = (long)((a.M + c.bm - 1) / c.bm) * ((a.N + c.bn - 1) / c.bn);
    const long rounds = (tiles + (long)ncu * c.per_cu - 1) / ((long)ncu * c.per_cu);
    const float cost = (float)rounds * c.per_cu * c.bm * c.bn / c.eff;  // co-resident blocks share the CU
    if (cost < best_cost) { best_cost = cost; best = c.id; }
  }
  return best;
}

// Row-band schedule of the ping-pong v2 kernel (see gemm_pp2_kernel): how many row bands B to cut the M rows into, and on
// which tile height (cfg 4 = up to 16 units of 16 rows, cfg 5 = up to 12).  Candidates are the B that fill R = 1, 2, ... whole
// rounds of the CUs (B = floor(R ncu / ntn)) and the fewest bands the tile height allows; cost = rounds x one block's time,
// with the block's time from profiles/r04_gemm_timeline.md (prologue 1.6 us; per 1024 of K the full tile's K loop takes
// 1.5 us per 16-row unit on the 12-unit tile and 1.43 on the 16-unit one, but a unit CUT from a tile gives back only ~0.5 us:
// the loop is bound by its LDS traffic, which does not shrink with the MFMAs; ~0.35 us of epilogue per unit).
// forced_cfg >= 0 keeps the tile height.
void pick_sched(const WmGemmArgs& a, int ncu, int forced_cfg, int& cfg, int& bands) {
  const int U = (a.M + 15) / 16, ntn = (a.N + 255) / 256;
  const float kf = (float)a.K / 1024.0f;
  float best = 1e30f;
  int best_cfg = cfg, best_b = 0;
  for (int c = 4; c <= 5; ++c) {
    if (forced_cfg >= 0 && c != forced_cfg) continue;
    const int full = c == 4 ? 16 : 12;
    const float unit = c == 4 ? 1.43f : 1.5f;
    const int bmin = (U + full - 1) / full;
    for (int k = 0; k < 6; ++k) {
      int B;
      if (k == 0) B = bmin;
      else {
        const long r0 = ((long)bmin * ntn + ncu - 1) / ncu;   // rounds of the fewest-bands candidate
        B = (int)(((r0 + k - 1) * ncu) / ntn);
      }
      if (B < bmin) continue;
      if (B > U) B = U;
      const int smax = (U + B - 1) / B;
      if (U / B < full - 4) continue;   // the kernel drops at most 2 units per wave group
      const long rounds = ((long)B * ntn + ncu - 1) / ncu;
      const float loop = kf * (full * unit - 0.5f * (float)(full - smax));
      const float cost = (float)rounds * (1.6f + loop + 0.35f * (float)smax);
      if (cost < best) { best = cost; best_cfg = c; best_b = B; }
    }
  }
  cfg = best_cfg;
  bands = best_b;
}

// gemm_nt_kernel's tiles by id (gemm_nt.hip): rows, columns, threads, LDS ring stages, K-tile
const struct { int bm, bn, threads, nstage, kt; } nt_tiles[7] = {{128, 128, 256, 2, 64}, {256, 128, 512, 3, 64}, {256, 128, 512, 3, 64}, {256, 256, 512, 2, 64},
                                                                 {256, 256, 512, 2, 64}, {192, 256, 512, 2, 64}, {256, 256, 512, 4, 32}};

}  // namespace

hipError_t wm_gemm_validate(const WmGemmArgs& a) {
  if (a.K <= 0 || a.K % 64 != 0 || a.N % 4 != 0) return hipErrorInvalidValue;
  if ((a.lda & 7) || (a.ldw & 7)) return hipErrorInvalidValue;  // 16-B aligned rows
  if (a.epi == WM_EPI_CONVT && (a.ct_cout & 3)) return hipErrorInvalidValue;
  if (a.epi != WM_EPI_CONVT && a.epi != WM_EPI_QKV && (a.ldc & 3)) return hipErrorInvalidValue;
  if (a.epi == WM_EPI_QKV && (a.N % 64 || a.N != 3 * a.qkv.H * 64)) return hipErrorInvalidValue;
  if (a.epi == WM_EPI_CONV && a.tc_k <= 0 && (a.cv_h <= 0 || a.cv_w <= 0 || a.cv_cin % 64 || a.K != 9 * a.cv_cin || a.M % (a.cv_h * a.cv_w) || !a.cv_zero || (a.N & 7))) return hipErrorInvalidValue;
  if (a.epi == WM_EPI_CONV && a.tc_k > 0 && (a.cv_h <= 0 || a.cv_w <= 0 || a.cv_cin % 64 || a.K != 4 * a.cv_cin || a.M % (a.cv_h * a.cv_w) || !a.cv_zero || a.tc_k > 4 ||
                                             a.N != a.tc_k * a.tc_k * 256 || a.ldc != 256 || a.cv_resid || a.cv_resid2))
    return hipErrorInvalidValue;
  if (a.split_n != 0) {
    if (a.epi != WM_EPI_ROWMAP_ADD || a.split_n < 0 || (a.split_n & 3) || a.N % a.split_n || a.N / a.split_n > 4 || a.accumulate) return hipErrorInvalidValue;
    for (int i = 0; i < a.N / a.split_n; ++i)
      if (!a.split_C[i]) return hipErrorInvalidValue;
  }
  if (a.epi == WM_EPI_QKV && (a.qkv.tokens_per_view <= 0 || a.qkv.grid_w <= 0 || a.M >= (1 << 20) || a.qkv.tokens_per_view >= (1 << 16))) return hipErrorInvalidValue;
  return hipSuccess;
}

GemmPlan wm_gemm_plan(const WmGemmArgs& a, int ncu) {
  GemmPlan p = {};
  p.err = hipSuccess;
  p.cfg = pick_cfg(a, ncu);
  // 16x16x32 MFMA main loop: measured +3..8 % on the N=1024 GEMMs (proj, fc2) and +0..2 % on QKV, neutral/negative
  // on fc1 (tools/bench_gemm.py (rounds 1-2; git history)); gemm_mfma16 = 0 / 2 forces it off / on for every backbone epilogue
  const int mf16 = wm_tune(WM_TUNE_GEMM_MFMA16, 1);
  // gemm_pp tuning: 0 no ping-pong kernel, 3 = v1, 4 = v3, anything else = v2
  const int pp = wm_tune(WM_TUNE_GEMM_PP, 1);
  const bool conv = a.epi == WM_EPI_CONV, big = p.cfg == 4 || p.cfg == 5;   // big: the 256- / 192-row tiles, the only ones of NT16 / PP1 / PP2
  const bool plain = a.epi == WM_EPI_F32 || a.epi == WM_EPI_T16 || a.epi == WM_EPI_GELU_T16, backbone = plain || a.epi == WM_EPI_RESID || a.epi == WM_EPI_QKV;

  // ---- family
#ifdef WM_GEMM_PP_DEBUG  // timing experiments only (results are wrong): 11 no DMA, 12 no ds_read, 13 no barriers (v1); 14 - 17, 100 + mask: v2
  if (const int m = pp - 100; pp > 10 && a.epi == WM_EPI_F32 && a.dtype == WM_T_BF16) {
    p.family = WM_GEMM_PP2;
    p.cfg = p.cfg == 5 && pp != 14 ? 5 : 4;   // (these launches never asked whether the tile id was 4 or 5; 14 always takes the 256-row tile)
    if (pp == 14 || pp == 17) p.dbg = 4;
    else if (pp == 15 || pp == 16) p.dbg = pp - 10;
    else if (m == 1 || m == 2 || m == 4 || m == 8 || m == 3 || m == 7 || m == 15 || m == 5 || m == 12) p.dbg = 16 + m;
    else { p.family = WM_GEMM_PP1; p.cfg = 4; p.dbg = pp == 11 ? 1 : pp == 12 ? 2 : 3; }
  } else
#endif
  if (conv) {
    p.family = WM_GEMM_PP2;   // the ping-pong v2 kernel only, whatever gemm_pp says
    if (!big) p.err = hipErrorInvalidValue;
  } else if (pp && big && (backbone || (a.epi == WM_EPI_ROWMAP_ADD && a.split_n > 0))) {   // (the plain ROWMAP_ADD form keeps gemm_nt_kernel)
    p.family = pp == 3 ? WM_GEMM_PP1 : WM_GEMM_PP2;
  } else if (mf16 && big && (a.epi == WM_EPI_RESID || a.epi == WM_EPI_QKV || (mf16 == 2 && plain))) {
    p.family = WM_GEMM_NT16;
  } else {
    p.family = WM_GEMM_NT32;
    if (a.epi < WM_EPI_F32 || a.epi > WM_EPI_QKV || p.cfg > 6) p.err = hipErrorInvalidValue;
  }
  if (p.family == WM_GEMM_PP2) p.ver = !conv && pp == 4 ? 3 : 2;

  // ---- row-band schedule: ping-pong v2 / v3 launches only
  const bool sched_ok = p.family == WM_GEMM_PP2 && (conv || pp == 1 || pp == 2 || pp == 4);
  const int ts = wm_tune(WM_TUNE_GEMM_SCHED, -1);   // -1 choose, 0 off (full-height tiles), > 0 that many bands
  if (sched_ok && ts != 0) {
    // Measured (profiles/r04_gemm_timeline.md, `sched` rows): at M = 11008 the schedule takes 2.4 - 5.1 % off all four backbone
    // GEMMs (2.7 -> 3.0 and 0.9 -> 1.0 rounds of shorter blocks); at M = 44032 (8 - 11 rounds, where a ragged last round
    // costs at most a tenth) it measured +5 / +4 / +1.6 / -2.3 %.  So: only launches of at most three rounds.
    const long legacy_tiles = (long)((a.M + (p.cfg == 4 ? 255 : 191)) / (p.cfg == 4 ? 256 : 192)) * ((a.N + 255) / 256);
    if (ts > 0) p.bands = ts;
    else if (legacy_tiles <= 3L * ncu && a.M <= 16384) pick_sched(a, ncu, wm_tune(WM_TUNE_GEMM_CFG, -1), p.cfg, p.bands);
    const int U = (a.M + 15) / 16, full = p.cfg == 4 ? 16 : 12;
    if (p.bands > U) p.bands = U;
    // bands taller than the tile, or shorter than the kernel's instantiations go (a wave group drops at most 2 units): full-height grid
    if (p.bands <= 0 || (U + p.bands - 1) / p.bands > full || U / p.bands < full - 4) p.bands = 0;
  }
  if (p.family == WM_GEMM_PP1 || p.family == WM_GEMM_PP2) p.qi = p.cfg == 5 ? 3 : 4;

  // ---- geometry
  const auto& t = nt_tiles[p.cfg <= 6 ? p.cfg : 4];   // (tiles 4 / 5 have one size, two 64-deep stages, in every family)
  const int rows = p.bands > 0 ? p.bands : (a.M + t.bm - 1) / t.bm;
  p.grid = (unsigned)(rows * ((a.N + t.bn - 1) / t.bn));
  p.block = (unsigned)t.threads;
  p.lds = (size_t)t.nstage * (t.bm + t.bn) * t.kt * 2;
  if (p.family == WM_GEMM_PP2 && a.epi == WM_EPI_RESID) p.lds += 2048;   // + the residual prefetch's scratch (8 waves x 256 B)

  p.group_bands = wm_tune(WM_TUNE_GEMM_GROUP, 6);  // row bands per supertile: 6 measured 2-3 % ahead of 4 / 8 at 32 views, equal at 8 (tools/bench_gemm_group.py)
  p.pf_c = a.epi == WM_EPI_RESID && wm_tune(WM_TUNE_RESID_PREFETCH, 0) == 1 ? 1 : 0;
  // The fused-LayerNorm epilogue.  OPT-IN (tuning ln_fuse = 1).  Built and proven in round 4 (tests/test_gpu_ops.py::test_gemm_residual_with_fused_layernorm, zero fallbacks in
  // the forward: tools/ln_fallback_count.py) and measured: per launch -2.5 us (proj) / -0.8 us (fc2) against GEMM + LayerNorm kernel in isolation,
  // and between -0.15 and +0.87 ms on the 8-view forward by box (interleaved: 52.38 / 52.50 fused vs 52.39 / 52.74 on one box, 53.49 vs 52.62 on
  // another): the rendezvous' signal -> poll -> partial loads chain costs what the LayerNorm kernel's second read of a stream that the residual
  // epilogue has just left in the memory-side cache costs.  No gain to ship a second synchronisation structure for: off by default.
  p.fuses_ln = a.ln_out && a.epi == WM_EPI_RESID && a.N == 1024 && a.ln_w && a.ln_b && a.ln_stats && a.ln_sync && a.ln_fallback && a.gamma &&
               wm_tune(WM_TUNE_LN_FUSE, 0) == 1 && !(a.ln_ld & 7) && !(a.ldc & 3) &&
               sched_ok && p.cfg == 5 &&   // the 192-row tile's kernel carries the fused epilogue
               (long)rows * 4 <= ncu;      // every block of the launch resident at once (one per CU): the rendezvous of a band's four blocks cannot wait on an undispatched one
  return p;
}
