// Ping-pong kernel v1 (GemmPlan family PP1, tuning gemm_pp = 3; gemm_pp2.hip is the shipped successor):
// (2 QI 32) x 256 x 64 tile, 8 waves as 2 (M) x 4 (N), wave tile (QI 32) x 64 on 16x16x32 MFMAs.
//
// The lock-step kernels (gemm_nt.hip, gemm_nt16.hip) lose ~half their time to the K-tile rendezvous: all 8 waves wait for the DMA, then all
// read LDS (the matrix pipe idles), then the two waves of a SIMD want the matrix pipe at the same moment.  Here the
// two wave groups (wr = 0 / 1; waves w and w + 4 share a SIMD) run ONE BARRIER APART: a K-tile is four phases (one
// 64 x 32 quadrant of the wave tile x K = 64 each: 16 MFMAs), every phase is {load stage: ds_read the quadrant's
// fragments, issue a share of the next K-tile's LDS-DMA | barrier | MFMA stage | barrier}, and group 1 executes one
// extra barrier before the loop, so on every SIMD one wave is in its MFMA stage (at s_setprio 1) while its partner
// is in its load stage (guides "The 256^2 8-phase template", MI355X_MICROARCH "Two waves per SIMD").
//
// Ordering (all waits are explicit):
//  RAW  the next K-tile's DMA is issued in phases 0-2 and drained by each wave (vmcnt(0)) in its phase-3 load stage,
//       i.e. before a barrier that every reader passes before its first read of that tile;
//  WAR  a wave retires its own ds_reads (lgkmcnt(0)) BEFORE the barrier that ends its load stage, so when any wave
//       starts overwriting the other buffer (phase 0 of the next K-tile, at least one barrier later) nobody is
//       still reading it.
#include "gemm_common.h"

namespace {

template <int T, int EPI, int QI, int PRIO, int DBG = 0>
__global__ __launch_bounds__(512) void gemm_pp_kernel(const WmGemmArgs p) {
  constexpr int SM = 2 * QI, SN = 4;
  constexpr int WROWS = SM * 16, BM = 2 * WROWS, BN = 256;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  constexpr int PA = BM / 8, PB = BN / 8, PPW = (PA + PB) / 8;  // 1-KiB DMA pieces: 8 or 7 per wave per K-tile
  static_assert((PA + PB) % 8 == 0, "pieces must divide over the 8 waves");
  constexpr int D0 = 3, D1 = PPW >= 8 ? 6 : 5;                   // DMA pieces issued in phases 0 / 1 / 2: [0,D0) [D0,D1) [D1,PPW)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + BM - 1) / BM;
  const int lid = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (lid / ntn) * BM, n0 = (lid % ntn) * BN;
  const int l15 = lane & 15, lq = lane >> 4;

  // per-lane global source of each DMA piece of this wave (advanced by 64 elements per K-tile) and its LDS offset
  const u16* gp[PPW];
  int loff[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int pc = wave * PPW + i;  // wave-uniform
    const bool isA = pc < PA;
    const int pl = isA ? pc : pc - PA;
    const int r = pl * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);  // LDS[r][chunk] = G[r][chunk ^ swz(r)]
    int gr = (isA ? m0 : n0) + r;
    const int lim = (isA ? p.M : p.N) - 1;
    gr = gr < lim ? gr : lim;  // clamped rows are masked in the epilogue
    gp[i] = (isA ? (const u16*)p.A + (size_t)gr * p.lda : (const u16*)p.W + (size_t)gr * p.ldw) + c * 8;
    loff[i] = (isA ? 0 : A_BYTES) + pl * 1024;
  }
  auto dma = [&](int buf, int i0, int i1) {
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      __builtin_amdgcn_global_load_lds((glb_vp)gp[i], (lds_vp)(smem + buf * STAGE + loff[i]), 16, 0, 0);
      gp[i] += 64;
    }
  };

  // fragment read offsets: row (base + l15), 16-B chunk 4 kh + lq, swizzle ((row >> 1) & 7) = ((l15 >> 1) & 7)
  const int sw = (l15 >> 1) & 7;
  const int foff0 = l15 * 128 + ((lq ^ sw) << 4), foff1 = l15 * 128 + (((4 + lq) ^ sw) << 4);
  const int a_base = wr * WROWS * 128, b_base = A_BYTES + wc * 64 * 128;

  f32x4 acc[SM][SN];
#pragma unroll
  for (int i = 0; i < SM; ++i)
#pragma unroll
    for (int j = 0; j < SN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  s16x8 a[QI][2], b[2][2];

  const int nk = p.K / 64;
  dma(0, 0, PPW);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // group 1 runs one barrier behind group 0

  for (int t = 0; t < nk; ++t) {
    const char* tile = smem + (t & 1) * STAGE;
    const bool more = t + 1 < nk;
    const int nbuf = (t + 1) & 1;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      const int qm = ph >> 1, qn = (ph == 1 || ph == 2) ? 1 : 0;
      // ---- load stage
      if (ph != 2 && (DBG != 2 || t == 0)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          b[j][0] = *(const s16x8*)(tile + b_base + (qn * 2 + j) * 2048 + foff0);
          b[j][1] = *(const s16x8*)(tile + b_base + (qn * 2 + j) * 2048 + foff1);
        }
      }
      if ((ph == 0 || ph == 2) && (DBG != 2 || t == 0)) {
#pragma unroll
        for (int i = 0; i < QI; ++i) {
          a[i][0] = *(const s16x8*)(tile + a_base + (qm * QI + i) * 2048 + foff0);
          a[i][1] = *(const s16x8*)(tile + a_base + (qm * QI + i) * 2048 + foff1);
        }
      }
      if (more && DBG != 1) {
        if (ph == 0) dma(nbuf, 0, D0);
        if (ph == 1) dma(nbuf, D0, D1);
        if (ph == 2) dma(nbuf, D1, PPW);
      }
      if (ph == 3) wait_vmcnt<0>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (DBG != 3) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- MFMA stage
      if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int i = 0; i < QI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[qm * QI + i][qn * 2 + j] = mfma16<T>(b[j][kh], a[i][kh], acc[qm * QI + i][qn * 2 + j]);
      if (PRIO) __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      if (DBG != 3) __builtin_amdgcn_s_barrier();
    }
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();  // balance group 1's extra barrier
  epilogue16<T, EPI, SM, SN>(p, acc, m0 + wr * WROWS, n0 + wc * 64, lane, p.M);
}

template <int T, int EPI>
hipError_t launch_E(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  return p.qi == 3 ? wm_gemm_launch_kernel<gemm_pp_kernel<T, EPI, 3, 1>>(a, p, s) : wm_gemm_launch_kernel<gemm_pp_kernel<T, EPI, 4, 1>>(a, p, s);
}

#ifdef WM_GEMM_PP_DEBUG  // timing experiments only (results are wrong): DBG 1 no DMA, 2 no ds_read, 3 no barriers
template <int T>
hipError_t launch_dbg(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  return p.dbg == 1 ? wm_gemm_launch_kernel<gemm_pp_kernel<T, WM_EPI_F32, 4, 1, 1>>(a, p, s)
       : p.dbg == 2 ? wm_gemm_launch_kernel<gemm_pp_kernel<T, WM_EPI_F32, 4, 1, 2>>(a, p, s) : wm_gemm_launch_kernel<gemm_pp_kernel<T, WM_EPI_F32, 4, 1, 3>>(a, p, s);
}
#endif

}  // namespace

hipError_t wm_gemm_launch_pp(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
#ifdef WM_GEMM_PP_DEBUG
  if (p.dbg) return a.dtype == WM_T_BF16 ? launch_dbg<WM_T_BF16>(a, p, s) : launch_dbg<WM_T_F16>(a, p, s);
#endif
  switch (a.epi) {
    WM_GEMM_EPI_CASE(WM_EPI_F32) WM_GEMM_EPI_CASE(WM_EPI_T16) WM_GEMM_EPI_CASE(WM_EPI_GELU_T16) WM_GEMM_EPI_CASE(WM_EPI_RESID)
    WM_GEMM_EPI_CASE(WM_EPI_QKV) WM_GEMM_EPI_CASE(WM_EPI_ROWMAP_ADD)
    default: return hipErrorInvalidValue;
  }
}
