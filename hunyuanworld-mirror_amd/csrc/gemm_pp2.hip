// Ping-pong kernel v2 / v3 (GemmPlan family PP2): the kernel behind every backbone nn.Linear, the shared tap projection and WM_EPI_CONV.
// Order of this file: the fused-LayerNorm epilogue of WM_EPI_RESID and its fallback kernel, the kernel (its design and ordering argument
// stand above it; v1 is gemm_pp.hip), the launcher, the entries of the stamps build.
#include "gemm_common.h"

namespace {

// WM_EPI_RESID + the following LayerNorm (see WmGemmArgs::ln_out).  Numerics: the row statistics are combined from partials
// (64 columns per wave -> 256 per tile -> 1024 per row) with the equal-count form of Chan's update, mean = avg(mean_k),
// M2 = sum(M2_k) + n_k sum((mean_k - mean)^2): as accurate as the two-pass form of layernorm_kernel, not bit-identical to it.
// ln_norm() is the one expression both this epilogue and the fallback kernel apply, with explicit roundings and one fma.
typedef __attribute__((address_space(1))) unsigned long long wm_gu64;
typedef __attribute__((address_space(1))) int wm_gi32;
#define WM_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ float ln_norm(float v, float mean, float rstd, float w, float b) {
  return __builtin_fmaf(__fmul_rn(__fsub_rn(v, mean), rstd), w, b);
}
// (mean, M2) of four equal-count partials; cnt = elements per partial
__device__ __forceinline__ void ln_combine4(const float (&m)[4], const float (&q)[4], float cnt, float& mean, float& M2) {
  mean = __fmul_rn(__fadd_rn(__fadd_rn(m[0], m[1]), __fadd_rn(m[2], m[3])), 0.25f);
  const float d0 = __fsub_rn(m[0], mean), d1 = __fsub_rn(m[1], mean), d2 = __fsub_rn(m[2], mean), d3 = __fsub_rn(m[3], mean);
  const float dd = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fadd_rn(__fmul_rn(d2, d2), __fmul_rn(d3, d3)));
  M2 = __fadd_rn(__fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3])), __fmul_rn(cnt, dd));
}
constexpr int WM_LN_SPIN_LIMIT = 4000;   // polls of ~64 cycles each: ~120 us, far beyond a band's skew when its four blocks are resident

// acc holds this wave's (SM x 16 rows) x 64 columns of acc; on return X (and the tap half) are updated and, unless the rendezvous
// timed out, ln_out holds the normalised rows of this block's 256 columns.
template <int T, int SM>
__device__ __forceinline__ void epilogue_resid_ln(const WmGemmArgs& p, f32x4 (&acc)[SM][4], char* smem, int tid, int lane, int wr, int wc,
                                                  int band, int nt, int rowb, int colb, int rl0, int mlim) {
  const int l15 = lane & 15, lq = lane >> 4;
  float4 bs4[4], gm4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = colb + j * 16 + 4 * lq;
    bs4[j] = p.bias ? *(const float4*)(p.bias + col) : make_float4(0, 0, 0, 0);
    gm4[j] = *(const float4*)(p.gamma + col);
  }
  // ---- A: new values gamma (acc + bias) + X into acc.  The X stores are NOT issued yet: the block's signal has to wait for every store
  // in front of it, so the 8-byte statistics go out first and the bulk stores (phase X below) run while the band's other blocks arrive
  float4 old[2][4];
  auto load_old = [&](int i, float4 (&o)[4]) {
    const int row = rowb + i * 16 + l15;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = row < mlim ? *(const float4*)((const float*)p.C + (size_t)row * p.ldc + colb + j * 16 + 4 * lq) : make_float4(0, 0, 0, 0);
  };
  load_old(0, old[0]);
#pragma unroll
  for (int i = 0; i < SM; ++i) {
    if (rowb + i * 16 >= mlim) break;
    if (i + 1 < SM) load_old(i + 1, old[(i + 1) & 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 o = old[i & 1][j], gm = gm4[j], bs = bs4[j];
      acc[i][j] = f32x4{o.x + gm.x * (acc[i][j][0] + bs.x), o.y + gm.y * (acc[i][j][1] + bs.y), o.z + gm.z * (acc[i][j][2] + bs.z), o.w + gm.w * (acc[i][j][3] + bs.w)};
    }
  }
  // ---- B: per row (mean, M2) over this wave's 64 columns -> LDS [tile row][wc]
  float2* lst = (float2*)smem;     // [256][4] (mean, M2): the K-tile ring is dead
  int* lflag = (int*)(smem + 256 * 4 * 8);
  __syncthreads();                 // every wave is out of the K loop: the ring may be overwritten
#pragma unroll
  for (int i = 0; i < SM; ++i) {
    if (rowb + i * 16 >= mlim) break;   // wave-uniform
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s1 += (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
    s1 += __shfl_xor(s1, 16);
    const float mw = __fmul_rn(xhalf_sum(s1), 1.0f / 64.0f);
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = acc[i][j][e] - mw; s2 = __builtin_fmaf(d, d, s2); }
    s2 += __shfl_xor(s2, 16);
    s2 = xhalf_sum(s2);
    if (lq == 0) lst[(rl0 + i * 16 + l15) * 4 + wc] = make_float2(mw, s2);
  }
  __syncthreads();
  // ---- C: the tile's (mean, M2) per row; the wc == 0 waves publish them (8-byte sc1 stores), then one arrival per block
#pragma unroll
  for (int i = 0; i < SM; ++i) {
    if (rowb + i * 16 >= mlim) break;
    const float4 a0 = *(const float4*)(lst + (rl0 + i * 16 + l15) * 4), a1 = *(const float4*)(lst + (rl0 + i * 16 + l15) * 4 + 2);
    const float m[4] = {a0.x, a0.z, a1.x, a1.z}, q[4] = {a0.y, a0.w, a1.y, a1.w};
    float tmean, tm2;
    ln_combine4(m, q, 64.0f, tmean, tm2);
    const int row = rowb + i * 16 + l15;
    if (wc == 0 && lq == 0 && row < mlim) {
      const unsigned long long bits = ((unsigned long long)__builtin_bit_cast(unsigned, tm2) << 32) | __builtin_bit_cast(unsigned, tmean);
      __hip_atomic_store((wm_gu64*)(p.ln_stats + ((size_t)row * 4 + nt) * 2), bits, WM_RLX_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains before the block signals
  __syncthreads();
  if (tid == 0) __hip_atomic_fetch_add((wm_gi32*)(p.ln_sync + band * 2), 1, WM_RLX_AGENT);
  // ---- X: the residual stream (and the tap half), while the other three blocks of the band arrive
#pragma unroll
  for (int i = 0; i < SM; ++i) {
    if (rowb + i * 16 >= mlim) break;
    const int row = rowb + i * 16 + l15;
    if (row < mlim) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 nv = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        *(float4*)((float*)p.C + (size_t)row * p.ldc + colb + j * 16 + 4 * lq) = nv;
        if (p.C2) *(float4*)(p.C2 + (size_t)row * p.ldc2 + colb + j * 16 + 4 * lq) = nv;
      }
    }
  }
  int ok = 0;
  if (tid == 0) {
    int spins = 0;
    while (true) {
      if (__hip_atomic_load((wm_gi32*)(p.ln_sync + band * 2), WM_RLX_AGENT) >= 4) { ok = 1; break; }
      if (++spins > WM_LN_SPIN_LIMIT) break;
      __builtin_amdgcn_s_sleep(1);
    }
    if (!ok) __hip_atomic_store((wm_gi32*)(p.ln_fallback + band), 1, WM_RLX_AGENT);
    *lflag = ok;
  }
  __syncthreads();
  ok = *lflag;
  // ---- D: the row's statistics from the four tiles' partials (sc1 loads of sc1-stored, drained bytes), normalise, 16-bit stores
  if (ok) {
    float4 w4[4], b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w4[j] = *(const float4*)(p.ln_w + colb + j * 16 + 4 * lq);
      b4[j] = *(const float4*)(p.ln_b + colb + j * 16 + 4 * lq);
    }
#pragma unroll
    for (int i = 0; i < SM; ++i) {
      if (rowb + i * 16 >= mlim) break;
      const int row = rowb + i * 16 + l15;
      const int rr = row < mlim ? row : mlim - 1;
      float m[4], q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long bits = __hip_atomic_load((wm_gu64*)(p.ln_stats + ((size_t)rr * 4 + k) * 2), WM_RLX_AGENT);
        m[k] = __builtin_bit_cast(float, (unsigned)bits); q[k] = __builtin_bit_cast(float, (unsigned)(bits >> 32));
      }
      float mean, M2;
      ln_combine4(m, q, 256.0f, mean, M2);
      const float rstd = 1.0f / sqrtf(__fadd_rn(__fmul_rn(M2, 1.0f / 1024.0f), p.ln_eps));
      uint2 u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float y0 = ln_norm(acc[i][j][0], mean, rstd, w4[j].x, b4[j].x), y1 = ln_norm(acc[i][j][1], mean, rstd, w4[j].y, b4[j].y);
        const float y2 = ln_norm(acc[i][j][2], mean, rstd, w4[j].z, b4[j].z), y3 = ln_norm(acc[i][j][3], mean, rstd, w4[j].w, b4[j].w);
        u[j].x = (uint32_t)f2t<T>(y0) | ((uint32_t)f2t<T>(y1) << 16);
        u[j].y = (uint32_t)f2t<T>(y2) | ((uint32_t)f2t<T>(y3) << 16);
      }
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {   // 16-B stores of 64-B row segments (see the T16 epilogue)
        swap16(u[2 * jp].x, u[2 * jp + 1].x);
        swap16(u[2 * jp].y, u[2 * jp + 1].y);
        const int col = colb + (2 * jp + (lq & 1)) * 16 + 4 * (lq & 2);
        if (row < mlim) *(uint4*)((u16*)p.ln_out + (size_t)row * p.ln_ld + col) = make_uint4(u[2 * jp].x, u[2 * jp].y, u[2 * jp + 1].x, u[2 * jp + 1].y);
      }
    }
  }
  // ---- E: departure; the band's last block to leave re-arms the counters for the next launch
  __syncthreads();
  if (tid == 0) {
    const int d = __hip_atomic_fetch_add((wm_gi32*)(p.ln_sync + band * 2 + 1), 1, WM_RLX_AGENT);
    if (d == 3) {
      __hip_atomic_store((wm_gi32*)(p.ln_sync + band * 2), 0, WM_RLX_AGENT);
      __hip_atomic_store((wm_gi32*)(p.ln_sync + band * 2 + 1), 0, WM_RLX_AGENT);
    }
  }
}

#ifdef WM_GEMM_STAMPS
__device__ int wm_ln_fallback_count;
#endif
// Bands whose rendezvous timed out (ln_fallback set): LayerNorm of their rows from X and the published partials, the epilogue's arithmetic.
template <int T>
__global__ __launch_bounds__(256) void gemm_ln_fallback_kernel(const WmGemmArgs p, int bands, int full_units) {
  const int band = blockIdx.x;
  if (__hip_atomic_load((wm_gi32*)(p.ln_fallback + band), WM_RLX_AGENT) == 0) return;   // block-uniform
  int u0, S;
  if (p.sched_bands > 0) {
    u0 = (int)((long long)band * p.sched_units / bands);
    S = (int)((long long)(band + 1) * p.sched_units / bands) - u0;
  } else {
    u0 = band * full_units; S = full_units;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#ifdef WM_GEMM_STAMPS
  if (threadIdx.x == 0) atomicAdd(&wm_ln_fallback_count, 1);   // diagnostic build: bands recomputed since the last read
#endif
  const int r1 = (u0 + S) * 16 < p.M ? (u0 + S) * 16 : p.M;
  for (int row = u0 * 16 + wave; row < r1; row += 4) {
    float m[4], q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long bits = __hip_atomic_load((wm_gu64*)(p.ln_stats + ((size_t)row * 4 + k) * 2), WM_RLX_AGENT);
      m[k] = __builtin_bit_cast(float, (unsigned)bits); q[k] = __builtin_bit_cast(float, (unsigned)(bits >> 32));
    }
    float mean, M2;
    ln_combine4(m, q, 256.0f, mean, M2);
    const float rstd = 1.0f / sqrtf(__fadd_rn(__fmul_rn(M2, 1.0f / 1024.0f), p.ln_eps));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (i * 64 + lane) * 4;
      const float4 v = *(const float4*)((const float*)p.C + (size_t)row * p.ldc + c);
      const float4 w = *(const float4*)(p.ln_w + c), b = *(const float4*)(p.ln_b + c);
      uint2 u;
      u.x = (uint32_t)f2t<T>(ln_norm(v.x, mean, rstd, w.x, b.x)) | ((uint32_t)f2t<T>(ln_norm(v.y, mean, rstd, w.y, b.y)) << 16);
      u.y = (uint32_t)f2t<T>(ln_norm(v.z, mean, rstd, w.z, b.z)) | ((uint32_t)f2t<T>(ln_norm(v.w, mean, rstd, w.w, b.w)) << 16);
      *(uint2*)((u16*)p.ln_out + (size_t)row * p.ln_ld + c) = u;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store((wm_gi32*)(p.ln_fallback + band), 0, WM_RLX_AGENT);
}

#ifdef WM_GEMM_STAMPS
// diagnostic build only (make stamps): wave 0 of every block records, on the 100 MHz s_memrealtime counter, its entry, the start and
// the end of its K loop and its exit (after its own stores have drained), the shader clock count of the loop and the CU it ran on;
// read back by wm_debug_gemm_stamps (tools/gemm_timeline.py).  No output depends on the stamps.
__device__ unsigned long long wm_gemm_stamp_buf[8 * 8192];
#endif

// Ping-pong v2 (256 x 256 only): same two-group structure, but the LDS-DMA runs TWO K-tiles ahead inside the same two
// 64-KiB buffers.  Quadrant order (0,0) (0,1) (1,1) (1,0) with B(qn=0) kept in registers for the whole K-tile, so the
// four regions of a buffer die one after the other — {A rows of qm=0, B cols of qn=0} after phase 0, B(qn=1) after
// phase 1, A(qm=1) after phase 2 — and each is refilled with K-tile t+2 in the very next phase (every wave issues
// 2 pieces per region).  In-order counted waits: with R = 4 / 2 / 2 pieces per wave for {A0,B0} / B1 / A1,
//   end of phase 3: {A0,B0}(t+1) landed  <=> at most  4 + 8[t+2 < nk]                  younger pieces outstanding
//   end of phase 0:  B1(t) landed        <=> at most  2 + 8[t+1 < nk]
//   end of phase 1:  A1(t) landed        <=> at most  8[t+1 < nk] + 4[t+2 < nk]
// RAW/WAR argument as for v1 (wait, then a barrier every reader passes; own reads retired before the stage's barrier).
// QI = 3 (192-row tile: wave tile 96 x 64, quadrants of 3 sub-tiles): the A regions have 12 pieces, so waves 0-3 carry
// two per region and waves 4-7 one; the counted waits then differ per wave half (R_A0B0 = nA + 2, R_B1 = 2, R_A1 = nA,
// nA = 2 | 1  ->  12 / 10 / 12 / 8 / 4 / 2  |  9 / 7 / 9 / 6 / 3 / 1), selected by a wave-uniform branch.
//
// VER = 3 (round 4) — HALF THE BARRIERS.  In-kernel stamps (profiles/r04_gemm_timeline.md) put a K-tile at 2 260 - 2 720 cycles
// against 1 536 / 2 048 of MFMA issue, the same with every operand row an L2 hit, 8 % less with the LDS-DMA removed, and
// barely less with MFMAs removed (a band cut from 12 to 10.75 units: -3 %): the eight s_barrier hand-offs of a K-tile
// (~ 90 cycles each in which the matrix pipe has nothing queued) are what the loop is made of.  v3 keeps the schedule of v2
// but lets group 0 ("X") put its barrier BEFORE its MFMA stage only and group 1 ("Y") BEFORE its load stage only:
//      X:  L(0) | B  M(k)  L(k+1) | B  M(k+1)  L(k+2) | ...
//      Y:       | B  L(k)  M(k)   | B  L(k+1)  M(k+1) | ...
// so inside an interval X's MFMAs run beside Y's loads, Y's MFMAs queue right behind them (no barrier in between) beside
// X's next loads, and only one hand-off per phase is left.  Ordering, with I_k the interval after barrier k = 4 t + p:
//  WAR  a region is refilled two phases after the phase whose load stage read it, instead of one: {A0,B0}(t+2) in L(t,2),
//       B1(t+2) in L(t,3), A1(t+2) in L(t+1,0).  Its readers were X's L(t,p) in I_(k-1) and Y's L(t,p) in I_k; the first
//       refill is X's in I_(k+1), behind barrier k+1, and Y retired its reads (lgkmcnt(0)) before its M(t,p).
//  RAW  a region of K-tile t+1 is first read by X in the interval before Y reads it; every wave waits for its own pieces of
//       it before the barrier that opens that interval: X at the end of the load stage in front of that barrier, Y after
//       the MFMA stage in front of it.  Pieces are issued in the order A0B0(k) B1(k) A1(k), k = 0, 1, ... by every wave
//       (c0 = nA + 2, c1 = 2, c2 = nA pieces, c = 2 nA + 4; nA = 2, or 1 for waves 4-7 of the 192-row tile), so with
//       n1 = [t+1 < nk], n2 = [t+2 < nk] the counted waits are
//         X  end of L(t,0): B1(t)       c2 + n1 c              end of L(t,1): A1(t)   n1 c
//            end of L(t,3): A0B0(t+1)   c1 + c2 + n2 (c0 + c1)
//         Y  end of M(t,0): A1(t)       n1 c                   end of M(t,2): A0B0(t+1)   c1 + c2 + n2 c0
//            end of M(t,3): B1(t+1)     c2 + n2 (c0 + c1)
//       and everybody waits for A0B0(0) and B1(0) (c2 + [nk > 1] c younger) before one common barrier in front of the loop.
template <int T, int EPI, int PRIO, int DBG = 0, int QI = 4, int VER = 2>
__global__ __launch_bounds__(512) void gemm_pp2_kernel(const WmGemmArgs p) {
  constexpr int SM = 2 * QI, SN = 4, WROWS = SM * 16, BM = 2 * WROWS, BN = 256;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  constexpr int APC = QI * 2;  // 8-row pieces per (wave row half, quadrant): 8 or 6
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef WM_GEMM_STAMPS
  const unsigned long long st_entry = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = (p.N + BN - 1) / BN, ntm = p.sched_bands > 0 ? p.sched_bands : (p.M + BM - 1) / BM;
  const int lid = xcd_remap(blockIdx.x, ntm * ntn);
  int band, nt;
  tile_of(lid, ntm, ntn, p.group_bands, band, nt);
  // Row band of this block, in 16-row units.  With a schedule (wm_launch_gemm) the M rows are cut into `ntm` bands of
  // floor / ceil(units / ntm) units, spread evenly (band b starts at floor(b units / ntm)), so that ntm x ntn fills whole
  // rounds of the CUs instead of leaving the last round a third empty (M = 11008: 696 tiles of 192 rows = 2.72 rounds ->
  // 768 tiles of 160 / 176 rows = 3.0).  A band of S units is S0 = ceil(S / 2) units for wave group 0 and S1 = S - S0 for
  // group 1; the LDS image keeps the full-tile layout (group 1's rows start at WROWS), only the SOURCE rows of group 1 move
  // up to follow group 0's, the MFMAs of the units a group does not have are skipped, and the epilogue stops at the band's end.
  int u0, S;
  if (p.sched_bands > 0) {
    u0 = (int)((long long)band * p.sched_units / ntm);
    S = (int)((long long)(band + 1) * p.sched_units / ntm) - u0;
  } else {
    u0 = band * 2 * SM;
    S = 2 * SM;
  }
  const int S0 = (S + 1) >> 1, Sw = wr ? S - S0 : S0;        // units of this wave's group (block- / wave-uniform)
  const int nB = Sw - QI;                                    // units in the group's second quadrant row: QI, QI - 1 or QI - 2
  const int m0 = u0 * 16, n0 = nt * BN;
  const int l15 = lane & 15, lq = lane >> 4;
  const bool two = QI == 4 || wave < 4;  // this wave carries two A pieces per region (wave-uniform)

  // this wave's DMA pieces per K-tile, in issue order: A0 A0 B0 B0 | B1 B1 | A1 A1 (the second A piece only if `two`)
  const u16* gp[8];
  int loff[8];
  // WM_EPI_CONV: the A rows are pixels; per A piece the lane's pixel, its border flags and its 16-B chunk, and (wave-uniform) the
  // tap / channel chunk of the K-tile the piece is issued for next (K-tile kt = tap * chunks + chunk: the weight's own K order)
  constexpr bool CONV = EPI == WM_EPI_CONV;
  int cv_pix[4], cv_fl[4], cv_c8[4], cv_tap[4] = {0, 0, 0, 0}, cv_cc[4] = {0, 0, 0, 0};
  const int cv_nch = CONV ? p.cv_cin >> 6 : 1;
  // token-conv form (p.tc_k > 0): column tile nt is an output phase; its word = neighbour count << 16 | 4 bits (di + 1, dj + 1) per neighbour
  const unsigned tc_word = CONV && p.tc_k > 0 ? p.tc_list[nt & 15] : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool isA = i < 2 || i >= 6;
    const int half = (i >= 4) ? 1 : 0;              // A1 / B1
    int pl;
    if (isA) {
      const int cl = QI == 4 ? 2 * wave + (i & 1) : (wave < 4 ? 2 * wave + (i & 1) : 8 + (wave - 4));  // index in the 2*APC-piece region
      pl = (cl < APC ? cl : cl - APC + 2 * APC) + APC * half;   // rows wr' * WROWS + 8 * APC * qm + ...
    } else {
      const int cl = 2 * wave + (i & 1);
      pl = (cl >> 2) * 8 + (cl & 3) + 4 * half;                 // cols wc' * 64 + 32 qn + ...
    }
    const int r = pl * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    int gr = (DBG == 4 ? 0 : (isA ? m0 : n0)) + (isA && r >= WROWS ? r - WROWS + 16 * S0 : r);
    const int lim = (isA ? p.M : p.N) - 1;
    gr = gr < lim ? gr : lim;
    gp[i] = (isA ? (const u16*)p.A + (size_t)gr * p.lda : (const u16*)p.W + (size_t)gr * p.ldw) + c * 8;
    loff[i] = (isA ? 0 : A_BYTES) + pl * 1024;
    if constexpr (CONV) {
      if (isA) {   // the row is a pixel (n, y, x) of the NHWC input: remember it and which image borders it touches
        const int ai = i < 2 ? i : i - 4;
        const int hw = p.cv_h * p.cv_w, n = gr / hw, rem = gr - n * hw, y = rem / p.cv_w, x = rem - y * p.cv_w;
        cv_pix[ai] = gr;
        cv_fl[ai] = (y == 0 ? 1 : 0) | (y == p.cv_h - 1 ? 2 : 0) | (x == 0 ? 4 : 0) | (x == p.cv_w - 1 ? 8 : 0);
        cv_c8[ai] = c * 8;
      }
    }
  }
  auto dma = [&](int buf, int i0, int i1, bool in_loop = false) {
    if ((DBG == 6 || (DBG >= 16 && (DBG & 1))) && in_loop) return;  // timing experiment: no LDS-DMA inside the K loop (the counted waits then never block)
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      if ((i == 1 || i == 7) && !two) continue;  // wave-uniform
      if constexpr (CONV) {
        if (i < 2 || i >= 6) {   // an A piece: the pixel shifted by the K-tile's tap, or the zero page outside the image
          const int ai = i < 2 ? i : i - 4;
          const int tap = cv_tap[ai], cc = cv_cc[ai];
          int dy, dx;
          if (p.tc_k > 0) { const unsigned nb = tc_word >> (4 * tap); dy = (int)(nb & 3) - 1; dx = (int)((nb >> 2) & 3) - 1; }
          else { const int ty = tap / 3; dy = ty - 1; dx = tap - ty * 3 - 1; }
          const int mask = (dy < 0 ? 1 : 0) | (dy > 0 ? 2 : 0) | (dx < 0 ? 4 : 0) | (dx > 0 ? 8 : 0);   // wave-uniform
          const u16* inside = (const u16*)p.A + ((long long)(cv_pix[ai] + dy * p.cv_w + dx) * p.cv_cin + cc * 64 + cv_c8[ai]);
          const u16* src = (cv_fl[ai] & mask) ? (const u16*)p.cv_zero + cv_c8[ai] : inside;
          __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(smem + buf * STAGE + loff[i]), 16, 0, 0);
          if (++cv_cc[ai] == cv_nch) { cv_cc[ai] = 0; ++cv_tap[ai]; }
          continue;
        }
      }
      __builtin_amdgcn_global_load_lds((glb_vp)gp[i], (lds_vp)(smem + buf * STAGE + loff[i]), 16, 0, 0);
      gp[i] += 64;
    }
  };
  auto wait2 = [&](auto n2c, auto n1c) {  // counted wait: immediates for the two-piece / one-piece wave halves
    if (two) wait_vmcnt<decltype(n2c)::value>(); else wait_vmcnt<decltype(n1c)::value>();
  };
#define WM_W2(a_, b_) wait2(std::integral_constant<int, a_>{}, std::integral_constant<int, b_>{})
  const int sw = (l15 >> 1) & 7;
  const int foff0 = l15 * 128 + ((lq ^ sw) << 4), foff1 = l15 * 128 + (((4 + lq) ^ sw) << 4);
  const int a_base = wr * WROWS * 128, b_base = A_BYTES + wc * 64 * 128;

  f32x4 acc[SM][SN];
#pragma unroll
  for (int i = 0; i < SM; ++i)
#pragma unroll
    for (int j = 0; j < SN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  s16x8 a[QI][2], b0[2][2], b1[2][2];

  // (token-conv form of WM_EPI_CONV: this column tile's own neighbour list sets the K length)
  const int nk = CONV && p.tc_k > 0 ? (int)(tc_word >> 16) * cv_nch : p.K / 64;
  dma(0, 0, 8);
  if (nk > 1) dma(1, 0, 8);
  if constexpr (VER == 3) {   // A0B0(0) and B1(0): group X reads B1(0) in the first interval, before group Y has had a wait of its own
    if (nk > 1) WM_W2(10, 7); else WM_W2(2, 1);
  } else {
    if (nk > 1) WM_W2(12, 9); else WM_W2(4, 3);
  }
  __builtin_amdgcn_s_barrier();
  if (VER == 2 && wr == 1) __builtin_amdgcn_s_barrier();

#ifdef WM_GEMM_STAMPS
  const unsigned long long st_loop0 = __builtin_amdgcn_s_memrealtime(), st_cyc0 = __builtin_amdgcn_s_memtime();
#endif
  if constexpr (VER == 3) {
    constexpr int NAY = QI == 4 ? 2 : 1;                      // A pieces per region of a group-1 wave (group 0 always carries 2)
    constexpr int CY = 2 * NAY + 4, C0Y = NAY + 2;
    auto lgk0 = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    auto bar = [&]() { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); };
    auto mfma_on = [&]() { __builtin_amdgcn_sched_barrier(0); if (PRIO) __builtin_amdgcn_s_setprio(1); };
    auto mfma_off = [&]() { if (PRIO) __builtin_amdgcn_s_setprio(0); __builtin_amdgcn_sched_barrier(0); };
    auto kloop3 = [&](auto nbc) __attribute__((always_inline)) {
      constexpr int NB = decltype(nbc)::value;
      // (Tried and dropped: reading only the k-half 0 fragments in the load stage and the k-half 1 fragments behind the k-half 0
      // MFMAs of the MFMA stage itself — the wait in the middle of the stage cost more than the shorter load stages gave: fc1
      // 101 -> 105 us, profiles/r04_gemm_timeline.md.)
      auto rd_a = [&](int t, int q0, int n) {   // A fragments of quadrant row q0 (first unit index), both k-halves
        const char* tile = smem + (t & 1) * STAGE;
#pragma unroll
        for (int i = 0; i < n; ++i) {
          a[i][0] = *(const s16x8*)(tile + a_base + (q0 + i) * 2048 + foff0);
          a[i][1] = *(const s16x8*)(tile + a_base + (q0 + i) * 2048 + foff1);
        }
      };
      auto rd_b = [&](int t, int j0, s16x8 (&b)[2][2]) {
        const char* tile = smem + (t & 1) * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          b[j][0] = *(const s16x8*)(tile + b_base + (j0 + j) * 2048 + foff0);
          b[j][1] = *(const s16x8*)(tile + b_base + (j0 + j) * 2048 + foff1);
        }
      };
      auto L0 = [&](int t) {
        rd_b(t, 0, b0); rd_a(t, 0, QI);
        if (t >= 1 && t + 1 < nk) dma((t + 1) & 1, 6, 8, true);   // A1(t+1): its last readers were the L(t-1,2)
      };
      auto L1 = [&](int t) { rd_b(t, 2, b1); };
      auto L2 = [&](int t) {
        rd_a(t, QI, NB);
        if (t + 2 < nk) dma(t & 1, 0, 4, true);                   // {A0,B0}(t+2): last readers the L(t,0)
      };
      auto L3 = [&](int t) {
        if (t + 2 < nk) dma(t & 1, 4, 6, true);                   // B1(t+2): last readers the L(t,1)
      };
      auto mm = [&](int r0, int n, int c0, s16x8 (&b)[2][2]) {
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
          for (int i = 0; i < n; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[r0 + i][c0 + j] = mfma16<T>(b[j][kh], a[i][kh], acc[r0 + i][c0 + j]);
      };
      auto M0 = [&](int) { mfma_on(); mm(0, QI, 0, b0); mfma_off(); };
      auto M1 = [&](int) { mfma_on(); mm(0, QI, 2, b1); mfma_off(); };
      auto M2 = [&](int) { mfma_on(); mm(QI, NB, 2, b1); mfma_off(); };
      auto M3 = [&](int) { mfma_on(); mm(QI, NB, 0, b0); mfma_off(); };
      if (wr == 0) {
        // ---- group X (nA = 2: c0 4, c1 2, c2 2, c 8): load stage one phase ahead of its barrier
        L0(0);
        if (nk > 1) wait_vmcnt<10>(); else wait_vmcnt<2>();
        for (int t = 0; t < nk; ++t) {
          const bool n1 = t + 1 < nk, n2 = t + 2 < nk;
          lgk0(); bar(); M0(t);
          L1(t);
          if (n1) wait_vmcnt<8>(); else wait_vmcnt<0>();
          lgk0(); bar(); M1(t);
          L2(t);
          lgk0(); bar(); M2(t);
          L3(t);
          if (n1) { if (n2) wait_vmcnt<10>(); else wait_vmcnt<4>(); }
          bar(); M3(t);
          if (n1) {
            L0(t + 1);
            if (n2) wait_vmcnt<10>(); else wait_vmcnt<2>();
          }
        }
      } else {
        // ---- group Y (nA = NAY): barrier, load stage, MFMA stage; its waits sit behind the MFMA stages
        for (int t = 0; t < nk; ++t) {
          const bool n1 = t + 1 < nk, n2 = t + 2 < nk;
          bar(); L0(t); lgk0(); M0(t);
          if (n1) wait_vmcnt<CY>(); else wait_vmcnt<0>();
          bar(); L1(t); lgk0(); M1(t);
          bar(); L2(t); lgk0(); M2(t);
          if (n1) { if (n2) wait_vmcnt<2 + NAY + C0Y>(); else wait_vmcnt<2 + NAY>(); }
          bar(); L3(t); M3(t);
          if (n1) { if (n2) wait_vmcnt<NAY + C0Y + 2>(); else wait_vmcnt<NAY>(); }
        }
      }
    };
    if (nB == QI) kloop3(std::integral_constant<int, QI>{});
    else if (nB == QI - 1) kloop3(std::integral_constant<int, QI - 1>{});
    else kloop3(std::integral_constant<int, QI - 2>{});
  } else {
  // timing experiments (stamps build, DBG = 16 + mask; results are wrong): 1 no LDS-DMA in the loop, 2 no fragment reads after the
  // first K-tile, 4 no barriers in the loop, 8 no s_setprio
  constexpr bool NO_RD = DBG >= 16 && (DBG & 2), NO_BAR = DBG >= 16 && (DBG & 4), NO_PRIO = DBG >= 16 && (DBG & 8);
  auto stage_end = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!NO_BAR) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (PRIO && !NO_PRIO) __builtin_amdgcn_s_setprio(1);
  };
  auto mfma_end = [&]() {
    if (PRIO && !NO_PRIO) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    if (!NO_BAR) __builtin_amdgcn_s_barrier();
  };

  // WM_EPI_RESID (p.pf_c): the epilogue's read-modify-write of the fp32 residual tile is a burst every CU issues at the same moment
  // (profiles/r04_gemm_ceiling.md: 11.9 us against 2 us for a plain epilogue).  In the last two K-tiles no refill is in flight: each lane
  // then touches one 128-B line of the block's old C tile per instruction (QI instructions cover the 64 QI rows x 8 lines) with a 4-byte
  // LDS-DMA into a scratch corner behind the ring — no destination register to keep alive, counted by vmcnt like the refills, never
  // read — so that the epilogue's loads find the lines on their way or in the L2.  The waits behind it allow PF more operations.
  constexpr bool PFX = EPI == WM_EPI_RESID && DBG == 0;
  constexpr int PF = QI;
  const bool do_pf = PFX && p.pf_c != 0 && nk >= 2;
  auto prefetch_c = [&]() __attribute__((always_inline)) {
    if constexpr (PFX) {
      const int rows = 16 * S, last = (p.M - 1 - m0) < rows - 1 ? (p.M - 1 - m0) : rows - 1;
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int l = tid + 512 * j;
        int row = l >> 3;
        row = row < last ? row : last;
        int col = n0 + (l & 7) * 32;
        col = col < p.N - 1 ? col : p.N - 4;
        const float* src = (const float*)p.C + (size_t)(m0 + row) * p.ldc + col;
        __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(smem + 2 * STAGE + wave * 256), 4, 0, 0);
      }
    }
  };
  // The K loop, instantiated per number NB of 16-row units in this wave group's SECOND quadrant row (a shortened band drops
  // units from the end of the group): the choice is made once, outside the loop (a guard per MFMA group inside it measured
  // +30 % on the loop).  The first quadrant row is always whole (wm_launch_gemm keeps bands >= 4 QI - 4 units).
  auto kloop = [&](auto nbc) __attribute__((always_inline)) {
  constexpr int NB = decltype(nbc)::value;
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const char* tile = smem + buf * STAGE;
    const bool n1 = t + 1 < nk, n2 = t + 2 < nk;
    // ---- phase 0: quadrant (0,0)
    if (!NO_RD || t == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      b0[j][0] = *(const s16x8*)(tile + b_base + j * 2048 + foff0);
      b0[j][1] = *(const s16x8*)(tile + b_base + j * 2048 + foff1);
    }
#pragma unroll
    for (int i = 0; i < QI; ++i) {
      a[i][0] = *(const s16x8*)(tile + a_base + i * 2048 + foff0);
      a[i][1] = *(const s16x8*)(tile + a_base + i * 2048 + foff1);
    }
    }
    if (n1) WM_W2(10, 7); else if (do_pf) WM_W2(2 + PF, 1 + PF); else WM_W2(2, 1);
    stage_end();
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < QI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<T>(b0[j][kh], a[i][kh], acc[i][j]);
    mfma_end();
    // ---- phase 1: quadrant (0,1); refill {A0,B0} with K-tile t+2
    if (!NO_RD || t == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      b1[j][0] = *(const s16x8*)(tile + b_base + (2 + j) * 2048 + foff0);
      b1[j][1] = *(const s16x8*)(tile + b_base + (2 + j) * 2048 + foff1);
    }
    }
    if (n2) { dma(buf, 0, 4, true); WM_W2(12, 9); }
    else if (n1) { if (do_pf) { prefetch_c(); WM_W2(8 + PF, 6 + PF); } else WM_W2(8, 6); }
    else if (do_pf) wait_vmcnt<PF>(); else wait_vmcnt<0>();
    stage_end();
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < QI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][2 + j] = mfma16<T>(b1[j][kh], a[i][kh], acc[i][2 + j]);
    mfma_end();
    // ---- phase 2: quadrant (1,1); refill B1
    if (!NO_RD) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      a[i][0] = *(const s16x8*)(tile + a_base + (QI + i) * 2048 + foff0);
      a[i][1] = *(const s16x8*)(tile + a_base + (QI + i) * 2048 + foff1);
    }
    }
    if (n2) dma(buf, 4, 6, true);
    stage_end();
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[QI + i][2 + j] = mfma16<T>(b1[j][kh], a[i][kh], acc[QI + i][2 + j]);
    mfma_end();
    // ---- phase 3: quadrant (1,0) from registers; refill A1; next K-tile's {A0,B0} must have landed
    if (n2) { dma(buf, 6, 8, true); WM_W2(12, 9); } else if (n1) { if (do_pf) WM_W2(4 + PF, 3 + PF); else WM_W2(4, 3); }
    stage_end();
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[QI + i][j] = mfma16<T>(b0[j][kh], a[i][kh], acc[QI + i][j]);
    mfma_end();
  }
  };
  if (nB == QI) kloop(std::integral_constant<int, QI>{});
  else if (nB == QI - 1) kloop(std::integral_constant<int, QI - 1>{});
  else kloop(std::integral_constant<int, QI - 2>{});
  }
#undef WM_W2
#ifdef WM_GEMM_STAMPS
  const unsigned long long st_loop1 = __builtin_amdgcn_s_memrealtime(), st_cyc1 = __builtin_amdgcn_s_memtime();
#endif
  if (VER == 2 && wr == 0) __builtin_amdgcn_s_barrier();
  if (DBG == 5 && acc[0][0][0] != 1.2345e-30f) return;  // timing experiment: no epilogue
  {
    const int rowb = m0 + (wr ? 16 * S0 : 0), rend = rowb + 16 * Sw;
    if constexpr (EPI == WM_EPI_RESID && DBG == 0 && QI == 3) {   // (192-row tile only: on the 256-row tile the fused epilogue does not fit 256 registers)
      if (p.ln_out) {   // block-uniform: the following LayerNorm rides in this epilogue
        epilogue_resid_ln<T, SM>(p, acc, smem, tid, lane, wr, wc, band, nt, rowb, n0 + wc * 64, wr ? 16 * S0 : 0, rend < p.M ? rend : p.M);
        return;
      }
    }
    epilogue16<T, EPI, SM, SN>(p, acc, rowb, n0 + wc * 64, lane, rend < p.M ? rend : p.M);
  }
#ifdef WM_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wave == 0 && blockIdx.x < 8192) {
    const unsigned long long st_exit = __builtin_amdgcn_s_memrealtime();
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_HW_ID, HW_REG_XCC_ID
    if (lane == 0) {
      unsigned long long* o = wm_gemm_stamp_buf + (size_t)blockIdx.x * 8;
      o[0] = st_entry; o[1] = st_loop0; o[2] = st_loop1; o[3] = st_exit; o[4] = st_cyc1 - st_cyc0;
      o[5] = ((unsigned long long)xcc << 32) | hw; o[6] = ((unsigned long long)m0 << 32) | (unsigned)n0; o[7] = 1;
    }
  }
#endif
}

// gemm_pp2_kernel<T, EPI, PRIO = 1, DBG, QI, VER>
template <int T, int EPI, int DBG = 0>
hipError_t launch_E(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  if constexpr (EPI != WM_EPI_CONV && DBG == 0) {   // (the pixel-row addressing of WM_EPI_CONV lives in v2 only)
    // v3 (half the barriers: bit-identical, measured +0.1 - 0.3 % on the forward, i.e. nothing — kept selectable and under test as the
    // record of that experiment); v2 has a barrier on both sides of every MFMA stage
    if (p.ver == 3) return p.qi == 4 ? wm_gemm_launch_kernel<gemm_pp2_kernel<T, EPI, 1, 0, 4, 3>>(a, p, s) : wm_gemm_launch_kernel<gemm_pp2_kernel<T, EPI, 1, 0, 3, 3>>(a, p, s);
  }
  return p.qi == 4 ? wm_gemm_launch_kernel<gemm_pp2_kernel<T, EPI, 1, DBG>>(a, p, s) : wm_gemm_launch_kernel<gemm_pp2_kernel<T, EPI, 1, DBG, 3>>(a, p, s);
}

#ifdef WM_GEMM_PP_DEBUG  // timing experiments only (results are wrong): gemm_plan.cpp maps the gemm_pp values to DBG
template <int T>
hipError_t launch_dbg(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  switch (p.dbg) {
#define WM_DBG(d_) case d_: return launch_E<T, WM_EPI_F32, d_>(a, p, s);
    WM_DBG(4) WM_DBG(5) WM_DBG(6)
    WM_DBG(16 + 1) WM_DBG(16 + 2) WM_DBG(16 + 4) WM_DBG(16 + 8) WM_DBG(16 + 3) WM_DBG(16 + 7) WM_DBG(16 + 15) WM_DBG(16 + 5) WM_DBG(16 + 12)
#undef WM_DBG
    default: return hipErrorInvalidValue;
  }
}
#endif

}  // namespace

hipError_t wm_gemm_launch_pp2(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
#ifdef WM_GEMM_PP_DEBUG
  if (p.dbg) return a.dtype == WM_T_BF16 ? launch_dbg<WM_T_BF16>(a, p, s) : launch_dbg<WM_T_F16>(a, p, s);
#endif
  switch (a.epi) {
    WM_GEMM_EPI_CASE(WM_EPI_F32) WM_GEMM_EPI_CASE(WM_EPI_T16) WM_GEMM_EPI_CASE(WM_EPI_GELU_T16) WM_GEMM_EPI_CASE(WM_EPI_RESID)
    WM_GEMM_EPI_CASE(WM_EPI_QKV) WM_GEMM_EPI_CASE(WM_EPI_ROWMAP_ADD) WM_GEMM_EPI_CASE(WM_EPI_CONV)
    default: return hipErrorInvalidValue;
  }
}

hipError_t wm_gemm_launch_ln_fallback(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  const int bands = (int)p.grid / 4;   // N = 1024: four column tiles per row band; 12 units = the 192-row tile of the fused epilogue
  if (a.dtype == WM_T_BF16) hipLaunchKernelGGL((gemm_ln_fallback_kernel<WM_T_BF16>), dim3(bands), dim3(256), 0, s, a, bands, 12);
  else hipLaunchKernelGGL((gemm_ln_fallback_kernel<WM_T_F16>), dim3(bands), dim3(256), 0, s, a, bands, 12);
  return hipGetLastError();
}

#ifdef WM_GEMM_STAMPS
extern "C" int wm_debug_gemm_stamps(unsigned long long* host_out, int nblocks) {
  if (nblocks > 8192) nblocks = 8192;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(wm_gemm_stamp_buf), (size_t)nblocks * 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
extern "C" int wm_debug_ln_fallback_count() {   // bands the fused-LayerNorm fallback kernel recomputed since the last call (then reset)
  int v = -1, z = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(wm_ln_fallback_count), 4) != hipSuccess) return -1;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(wm_ln_fallback_count), &z, 4);
  return v;
}
extern "C" int wm_debug_gemm_stamps_clear() {
  void* d = nullptr;
  if (hipGetSymbolAddress(&d, HIP_SYMBOL(wm_gemm_stamp_buf)) != hipSuccess) return 1;
  return hipMemset(d, 0, sizeof(unsigned long long) * 8 * 8192) == hipSuccess ? 0 : 1;
}
#endif
