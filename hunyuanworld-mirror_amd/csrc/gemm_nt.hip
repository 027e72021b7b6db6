// Lock-step GEMM on the 32x32x16 MFMA (GemmPlan family NT32): the kernel of every launch the ping-pong kernels do not take — small
// shapes, forced tiles, plain WM_EPI_ROWMAP_ADD and WM_EPI_CONVT — with its own epilogue (the 32x32 register layout).
//
// Structure
//  * tile (WM*TM*32) x (WN*TN*32) x 64, WM x WN waves, each wave TM x TN MFMA 32x32 tiles;
//  * NSTAGE-deep LDS ring, one raw s_barrier per K-tile, counted s_waitcnt vmcnt(N) so NSTAGE-2
//    tiles stay in flight across the barrier (guides "Pipelining across barriers", T3+T4);
//  * staging and operand order as in gemm_common.h.
#include "gemm_common.h"

namespace {

template <int T, int EPI, int WM, int WN, int TM, int TN, int NSTAGE, int ILV, int KT = 64>
__global__ __launch_bounds__(WM * WN * 64) void gemm_nt_kernel(const WmGemmArgs p) {
  constexpr int BK = KT;
  constexpr int NW = WM * WN, BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int PA = BM * BK * 2 / 1024, PB = BN * BK * 2 / 1024;  // 1-KiB pieces per operand tile
  constexpr int PPW = (PA + PB) / NW;           // pieces per wave per K-tile
  static_assert((PA + PB) % NW == 0, "pieces must divide over waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + BM - 1) / BM;
  const int lid = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (lid / ntn) * BM, n0 = (lid % ntn) * BN;
  const u16* A = (const u16*)p.A;
  const u16* W = (const u16*)p.W;

  auto stage_part = [&](int kt, int s, int i0, int i1) {
    char* base = smem + s * STAGE;
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      const int pc = wave * PPW + i;  // wave-uniform
      if constexpr (BK == 64) {
        if (pc < PA) stage_piece(A, p.lda, m0, p.M, kt * BK, base, pc, lane);
        else stage_piece(W, p.ldw, n0, p.N, kt * BK, base + A_BYTES, pc - PA, lane);
      } else {
        if (pc < PA) stage_piece32(A, p.lda, m0, p.M, kt * BK, base, pc, lane);
        else stage_piece32(W, p.ldw, n0, p.N, kt * BK, base + A_BYTES, pc - PA, lane);
      }
    }
  };
  auto stage = [&](int kt, int s) { stage_part(kt, s, 0, PPW); };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.K / BK;
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < nk) stage(s, s);

  for (int t = 0; t < nk; ++t) {
    // tile t must have landed; tiles t+1 .. t+NSTAGE-2 may stay in flight
    const int ahead = min(nk - 1 - t, NSTAGE - 2);
    if (ahead >= 3) wait_vmcnt<3 * PPW>();
    else if (ahead >= 2) wait_vmcnt<2 * PPW>();
    else if (ahead == 1) wait_vmcnt<PPW>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // everyone's pieces of tile t landed; everyone finished tile t-1
    const bool more = t + NSTAGE - 1 < nk;
    if (!ILV && more) stage(t + NSTAGE - 1, (t + NSTAGE - 1) % NSTAGE);
    const char* tA = smem + (t % NSTAGE) * STAGE;
    const char* tB = tA + A_BYTES;
    if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      if (ILV && more) {  // spread the LDS-DMA issue over the four MFMA groups of this K-tile
        constexpr int Q = (PPW + 3) / 4;
        stage_part(t + NSTAGE - 1, (t + NSTAGE - 1) % NSTAGE, ks * Q < PPW ? ks * Q : PPW, (ks + 1) * Q < PPW ? (ks + 1) * Q : PPW);
      }
      const int ch = 2 * ks + (lane >> 5);
      s16x8 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[i] = BK == 64 ? lds_frag(tA, (wm * TM + i) * 32 + (lane & 31), ch) : lds_frag32(tA, (wm * TM + i) * 32 + (lane & 31), ch);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b[j] = BK == 64 ? lds_frag(tB, (wn * TN + j) * 32 + (lane & 31), ch) : lds_frag32(tB, (wn * TN + j) * 32 + (lane & 31), ch);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32<T>(b[j], a[i], acc[i][j]);  // D[n][m]: lane = row m
      if (ILV) __builtin_amdgcn_sched_barrier(0);
    }
    if (PRIO) __builtin_amdgcn_s_setprio(0);
  }

  // ---------------- epilogue: lane (m = lane&31, h = lane>>5), reg 4g+e <-> col 8g + 4h + e ----------------
  const int h4 = (lane >> 5) * 4;
  if constexpr (EPI == WM_EPI_QKV) {
    // attention.py:50-56 fused: the wave's 64 columns are exactly one head of q, k or v (TN == 2, tiles
    // aligned to 64): bias -> LayerNorm(64, eps 1e-5, affine) -> 2-D RoPE (rope.py:148-181) -> q scale ->
    // 16-bit store in the head-major layout the attention kernel reads.  A lane holds 32 of its row's 64
    // values (the other 32 sit in lane^32), and every RoPE pair (c, c+16) is lane-local (g <-> g+2).
    static_assert(EPI != WM_EPI_QKV || TN == 2, "QKV epilogue needs 64 columns per wave");
    const WmQkvArgs& q = p.qkv;
    const int D = q.H * 64;
    const int col0 = n0 + wn * 64;             // wave-uniform
    const int which = col0 / D, head = (col0 - which * D) >> 6;
    if (col0 < p.N) {
      const float* nw = which == 0 ? q.qn_w : q.kn_w;
      const float* nb = which == 0 ? q.qn_b : q.kn_b;
      const bool do_norm = which < 2 && nw != nullptr;
      const bool do_rope = which < 2 && q.rope_cos != nullptr;
      u16* dst = (u16*)(which == 0 ? q.q : which == 1 ? q.k : q.v);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = m0 + (wm * TM + i) * 32 + (lane & 31);
        const bool row_ok = row < p.M;
        float v[2][4][4];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 bs = p.bias ? *(const float4*)(p.bias + col0 + 32 * j + 8 * g + h4) : make_float4(0, 0, 0, 0);
            v[j][g][0] = acc[i][j][4 * g] + bs.x; v[j][g][1] = acc[i][j][4 * g + 1] + bs.y;
            v[j][g][2] = acc[i][j][4 * g + 2] + bs.z; v[j][g][3] = acc[i][j][4 * g + 3] + bs.w;
          }
        if (do_norm) {
          float sm = 0.f;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int e = 0; e < 4; ++e) sm += v[j][g][e];
          const float mean = xhalf_sum(sm) * (1.0f / 64.0f);
          float ss = 0.f;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[j][g][e] -= mean; ss += v[j][g][e] * v[j][g][e]; }
          const float rstd = 1.0f / sqrtf(xhalf_sum(ss) * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const float4 w4 = *(const float4*)(nw + 32 * j + 8 * g + h4), b4 = *(const float4*)(nb + 32 * j + 8 * g + h4);
              v[j][g][0] = v[j][g][0] * rstd * w4.x + b4.x; v[j][g][1] = v[j][g][1] * rstd * w4.y + b4.y;
              v[j][g][2] = v[j][g][2] * rstd * w4.z + b4.z; v[j][g][3] = v[j][g][3] * rstd * w4.w + b4.w;
            }
        }
        if (do_rope) {
          const int rr = row_ok ? row : 0;
          // row / tokens_per_view and idx / grid_w by float multiplication (exact here: rows < 2^20, quotients < 2^11,
          // the +0.5 keeps the product > 1e-4 away from an integer) — two runtime integer divisions were ~80 VALU per row
          const int t = rr - (int)(((float)rr + 0.5f) * q.inv_tpv) * q.tokens_per_view;
          int py = 0, px = 0;
          if (t >= q.patch_start) {
            const int idx = t - q.patch_start;
            py = (int)(((float)idx + 0.5f) * q.inv_gw) + 1;
            px = idx - (py - 1) * q.grid_w + 1;
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int pos = j == 0 ? py : px;  // first 32 channels rotate by y, last 32 by x
#pragma unroll
            for (int g = 0; g < 2; ++g) {      // pair (g, g+2): elements c and c+16; frequency index 8g + 4h + e
              const float4 cs = *(const float4*)(q.rope_cos + pos * 16 + 8 * g + h4);
              const float4 sn = *(const float4*)(q.rope_sin + pos * 16 + 8 * g + h4);
              const float c4[4] = {cs.x, cs.y, cs.z, cs.w}, s4[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float lo = v[j][g][e], hi = v[j][g + 2][e];
                v[j][g][e] = lo * c4[e] - hi * s4[e];
                v[j][g + 2][e] = hi * c4[e] + lo * s4[e];
              }
            }
          }
        }
        const float sc = which == 0 ? q.q_scale : 1.0f;
        if (row_ok) {
          u16* o = dst + ((size_t)head * q.head_stride + row) * 64 + h4;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              uint2 u;
              u.x = (uint32_t)f2t<T>(v[j][g][0] * sc) | ((uint32_t)f2t<T>(v[j][g][1] * sc) << 16);
              u.y = (uint32_t)f2t<T>(v[j][g][2] * sc) | ((uint32_t)f2t<T>(v[j][g][3] * sc) << 16);
              *(uint2*)(o + 32 * j + 8 * g) = u;
            }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = m0 + (wm * TM + i) * 32 + (lane & 31);
    if (row >= p.M) continue;
    size_t orow = (size_t)row;
    int q = 0;
    if constexpr (EPI == WM_EPI_ROWMAP_ADD) {
      const int g = row / p.rows_per_group;
      q = row - g * p.rows_per_group;
      orow = (size_t)g * p.out_group + p.out_off + q;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int cb = n0 + (wn * TN + j) * 32 + h4;
      if constexpr (EPI == WM_EPI_CONVT) {
        // k==stride ConvTranspose2d as GEMM: col = (ii*k + jj)*Cout + co; row = (n*gh + y)*gw + x
        const int hw = p.ct_gh * p.ct_gw;
        const int n = row / hw, yx = row - n * hw, y = yx / p.ct_gw, x = yx - y * p.ct_gw;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = cb + 8 * g;
          if (col >= p.N) continue;
          const int co = col % p.ct_cout, ij = col / p.ct_cout;  // 4 consecutive cols share (ii,jj): Cout % 4 == 0
          const int ii = ij / p.ct_k, jj = ij - ii * p.ct_k;
          const size_t o = (((size_t)n * p.ct_gh * p.ct_k + (y * p.ct_k + ii)) * (p.ct_gw * p.ct_k) + (x * p.ct_k + jj)) * p.ct_cout + co;
          const float4 bs = *(const float4*)(p.bias + co);
          *(float4*)((float*)p.C + o) = make_float4(acc[i][j][4 * g] + bs.x, acc[i][j][4 * g + 1] + bs.y,
                                                    acc[i][j][4 * g + 2] + bs.z, acc[i][j][4 * g + 3] + bs.w);
        }
      } else {
        float4 v[4];
        bool ok[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = cb + 8 * g;
          ok[g] = col < p.N;  // N % 4 == 0: a float4 is all-in or all-out
          const int cc = ok[g] ? col : 0;
          const float4 bs = p.bias ? *(const float4*)(p.bias + cc) : make_float4(0, 0, 0, 0);
          v[g] = make_float4(acc[i][j][4 * g] + bs.x, acc[i][j][4 * g + 1] + bs.y, acc[i][j][4 * g + 2] + bs.z,
                             acc[i][j][4 * g + 3] + bs.w);
        }
        if constexpr (EPI == WM_EPI_F32) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (ok[g]) *(float4*)((float*)p.C + orow * p.ldc + cb + 8 * g) = v[g];
        } else if constexpr (EPI == WM_EPI_T16 || EPI == WM_EPI_GELU_T16) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (!ok[g]) continue;
            float4 x = v[g];
            if constexpr (EPI == WM_EPI_GELU_T16) x = gelu_erf4(x);
            uint2 u;
            u.x = (uint32_t)f2t<T>(x.x) | ((uint32_t)f2t<T>(x.y) << 16);
            u.y = (uint32_t)f2t<T>(x.z) | ((uint32_t)f2t<T>(x.w) << 16);
            *(uint2*)((u16*)p.C + orow * p.ldc + cb + 8 * g) = u;
          }
        } else if constexpr (EPI == WM_EPI_RESID) {
          float4 old[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) old[g] = ok[g] ? *(const float4*)((const float*)p.C + orow * p.ldc + cb + 8 * g) : make_float4(0, 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (!ok[g]) continue;
            const float4 gm = *(const float4*)(p.gamma + cb + 8 * g);
            const float4 nv = make_float4(old[g].x + gm.x * v[g].x, old[g].y + gm.y * v[g].y, old[g].z + gm.z * v[g].z, old[g].w + gm.w * v[g].w);
            *(float4*)((float*)p.C + orow * p.ldc + cb + 8 * g) = nv;
            if (p.C2) *(float4*)(p.C2 + orow * p.ldc2 + cb + 8 * g) = nv;
          }
        } else if constexpr (EPI == WM_EPI_ROWMAP_ADD) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (!ok[g]) continue;
            int col = cb + 8 * g, addn = p.N;
            void* Cb = p.C;
            if (p.split_n > 0) rowmap_slice(p, col, addn, Cb);   // (kernel-uniform) several consumers' columns side by side
            float4 x = v[g];
            if (p.relu) x = make_float4(fmaxf(x.x, 0.f), fmaxf(x.y, 0.f), fmaxf(x.z, 0.f), fmaxf(x.w, 0.f));
            if (p.add) {
              const float4 ad = *(const float4*)(p.add + (size_t)q * addn + col);
              x.x += ad.x; x.y += ad.y; x.z += ad.z; x.w += ad.w;
            }
            const size_t o = orow * p.ldc + col;
            if (p.out16) {
              uint2 u;
              u.x = (uint32_t)f2t<T>(x.x) | ((uint32_t)f2t<T>(x.y) << 16);
              u.y = (uint32_t)f2t<T>(x.z) | ((uint32_t)f2t<T>(x.w) << 16);
              *(uint2*)((u16*)Cb + o) = u;
            } else {
              float* c = (float*)Cb + o;
              if (p.accumulate) {
                const float4 od = *(const float4*)c;
                x.x += od.x; x.y += od.y; x.z += od.z; x.w += od.w;
              }
              *(float4*)c = x;
            }
          }
        }
      }
    }
  }
}

// tile configurations: id -> (WM, WN, TM, TN, NSTAGE)
//  0: 128x128, 4 waves, 2-stage (64 KiB, 2 blocks/CU)     1: 256x128, 8 waves, 3-stage (144 KiB)
//  2: 128x256, 8 waves, 3-stage (144 KiB)                 3: 128x128, 8 waves (32x64 per wave), 4-stage (128 KiB)
//  4: 256x256, 8 waves (128x64 per wave), 2-stage (128 KiB)   5: 192x256, 8 waves (96x64 per wave), 2-stage (112 KiB)
// (the sizes the plan launches them with: nt_tiles in gemm_plan.cpp)
template <int T, int EPI>
hipError_t launch_E(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  switch (p.cfg) {
    case 0: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 2, 2, 2, 2, 2, 0>>(a, p, s);
    case 1: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 4, 2, 2, 2, 3, 0>>(a, p, s);
    case 2: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 4, 2, 2, 2, 3, 1>>(a, p, s);
    case 3: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 2, 4, 4, 2, 2, 1>>(a, p, s);
    case 4: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 2, 4, 4, 2, 2, 0>>(a, p, s);
    case 5: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 2, 4, 3, 2, 2, 0>>(a, p, s);
    case 6: return wm_gemm_launch_kernel<gemm_nt_kernel<T, EPI, 2, 4, 4, 2, 4, 0, 32>>(a, p, s);  // 256x256, K-tile 32, 4-stage ring (128 KiB)
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t wm_gemm_launch_nt(const WmGemmArgs& a, const GemmPlan& p, hipStream_t s) {
  switch (a.epi) {
    WM_GEMM_EPI_CASE(WM_EPI_F32) WM_GEMM_EPI_CASE(WM_EPI_T16) WM_GEMM_EPI_CASE(WM_EPI_GELU_T16) WM_GEMM_EPI_CASE(WM_EPI_RESID)
    WM_GEMM_EPI_CASE(WM_EPI_ROWMAP_ADD) WM_GEMM_EPI_CASE(WM_EPI_CONVT) WM_GEMM_EPI_CASE(WM_EPI_QKV)
    default: return hipErrorInvalidValue;
  }
}
