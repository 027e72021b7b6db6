// C[M,N] = A[M,K] * W[N,K]^T with fused epilogues — 16-bit (bf16/f16) MFMA, fp32 accumulate.
//
// Replaces every nn.Linear / 1x1 conv / k==stride ConvTranspose on the hot path
// (reference: src/models/layers/attention.py:50,67; mlp.py:29-35; patch_embed.py:70;
//  heads/dense_head.py:53-68,204-208).  Both operands are K-contiguous ("NT"), which is what
// torch's Linear weight layout gives for free and what the 32x32x16 MFMA fragments want.
//
// What the four kernel families (gemm_nt.hip, gemm_nt16.hip, gemm_pp.hip, gemm_pp2.hip) share: the device side of this header.
//  * global -> LDS by LDS-DMA (global_load_lds, 16 B/lane, 1 KiB per wave-instruction); the XOR
//    swizzle that makes the ds_read_b128 fragment reads conflict-free is applied to the per-lane
//    SOURCE address (guides §5.4 rule 21);
//  * the MFMA is issued as D = W_frag * A_frag (operands swapped), so a lane owns one output ROW
//    and 4 consecutive COLUMNS per register group: the epilogue reads/writes float4 (16 B/lane).
// Which family runs a launch is decided in gemm_plan.cpp (gemm_launch.h).
#pragma once
#include "wm_common.h"
#include "gemm_launch.h"

#include <type_traits>

namespace {

#ifndef WM_GEMM_PRIO
#define WM_GEMM_PRIO 0
#endif
constexpr int PRIO = WM_GEMM_PRIO;
constexpr int BK = 64;  // default K-tile; the 32x32 kernel is also instantiated with BK = 32 (KT template parameter)

typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

// K-tile 32: rows are 64 B, a 1-KiB piece is 16 rows x 4 chunks; slot swizzle (row>>2)&3 keeps ds_read_b128 conflict-free
__device__ __forceinline__ void stage_piece32(const u16* __restrict__ g, int ld, int row0, int nrows, int k0, char* lds_tile,
                                              int piece, int lane) {
  const int r = piece * 16 + (lane >> 2);
  const int c = (lane & 3) ^ ((r >> 2) & 3);
  int gr = row0 + r;
  gr = gr < nrows ? gr : nrows - 1;
  __builtin_amdgcn_global_load_lds((glb_vp)(g + (size_t)gr * ld + k0 + c * 8), (lds_vp)(lds_tile + piece * 1024), 16, 0, 0);
}
__device__ __forceinline__ s16x8 lds_frag32(const char* tile, int row, int chunk) {
  return *(const s16x8*)(tile + row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4));
}

// one 1-KiB LDS-DMA piece = 8 rows x 128 B of an operand tile
__device__ __forceinline__ void stage_piece(const u16* __restrict__ g, int ld, int row0, int nrows, int k0, char* lds_tile,
                                            int piece, int lane) {
  const int r = piece * 8 + (lane >> 3);
  const int c = (lane & 7) ^ ((r >> 1) & 7);  // LDS[r][p] = G[r][p ^ swz(r)]
  int gr = row0 + r;
  gr = gr < nrows ? gr : nrows - 1;  // clamp: out-of-range rows are masked in the epilogue
  __builtin_amdgcn_global_load_lds((glb_vp)(g + (size_t)gr * ld + k0 + c * 8), (lds_vp)(lds_tile + piece * 1024), 16, 0, 0);
}

__device__ __forceinline__ s16x8 lds_frag(const char* tile, int row, int chunk) {
  return *(const s16x8*)(tile + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
}

// logical tile id -> (row band, column tile).  With more than 4 column tiles the tiles that run together on an XCD (32 CUs,
// consecutive ids) are arranged as G row bands x 8 column tiles instead of 2 x 16: per round the XCD's L2 then fetches
// (G x A band + 32 / G x W slab) instead of (2 x A + 16 x W) — e.g. fc1 at 8 views 144 instead of 216 MB of L2 misses.
__device__ __forceinline__ void tile_of(int lid, int ntm, int ntn, int G, int& band, int& nt) {
  if (G <= 1 || ntn <= 4) { band = lid / ntn; nt = lid - band * ntn; return; }
  const int per = G * ntn, sg = lid / per, r = lid - sg * per;
  const int here = ntm - sg * G < G ? ntm - sg * G : G;
  nt = r / here;
  band = sg * G + (r - nt * here);
}

// WM_EPI_ROWMAP_ADD with split_n > 0: column `col` of the launch belongs to slice col / split_n; returns the column inside the slice, the slice's
// width (the pitch of the `add` table) and its output tensor
__device__ __forceinline__ void rowmap_slice(const WmGemmArgs& p, int& col, int& addn, void*& Cb) {
  const int hd = col / p.split_n;
  col -= hd * p.split_n;
  addn = p.split_n;
  Cb = hd == 0 ? p.split_C[0] : hd == 1 ? p.split_C[1] : hd == 2 ? p.split_C[2] : p.split_C[3];
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Epilogue shared by the 16x16x32 kernels.  acc[i][j] is the 16x16 sub-tile at rows rowb + 16 i, columns colb + 16 j of
// the wave's SM x SN grid; operands were swapped (D = W_frag * A_frag), so lane (l15 = lane & 15, lq = lane >> 4) owns
// row 16 i + l15 and the 4 consecutive columns 16 j + 4 lq .. + 3.
template <int T, int EPI, int SM, int SN>
__device__ __forceinline__ void epilogue16(const WmGemmArgs& p, f32x4 (&acc)[SM][SN], int rowb, int colb, int lane, int mlim) {
  // mlim: first row this wave must NOT write (p.M, or the end of the wave's share of a shortened row band)
  const int l15 = lane & 15, lq = lane >> 4;
  // ---------------- epilogue ----------------
  if constexpr (EPI == WM_EPI_QKV) {
    static_assert(EPI != WM_EPI_QKV || SN == 4, "QKV epilogue needs 64 columns per wave");
    const WmQkvArgs& q = p.qkv;
    const int D = q.H * 64;
    const int col0 = colb;
    const int which = col0 / D, head = (col0 - which * D) >> 6;
    if (col0 >= p.N) return;
    const float* nw = which == 0 ? q.qn_w : q.kn_w;
    const float* nb = which == 0 ? q.qn_b : q.kn_b;
    const bool do_norm = which < 2 && nw != nullptr, do_rope = which < 2 && q.rope_cos != nullptr;
    u16* dst = (u16*)(which == 0 ? q.q : which == 1 ? q.k : q.v);
    const float sc = which == 0 ? q.q_scale : 1.0f;
    // column vectors of this head are the same for every row group: loaded once.  The per-row RoPE table rows are
    // requested one row group ahead, i.e. BEFORE the previous group's stores (the compiler may not move a load across
    // a possibly aliasing store, so loads placed after them would each pay a full L2 round trip per row group).
    float4 bs4[4], w4[4], b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bs4[j] = p.bias ? *(const float4*)(p.bias + col0 + 16 * j + 4 * lq) : make_float4(0, 0, 0, 0);
      w4[j] = do_norm ? *(const float4*)(nw + 16 * j + 4 * lq) : make_float4(1, 1, 1, 1);
      b4[j] = do_norm ? *(const float4*)(nb + 16 * j + 4 * lq) : make_float4(0, 0, 0, 0);
    }
    auto rope_rows = [&](int i, float4 (&cs)[2], float4 (&sn)[2]) {
      const int row = rowb + i * 16 + l15;
      const int rr = row < mlim ? row : 0;
      const int t = rr - (int)(((float)rr + 0.5f) * q.inv_tpv) * q.tokens_per_view;  // see gemm_nt_kernel
      int py = 0, px = 0;
      if (t >= q.patch_start) {
        const int idx = t - q.patch_start;
        py = (int)(((float)idx + 0.5f) * q.inv_gw) + 1;
        px = idx - (py - 1) * q.grid_w + 1;
      }
      cs[0] = *(const float4*)(q.rope_cos + py * 16 + 4 * lq); sn[0] = *(const float4*)(q.rope_sin + py * 16 + 4 * lq);
      cs[1] = *(const float4*)(q.rope_cos + px * 16 + 4 * lq); sn[1] = *(const float4*)(q.rope_sin + px * 16 + 4 * lq);
    };
    float4 csn[2][2], snn[2][2];  // [parity of the row group][y | x]
    if (do_rope) rope_rows(0, csn[0], snn[0]);
#pragma unroll
    for (int i = 0; i < SM; ++i) {
      if (rowb + i * 16 >= mlim) break;  // wave-uniform: the rest of the wave's rows are past the band / matrix end
      const int row = rowb + i * 16 + l15;
      const bool row_ok = row < mlim;
      if (do_rope && i + 1 < SM) rope_rows(i + 1, csn[(i + 1) & 1], snn[(i + 1) & 1]);
      float v[4][4];  // [j: 16-col group][e]: column 16j + 4*lq + e of this head
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j][0] = acc[i][j][0] + bs4[j].x; v[j][1] = acc[i][j][1] + bs4[j].y; v[j][2] = acc[i][j][2] + bs4[j].z; v[j][3] = acc[i][j][3] + bs4[j].w;
      }
      if (do_norm) {  // the row's 64 values live in the 4 lanes l15 + 16*{0..3}
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) sm += v[j][e];
        sm += __shfl_xor(sm, 16);
        const float mean = xhalf_sum(sm) * (1.0f / 64.0f);
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[j][e] -= mean; ss += v[j][e] * v[j][e]; }
        ss += __shfl_xor(ss, 16);
        const float rstd = 1.0f / sqrtf(xhalf_sum(ss) * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j][0] = v[j][0] * rstd * w4[j].x + b4[j].x; v[j][1] = v[j][1] * rstd * w4[j].y + b4[j].y;
          v[j][2] = v[j][2] * rstd * w4[j].z + b4[j].z; v[j][3] = v[j][3] * rstd * w4[j].w + b4[j].w;
        }
      }
      if (do_rope) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {  // columns [0,32) rotate by y, [32,64) by x; pair (c, c+16) = groups (2hh, 2hh+1)
          const float4 cs = csn[i & 1][hh], sn = snn[i & 1][hh];
          const float c4[4] = {cs.x, cs.y, cs.z, cs.w}, s4[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = v[2 * hh][e], hi = v[2 * hh + 1][e];
            v[2 * hh][e] = lo * c4[e] - hi * s4[e];
            v[2 * hh + 1][e] = hi * c4[e] + lo * s4[e];
          }
        }
      }
      // 16-B stores (swap16: even quads take sub-tile 2jp, odd quads 2jp + 1); all lanes take part in the swaps
      uint2 u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u[j].x = (uint32_t)f2t<T>(v[j][0] * sc) | ((uint32_t)f2t<T>(v[j][1] * sc) << 16);
        u[j].y = (uint32_t)f2t<T>(v[j][2] * sc) | ((uint32_t)f2t<T>(v[j][3] * sc) << 16);
      }
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        swap16(u[2 * jp].x, u[2 * jp + 1].x);
        swap16(u[2 * jp].y, u[2 * jp + 1].y);
      }
      if (row_ok) {
        u16* o = dst + ((size_t)head * q.head_stride + row) * 64 + 16 * (lq & 1) + 4 * (lq & 2);
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) *(uint4*)(o + 32 * jp) = make_uint4(u[2 * jp].x, u[2 * jp].y, u[2 * jp + 1].x, u[2 * jp + 1].y);
      }
    }
    return;
  } else {
    // Column vectors (bias, LayerScale gamma) depend on j only: loaded once, ahead of every store (the compiler may not
    // move a load across a possibly aliasing store, so a load inside the (i, j) loop pays its latency per iteration).
    float4 bs4[SN], gm4[SN];
#pragma unroll
    for (int j = 0; j < SN; ++j) {
      const int col = colb + j * 16 + 4 * lq;
      bs4[j] = (p.bias && col < p.N) ? *(const float4*)(p.bias + col) : make_float4(0, 0, 0, 0);
      if constexpr (EPI == WM_EPI_RESID) gm4[j] = col < p.N ? *(const float4*)(p.gamma + col) : make_float4(0, 0, 0, 0);
    }
    if constexpr ((EPI == WM_EPI_T16 || EPI == WM_EPI_GELU_T16) && SN % 2 == 0) {
      // 16-bit outputs: pair the sub-tiles (2jp, 2jp + 1) through swap16 and store 16 B per lane
      if ((p.N & 7) == 0 && (p.ldc & 7) == 0 && ((uintptr_t)p.C & 15) == 0) {
#pragma unroll
        for (int i = 0; i < SM; ++i) {
          if (rowb + i * 16 >= mlim) break;  // wave-uniform: the rest of the wave's rows are past the band / matrix end
          const int row = rowb + i * 16 + l15;
#pragma unroll
          for (int jp = 0; jp < SN / 2; ++jp) {
            uint2 u[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int j = 2 * jp + h;
              float4 x = make_float4(acc[i][j][0] + bs4[j].x, acc[i][j][1] + bs4[j].y, acc[i][j][2] + bs4[j].z, acc[i][j][3] + bs4[j].w);
              if constexpr (EPI == WM_EPI_GELU_T16) x = gelu_erf4(x);
              u[h].x = (uint32_t)f2t<T>(x.x) | ((uint32_t)f2t<T>(x.y) << 16);
              u[h].y = (uint32_t)f2t<T>(x.z) | ((uint32_t)f2t<T>(x.w) << 16);
            }
            swap16(u[0].x, u[1].x);
            swap16(u[0].y, u[1].y);
            const int col = colb + (2 * jp + (lq & 1)) * 16 + 4 * (lq & 2);  // 8 columns from here
            if (row < mlim && col < p.N) *(uint4*)((u16*)p.C + (size_t)row * p.ldc + col) = make_uint4(u[0].x, u[0].y, u[1].x, u[1].y);
          }
        }
        return;
      }
    }
    if constexpr (EPI == WM_EPI_RESID) {
      // in-place X += gamma * (acc + bias): the old values of row group i + 1 are requested before row group i is stored
      float4 old[2][SN];
      auto load_old = [&](int i, float4 (&o)[SN]) {
        const int row = rowb + i * 16 + l15;
#pragma unroll
        for (int j = 0; j < SN; ++j) {
          const int col = colb + j * 16 + 4 * lq;
          o[j] = (row < mlim && col < p.N) ? *(const float4*)((const float*)p.C + (size_t)row * p.ldc + col) : make_float4(0, 0, 0, 0);
        }
      };
      load_old(0, old[0]);
#pragma unroll
      for (int i = 0; i < SM; ++i) {
        if (rowb + i * 16 >= mlim) break;  // wave-uniform: the rest of the wave's rows are past the band / matrix end
        if (i + 1 < SM) load_old(i + 1, old[(i + 1) & 1]);
        const int row = rowb + i * 16 + l15;
#pragma unroll
        for (int j = 0; j < SN; ++j) {
          const int col = colb + j * 16 + 4 * lq;
          const float4 o = old[i & 1][j], gm = gm4[j], bs = bs4[j];
          if (row < mlim && col < p.N) {
            const float4 nv = make_float4(o.x + gm.x * (acc[i][j][0] + bs.x), o.y + gm.y * (acc[i][j][1] + bs.y), o.z + gm.z * (acc[i][j][2] + bs.z), o.w + gm.w * (acc[i][j][3] + bs.w));
            *(float4*)((float*)p.C + (size_t)row * p.ldc + col) = nv;
            if (p.C2) *(float4*)(p.C2 + (size_t)row * p.ldc2 + col) = nv;  // tap half (block-uniform branch)
          }
        }
      }
      return;
    }
    if constexpr (EPI == WM_EPI_CONV) {
      // y = acc + bias + relu?(resid) + resid2 (ResidualConvUnit skip and fusion add, dense_head.py:435-455), optional ReLU; fp32 NHWC, or
      // 16-bit when the only consumer rounds to the operand type anyway.  The residuals of row group i + 1 are requested before row
      // group i is stored (the output may alias neither).
      // token-conv form: row = token (n, i, j), this column tile = phase (a, b): the output row is pixel (k i + a, k j + b) and the tile's
      // 256 columns are the channels (the ConvTranspose's depth-to-space, dense_head.py:57-66, composed with the 3x3 conv behind it)
      auto out_row = [&](int row) -> size_t {
        if (p.tc_k <= 0) return (size_t)row;
        const int hw = p.cv_h * p.cv_w, n = row / hw, rem = row - n * hw, ti = rem / p.cv_w, tj = rem - ti * p.cv_w;
        const int ph = colb / 256, a = ph / p.tc_k, b = ph - a * p.tc_k;
        return ((size_t)(n * p.cv_h + ti) * p.tc_k + a) * (size_t)(p.cv_w * p.tc_k) + (size_t)(tj * p.tc_k + b);
      };
      const int cshift = p.tc_k > 0 ? (colb / 256) * 256 : 0;
      float4 rs[2][SN], r2[2][SN];
      auto load_res = [&](int i, float4 (&a)[SN], float4 (&b)[SN]) {
        const int row = rowb + i * 16 + l15;
#pragma unroll
        for (int j = 0; j < SN; ++j) {
          const int col = colb + j * 16 + 4 * lq;
          const bool ok = row < mlim && col < p.N;
          a[j] = (p.cv_resid && ok) ? *(const float4*)(p.cv_resid + (size_t)row * p.ldc + col) : make_float4(0, 0, 0, 0);
          b[j] = (p.cv_resid2 && ok) ? *(const float4*)(p.cv_resid2 + (size_t)row * p.ldc + col) : make_float4(0, 0, 0, 0);
        }
      };
      load_res(0, rs[0], r2[0]);
#pragma unroll
      for (int i = 0; i < SM; ++i) {
        if (rowb + i * 16 >= mlim) break;
        if (i + 1 < SM) load_res(i + 1, rs[(i + 1) & 1], r2[(i + 1) & 1]);
        const int row = rowb + i * 16 + l15;
        float4 y[SN];
#pragma unroll
        for (int j = 0; j < SN; ++j) {
          float4 a = rs[i & 1][j];
          if (p.cv_resid_relu) a = make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f));
          const float4 b = r2[i & 1][j], bs = bs4[j];
          y[j] = make_float4(acc[i][j][0] + bs.x + a.x + b.x, acc[i][j][1] + bs.y + a.y + b.y, acc[i][j][2] + bs.z + a.z + b.z, acc[i][j][3] + bs.w + a.w + b.w);
          if (p.relu) y[j] = make_float4(fmaxf(y[j].x, 0.f), fmaxf(y[j].y, 0.f), fmaxf(y[j].z, 0.f), fmaxf(y[j].w, 0.f));
        }
        if (p.out16) {
          if constexpr (SN % 2 == 0) {
#pragma unroll
            for (int jp = 0; jp < SN / 2; ++jp) {
              uint2 u[2];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const float4 x = y[2 * jp + h];
                u[h].x = (uint32_t)f2t<T>(x.x) | ((uint32_t)f2t<T>(x.y) << 16);
                u[h].y = (uint32_t)f2t<T>(x.z) | ((uint32_t)f2t<T>(x.w) << 16);
              }
              swap16(u[0].x, u[1].x);
              swap16(u[0].y, u[1].y);
              const int col = colb + (2 * jp + (lq & 1)) * 16 + 4 * (lq & 2);
              if (row < mlim && col < p.N) *(uint4*)((u16*)p.C + out_row(row) * p.ldc + col - cshift) = make_uint4(u[0].x, u[0].y, u[1].x, u[1].y);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < SN; ++j) {
            const int col = colb + j * 16 + 4 * lq;
            if (row < mlim && col < p.N) *(float4*)((float*)p.C + out_row(row) * p.ldc + col - cshift) = y[j];
          }
        }
      }
      return;
    }
    if constexpr (EPI == WM_EPI_ROWMAP_ADD) {
      // acc + bias, ReLU?, + add[row inside its group][col], into the remapped row (and, with split_n, the column's own slice tensor)
#pragma unroll
      for (int i = 0; i < SM; ++i) {
        if (rowb + i * 16 >= mlim) break;
        const int row = rowb + i * 16 + l15;
        if (row >= mlim) continue;
        const int gI = row / p.rows_per_group, q = row - gI * p.rows_per_group;
        const size_t orow = (size_t)gI * p.out_group + p.out_off + q;
#pragma unroll
        for (int j = 0; j < SN; ++j) {
          int col = colb + j * 16 + 4 * lq, addn = p.N;
          if (col >= p.N) continue;
          void* Cb = p.C;
          if (p.split_n > 0) rowmap_slice(p, col, addn, Cb);
          const float4 bs = bs4[j];
          float4 x = make_float4(acc[i][j][0] + bs.x, acc[i][j][1] + bs.y, acc[i][j][2] + bs.z, acc[i][j][3] + bs.w);
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
      return;
    }
#pragma unroll
    for (int i = 0; i < SM; ++i) {
      if (rowb + i * 16 >= mlim) break;  // wave-uniform: the rest of the wave's rows are past the band / matrix end
      const int row = rowb + i * 16 + l15;
      if (row >= mlim) continue;
#pragma unroll
      for (int j = 0; j < SN; ++j) {
        const int col = colb + j * 16 + 4 * lq;
        if (col >= p.N) continue;
        const float4 bs = bs4[j];
        float4 x = make_float4(acc[i][j][0] + bs.x, acc[i][j][1] + bs.y, acc[i][j][2] + bs.z, acc[i][j][3] + bs.w);
        const size_t o = (size_t)row * p.ldc + col;
        if constexpr (EPI == WM_EPI_F32) {
          *(float4*)((float*)p.C + o) = x;
        } else if constexpr (EPI == WM_EPI_T16 || EPI == WM_EPI_GELU_T16) {
          if constexpr (EPI == WM_EPI_GELU_T16) x = gelu_erf4(x);
          uint2 u;
          u.x = (uint32_t)f2t<T>(x.x) | ((uint32_t)f2t<T>(x.y) << 16);
          u.y = (uint32_t)f2t<T>(x.z) | ((uint32_t)f2t<T>(x.w) << 16);
          *(uint2*)((u16*)p.C + o) = u;
        }
      }
    }
  }
}

}  // namespace
