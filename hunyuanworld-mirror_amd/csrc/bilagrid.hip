// Bilateral-grid appearance correction of the post-3DGS trainer (gsplat's examples/lib_bilagrid.py: slice :180-244 through
// BilateralGrid.forward :310-365 and color_affine_transform :141-154; total_variation_loss :161-177), forward and backward.
//
// slice.  grids [G,12,L,Hg,Wg] hold a 3 x 4 affine colour matrix per cell (channel 4 r + c = entry (r, c)).  A sample (x, y, rgb) of
// row b reads grid g = grid_idx[b] at (2 (x - .5), 2 (y - .5), 2 (.299 r + .587 g + .114 b) - 1) the way torch's 5-D grid_sample does
// with align_corners = True, padding_mode = "border": u = (c + 1) / 2 * (size - 1), clamped to [0, size - 1], trilinear between
// floor(u) and floor(u) + 1; d u / d c = (size - 1) / 2 strictly inside the clamp range and 0 from its ends outwards.
// out = A[:, :3] rgb + A[:, 3] with A the 12 interpolated numbers; the [.., 3, 4] matrices never reach memory.
//   forward            one sample per lane: 8 corners x 12 channels straight from the grid (98 KB at 16 x 16 x 8: L2 / L1 resident)
//   backward, rgb      one sample per lane: the same gather; v_rgb = A[:, :3]^T v_out + (L - 1) (.299, .587, .114) sum_k dA_k/du_z M_k,
//                      M = outer(v_out, [rgb, 1]), the second term only strictly inside the z clamp range
//   backward, grids    v_grids[g, k, cell] = sum over the samples of the rows naming g of weight(cell, sample) M_k(sample): hundreds of
//                      thousands of samples into 12 L Hg Wg numbers without atomics.  A block of 1024 threads takes one segment of one
//                      row; thread t owns cells t, t + 1024, .. (WM_BILAGRID_MAX_CELLS = 4096 cells: at most four per thread, the 12
//                      accumulators of each in registers for the whole segment).  The segment goes through LDS 512 samples at a time:
//                      coordinates, M, and per sample the 64-bit set of slots (64 consecutive cells = one wave's cells of one pass) its
//                      at most 8 corners fall into.  Every wave compacts, per slot it owns, the samples that touch the slot into a list
//                      (ballot + prefix count: sample order is kept) and walks only that list, every lane evaluating its own cell's
//                      weight (zero for all but the sample's corners) and adding weight * M_k.  At 16 x 16 x 8 a sample touches 2 - 4 of
//                      the 32 slots.  Per block the 12 x cells partial sums go to the workspace; a second kernel adds, per grid
//                      element, the partials of the rows that name its grid in (row, segment) order, and writes every element (zeros
//                      for a grid no row names).
// Order of every sum: fixed by the shapes alone (sample order inside a segment, then row, then segment), no atomics of any kind:
// identical bits run to run.
// A row whose index is outside [0, G) dereferences nothing: its outputs and its v_rgb are NaN, it adds nothing to v_grids.
//
// total variation of x [B,C,L,H,W]: sum over the three trailing axes of sum (first differences)^2 / (C L H W with that axis one
// shorter, at least 1), over B.  Value: squares in fp32 as the reference forms them, sums in fp64, one partial per block, one small
// kernel adds them in index order.  Gradient: one pass, 2 / count (x_e - x_{e-1}) - 2 / count (x_{e+1} - x_e) per axis, times g / B.
#include <algorithm>

#include "wm_common.h"
#include "wm_kernels.h"

namespace {

constexpr int BG_THREADS = 256;                       // forward, rgb backward, TV
constexpr int BG_GT = 1024, BG_GW = BG_GT / 64;       // grid backward: threads, waves
constexpr int BG_RUN = 512;                           // samples staged at a time
constexpr int BG_PMAX = 4;                            // cells per thread
constexpr int BG_TV_BLOCKS_MAX = 1024;

struct BgGeom {
  int G, L, Hg, Wg, B, n;
};

// the sample's place along one axis: u clamped, i0 = floor(u) in [0, size - 1], t = u - i0; inside: strictly within the clamp range
struct BgAxis {
  int i0;
  float t;
  bool inside;
};

__device__ __forceinline__ BgAxis bg_axis(float c, int size) {
  const float top = (float)(size - 1);
  const float raw = (c + 1.f) * 0.5f * top;
  const float u = fminf(fmaxf(raw, 0.f), top);        // NaN -> 0
  BgAxis a;
  a.i0 = min(max((int)floorf(u), 0), size - 1);
  a.t = u - (float)a.i0;
  a.inside = raw > 0.f && raw < top;
  return a;
}

__device__ __forceinline__ float bg_guidance(float r, float g, float b) { return (0.299f * r + 0.587f * g + 0.114f * b) * 2.f - 1.f; }

// A[k] = trilinear lookup of channel k; dAz[k] = d A[k] / d u_z (the interpolation's own slope along z, before any clamp rule)
template <bool WANT_DZ>
__device__ __forceinline__ void bg_gather(const float* __restrict__ grid, const BgGeom& g, const BgAxis& ax, const BgAxis& ay, const BgAxis& az,
                                          float* A, float* dAz) {
  const int x1 = min(ax.i0 + 1, g.Wg - 1), y1 = min(ay.i0 + 1, g.Hg - 1), z1 = min(az.i0 + 1, g.L - 1);
  const int plane = g.Hg * g.Wg, cells = g.L * plane;
  const int o00 = ay.i0 * g.Wg + ax.i0, o01 = ay.i0 * g.Wg + x1, o10 = y1 * g.Wg + ax.i0, o11 = y1 * g.Wg + x1;
  const float* p0 = grid + az.i0 * plane;
  const float* p1 = grid + z1 * plane;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    // nested a + t (b - a): a field that is constant over the cell comes back exactly (identity grids return rgb itself)
    const float a0 = p0[o00] + ax.t * (p0[o01] - p0[o00]), b0 = p0[o10] + ax.t * (p0[o11] - p0[o10]);
    const float a1 = p1[o00] + ax.t * (p1[o01] - p1[o00]), b1 = p1[o10] + ax.t * (p1[o11] - p1[o10]);
    const float lo = a0 + ay.t * (b0 - a0), hi = a1 + ay.t * (b1 - a1);
    A[k] = lo + az.t * (hi - lo);
    if (WANT_DZ) dAz[k] = hi - lo;
    p0 += cells; p1 += cells;
  }
}

__global__ __launch_bounds__(BG_THREADS) WM_NO_PACKED_FP32 void bg_slice_fwd_kernel(const float* __restrict__ grids, BgGeom g,
                                                                                    const int* __restrict__ grid_idx,
                                                                                    const float* __restrict__ xy, const float* __restrict__ rgb,
                                                                                    float* __restrict__ out, int blocks_per_row) {
  const int b = blockIdx.x / blocks_per_row;
  const int s = (blockIdx.x - b * blocks_per_row) * BG_THREADS + threadIdx.x;
  if (s >= g.n) return;
  const size_t e = (size_t)b * g.n + s;
  const int gi = grid_idx[b];
  if (gi < 0 || gi >= g.G) {
    const float q = __builtin_nanf("");
    out[3 * e] = q; out[3 * e + 1] = q; out[3 * e + 2] = q;
    return;
  }
  const float r = rgb[3 * e], gr = rgb[3 * e + 1], bl = rgb[3 * e + 2];
  const BgAxis ax = bg_axis((xy[2 * e] - 0.5f) * 2.f, g.Wg), ay = bg_axis((xy[2 * e + 1] - 0.5f) * 2.f, g.Hg);
  const BgAxis az = bg_axis(bg_guidance(r, gr, bl), g.L);
  float A[12];
  bg_gather<false>(grids + (size_t)gi * 12 * g.L * g.Hg * g.Wg, g, ax, ay, az, A, nullptr);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[3 * e + i] = A[4 * i] * r + A[4 * i + 1] * gr + A[4 * i + 2] * bl + A[4 * i + 3];
}

__global__ __launch_bounds__(BG_THREADS) WM_NO_PACKED_FP32 void bg_slice_bwd_rgb_kernel(const float* __restrict__ grids, BgGeom g,
                                                                                        const int* __restrict__ grid_idx,
                                                                                        const float* __restrict__ xy, const float* __restrict__ rgb,
                                                                                        const float* __restrict__ v_out, float* __restrict__ v_rgb,
                                                                                        int blocks_per_row) {
  const int b = blockIdx.x / blocks_per_row;
  const int s = (blockIdx.x - b * blocks_per_row) * BG_THREADS + threadIdx.x;
  if (s >= g.n) return;
  const size_t e = (size_t)b * g.n + s;
  const int gi = grid_idx[b];
  if (gi < 0 || gi >= g.G) {
    const float q = __builtin_nanf("");
    v_rgb[3 * e] = q; v_rgb[3 * e + 1] = q; v_rgb[3 * e + 2] = q;
    return;
  }
  const float c[4] = {rgb[3 * e], rgb[3 * e + 1], rgb[3 * e + 2], 1.f};
  const float v[3] = {v_out[3 * e], v_out[3 * e + 1], v_out[3 * e + 2]};
  const BgAxis ax = bg_axis((xy[2 * e] - 0.5f) * 2.f, g.Wg), ay = bg_axis((xy[2 * e + 1] - 0.5f) * 2.f, g.Hg);
  const BgAxis az = bg_axis(bg_guidance(c[0], c[1], c[2]), g.L);
  float A[12], dAz[12];
  bg_gather<true>(grids + (size_t)gi * 12 * g.L * g.Hg * g.Wg, g, ax, ay, az, A, dAz);
  float slope = 0.f;          // d (v_out . out) / d u_z
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) slope += dAz[4 * i + j] * (v[i] * c[j]);
  // u_z = (z + 1) / 2 (L - 1), z = 2 (w . rgb) - 1  ->  d u_z / d rgb_j = (L - 1) w_j
  const float gz = az.inside ? slope * (float)(g.L - 1) : 0.f;
  const float wj[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int j = 0; j < 3; ++j) v_rgb[3 * e + j] = A[j] * v[0] + A[4 + j] * v[1] + A[8 + j] * v[2] + gz * wj[j];
}

// ---------------------------------------------------------------------------------------------------------------- grid backward
struct BgGridArgs {
  const int* grid_idx; const float* xy; const float* rgb; const float* v_out;
  BgGeom g;
  int nseg, seglen;          // segments per row, samples per segment (a multiple of BG_RUN)
  float* partials;           // [B * nseg][12][cells]
};

__device__ __forceinline__ float bg_w1(int d, float t) { return d == 0 ? 1.f - t : (d == 1 ? t : 0.f); }

template <int P>
__global__ __launch_bounds__(BG_GT) WM_NO_PACKED_FP32 void bg_grid_partial_kernel(BgGridArgs a) {
  __shared__ float4 sC[BG_RUN];                          // bits of (x0 | y0 << 10 | z0 << 20), tx, ty, tz
  __shared__ float4 sM[BG_RUN][3];                       // outer(v_out, [rgb, 1]), row-major
  __shared__ unsigned long long sMask[BG_RUN];           // slots the sample's corners fall into
  __shared__ unsigned short sList[P * BG_GW][BG_RUN];    // per slot: the samples that touch it, in sample order
  const BgGeom g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.nseg, seg = blockIdx.x - b * a.nseg;
  const int gi = a.grid_idx[b];
  if (gi < 0 || gi >= g.G) return;                       // block-uniform, before any barrier; the reducer never reads this row
  const int plane = g.Hg * g.Wg, cells = g.L * plane;
  int vx[P], vy[P], vz[P];
  float acc[P][12];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int cell = p * BG_GT + tid;
    vx[p] = cell % g.Wg; vy[p] = (cell / g.Wg) % g.Hg;
    vz[p] = cell < cells ? cell / plane : (1 << 20);     // beyond the grid: matches no sample
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[p][k] = 0.f;
  }
  const int s_begin = min(seg * a.seglen, g.n), s_end = min(s_begin + a.seglen, g.n);
  for (int run = s_begin; run < s_end; run += BG_RUN) {
    const int cnt = min(BG_RUN, s_end - run);
    if (tid < cnt) {
      const size_t e = (size_t)b * g.n + run + tid;
      const float c[4] = {a.rgb[3 * e], a.rgb[3 * e + 1], a.rgb[3 * e + 2], 1.f};
      const float v[3] = {a.v_out[3 * e], a.v_out[3 * e + 1], a.v_out[3 * e + 2]};
      const BgAxis ax = bg_axis((a.xy[2 * e] - 0.5f) * 2.f, g.Wg), ay = bg_axis((a.xy[2 * e + 1] - 0.5f) * 2.f, g.Hg);
      const BgAxis az = bg_axis(bg_guidance(c[0], c[1], c[2]), g.L);
      sC[tid] = make_float4(__int_as_float(ax.i0 | (ay.i0 << 10) | (az.i0 << 20)), ax.t, ay.t, az.t);
#pragma unroll
      for (int i = 0; i < 3; ++i) sM[tid][i] = make_float4(v[i] * c[0], v[i] * c[1], v[i] * c[2], v[i]);
      unsigned long long m = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int x = ax.i0 + (q & 1), y = ay.i0 + ((q >> 1) & 1), z = az.i0 + (q >> 2);
        if (x < g.Wg && y < g.Hg && z < g.L) m |= 1ull << (((z * g.Hg + y) * g.Wg + x) >> 6);     // cell < 4096: slot < 64
      }
      sMask[tid] = m;
    }
    __syncthreads();
    int nl[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int slot = p * BG_GW + wave;
      int count = 0;
      for (int base = 0; base < cnt; base += 64) {       // wave-uniform trip count
        const int s = base + lane;
        const bool hit = s < cnt && ((sMask[s < cnt ? s : 0] >> slot) & 1ull);
        const unsigned long long bal = __ballot(hit);
        if (hit) sList[slot][count + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)s;
        count += __popcll(bal);
      }
      nl[p] = count;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int slot = p * BG_GW + wave;
      for (int i = 0; i < nl[p]; ++i) {
        const int s = sList[slot][i];                    // the same for every lane
        const float4 c = sC[s];
        const int key = __float_as_int(c.x);
        const float w = bg_w1(vx[p] - (key & 1023), c.y) * bg_w1(vy[p] - ((key >> 10) & 1023), c.z) * bg_w1(vz[p] - (key >> 20), c.w);
        const float4 m0 = sM[s][0], m1 = sM[s][1], m2 = sM[s][2];
        acc[p][0] = fmaf(w, m0.x, acc[p][0]); acc[p][1] = fmaf(w, m0.y, acc[p][1]); acc[p][2] = fmaf(w, m0.z, acc[p][2]);
        acc[p][3] = fmaf(w, m0.w, acc[p][3]); acc[p][4] = fmaf(w, m1.x, acc[p][4]); acc[p][5] = fmaf(w, m1.y, acc[p][5]);
        acc[p][6] = fmaf(w, m1.z, acc[p][6]); acc[p][7] = fmaf(w, m1.w, acc[p][7]); acc[p][8] = fmaf(w, m2.x, acc[p][8]);
        acc[p][9] = fmaf(w, m2.y, acc[p][9]); acc[p][10] = fmaf(w, m2.z, acc[p][10]); acc[p][11] = fmaf(w, m2.w, acc[p][11]);
      }
    }
    __syncthreads();                                     // the next run overwrites sC / sM / sMask / sList
  }
  float* dst = a.partials + (size_t)blockIdx.x * 12 * cells;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int cell = p * BG_GT + tid;
    if (cell < cells) {
#pragma unroll
      for (int k = 0; k < 12; ++k) dst[(size_t)k * cells + cell] = acc[p][k];
    }
  }
}

// v_grids[g][k][cell] = sum over rows b with grid_idx[b] == g, in row order, over that row's segments in order
__global__ __launch_bounds__(BG_THREADS) void bg_grid_reduce_kernel(const float* __restrict__ partials, const int* __restrict__ grid_idx,
                                                                    BgGeom g, int nseg, float* __restrict__ v_grids) {
  const int per_grid = 12 * g.L * g.Hg * g.Wg;
  const size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= (size_t)g.G * per_grid) return;
  const int gi = (int)(e / per_grid), r = (int)(e - (size_t)gi * per_grid);
  float sum = 0.f;
  for (int b = 0; b < g.B; ++b) {
    if (grid_idx[b] != gi) continue;
    const float* p = partials + (size_t)b * nseg * per_grid + r;
    for (int s = 0; s < nseg; ++s) sum += p[(size_t)s * per_grid];
  }
  v_grids[e] = sum;
}

// ---------------------------------------------------------------------------------------------------------------- total variation
struct BgTvGeom {
  int B, C, L, H, W;
  double inv_l, inv_h, inv_w;      // 1 / (C (L-1) H W) .., 1 / max(count, 1): an axis of length 1 has no differences
};

__global__ __launch_bounds__(BG_THREADS) WM_NO_PACKED_FP32 void bg_tv_kernel(const float* __restrict__ x, BgTvGeom t, double* __restrict__ partials) {
  __shared__ double sRed[BG_THREADS];
  const size_t total = (size_t)t.B * t.C * t.L * t.H * t.W;
  const size_t sw = 1, sh = t.W, sl = (size_t)t.H * t.W;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * BG_THREADS) {
    const int w = (int)(e % t.W), h = (int)((e / sh) % t.H), l = (int)((e / sl) % t.L);
    const float v = x[e];
    if (w + 1 < t.W) { const float d = x[e + sw] - v; acc += (double)(d * d) * t.inv_w; }
    if (h + 1 < t.H) { const float d = x[e + sh] - v; acc += (double)(d * d) * t.inv_h; }
    if (l + 1 < t.L) { const float d = x[e + sl] - v; acc += (double)(d * d) * t.inv_l; }
  }
  // every thread reaches the tree: no return above it
  sRed[threadIdx.x] = acc;
  __syncthreads();
  for (int h = BG_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sRed[threadIdx.x] += sRed[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sRed[0];
}

__global__ __launch_bounds__(BG_THREADS) void bg_tv_reduce_kernel(const double* __restrict__ partials, int nblk, double inv_b, float* out) {
  __shared__ double sRed[BG_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nblk; i += BG_THREADS) s += partials[i];
  sRed[tid] = s;
  __syncthreads();
  for (int h = BG_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) sRed[tid] += sRed[tid + h];
    __syncthreads();
  }
  if (tid == 0) *out = (float)(sRed[0] * inv_b);
}

__global__ __launch_bounds__(BG_THREADS) WM_NO_PACKED_FP32 void bg_tv_bwd_kernel(const float* __restrict__ x, BgTvGeom t, const float* __restrict__ gout,
                                                                                 float* __restrict__ v_x) {
  const size_t total = (size_t)t.B * t.C * t.L * t.H * t.W;
  const size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= total) return;
  const size_t sw = 1, sh = t.W, sl = (size_t)t.H * t.W;
  const int w = (int)(e % t.W), h = (int)((e / sh) % t.H), l = (int)((e / sl) % t.L);
  const float v = x[e];
  double d = 0.0;
  if (w > 0) d += (double)(v - x[e - sw]) * t.inv_w;
  if (w + 1 < t.W) d -= (double)(x[e + sw] - v) * t.inv_w;
  if (h > 0) d += (double)(v - x[e - sh]) * t.inv_h;
  if (h + 1 < t.H) d -= (double)(x[e + sh] - v) * t.inv_h;
  if (l > 0) d += (double)(v - x[e - sl]) * t.inv_l;
  if (l + 1 < t.L) d -= (double)(x[e + sl] - v) * t.inv_l;
  v_x[e] = (float)(2.0 * d * (double)*gout / (double)t.B);
}

bool bg_geom_ok(const WmBilagridArgs& a) {
  if (a.G <= 0 || a.L <= 0 || a.Hg <= 0 || a.Wg <= 0 || a.B <= 0 || a.n <= 0) return false;
  if (a.L > 1024 || a.Hg > 1024 || a.Wg > 1024) return false;          // ten bits per axis in the staged key
  if ((long long)a.L * a.Hg * a.Wg > WM_BILAGRID_MAX_CELLS) return false;
  if ((long long)a.B * a.n >= (1LL << 31) / 4) return false;
  return true;
}

BgGeom bg_geom(const WmBilagridArgs& a) { return BgGeom{a.G, a.L, a.Hg, a.Wg, a.B, a.n}; }

// segments per row and samples per segment: about one block per CU over all rows, a segment a whole number of runs
void bg_segments(int B, int n, int& nseg, int& seglen) {
  const int runs = (n + BG_RUN - 1) / BG_RUN;
  nseg = std::max(1, std::min(runs, 256 / B));
  seglen = ((runs + nseg - 1) / nseg) * BG_RUN;
  nseg = (n + seglen - 1) / seglen;          // no segment without samples
}

bool bg_tv_geom(int B, int C, int L, int H, int W, BgTvGeom& t, long long& total) {
  if (B <= 0 || C <= 0 || L <= 0 || H <= 0 || W <= 0) return false;
  total = (long long)B * C * L * H * W;
  if (total >= (1LL << 31)) return false;
  auto inv = [](double c) { return 1.0 / (c > 1.0 ? c : 1.0); };
  t.B = B; t.C = C; t.L = L; t.H = H; t.W = W;
  t.inv_l = inv((double)C * (L - 1) * H * W); t.inv_h = inv((double)C * L * (H - 1) * W); t.inv_w = inv((double)C * L * H * (W - 1));
  return true;
}

int bg_tv_blocks(long long total) { return (int)std::min<long long>((total + BG_THREADS - 1) / BG_THREADS, BG_TV_BLOCKS_MAX); }

}  // namespace

size_t wm_bilagrid_bwd_workspace_bytes(int G, int L, int Hg, int Wg, int B, int n) {
  WmBilagridArgs a{};
  a.G = G; a.L = L; a.Hg = Hg; a.Wg = Wg; a.B = B; a.n = n;
  if (!bg_geom_ok(a)) return 0;
  int nseg, seglen;
  bg_segments(B, n, nseg, seglen);
  return (size_t)B * nseg * 12 * L * Hg * Wg * sizeof(float);
}

hipError_t wm_launch_bilagrid_slice(const WmBilagridArgs& a, float* out, hipStream_t s) {
  if (!bg_geom_ok(a)) return hipErrorInvalidValue;
  const int bpr = (a.n + BG_THREADS - 1) / BG_THREADS;
  hipLaunchKernelGGL(bg_slice_fwd_kernel, dim3((unsigned)(a.B * bpr)), dim3(BG_THREADS), 0, s, a.grids, bg_geom(a), a.grid_idx, a.xy, a.rgb, out, bpr);
  return hipGetLastError();
}

hipError_t wm_launch_bilagrid_slice_bwd(const WmBilagridArgs& a, const float* v_out, float* v_grids, float* v_rgb, void* ws, size_t ws_bytes,
                                        hipStream_t s) {
  if (!bg_geom_ok(a)) return hipErrorInvalidValue;
  const BgGeom g = bg_geom(a);
  if (v_grids && (!ws || ws_bytes < wm_bilagrid_bwd_workspace_bytes(a.G, a.L, a.Hg, a.Wg, a.B, a.n))) return hipErrorInvalidValue;
  if (v_rgb) {
    const int bpr = (a.n + BG_THREADS - 1) / BG_THREADS;
    hipLaunchKernelGGL(bg_slice_bwd_rgb_kernel, dim3((unsigned)(a.B * bpr)), dim3(BG_THREADS), 0, s, a.grids, g, a.grid_idx, a.xy, a.rgb, v_out, v_rgb,
                       bpr);
  }
  if (v_grids) {
    BgGridArgs k;
    k.grid_idx = a.grid_idx; k.xy = a.xy; k.rgb = a.rgb; k.v_out = v_out; k.g = g; k.partials = (float*)ws;
    bg_segments(a.B, a.n, k.nseg, k.seglen);
    const int cells = a.L * a.Hg * a.Wg, P = (cells + BG_GT - 1) / BG_GT;
    const dim3 grid((unsigned)(a.B * k.nseg)), block(BG_GT);
    if (P == 1) hipLaunchKernelGGL(bg_grid_partial_kernel<1>, grid, block, 0, s, k);
    else if (P == 2) hipLaunchKernelGGL(bg_grid_partial_kernel<2>, grid, block, 0, s, k);
    else if (P == 3) hipLaunchKernelGGL(bg_grid_partial_kernel<3>, grid, block, 0, s, k);
    else hipLaunchKernelGGL(bg_grid_partial_kernel<BG_PMAX>, grid, block, 0, s, k);
    const size_t total = (size_t)a.G * 12 * cells;
    hipLaunchKernelGGL(bg_grid_reduce_kernel, dim3((unsigned)((total + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, s, (const float*)ws,
                       a.grid_idx, g, k.nseg, v_grids);
  }
  return hipGetLastError();
}

size_t wm_bilagrid_tv_ws_bytes(int B, int C, int L, int H, int W) {
  BgTvGeom t;
  long long total;
  if (!bg_tv_geom(B, C, L, H, W, t, total)) return 0;
  return (size_t)bg_tv_blocks(total) * sizeof(double);
}

hipError_t wm_launch_bilagrid_tv(const float* x, int B, int C, int L, int H, int W, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  BgTvGeom t;
  long long total;
  if (!bg_tv_geom(B, C, L, H, W, t, total)) return hipErrorInvalidValue;
  const int nblk = bg_tv_blocks(total);
  if (!ws || ws_bytes < (size_t)nblk * sizeof(double)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bg_tv_kernel, dim3(nblk), dim3(BG_THREADS), 0, s, x, t, (double*)ws);
  hipLaunchKernelGGL(bg_tv_reduce_kernel, dim3(1), dim3(BG_THREADS), 0, s, (const double*)ws, nblk, 1.0 / B, out);
  return hipGetLastError();
}

hipError_t wm_launch_bilagrid_tv_bwd(const float* x, int B, int C, int L, int H, int W, const float* g, float* v_x, hipStream_t s) {
  BgTvGeom t;
  long long total;
  if (!bg_tv_geom(B, C, L, H, W, t, total)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bg_tv_bwd_kernel, dim3((unsigned)((total + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, s, x, t, g, v_x);
  return hipGetLastError();
}
