// The fly-through video around the rasteriser (reference: src/utils/render_utils.py:196-368 render_interpolated_video and
// src/utils/gs_effects.py:162-242 GSEffects.apply_effect).  Two parts, both HBM-bound with no matrix work:
//
//  * gs_effect_spread_kernel: apply_effect's effect_type 2 in one pass over the Gaussians (the reference: about 40 torch launches), with the
//    driver's composition around it folded in: (means - shift) * inv_scale and scales * inv_scale on the way in (render_utils.py:230), degree-0
//    SH in and out (SH2RGB :231, RGB2SH :234).  Beside the five outputs and flag (the reference's smoothstep_val) it leaves the two numbers
//    the driver reads each frame, the count of flag < 0.99 (:228) and the sum of flag (:281), through a fixed-order two-stage reduction:
//    per block a tree over 256 lanes (count in integers, sum in fp64), then one block over the partials.  Same input, same bits.
//    The reference's 8-corner hash noise is not evaluated: its result is multiplied by 0.0 (gs_effects.py:218), which only shows for a
//    non-finite position (0 * inf), and those are out of contract.
//
//  * the frame pass: per frame near = log(quantile(d[d > 0], 0.01)) (0.0 where no pixel is valid) and far = log(quantile(d, 0.99)) as
//    torch.quantile gives them (render_utils.py:326-332) by an exact order-statistic selection, then the turbo colour map in bytes
//    (:333-335, color_map.py:11-21, _make_video :355-357), and the colour frames' clamp * 255 -> uint8.
//    Selection: the 4 x 8-bit radix select of pointmask.hip, with four targets per frame (the two neighbours of either rank) and the
//    masked subset selected in place: a pixel with d <= 0 simply does not count in the near histograms, nothing is compacted.  One
//    histogram launch per digit covers every frame (blockIdx.y = frame).  The near rank depends on the number of valid pixels, which the
//    first digit's histogram gives, so the ranks are set on the device by the first pick.  Histogram counts are integer adds (LDS, then
//    one global add per bin and block): their result does not depend on the order.
//    torch.quantile, linear: rank = q * (n - 1) as an fp32 product of the fp32 q, below = floor, above = ceil, weight = rank - below,
//    value = lerp(below, above, weight) = weight < 0.5 ? a + weight (b - a) : b - (b - a)(1 - weight), the multiply-add fused as in
//    torch's kernels.  The log is taken in fp64 and rounded once.
//    pointmask.hip's select keeps its own helpers: its lerp is numpy's (no FMA, gamma >= 0.5 on the other side) and it counts NaN, so a
//    shared header would have to change its code; here NaN depths are out of contract.
#include "wm_api.h"
#include "scene_common.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ spread effect
constexpr float FX_SH_C0 = 0.28209479177387814f;

struct FxArgs {
  const float* means;      // [N][3]
  const float* scales;     // [N][3]
  const float* opacities;  // [N]
  const float* colors;     // [N][3] rgb, or degree-0 SH when is_sh
  const float* random_vals;  // [N]
  const float* shift;      // [3] on the device, or null
  float* out_means;
  float* out_scales;
  float* out_opacities;
  float* out_colors;
  float* flag;
  unsigned long long* part_count;  // [blocks]
  double* part_sum;                // [blocks]
  long long N;
  float inv_scale;
  float s, edge0, width;   // s = smoothstep(0, 10, t_n - 3.2) * 10; smoothstep(s - 0.5, s, .): edge0 = s - 0.5, width = s - (s - 0.5)
  float t_n, t_edge;       // t_n and t_n - 3.1416 (taken in fp64), as fp32
  int ignore_scale, is_sh;
};

__global__ __launch_bounds__(256) void gs_effect_spread_kernel(const FxArgs a) {
  __shared__ double ssum[256];
  __shared__ unsigned int scnt[256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float fl = 0.f;
  unsigned int below = 0;
  if (i < a.N) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (a.shift) { sx = a.shift[0]; sy = a.shift[1]; sz = a.shift[2]; }
    const float k = a.inv_scale;
    const float x = (a.means[3 * i] - sx) * k, y = (a.means[3 * i + 1] - sy) * k, z = (a.means[3 * i + 2] - sz) * k;
    float c0 = a.colors[3 * i], c1 = a.colors[3 * i + 1], c2 = a.colors[3 * i + 2];
    if (a.is_sh) { c0 = c0 * FX_SH_C0 + 0.5f; c1 = c1 * FX_SH_C0 + 0.5f; c2 = c2 * FX_SH_C0 + 0.5f; }
    float s0 = a.scales[3 * i] * k, s1 = a.scales[3 * i + 1] * k, s2 = a.scales[3 * i + 2] * k;
    float op = a.opacities[i];

    const float l = __builtin_sqrtf(x * x + z * z);
    const float border = fabsf(a.s - l - 0.5f);
    const float e20 = expf(-20.f * border);
    const float decay = 1.f - 0.2f * e20;
    float px = x * decay, py = y * decay, pz = z * decay;
    // smoothstep(s - 0.5, s, l + 0.5)
    const float u = l + 0.5f;
    if (u < a.edge0) fl = 0.f;
    else if (u > a.s) fl = 1.f;
    else { const float t = (u - a.edge0) / a.width; fl = t * t * (3.f - 2.f * t); }
    if (!a.ignore_scale) {   // mix(scales, 1e-9, flag)
      const float w = 1.f - fl, m = 1e-9f * fl;
      s0 = s0 * w + m; s1 = s1 * w + m; s2 = s2 * w + m;
    }
    const float at = atan2f(px, pz) / 3.1416f;
    const float st = a.t_edge >= at ? 1.f : 0.f;
    const float glow = e20 + expf(-50.f * fabsf(a.t_n - at - 3.1416f)) * 0.5f;
    c0 = c0 * st + glow; c1 = c1 * st + glow; c2 = c2 * st + glow;
    op = op * st + glow;
    if (!a.ignore_scale && a.random_vals[i] < fl * 0.8f) {   // the reference's `*= 0`
      px *= 0.f; py *= 0.f; pz *= 0.f;
      s0 *= 0.f; s1 *= 0.f; s2 *= 0.f;
      op *= 0.f;
    }
    if (a.is_sh) { c0 = (c0 - 0.5f) / FX_SH_C0; c1 = (c1 - 0.5f) / FX_SH_C0; c2 = (c2 - 0.5f) / FX_SH_C0; }
    a.out_means[3 * i] = px; a.out_means[3 * i + 1] = py; a.out_means[3 * i + 2] = pz;
    a.out_scales[3 * i] = s0; a.out_scales[3 * i + 1] = s1; a.out_scales[3 * i + 2] = s2;
    a.out_colors[3 * i] = c0; a.out_colors[3 * i + 1] = c1; a.out_colors[3 * i + 2] = c2;
    a.out_opacities[i] = op;
    a.flag[i] = fl;
    below = fl < 0.99f ? 1u : 0u;
  }
  ssum[threadIdx.x] = (double)fl;
  scnt[threadIdx.x] = below;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {   // fixed-order tree
    if ((int)threadIdx.x < w) {
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
      scnt[threadIdx.x] += scnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.part_sum[blockIdx.x] = ssum[0];
    a.part_count[blockIdx.x] = scnt[0];
  }
}

// stats[0] = count of flag < 0.99, stats[1] = sum of flag; lane t sums the partials t, t + 256, ... in that order, then the tree
__global__ __launch_bounds__(256) void gs_effect_stats_kernel(const unsigned long long* __restrict__ part_count, const double* __restrict__ part_sum,
                                                              long long nparts, double* __restrict__ stats) {
  __shared__ double ssum[256];
  __shared__ unsigned long long scnt[256];
  double s = 0.0;
  unsigned long long c = 0;
  for (long long p = threadIdx.x; p < nparts; p += 256) { s += part_sum[p]; c += part_count[p]; }
  ssum[threadIdx.x] = s;
  scnt[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
      scnt[threadIdx.x] += scnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { stats[0] = (double)scnt[0]; stats[1] = ssum[0]; }
}

// ------------------------------------------------------------------ per-frame quantiles (torch.quantile, linear)
struct VState {
  unsigned int prefix[4];     // targets: 0 / 1 = the neighbours of the near rank (over d > 0), 2 / 3 = of the far rank (over every pixel)
  unsigned int remaining[4];  // 1-based rank still to find inside the fixed prefix
  float weight[2];            // lerp weight of near, far
  unsigned int n_valid;
  unsigned int pad[5];
  unsigned int hist[4][256];
};

// order-preserving uint32 image of an fp32 value; -0 folds onto +0 (a sort holds them equal and either gives log = -inf)
__device__ __forceinline__ unsigned int v_key(float c) {
  return ordered_key(c == 0.f ? 0.f : c);
}

constexpr int V_EPT = 16;
constexpr int V_CHUNK = 256 * V_EPT;

__global__ __launch_bounds__(256) void v_init_kernel(VState* st) {
  VState& q = st[blockIdx.x];
  for (int t = 0; t < 4; ++t) q.hist[t][threadIdx.x] = 0;
  if (threadIdx.x < 4) { q.prefix[threadIdx.x] = 0; q.remaining[threadIdx.x] = 1; }
  if (threadIdx.x < 2) q.weight[threadIdx.x] = 0.f;
  if (threadIdx.x == 0) q.n_valid = 0;
}

// histograms of byte shift/8 of the frame's keys whose higher bits equal each target's prefix; grid (blocks, frames).  The first digit
// (shift 24) has no prefix yet and the two targets of a set coincide: only the histograms 0 (valid pixels) and 2 (all pixels) are built.
__global__ __launch_bounds__(256) void v_hist_kernel(const float* __restrict__ depth, int n, VState* st, int shift) {
  __shared__ unsigned int lh[4][256];
  for (int t = 0; t < 4; ++t) lh[t][threadIdx.x] = 0;
  __syncthreads();
  VState& q = st[blockIdx.y];
  const float* d = depth + (size_t)blockIdx.y * n;
  if (shift == 24) {
#pragma unroll
    for (int e = 0; e < V_EPT; ++e) {
      const int i = blockIdx.x * V_CHUNK + e * 256 + threadIdx.x;
      if (i < n) {
        const float v = d[i];
        const unsigned int b = v_key(v) >> 24;
        if (v > 0.f) atomicAdd(&lh[0][b], 1u);
        atomicAdd(&lh[2][b], 1u);
      }
    }
  } else {
    const unsigned int p0 = q.prefix[0], p1 = q.prefix[1], p2 = q.prefix[2], p3 = q.prefix[3];
    const unsigned int himask = ~0u << (shift + 8);
#pragma unroll
    for (int e = 0; e < V_EPT; ++e) {
      const int i = blockIdx.x * V_CHUNK + e * 256 + threadIdx.x;
      if (i < n) {
        const float v = d[i];
        const unsigned int k = v_key(v), hi = k & himask, b = (k >> shift) & 255u;
        if (v > 0.f) {
          if (hi == p0) atomicAdd(&lh[0][b], 1u);
          if (hi == p1) atomicAdd(&lh[1][b], 1u);
        }
        if (hi == p2) atomicAdd(&lh[2][b], 1u);
        if (hi == p3) atomicAdd(&lh[3][b], 1u);
      }
    }
  }
  __syncthreads();
  for (int t = 0; t < 4; ++t)
    if (lh[t][threadIdx.x]) atomicAdd(&q.hist[t][threadIdx.x], lh[t][threadIdx.x]);
}

// one block per frame: the first pick sets the ranks (the near one from the number of valid pixels), every pick walks each target's bins
// from the bottom, the last one interpolates and writes near_far[frame] = {near, far}
__global__ __launch_bounds__(256) void v_pick_kernel(VState* st, int shift, int npix, float* __restrict__ near_far) {
  __shared__ unsigned int h[4][256];
  VState& q = st[blockIdx.x];
  for (int t = 0; t < 4; ++t) h[t][threadIdx.x] = q.hist[t][threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int t = threadIdx.x, set = t >> 1, src = shift == 24 ? (t & 2) : t;
    if (shift == 24) {
      unsigned int n = (unsigned int)npix;
      if (set == 0) {
        n = 0;
        for (int b = 0; b < 256; ++b) n += h[0][b];
        if (t == 0) q.n_valid = n;
      }
      unsigned int rank = 0;
      float w = 0.f;
      if (n > 0) {
        const float r = (set == 0 ? 0.01f : 0.99f) * (float)(n - 1);   // q * (n - 1) in fp32
        const float lo = floorf(r);
        w = r - lo;
        rank = (unsigned int)((t & 1) ? ceilf(r) : lo);
        if (rank > n - 1) rank = n - 1;
      }
      q.remaining[t] = rank + 1;
      if (!(t & 1)) q.weight[set] = w;
    }
    unsigned int rem = q.remaining[t], bin = 255;
    for (int b = 0; b < 256; ++b) {
      if (h[src][b] >= rem) { bin = (unsigned int)b; break; }
      rem -= h[src][b];
    }
    q.prefix[t] |= bin << shift;
    q.remaining[t] = rem;
  }
  __syncthreads();
  for (int t = 0; t < 4; ++t) q.hist[t][threadIdx.x] = 0;
  if (shift == 0 && threadIdx.x < 2) {
    const int set = threadIdx.x;
    const float a = ordered_value(q.prefix[2 * set]), b = ordered_value(q.prefix[2 * set + 1]), w = q.weight[set];
    const float diff = b - a;
    const float v = w < 0.5f ? fmaf(w, diff, a) : fmaf(-diff, 1.f - w, b);
    float r = (float)log((double)v);
    if (set == 0 && q.n_valid == 0) r = 0.f;   // render_utils.py:331
    near_far[2 * blockIdx.x + set] = r;
  }
}

// ------------------------------------------------------------------ frames in bytes
// turbo, 256 rows, each byte = uint8(float32(row) * 255) as clamp(0, 1) * 255 -> uint8 gives it; packed r | g << 8 | b << 16
#define WM_TURBO_ROWS \
    0x3b1230, 0x421531, 0x4a1832, 0x511b34, 0x581e35, 0x5f2136, 0x652337, 0x6c2638, \
    0x722939, 0x792c3a, 0x7f2f3b, 0x85323c, 0x8b353c, 0x91373d, 0x963a3e, 0x9c3d3f, \
    0xa14040, 0xa64340, 0xab4541, 0xb04841, 0xb54b42, 0xba4e43, 0xbe5043, 0xc25343, \
    0xc75644, 0xcb5844, 0xce5b45, 0xd25e45, 0xd66045, 0xd96345, 0xdd6646, 0xe06846, \
    0xe36b46, 0xe66d46, 0xe87046, 0xeb7346, 0xed7546, 0xf07846, 0xf27a46, 0xf47d46, \
    0xf67f46, 0xf88246, 0xf98445, 0xfb8745, 0xfc8945, 0xfd8c44, 0xfd8e43, 0xfe9142, \
    0xfe9341, 0xfe9640, 0xfe983f, 0xfe9b3e, 0xfd9d3c, 0xfca03b, 0xfca239, 0xfba538, \
    0xf9a836, 0xf8aa34, 0xf6ac33, 0xf5af31, 0xf3b12f, 0xf1b42d, 0xefb62b, 0xedb92a, \
    0xebbb28, 0xe9bd26, 0xe6c025, 0xe4c223, 0xe1c421, 0xdfc620, 0xdcc91e, 0xdacb1d, \
    0xd7cd1c, 0xd4cf1b, 0xd2d11a, 0xcfd319, 0xccd518, 0xcad718, 0xc7d917, 0xc4da17, \
    0xc2dc17, 0xbfde17, 0xbde018, 0xbae118, 0xb8e319, 0xb6e41a, 0xb4e51b, 0xb1e71d, \
    0xafe81e, 0xace920, 0xa9eb22, 0xa6ec24, 0xa3ed27, 0xa0ee29, 0x9def2c, 0x9af02f, \
    0x97f132, 0x94f335, 0x91f438, 0x8df43b, 0x8af53f, 0x87f642, 0x83f746, 0x80f84a, \
    0x7cf94d, 0x79f951, 0x76fa55, 0x72fb59, 0x6ffb5d, 0x6cfc61, 0x68fc65, 0x65fd69, \
    0x62fd6d, 0x5ffd71, 0x5cfe74, 0x59fe78, 0x56fe7c, 0x53fe80, 0x50fe84, 0x4dfe87, \
    0x4bfe8b, 0x48fe8e, 0x46fe92, 0x44fe95, 0x42fe98, 0x40fd9b, 0x3efd9e, 0x3dfca1, \
    0x3bfca4, 0x3afba6, 0x39fba9, 0x37faac, 0x37f9ae, 0x36f8b1, 0x35f8b3, 0x35f7b6, \
    0x34f5b9, 0x34f4bb, 0x34f3be, 0x33f2c0, 0x33f1c3, 0x33efc5, 0x33eec8, 0x33edca, \
    0x34ebcd, 0x34eacf, 0x34e8d1, 0x35e7d4, 0x35e5d6, 0x35e3d8, 0x36e2da, 0x36e0dd, \
    0x36dedf, 0x37dce1, 0x37dae3, 0x38d8e5, 0x38d7e7, 0x38d5e8, 0x39d3ea, 0x39d1ec, \
    0x39cfed, 0x39cdef, 0x3acbf0, 0x3ac8f2, 0x3ac6f3, 0x3ac4f4, 0x3ac2f6, 0x39c0f7, \
    0x39bef8, 0x39bcf9, 0x38baf9, 0x37b7fa, 0x37b5fb, 0x36b3fb, 0x35b0fc, 0x34aefc, \
    0x33abfd, 0x32a9fd, 0x31a6fd, 0x30a3fd, 0x2fa1fe, 0x2e9efe, 0x2d9bfe, 0x2c98fe, \
    0x2b95fd, 0x2992fd, 0x288ffd, 0x278cfd, 0x2689fc, 0x2486fc, 0x2383fb, 0x2280fb, \
    0x207dfa, 0x1f7afa, 0x1e77f9, 0x1c74f8, 0x1b71f7, 0x1a6ef7, 0x186bf6, 0x1768f5, \
    0x1665f4, 0x1563f3, 0x1460f2, 0x135df1, 0x115aef, 0x1058ee, 0x0f55ed, 0x0e52ec, \
    0x0d50ea, 0x0d4de9, 0x0c4be8, 0x0b49e6, 0x0a46e5, 0x0a44e3, 0x0942e2, 0x0840e0, \
    0x083ede, 0x073cdd, 0x073adb, 0x0638d9, 0x0636d7, 0x0534d6, 0x0532d4, 0x0530d2, \
    0x042fd0, 0x042dce, 0x032bcb, 0x0329c9, 0x0328c7, 0x0226c5, 0x0224c3, 0x0223c0, \
    0x0221be, 0x011fbb, 0x011eb9, 0x011cb6, 0x011bb4, 0x0119b1, 0x0118ae, 0x0116ac, \
    0x0115a9, 0x0114a6, 0x0112a3, 0x0111a0, 0x01109d, 0x010e9a, 0x010d97, 0x010c94, \
    0x010b91, 0x010a8e, 0x01098b, 0x010887, 0x010784, 0x020681, 0x02057d, 0x02047a
__device__ const unsigned int TURBO_LUT[256] = {WM_TURBO_ROWS};
const unsigned int TURBO_LUT_HOST[256] = {WM_TURBO_ROWS};   // a __device__ array has no host storage

// 4 consecutive pixels per lane over the flat [F * H * W] range (12 output bytes = three words where the buffers are aligned)
__global__ __launch_bounds__(256) void depth_frames_kernel(const float* __restrict__ depth, const float* __restrict__ near_far, long long total, int npix,
                                                           unsigned char* __restrict__ out, int aligned) {
  __shared__ unsigned int lut[256];
  lut[threadIdx.x] = TURBO_LUT[threadIdx.x];
  __syncthreads();
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  const bool full = p0 + 4 <= total;
  float d[4];
  if (full && aligned) {
    const float4 v = *reinterpret_cast<const float4*>(depth + p0);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  } else {
    for (int j = 0; j < 4; ++j) d[j] = p0 + j < total ? depth[p0 + j] : 0.f;
  }
  unsigned int c[4];
  long long f = p0 / npix;
  long long next = (f + 1) * npix;   // first pixel of the next frame
  float nr = near_far[2 * f], den = near_far[2 * f + 1] - nr + 1e-9f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j >= next && p0 + j < total) {
      f = (p0 + j) / npix;
      next = (f + 1) * npix;
      nr = near_far[2 * f];
      den = near_far[2 * f + 1] - nr + 1e-9f;
    }
    float x = 1.f - (logf(fmaxf(d[j], 1e-9f)) - nr) / den;
    x = fminf(fmaxf(x, 0.f), 1.f);
    int k = (int)(x * 256.f);
    k = k > 255 ? 255 : k;
    c[j] = lut[k];
  }
  if (full && aligned) {
    unsigned int* o = reinterpret_cast<unsigned int*>(out + 3 * p0);
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int j = 0; j < 4; ++j)
      if (p0 + j < total) {
        unsigned char* o = out + 3 * (p0 + j);
        o[0] = (unsigned char)(c[j] & 255u); o[1] = (unsigned char)((c[j] >> 8) & 255u); o[2] = (unsigned char)((c[j] >> 16) & 255u);
      }
  }
}

__device__ __forceinline__ unsigned int to_byte(float v) {   // clamp(0, 1) * 255 -> uint8 (truncation); NaN gives 0
  return (unsigned int)(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
}

// 4 values per lane over the flat [F * H * W * 3] range
__global__ __launch_bounds__(256) void rgb_frames_kernel(const float* __restrict__ rgb, long long total, unsigned char* __restrict__ out, int aligned) {
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  if (p0 + 4 <= total && aligned) {
    const float4 v = *reinterpret_cast<const float4*>(rgb + p0);
    *reinterpret_cast<unsigned int*>(out + p0) = to_byte(v.x) | (to_byte(v.y) << 8) | (to_byte(v.z) << 16) | (to_byte(v.w) << 24);
  } else {
    for (int j = 0; j < 4; ++j)
      if (p0 + j < total) out[p0 + j] = (unsigned char)to_byte(rgb[p0 + j]);
  }
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t wm_gs_effect_ws_bytes(long long N) {
  if (N < 0 || N >= (1LL << 31)) return 0;
  const long long blocks = (N + 255) / 256;
  return (size_t)(blocks > 0 ? blocks : 1) * 16 + 256;
}

hipError_t wm_launch_gs_effect_spread(const float* means, const float* scales, const float* opacities, const float* colors, const float* random_vals,
                                      long long N, double t_n, int ignore_scale, const float* shift, float inv_scale, int colors_are_sh0,
                                      float* out_means, float* out_scales, float* out_opacities, float* out_colors, float* flag, double* stats,
                                      void* workspace, hipStream_t s) {
  if (N < 0 || N >= (1LL << 31) || !stats || !workspace) return hipErrorInvalidValue;
  if (N > 0 && (!means || !scales || !opacities || !colors || !random_vals || !out_means || !out_scales || !out_opacities || !out_colors || !flag))
    return hipErrorInvalidValue;
  const long long blocks = (N + 255) / 256;
  FxArgs a{};
  a.means = means; a.scales = scales; a.opacities = opacities; a.colors = colors; a.random_vals = random_vals; a.shift = shift;
  a.out_means = out_means; a.out_scales = out_scales; a.out_opacities = out_opacities; a.out_colors = out_colors; a.flag = flag;
  a.part_sum = (double*)workspace;
  a.part_count = (unsigned long long*)((char*)workspace + (size_t)(blocks > 0 ? blocks : 1) * 8);
  a.N = N; a.inv_scale = inv_scale; a.ignore_scale = ignore_scale ? 1 : 0; a.is_sh = colors_are_sh0 ? 1 : 0;
  // gs_effects.py:192 in Python floats (fp64): s = smoothstep(0, 10, t_n - 3.2) * 10; the tensor ops then take each scalar as fp32
  const double x = t_n - 3.2;
  double sm;
  if (x < 0.0) sm = 0.0;
  else if (x > 10.0) sm = 1.0;
  else { const double t = (x - 0.0) / (10.0 - 0.0); sm = t * t * (3.0 - 2.0 * t); }
  const double sd = sm * 10.0, e0 = sd - 0.5;
  a.s = (float)sd; a.edge0 = (float)e0; a.width = (float)(sd - e0);
  a.t_n = (float)t_n; a.t_edge = (float)(t_n - 3.1416);
  if (blocks > 0) hipLaunchKernelGGL(gs_effect_spread_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(gs_effect_stats_kernel, dim3(1), dim3(256), 0, s, a.part_count, a.part_sum, blocks, stats);
  return hipGetLastError();
}

static bool video_shape_ok(int F, int H, int W) {
  if (F < 0 || H < 0 || W < 0 || F > 65535) return false;
  if ((long long)H * W >= (1LL << 31)) return false;
  return (long long)F * H * W * 3 < (1LL << 40);
}

size_t wm_video_frames_ws_bytes(int F, int H, int W) {
  if (!video_shape_ok(F, H, W)) return 0;
  return (size_t)(F > 0 ? F : 1) * sizeof(VState) + 256;
}

hipError_t wm_launch_video_frames(const float* rgbs, const float* depths, int F, int H, int W, unsigned char* rgb_out, unsigned char* depth_out,
                                  float* near_far, void* workspace, hipStream_t s) {
  if (!video_shape_ok(F, H, W)) return hipErrorInvalidValue;
  if ((rgbs && !rgb_out) || (depths && (!depth_out || !near_far || !workspace))) return hipErrorInvalidValue;
  if (F == 0 || H == 0 || W == 0) return hipSuccess;
  const int npix = H * W;
  const long long total = (long long)F * npix;
  if (depths) {
    VState* st = (VState*)workspace;
    const unsigned int nblk = (unsigned int)((npix + V_CHUNK - 1) / V_CHUNK);
    hipLaunchKernelGGL(v_init_kernel, dim3(F), dim3(256), 0, s, st);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(v_hist_kernel, dim3(nblk, F), dim3(256), 0, s, depths, npix, st, shift);
      hipLaunchKernelGGL(v_pick_kernel, dim3(F), dim3(256), 0, s, st, shift, npix, near_far);
    }
    const int aligned = (((size_t)depths & 15) == 0 && ((size_t)depth_out & 3) == 0) ? 1 : 0;
    const long long groups = (total + 3) / 4;
    hipLaunchKernelGGL(depth_frames_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, depths, near_far, total, npix, depth_out, aligned);
  }
  if (rgbs) {
    const long long n = total * 3, groups = (n + 3) / 4;
    const int aligned = (((size_t)rgbs & 15) == 0 && ((size_t)rgb_out & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(rgb_frames_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, rgbs, n, rgb_out, aligned);
  }
  return hipGetLastError();
}

void wm_turbo_lut_bytes(unsigned char* out) {
  for (int k = 0; k < 256; ++k) {
    out[3 * k] = (unsigned char)(TURBO_LUT_HOST[k] & 255u);
    out[3 * k + 1] = (unsigned char)((TURBO_LUT_HOST[k] >> 8) & 255u);
    out[3 * k + 2] = (unsigned char)((TURBO_LUT_HOST[k] >> 16) & 255u);
  }
}
