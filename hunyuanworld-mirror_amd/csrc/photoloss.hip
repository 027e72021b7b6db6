// Fused L1 + SSIM photometric loss with backward (the loss of the reference's post-3DGS optimisation: gsplat's
// simple_trainer_worldmirror.py:785-792, F.l1_loss + 1 - fused_ssim).  Definition (the published one fused_ssim implements): 11-tap
// Gaussian window, sigma 1.5, normalised; five zero-padded depthwise filters mu1 = G*a, mu2 = G*b, G*(a a), G*(b b), G*(a b);
//   map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  C1 = 0.01^2, C2 = 0.03^2
// ssim = mean of the map ("valid": over the map cropped by 5 on every side), l1 = mean |a - b|.
//
// Forward: one block per 32 x 32 tile of one image, all channels (three at a time: a channels-last tile row is then one contiguous
// run of 42 * 3 floats).  Tile + 5-pixel halo of a and b -> LDS, horizontal pass -> LDS, vertical pass -> registers, map and its
// three partial derivatives in registers.  Backward: the same separable filter over the three stored derivative maps.
// Arithmetic: the filter sums, the moments and the map run in fp64.  s1 = G*(a a) - mu1^2 cancels against C2 = 9e-4 where the
// image is flat (fp32 sums leave ~1e-5 relative there, the error the fp32 torch spelling shows), so the cancellation is not allowed
// to happen.  The price: the fp64 horizontal results are 55 KB of the forward's LDS and the accumulators push it past 200 VGPRs,
// which is what holds the forward to one block per CU.  A centred fp32 variance form was not tried (profiles/r06_photometric_loss.md
// §1 has the argument and the measured kernel times).  Inputs, derivative maps and the gradient are fp32.
// LDS (160 KiB per CU): forward 2 * 3 * 42 * 43 * 4 (a, b) + 5 * 42 * 33 * 8 (horizontal results) = 98.8 KB, one block per CU;
// backward 3 * 42 * 43 * 4 + 3 * 42 * 33 * 8 = 54.9 KB, two blocks per CU.
// Reproducibility: no atomics.  Each block writes its two partial sums to the workspace, one small kernel adds them in index
// order.  Nothing in a plane's arithmetic or in the order of the partials depends on the strides: NCHW and channels-last give
// the same bits.
#include "scene_common.h"
#include "wm_kernels.h"

namespace {

constexpr int PL_TILE = 32, PL_R = 5, PL_IN = PL_TILE + 2 * PL_R, PL_PITCH = PL_IN + 1, PL_HP = PL_TILE + 1, PL_CCH = 3, PL_THREADS = 256;
constexpr int PL_SEG = 4;                      // outputs per thread and pass: 4 + 10 inputs feed 4 outputs
constexpr int PL_NIN = PL_SEG + 2 * PL_R;      // 14
constexpr double PL_C1 = 0.01 * 0.01, PL_C2 = 0.03 * 0.03;

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum
__device__ __forceinline__ constexpr double pl_g(int k) {
  constexpr double g[11] = {0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537,
                            0.26601172486179436, 0.2130055377112537, 0.10936068950970002, 0.03600077212843083, 0.007598758135239185,
                            0.00102838008447911};
  return g[k];
}

struct PlGeom {
  int B, C, H, W, gx, gy, valid;
};

// Tile + halo of channels [c0, c0 + nc) of image bi -> dst[cc][ly][lx], zero outside the image.  The innermost index of the sweep is
// whichever of channel / x has the smaller stride, so that consecutive lanes read consecutive addresses in both layouts.
__device__ __forceinline__ void pl_stage(float (*dst)[PL_IN][PL_PITCH], const float* __restrict__ img, const long long* st, int bi, int c0,
                                         int nc, int y0, int x0, int H, int W) {
  const bool chan_inner = st[1] < st[3];
  const int total = nc * PL_IN * PL_IN;
  for (int i = threadIdx.x; i < total; i += PL_THREADS) {
    int cc, p;
    if (chan_inner) { cc = i % nc; p = i / nc; } else { p = i % (PL_IN * PL_IN); cc = i / (PL_IN * PL_IN); }
    const int ly = p / PL_IN, lx = p - ly * PL_IN;
    const int y = y0 + ly - PL_R, x = x0 + lx - PL_R;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) v = img[bi * st[0] + (c0 + cc) * st[1] + y * st[2] + x * st[3]];
    dst[cc][ly][lx] = v;
  }
}

// acc[o] += g[j - o] * v for the outputs o in [0, 4) that input j in [0, 14) reaches
#define PL_SCATTER(acc, j, v)                                       \
  _Pragma("unroll") for (int o = 0; o < PL_SEG; ++o) {              \
    if ((j) - o >= 0 && (j) - o < 11) acc[o] = fma(pl_g((j) - o), (v), acc[o]); \
  }

struct PlFwdArgs {
  const float* a; const float* b;
  long long sa[4], sb[4];
  PlGeom g;
  double* partials;      // [blocks][2]: sum of the counted map values, sum |a - b|
  float* maps;           // [3][B][C][H][W] planar: d map / d mu1 (total), d map / d s1, d map / d s12; zero outside the counted region
};

template <bool WANT_BWD>
__global__ __launch_bounds__(PL_THREADS) WM_NO_PACKED_FP32 void photoloss_fwd_kernel(PlFwdArgs A) {
  __shared__ float sA[PL_CCH][PL_IN][PL_PITCH];
  __shared__ float sB[PL_CCH][PL_IN][PL_PITCH];
  __shared__ double sH[5][PL_IN][PL_HP];
  __shared__ double sRed[2][PL_THREADS / 64];
  const PlGeom g = A.g;
  const int blk = blockIdx.x;
  const int tx = blk % g.gx, ty = (blk / g.gx) % g.gy, bi = blk / (g.gx * g.gy);
  const int x0 = tx * PL_TILE, y0 = ty * PL_TILE;
  const int tid = threadIdx.x, vcol = tid & 31, vseg = tid >> 5;
  const size_t plane = (size_t)g.H * g.W, total = plane * g.C * g.B;
  double acc_s = 0.0, acc_l = 0.0;
  for (int c0 = 0; c0 < g.C; c0 += PL_CCH) {
    const int nc = min(PL_CCH, g.C - c0);
    pl_stage(sA, A.a, A.sa, bi, c0, nc, y0, x0, g.H, g.W);
    pl_stage(sB, A.b, A.sb, bi, c0, nc, y0, x0, g.H, g.W);
    __syncthreads();
    for (int cc = 0; cc < nc; ++cc) {
      // horizontal: 42 rows x 8 segments of 4 columns
      for (int it = tid; it < PL_IN * (PL_TILE / PL_SEG); it += PL_THREADS) {
        const int row = it >> 3, seg = it & 7;
        double m1[PL_SEG] = {}, m2[PL_SEG] = {}, e11[PL_SEG] = {}, e22[PL_SEG] = {}, e12[PL_SEG] = {};
#pragma unroll
        for (int j = 0; j < PL_NIN; ++j) {
          const double x = sA[cc][row][seg * PL_SEG + j], y = sB[cc][row][seg * PL_SEG + j];
          const double xx = x * x, yy = y * y, xy = x * y;
          PL_SCATTER(m1, j, x) PL_SCATTER(m2, j, y) PL_SCATTER(e11, j, xx) PL_SCATTER(e22, j, yy) PL_SCATTER(e12, j, xy)
        }
#pragma unroll
        for (int o = 0; o < PL_SEG; ++o) {
          const int col = seg * PL_SEG + o;
          sH[0][row][col] = m1[o]; sH[1][row][col] = m2[o]; sH[2][row][col] = e11[o]; sH[3][row][col] = e22[o]; sH[4][row][col] = e12[o];
        }
      }
      __syncthreads();
      // vertical: column vcol, rows vseg * 4 .. + 3
      double m1[PL_SEG] = {}, m2[PL_SEG] = {}, e11[PL_SEG] = {}, e22[PL_SEG] = {}, e12[PL_SEG] = {};
#pragma unroll
      for (int j = 0; j < PL_NIN; ++j) {
        const int row = vseg * PL_SEG + j;
        const double h0 = sH[0][row][vcol], h1 = sH[1][row][vcol], h2 = sH[2][row][vcol], h3 = sH[3][row][vcol], h4 = sH[4][row][vcol];
        PL_SCATTER(m1, j, h0) PL_SCATTER(m2, j, h1) PL_SCATTER(e11, j, h2) PL_SCATTER(e22, j, h3) PL_SCATTER(e12, j, h4)
      }
      const int x = x0 + vcol;
#pragma unroll
      for (int o = 0; o < PL_SEG; ++o) {
        const int ly = vseg * PL_SEG + o, y = y0 + ly;
        if (y < g.H && x < g.W) {
          const double mu1 = m1[o], mu2 = m2[o];
          const double s1 = e11[o] - mu1 * mu1, s2 = e22[o] - mu2 * mu2, s12 = e12[o] - mu1 * mu2;
          const double cn = 2.0 * mu1 * mu2 + PL_C1, dn = 2.0 * s12 + PL_C2;
          const double am = mu1 * mu1 + mu2 * mu2 + PL_C1, bs = s1 + s2 + PL_C2;
          const double iam = 1.0 / am, ibs = 1.0 / bs;
          const double map = cn * dn * iam * ibs;
          const bool counted = !g.valid || (y >= PL_R && y < g.H - PL_R && x >= PL_R && x < g.W - PL_R);
          if (counted) acc_s += map;
          acc_l += fabs((double)sA[cc][ly + PL_R][vcol + PL_R] - (double)sB[cc][ly + PL_R][vcol + PL_R]);
          if (WANT_BWD) {
            // partial derivatives with mu1, s1, s12 as independent variables, then d/d mu1 taken through s1 = E11 - mu1^2 and
            // s12 = E12 - mu1 mu2 as well: what multiplies G in d ssim / d a = G*(d_mu) + 2 a G*(d_s1) + b G*(d_s12)
            const double d_s1 = -map * ibs;
            const double d_s12 = 2.0 * cn * iam * ibs;
            const double d_mu_direct = 2.0 * mu2 * dn * iam * ibs - 2.0 * mu1 * map * iam;
            const double d_mu = d_mu_direct - 2.0 * mu1 * d_s1 - mu2 * d_s12;
            const size_t idx = ((size_t)bi * g.C + (c0 + cc)) * plane + (size_t)y * g.W + x;
            A.maps[idx] = counted ? (float)d_mu : 0.f;
            A.maps[total + idx] = counted ? (float)d_s1 : 0.f;
            A.maps[2 * total + idx] = counted ? (float)d_s12 : 0.f;
          }
        }
      }
      __syncthreads();   // sH is rewritten by the next channel, sA / sB by the next chunk
    }
  }
  acc_s = wave_sum(acc_s);
  acc_l = wave_sum(acc_l);
  if ((tid & 63) == 0) { sRed[0][tid >> 6] = acc_s; sRed[1][tid >> 6] = acc_l; }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, l = 0.0;
    for (int w = 0; w < PL_THREADS / 64; ++w) { s += sRed[0][w]; l += sRed[1][w]; }
    A.partials[2 * (size_t)blk] = s;
    A.partials[2 * (size_t)blk + 1] = l;
  }
}

// the per-block partials in index order -> the two means
__global__ __launch_bounds__(PL_THREADS) void photoloss_reduce_kernel(const double* __restrict__ partials, int nblk, double inv_count,
                                                                      double inv_total, float* out_ssim, float* out_l1) {
  __shared__ double sS[PL_THREADS], sL[PL_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, l = 0.0;
  for (int i = tid; i < nblk; i += PL_THREADS) { s += partials[2 * (size_t)i]; l += partials[2 * (size_t)i + 1]; }
  sS[tid] = s; sL[tid] = l;
  __syncthreads();
  for (int h = PL_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) { sS[tid] += sS[tid + h]; sL[tid] += sL[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) { *out_ssim = (float)(sS[0] * inv_count); *out_l1 = (float)(sL[0] * inv_total); }
}

struct PlBwdArgs {
  const float* a; const float* b;
  long long sa[4], sb[4];
  PlGeom g;
  const float* maps;
  const float* g_ssim; const float* g_l1;    // device scalars
  double inv_count, inv_total;
  float* grad;                               // img1's strides
};

__global__ __launch_bounds__(PL_THREADS) WM_NO_PACKED_FP32 void photoloss_bwd_kernel(PlBwdArgs A) {
  __shared__ float sM[3][PL_IN][PL_PITCH];
  __shared__ double sH[3][PL_IN][PL_HP];
  const PlGeom g = A.g;
  const int blk = blockIdx.x;
  const int tx = blk % g.gx, ty = (blk / g.gx) % g.gy, bi = blk / (g.gx * g.gy);
  const int x0 = tx * PL_TILE, y0 = ty * PL_TILE;
  const int tid = threadIdx.x, vcol = tid & 31, vseg = tid >> 5;
  const size_t plane = (size_t)g.H * g.W, total = plane * g.C * g.B;
  const double gs = (double)*A.g_ssim * A.inv_count, gl = (double)*A.g_l1 * A.inv_total;
  const int x = x0 + vcol;
  for (int c0 = 0; c0 < g.C; c0 += PL_CCH) {
    const int nc = min(PL_CCH, g.C - c0);
    float av[PL_CCH][PL_SEG], bv[PL_CCH][PL_SEG], gr[PL_CCH][PL_SEG];
    // this thread's pixels of the chunk, channel innermost (a channels-last pixel is nc consecutive floats)
#pragma unroll
    for (int o = 0; o < PL_SEG; ++o) {
      const int y = y0 + vseg * PL_SEG + o;
#pragma unroll
      for (int cc = 0; cc < PL_CCH; ++cc) {
        const bool in = cc < nc && y < g.H && x < g.W;
        av[cc][o] = in ? A.a[bi * A.sa[0] + (c0 + cc) * A.sa[1] + y * A.sa[2] + x * A.sa[3]] : 0.f;
        bv[cc][o] = in ? A.b[bi * A.sb[0] + (c0 + cc) * A.sb[1] + y * A.sb[2] + x * A.sb[3]] : 0.f;
      }
    }
#pragma unroll
    for (int cc = 0; cc < PL_CCH; ++cc) {
      if (cc < nc) {     // block-uniform
        const size_t base = ((size_t)bi * g.C + (c0 + cc)) * plane;
        for (int i = tid; i < 3 * PL_IN * PL_IN; i += PL_THREADS) {
          const int q = i / (PL_IN * PL_IN), p = i - q * (PL_IN * PL_IN);
          const int ly = p / PL_IN, lx = p - ly * PL_IN;
          const int yy = y0 + ly - PL_R, xx = x0 + lx - PL_R;
          float v = 0.f;
          if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) v = A.maps[q * total + base + (size_t)yy * g.W + xx];
          sM[q][ly][lx] = v;
        }
        __syncthreads();
        for (int it = tid; it < PL_IN * (PL_TILE / PL_SEG); it += PL_THREADS) {
          const int row = it >> 3, seg = it & 7;
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            double h[PL_SEG] = {};
#pragma unroll
            for (int j = 0; j < PL_NIN; ++j) {
              const double v = sM[q][row][seg * PL_SEG + j];
              PL_SCATTER(h, j, v)
            }
#pragma unroll
            for (int o = 0; o < PL_SEG; ++o) sH[q][row][seg * PL_SEG + o] = h[o];
          }
        }
        __syncthreads();   // (the next channel's sH writes come two barriers after this channel's last sH read)
        double f[3][PL_SEG] = {};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
          for (int j = 0; j < PL_NIN; ++j) {
            const double v = sH[q][vseg * PL_SEG + j][vcol];
            PL_SCATTER(f[q], j, v)
          }
        }
#pragma unroll
        for (int o = 0; o < PL_SEG; ++o) {
          const double a = av[cc][o], b = bv[cc][o];
          const double sgn = (a > b) - (a < b);
          gr[cc][o] = (float)(gs * (f[0][o] + 2.0 * a * f[1][o] + b * f[2][o]) + gl * sgn);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < PL_SEG; ++o) {
      const int y = y0 + vseg * PL_SEG + o;
#pragma unroll
      for (int cc = 0; cc < PL_CCH; ++cc)
        if (cc < nc && y < g.H && x < g.W) A.grad[bi * A.sa[0] + (c0 + cc) * A.sa[1] + y * A.sa[2] + x * A.sa[3]] = gr[cc][o];
    }
  }
}

bool pl_geom(const WmPhotoLossArgs& a, PlGeom& g, long long& nblk) {
  if (a.B <= 0 || a.C <= 0 || a.H <= 0 || a.W <= 0) return false;
  if (a.padding_valid && (a.H < 2 * PL_R + 1 || a.W < 2 * PL_R + 1)) return false;   // the mean of an empty map
  g.B = a.B; g.C = a.C; g.H = a.H; g.W = a.W; g.valid = a.padding_valid ? 1 : 0;
  g.gx = (a.W + PL_TILE - 1) / PL_TILE; g.gy = (a.H + PL_TILE - 1) / PL_TILE;
  nblk = (long long)a.B * g.gx * g.gy;
  return nblk < (1LL << 31);
}

double pl_count(const PlGeom& g) {
  const double h = g.valid ? g.H - 2 * PL_R : g.H, w = g.valid ? g.W - 2 * PL_R : g.W;
  return (double)g.B * g.C * h * w;
}

}  // namespace

size_t wm_photoloss_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return align256(wm_photoloss_forward_only_bytes(B, H, W)) + 3 * (size_t)B * C * H * W * sizeof(float);
}
// the per-tile partials alone: what a forward without a backward to follow touches
size_t wm_photoloss_forward_only_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * ((H + PL_TILE - 1) / PL_TILE) * ((W + PL_TILE - 1) / PL_TILE) * 2 * sizeof(double);
}

hipError_t wm_launch_photoloss_fwd(const WmPhotoLossArgs& a, int want_backward, float* out_ssim, float* out_l1, hipStream_t s) {
  PlGeom g;
  long long nblk;
  if (!pl_geom(a, g, nblk)) return hipErrorInvalidValue;
  if (a.workspace_bytes < (want_backward ? wm_photoloss_workspace_bytes(a.B, a.C, a.H, a.W) : wm_photoloss_forward_only_bytes(a.B, a.H, a.W)))
    return hipErrorInvalidValue;
  PlFwdArgs k;
  k.a = a.img1; k.b = a.img2; k.g = g;
  for (int i = 0; i < 4; ++i) { k.sa[i] = a.strides1[i]; k.sb[i] = a.strides2[i]; }
  k.partials = (double*)a.workspace;
  k.maps = (float*)((char*)a.workspace + align256((size_t)nblk * 2 * sizeof(double)));
  if (want_backward) hipLaunchKernelGGL(photoloss_fwd_kernel<true>, dim3((unsigned)nblk), dim3(PL_THREADS), 0, s, k);
  else hipLaunchKernelGGL(photoloss_fwd_kernel<false>, dim3((unsigned)nblk), dim3(PL_THREADS), 0, s, k);
  hipLaunchKernelGGL(photoloss_reduce_kernel, dim3(1), dim3(PL_THREADS), 0, s, (const double*)k.partials, (int)nblk, 1.0 / pl_count(g),
                     1.0 / ((double)g.B * g.C * g.H * g.W), out_ssim, out_l1);
  return hipGetLastError();
}

hipError_t wm_launch_photoloss_bwd(const WmPhotoLossArgs& a, const float* g_ssim, const float* g_l1, float* grad_img1, hipStream_t s) {
  PlGeom g;
  long long nblk;
  if (!pl_geom(a, g, nblk) || a.workspace_bytes < wm_photoloss_workspace_bytes(a.B, a.C, a.H, a.W)) return hipErrorInvalidValue;
  PlBwdArgs k;
  k.a = a.img1; k.b = a.img2; k.g = g;
  for (int i = 0; i < 4; ++i) { k.sa[i] = a.strides1[i]; k.sb[i] = a.strides2[i]; }
  k.maps = (const float*)((const char*)a.workspace + align256((size_t)nblk * 2 * sizeof(double)));
  k.g_ssim = g_ssim; k.g_l1 = g_l1;
  k.inv_count = 1.0 / pl_count(g); k.inv_total = 1.0 / ((double)g.B * g.C * g.H * g.W);
  k.grad = grad_img1;
  hipLaunchKernelGGL(photoloss_bwd_kernel, dim3((unsigned)nblk), dim3(PL_THREADS), 0, s, k);
  return hipGetLastError();
}
