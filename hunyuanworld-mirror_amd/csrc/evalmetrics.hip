// Trainer evaluation (gsplat's simple_trainer_worldmirror.py Runner.eval, :1005-1091): the clamp, the side-by-side canvas and the PSNR of
// one render batch in one pass, and the iterative colour correction of examples/lib_bilagrid.py:56-126 as masked normal equations.
// Every sum here is fp64 in a fixed order (a lane adds its values in index order, a block's lanes are added by a fixed tree or one lane
// per sum, the blocks' partials are added in block order): no floating-point atomics, the bits repeat from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wm_api.h"

namespace {

// ------------------------------------------------------------------ eval frame: clamp, canvas, squared error
constexpr int EF_PIX = 1024;   // pixels of one block: 4 per lane, 256 apart

struct EfArgs {
  const float* colors; const float* pixels;
  long long cs[4], ps[4];      // element strides (B, H, W, C)
  int B, H, W, clamp, nblk;
  float* clamped;              // [B,H,W,3] or null
  unsigned char* canvas;       // [B,H,2W,3] or null
  double* part;                // [B][nblk]
};

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // NaN stays NaN, as torch.clamp
// (canvas * 255).astype(np.uint8): the fp32 product truncated toward zero; values outside [0, 1] (out of contract) saturate
__device__ __forceinline__ unsigned char canvas_byte(float v) {
  const float s = v * 255.0f;
  const int k = s >= 255.f ? 255 : (s > 0.f ? (int)s : 0);
  return (unsigned char)k;
}

// fixed tree over the 256 lanes' values
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void eval_frame_kernel(EfArgs a) {
  __shared__ double red[256];
  const int b = blockIdx.y, t = threadIdx.x;
  const int npix = a.H * a.W;
  const float* col = a.colors + (long long)b * a.cs[0];
  const float* pix = a.pixels + (long long)b * a.ps[0];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < EF_PIX / 256; ++j) {
    const long long p = (long long)blockIdx.x * EF_PIX + j * 256 + t;
    if (p < npix) {
      const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
      const float* cp = col + y * a.cs[1] + x * a.cs[2];
      const float* pp = pix + y * a.ps[1] + x * a.ps[2];
      float c[3], q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float v = cp[k * a.cs[3]];
        c[k] = a.clamp ? clamp01(v) : v;
        q[k] = pp[k * a.ps[3]];
        const double d = (double)c[k] - (double)q[k];
        acc += d * d;
      }
      if (a.clamped) {
        float* o = a.clamped + ((long long)b * npix + p) * 3;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
      }
      if (a.canvas) {
        unsigned char* l = a.canvas + (((long long)b * a.H + y) * (2LL * a.W) + x) * 3;
        unsigned char* r = l + 3LL * a.W;
#pragma unroll
        for (int k = 0; k < 3; ++k) { l[k] = canvas_byte(q[k]); r[k] = canvas_byte(c[k]); }
      }
    }
  }
  const double s = block_sum_256(acc, red);
  if (t == 0) a.part[(long long)b * a.nblk + blockIdx.x] = s;
}

__device__ __forceinline__ float psnr_of(double sse, double count, double data_range) {
  const double mse = sse / count;
  if (mse == 0.0) return INFINITY;
  return (float)(10.0 * log10(data_range * data_range / mse));
}

// one block: per image the block partials (lane t takes t, t + 256, ... in order, then the tree), the images in order
__global__ __launch_bounds__(256) void eval_frame_finish_kernel(const double* __restrict__ part, int B, int nblk, double per_image_count,
                                                                double data_range, float* __restrict__ psnr_all, float* __restrict__ psnr_each) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    double acc = 0.0;
    for (int i = t; i < nblk; i += 256) acc += part[(long long)b * nblk + i];
    const double sse = block_sum_256(acc, red);
    total += sse;
    if (t == 0 && psnr_each) psnr_each[b] = psnr_of(sse, per_image_count, data_range);
  }
  if (t == 0 && psnr_all) *psnr_all = psnr_of(total, per_image_count * (double)B, data_range);
}

// ------------------------------------------------------------------ colour correction
// Per pixel a row of 16 doubles in LDS: the 10 features of the current image (rr rg rb gg gb bb r g b 1), the 3 reference values, the 3
// channel masks (1.0 / 0.0).  Sum k of the 195 = 3 x (55 + 10): channel c = k / 65; within it the 55 products f_i f_j (i <= j, row-major
// upper triangle), then the 10 products f_i ref_c; all under mask c.  Lane k of the block owns sum k and walks the staged pixels in order.
constexpr int CC_NACC = 195, CC_ROW = 16, CC_ROUND = 256, CC_ROUNDS = 2, CC_TILE = CC_ROUND * CC_ROUNDS;
constexpr int CC_MAX_SWEEPS = 15;
constexpr double CC_CUTOFF = 1e-10;   // relative eigenvalue cut-off of the pseudo-inverse

struct CcArgs {
  const float* img; const float* ref; float* out;
  const double* warp;          // [nsys][10][3] of the previous solve, or null (first pass: out = img)
  double* part;                // [nsys][nblk][195]
  long long P;
  int nblk, accumulate;
  float lo, hi;
};

__device__ __forceinline__ void cc_features(float r, float g, float b, double* f) {
  const double R = r, G = g, B = b;
  f[0] = R * R; f[1] = R * G; f[2] = R * B; f[3] = G * G; f[4] = G * B; f[5] = B * B; f[6] = R; f[7] = G; f[8] = B; f[9] = 1.0;
}

__global__ __launch_bounds__(256) void cc_pass_kernel(CcArgs a) {
  __shared__ double row[CC_ROUND * CC_ROW];
  const int t = threadIdx.x, sys = blockIdx.y;
  const long long off = (long long)sys * a.P * 3;
  const float* img = a.img + off;
  const float* ref = a.ref + off;
  float* out = a.out + off;
  __shared__ double w[30];
  if (a.warp) {
    if (t < 30) w[t] = a.warp[sys * 30 + t];
    __syncthreads();
  }
  // this lane's sum: row slots ia, ib under mask slot im
  int ia = 0, ib = 0, im = 13;
  if (t < CC_NACC) {
    const int c = t / 65, r = t - c * 65;
    im = 13 + c;
    if (r < 55) {
      int i = 0, rr = r;
      while (rr >= 10 - i) { rr -= 10 - i; ++i; }
      ia = i; ib = i + rr;
    } else {
      ia = r - 55; ib = 10 + c;
    }
  }
  double acc = 0.0;
  for (int round = 0; round < CC_ROUNDS; ++round) {
    const long long base = (long long)blockIdx.x * CC_TILE + round * CC_ROUND;
    if (base >= a.P) break;                                  // (the same for every lane of the block)
    const long long left = a.P - base;
    const int n = left < CC_ROUND ? (int)left : CC_ROUND;
    if (t < n) {
      const long long p = base + t;
      const float o0 = img[3 * p], o1 = img[3 * p + 1], o2 = img[3 * p + 2];
      float c0, c1, c2;
      double f[10];
      if (a.warp) {
        cc_features(out[3 * p], out[3 * p + 1], out[3 * p + 2], f);
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < 10; ++j) s += f[j] * w[j * 3 + c];
          v[c] = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);        // torch.clip: NaN stays
        }
        c0 = (float)v[0]; c1 = (float)v[1]; c2 = (float)v[2];
      } else {
        c0 = o0; c1 = o1; c2 = o2;
      }
      out[3 * p] = c0; out[3 * p + 1] = c1; out[3 * p + 2] = c2;
      if (a.accumulate) {
        const float r0 = ref[3 * p], r1 = ref[3 * p + 1], r2 = ref[3 * p + 2];
        cc_features(c0, c1, c2, f);
        double* q = row + t * CC_ROW;
#pragma unroll
        for (int j = 0; j < 10; ++j) q[j] = f[j];
        q[10] = r0; q[11] = r1; q[12] = r2;
        const float lo = a.lo, hi = a.hi;
#define CC_UNCLIPPED(z) ((z) >= lo && (z) <= hi)
        q[13] = (CC_UNCLIPPED(o0) && CC_UNCLIPPED(c0) && CC_UNCLIPPED(r0)) ? 1.0 : 0.0;
        q[14] = (CC_UNCLIPPED(o1) && CC_UNCLIPPED(c1) && CC_UNCLIPPED(r1)) ? 1.0 : 0.0;
        q[15] = (CC_UNCLIPPED(o2) && CC_UNCLIPPED(c2) && CC_UNCLIPPED(r2)) ? 1.0 : 0.0;
#undef CC_UNCLIPPED
      }
    }
    if (!a.accumulate) continue;
    __syncthreads();
    if (t < CC_NACC) {
      const double* q = row;
#pragma unroll 8
      for (int i = 0; i < n; ++i, q += CC_ROW) {
        const double m = q[im], x = q[ia], y = q[ib];
        acc += m != 0.0 ? x * y : 0.0;                       // a masked row adds +0 whatever it holds, as torch.where
      }
    }
    __syncthreads();
  }
  if (a.accumulate && t < CC_NACC) a.part[((long long)sys * a.nblk + blockIdx.x) * CC_NACC + t] = acc;
}

__device__ __forceinline__ int cc_pair(int i, int j) {   // slot of f_i f_j in the upper triangle, any order of i, j
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo * 10 - lo * (lo - 1) / 2 + (hi - lo);
}

// The block partials of a pass in block order, one lane per sum; the loads of 16 blocks are issued together, the adds stay sequential.
__global__ __launch_bounds__(256) void cc_reduce_kernel(const double* __restrict__ part, int nblk, double* __restrict__ sums) {
  const int k = threadIdx.x, sys = blockIdx.x;
  if (k >= CC_NACC) return;
  const double* ps = part + (long long)sys * nblk * CC_NACC + k;
  double acc = 0.0;
  int b = 0;
  for (; b + 16 <= nblk; b += 16) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = ps[(long long)(b + j) * CC_NACC];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += v[j];
  }
  for (; b < nblk; ++b) acc += ps[(long long)b * CC_NACC];
  sums[sys * CC_NACC + k] = acc;
}

// One wave per system: for the three 10 x 10 normal equations a cyclic Jacobi eigendecomposition (lane = (channel, row); the matrices
// in LDS) and the minimum-norm solution over the eigenvalues above CC_CUTOFF * max.
__global__ __launch_bounds__(64) void cc_solve_kernel(const double* __restrict__ sums, double* __restrict__ warp) {
  __shared__ double S[CC_NACC];
  __shared__ double A[3][10][10], V[3][10][10], rhs[3][10], coef[3][10];
  const int lane = threadIdx.x, sys = blockIdx.x;
  for (int k = lane; k < CC_NACC; k += 64) S[k] = sums[sys * CC_NACC + k];
  __syncthreads();
  const bool active = lane < 30;
  const int c = active ? lane / 10 : 0, k = active ? lane - c * 10 : 0;
  if (active) {
    for (int j = 0; j < 10; ++j) {
      A[c][k][j] = S[c * 65 + cc_pair(k, j)];
      V[c][k][j] = j == k ? 1.0 : 0.0;
    }
    rhs[c][k] = S[c * 65 + 55 + k];
  }
  __syncthreads();
  for (int sweep = 0; sweep < CC_MAX_SWEEPS; ++sweep) {
    // converged when the off-diagonal part has vanished against the diagonal (squared Frobenius norms; the same value in the 10 lanes
    // of a system), for all three systems
    double offn = 0.0, diagn = 0.0;
    for (int i = 0; i < 10; ++i)
      for (int j = 0; j < 10; ++j) {
        const double v = A[c][i][j];
        if (i == j) diagn += v * v; else offn += v * v;
      }
    const int done = !active || offn <= 1e-30 * diagn;
    if (__all(done)) break;
    for (int p = 0; p < 9; ++p)
      for (int q = p + 1; q < 10; ++q) {
        const double apq = A[c][p][q], app = A[c][p][p], aqq = A[c][q][q];
        double tt = 0.0;
        if (apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
          if (theta < 0.0) tt = -tt;
        }
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        __syncthreads();                                     // everyone has read the pivot before rows p, q change
        if (active) {
          // A <- J^T A J with J = [[cs, sn], [-sn, cs]] on (p, q).  Lane k (neither p nor q) rotates its row's two entries and mirrors
          // them into rows p, q (A stays exactly symmetric); lanes p and q write the pivot block in closed form, the pair itself zero.
          if (k == p) {
            A[c][p][p] = app - tt * apq; A[c][p][q] = 0.0;
          } else if (k == q) {
            A[c][q][q] = aqq + tt * apq; A[c][q][p] = 0.0;
          } else {
            const double akp = A[c][k][p], akq = A[c][k][q];
            const double np = cs * akp - sn * akq, nq = sn * akp + cs * akq;
            A[c][k][p] = np; A[c][p][k] = np;
            A[c][k][q] = nq; A[c][q][k] = nq;
          }
          const double vkp = V[c][k][p], vkq = V[c][k][q];   // columns p, q of V: lane = row k
          V[c][k][p] = cs * vkp - sn * vkq;
          V[c][k][q] = sn * vkp + cs * vkq;
        }
        __syncthreads();
      }
  }
  __syncthreads();
  double lmax = 0.0;
  for (int j = 0; j < 10; ++j) lmax = fmax(lmax, A[c][j][j]);
  if (active) {                                              // lane = eigenpair k: (v_k . rhs) / lambda_k, or 0 below the cut-off
    const double lam = A[c][k][k];
    double d = 0.0;
    for (int i = 0; i < 10; ++i) d += V[c][i][k] * rhs[c][i];
    coef[c][k] = (lmax > 0.0 && lam > CC_CUTOFF * lmax) ? d / lam : 0.0;
  }
  __syncthreads();
  if (active) {
    double wv = 0.0;
    for (int j = 0; j < 10; ++j) wv += V[c][k][j] * coef[c][j];
    warp[sys * 30 + k * 3 + c] = wv;
  }
}

inline bool ef_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && (long long)H * W * 6 < (1LL << 31);
}
inline bool cc_shape_ok(int nsys, long long P) { return nsys >= 1 && nsys <= 65535 && P >= 1 && P < (1LL << 31); }

}  // namespace

// ------------------------------------------------------------------ launchers
size_t wm_eval_frame_ws_bytes(int B, int H, int W) {
  if (!ef_shape_ok(B, H, W)) return 0;
  const long long nblk = ((long long)H * W + EF_PIX - 1) / EF_PIX;
  return (size_t)B * nblk * sizeof(double);
}

hipError_t wm_launch_eval_frame(const float* colors, const long long* cs, const float* pixels, const long long* ps, int B, int H, int W, int clamp,
                                double data_range, float* clamped, unsigned char* canvas, float* psnr_all, float* psnr_each, void* workspace,
                                hipStream_t s) {
  if (!ef_shape_ok(B, H, W) || !colors || !pixels || !cs || !ps || !workspace) return hipErrorInvalidValue;
  EfArgs a{};
  a.colors = colors; a.pixels = pixels;
  for (int i = 0; i < 4; ++i) { a.cs[i] = cs[i]; a.ps[i] = ps[i]; }
  a.B = B; a.H = H; a.W = W; a.clamp = clamp ? 1 : 0;
  a.nblk = (int)(((long long)H * W + EF_PIX - 1) / EF_PIX);
  a.clamped = clamped; a.canvas = canvas; a.part = (double*)workspace;
  hipLaunchKernelGGL(eval_frame_kernel, dim3((unsigned)a.nblk, (unsigned)B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(eval_frame_finish_kernel, dim3(1), dim3(256), 0, s, a.part, B, a.nblk, (double)H * W * 3.0, data_range, psnr_all, psnr_each);
  return hipGetLastError();
}

size_t wm_color_correct_ws_bytes(int nsys, long long P) {
  if (!cc_shape_ok(nsys, P)) return 0;
  const long long nblk = (P + CC_TILE - 1) / CC_TILE;
  return ((size_t)nsys * (nblk + 1) * CC_NACC + (size_t)nsys * 30) * sizeof(double);
}

hipError_t wm_launch_color_correct(const float* img, const float* ref, int nsys, long long P, int num_iters, double eps, float* out, void* workspace,
                                   hipStream_t s) {
  if (!cc_shape_ok(nsys, P) || !img || !ref || !out || !workspace || num_iters < 0 || !(eps > 0.0) || !(eps < 0.5)) return hipErrorInvalidValue;
  if (num_iters == 0) return hipMemcpyAsync(out, img, (size_t)nsys * P * 3 * sizeof(float), hipMemcpyDeviceToDevice, s);
  CcArgs a{};
  a.img = img; a.ref = ref; a.out = out; a.P = P;
  a.nblk = (int)((P + CC_TILE - 1) / CC_TILE);
  a.part = (double*)workspace;
  double* sums = a.part + (size_t)nsys * a.nblk * CC_NACC;
  double* warp = sums + (size_t)nsys * CC_NACC;
  a.lo = (float)eps; a.hi = (float)(1.0 - eps);              // the thresholds as the reference's fp32 comparison takes them
  const dim3 grid((unsigned)a.nblk, (unsigned)nsys);
  for (int it = 0; it <= num_iters; ++it) {
    a.warp = it == 0 ? nullptr : warp;
    a.accumulate = it < num_iters ? 1 : 0;
    hipLaunchKernelGGL(cc_pass_kernel, grid, dim3(256), 0, s, a);
    if (a.accumulate) {
      hipLaunchKernelGGL(cc_reduce_kernel, dim3((unsigned)nsys), dim3(256), 0, s, a.part, a.nblk, sums);
      hipLaunchKernelGGL(cc_solve_kernel, dim3((unsigned)nsys), dim3(64), 0, s, sums, warp);
    }
  }
  return hipGetLastError();
}
