// Sparse disparity loss of the post-3DGS trainer's --depth_loss branch (gsplat's simple_trainer_worldmirror.py:793-811) with its
// backward, and the projection of world points into the training views that feeds it (examples/datasets/colmap.py:412-433).
//
// loss.  Row (c, m) flagged valid samples the depth image of camera c at the pixel coordinate (x, y) = points[c, m] the way
// F.grid_sample(align_corners=True, bilinear, zero padding) does after the trainer's normalisation with (W - 1, H - 1): pixel centres
// at integers, x0 = floor(x), the four corners (x0 .. x0 + 1, y0 .. y0 + 1) weighted (1 - fx | fx)(1 - fy | fy), a corner outside the
// image counts as zero.  disp = d > 0 ? 1 / d : 0, term = |disp - 1 / depth_gt|, loss = mean of the terms over the valid rows.
//   forward   one row per lane: the gather, the term; per block one (sum, count) pair in fp64 to the workspace, one small kernel adds
//             the pairs in index order, divides and rounds once (n = 0: 0 / 0 = NaN, torch's mean of nothing).  With a backward to
//             follow the lane also stores coef = sign(disp - disp_gt) * (-1 / d^2) (0 for an invalid row, d <= 0 or sign 0).
//             The sample, the reciprocal and the term are formed in fp64 from the fp32 inputs: one row costs four loads either way.
//   backward  v_depth[c, y, x] = (g / n) sum_m w_m(y, x) coef_m in POINT ORDER within a pixel, without atomics in these kernels:
//             every row with a coefficient gets the key of its base cell (c, y0 + 1, x0 + 1) on a (H + 1) x (W + 1) grid (x0 = -1 /
//             y0 = -1: only the right / lower corners are inside), rows without one a key past the grid; a STABLE radix sort of
//             (key, row) leaves each cell's rows as one run in row order; a pass over the sorted keys notes where each run begins;
//             then one lane per pixel walks the runs of the four cells whose footprint holds the pixel as a four-way merge by row
//             index, adding weight * coef in fp64, and stores (g / n) * sum: every pixel is written, the untouched ones with 0.
//             The order of a pixel's sum is the row order and nothing else, so two runs give the same bits, and so do two layouts
//             of the same depth values.  n = 0 (or M = 0) stores zeros.  (The library sort uses integer atomics and look-back inside; a stable
//             sort has one result.)  A cell's run is walked serially by the lane of each of its four pixels: the time grows with the most
//             crowded cell, O(M) steps of one lane when all rows of a camera share a cell.  The image, depth_gt and valid are not read again.
// projection.  One (camera, world point) per lane, all arithmetic in fp64 from the fp32 inputs, one rounding per output:
//   p_cam = R^T (p_world - t) with [R | t] = camtoworld[:3] (the RIGID inverse, taken here per camera: the call assumes R orthonormal,
//   where the reference inverts a general 4 x 4), q = K p_cam, (x, y) = q.xy / q.z, depth = p_cam.z,
//   valid = visible && 0 <= x < W && 0 <= y < H && depth > 0, decided on the fp64 values as the reference decides it in numpy.
#include "scene_common.h"
#include "wm_kernels.h"

namespace {

constexpr int DL_THREADS = 256;

struct DlGeom {
  int C, H, W, M;
  long long sc, sh, sw;      // element strides of the depth image
};

// header of the workspace, behind the per-block pairs: what the backward reads of the forward's result
struct DlHeader {
  double n;                  // valid rows
  double sum;                // sum of their terms
};

template <bool WANT_BWD>
__global__ __launch_bounds__(DL_THREADS) WM_NO_PACKED_FP32 void depthloss_fwd_kernel(const float* __restrict__ depth, DlGeom g,
                                                                                     const float* __restrict__ points,
                                                                                     const float* __restrict__ depth_gt,
                                                                                     const unsigned char* __restrict__ valid,
                                                                                     double* __restrict__ partials, float* __restrict__ coef) {
  __shared__ double sRed[2][DL_THREADS / 64];
  const long long rows = (long long)g.C * g.M;
  const long long e = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
  double term = 0.0, cnt = 0.0;
  float cf = 0.f;
  if (e < rows && (!valid || valid[e])) {
    const int c = (int)(e / g.M);
    const double px = points[2 * e], py = points[2 * e + 1];
    const double fx0 = floor(px), fy0 = floor(py);
    double d = 0.0;
    // a corner is read only when it lies inside the image; a coordinate that is NaN or far outside fails every test
    if (px >= -1.0 && px < (double)g.W && py >= -1.0 && py < (double)g.H) {
      const int x0 = (int)fx0, y0 = (int)fy0;
      const double fx = px - fx0, fy = py - fy0;
      const float* img = depth + c * g.sc;
      const bool xa = x0 >= 0, xb = x0 + 1 < g.W, ya = y0 >= 0, yb = y0 + 1 < g.H;
      const double v00 = xa && ya ? (double)img[y0 * g.sh + x0 * g.sw] : 0.0;
      const double v01 = xb && ya ? (double)img[y0 * g.sh + (x0 + 1) * g.sw] : 0.0;
      const double v10 = xa && yb ? (double)img[(y0 + 1) * g.sh + x0 * g.sw] : 0.0;
      const double v11 = xb && yb ? (double)img[(y0 + 1) * g.sh + (x0 + 1) * g.sw] : 0.0;
      d = v00 * ((1.0 - fx) * (1.0 - fy)) + v01 * (fx * (1.0 - fy)) + v10 * ((1.0 - fx) * fy) + v11 * (fx * fy);
    }
    const double disp = d > 0.0 ? 1.0 / d : 0.0;
    const double diff = disp - 1.0 / (double)depth_gt[e];
    term = fabs(diff);
    cnt = 1.0;
    if (WANT_BWD && d > 0.0) cf = (float)(((diff > 0.0) - (diff < 0.0)) * (-1.0 / (d * d)));
  }
  if (WANT_BWD && e < rows) coef[e] = cf;
  // every thread reaches the barrier: no return above it
  term = wave_sum(term);
  cnt = wave_sum(cnt);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sRed[0][tid >> 6] = term; sRed[1][tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, n = 0.0;
    for (int w = 0; w < DL_THREADS / 64; ++w) { s += sRed[0][w]; n += sRed[1][w]; }
    partials[2 * (size_t)blockIdx.x] = s;
    partials[2 * (size_t)blockIdx.x + 1] = n;
  }
}

// the per-block pairs in index order -> the mean and the header
__global__ __launch_bounds__(DL_THREADS) void depthloss_reduce_kernel(const double* __restrict__ partials, int nblk, DlHeader* hdr, float* out) {
  __shared__ double sS[DL_THREADS], sN[DL_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, n = 0.0;
  for (int i = tid; i < nblk; i += DL_THREADS) { s += partials[2 * (size_t)i]; n += partials[2 * (size_t)i + 1]; }
  sS[tid] = s; sN[tid] = n;
  __syncthreads();
  for (int h = DL_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) { sS[tid] += sS[tid + h]; sN[tid] += sN[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    hdr->n = sN[0]; hdr->sum = sS[0];
    *out = (float)(sS[0] / sN[0]);      // n = 0: 0 / 0 = NaN
  }
}

// key of row e: its base cell, or `none` (past every cell) when the row adds to no pixel
__global__ __launch_bounds__(DL_THREADS) void depthloss_keys_kernel(DlGeom g, const float* __restrict__ points, const float* __restrict__ coef,
                                                                    unsigned int none, unsigned int* __restrict__ keys,
                                                                    unsigned int* __restrict__ vals) {
  const long long rows = (long long)g.C * g.M;
  const long long e = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
  if (e >= rows) return;
  unsigned int key = none;
  if (coef[e] != 0.f) {      // (an invalid row has coef 0: its coordinates are not looked at)
    const double px = points[2 * e], py = points[2 * e + 1];
    if (px >= -1.0 && px < (double)g.W && py >= -1.0 && py < (double)g.H) {
      const int c = (int)(e / g.M);
      const int x0 = (int)floor(px), y0 = (int)floor(py);       // -1 .. W - 1, -1 .. H - 1
      key = (unsigned int)((c * (g.H + 1) + (y0 + 1)) * (g.W + 1) + (x0 + 1));
    }
  }
  keys[e] = key;
  vals[e] = (unsigned int)e;
}

// start[cell] = first position of the cell's run in the sorted keys (start was filled with -1)
__global__ __launch_bounds__(DL_THREADS) void depthloss_starts_kernel(const unsigned int* __restrict__ keys, long long rows, unsigned int none,
                                                                      int* __restrict__ start) {
  const long long i = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
  if (i >= rows) return;
  const unsigned int k = keys[i];
  if (k < none && (i == 0 || keys[i - 1] != k)) start[k] = (int)i;
}

struct DlBwdArgs {
  DlGeom g;
  long long vc, vh, vw;      // element strides of v_depth
  const float* points; const float* coef;
  const unsigned int* keys; const unsigned int* vals;      // sorted
  const int* start;
  const DlHeader* hdr; const float* gout;
  float* v_depth;
  int have_lists;            // 0: no rows at all (M = 0), nothing was sorted
};

__global__ __launch_bounds__(DL_THREADS) WM_NO_PACKED_FP32 void depthloss_bwd_kernel(DlBwdArgs a) {
  const DlGeom g = a.g;
  const long long pixels = (long long)g.C * g.H * g.W;
  const long long p = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
  if (p >= pixels) return;
  const int x = (int)(p % g.W), y = (int)((p / g.W) % g.H), c = (int)(p / ((long long)g.W * g.H));
  const double n = a.hdr->n;
  double acc = 0.0;
  if (a.have_lists && n > 0.0) {
    const long long rows = (long long)g.C * g.M;
    // the four cells whose footprint holds (x, y): base (x - dx, y - dy); cell index of base (bx, by) is (by + 1, bx + 1)
    long long pos[4];
    unsigned int cell[4], head[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int dx = q & 1, dy = q >> 1;
      cell[q] = (unsigned int)((c * (g.H + 1) + (y - dy + 1)) * (g.W + 1) + (x - dx + 1));
      const int s = a.start[cell[q]];
      pos[q] = s;
      head[q] = s >= 0 ? a.vals[s] : 0xffffffffu;
    }
    for (;;) {
      // the run whose next row has the smallest index
      int q = 0;
      unsigned int m = head[0];
#pragma unroll
      for (int r = 1; r < 4; ++r)
        if (head[r] < m) { m = head[r]; q = r; }
      if (m == 0xffffffffu) break;
      const double px = a.points[2 * (size_t)m], py = a.points[2 * (size_t)m + 1];
      const double fx = px - floor(px), fy = py - floor(py);
      const double w = ((q & 1) ? fx : 1.0 - fx) * ((q >> 1) ? fy : 1.0 - fy);
      acc += w * (double)a.coef[m];
      // advance run q (selected without indexing the arrays by a run-time value: they stay in registers)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r == q) {
          const long long nx = pos[r] + 1;
          const bool more = nx < rows && a.keys[nx] == cell[r];
          pos[r] = nx;
          head[r] = more ? a.vals[nx] : 0xffffffffu;
        }
      }
    }
    acc *= (double)*a.gout / n;
  }
  a.v_depth[c * a.vc + y * a.vh + x * a.vw] = (float)acc;
}

__global__ __launch_bounds__(DL_THREADS) WM_NO_PACKED_FP32 void depth_project_kernel(const float* __restrict__ pw, const float* __restrict__ c2w,
                                                                                     const float* __restrict__ Ks,
                                                                                     const unsigned char* __restrict__ visible, int C, int P, int W,
                                                                                     int H, float* __restrict__ points, float* __restrict__ depths,
                                                                                     unsigned char* __restrict__ valid) {
  const long long e = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
  if (e >= (long long)C * P) return;
  const int c = (int)(e / P), p = (int)(e - (long long)c * P);
  const float* T = c2w + 16 * c;
  const float* K = Ks + 9 * c;
  const double dx = (double)pw[3 * (size_t)p] - (double)T[3], dy = (double)pw[3 * (size_t)p + 1] - (double)T[7], dz = (double)pw[3 * (size_t)p + 2] - (double)T[11];
  double pc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) pc[i] = (double)T[i] * dx + (double)T[4 + i] * dy + (double)T[8 + i] * dz;      // R^T (p - t)
  double q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = (double)K[3 * i] * pc[0] + (double)K[3 * i + 1] * pc[1] + (double)K[3 * i + 2] * pc[2];
  const double x = q[0] / q[2], y = q[1] / q[2];
  points[2 * e] = (float)x;
  points[2 * e + 1] = (float)y;
  depths[e] = (float)pc[2];
  const bool vis = !visible || visible[e];
  valid[e] = (vis && x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H && pc[2] > 0.0) ? 1 : 0;
}

bool dl_sizes_ok(int C, int H, int W, int M) {
  if (C < 1 || H < 2 || W < 2 || M < 0) return false;
  if ((long long)C * (H + 1) * (W + 1) >= (1LL << 31) - 1) return false;      // cell keys (and one past them) in 31 bits
  if ((long long)C * M >= (1LL << 30)) return false;                           // row indices, 2 * row + 1 for a coordinate
  return true;
}

struct DlWs {
  double* partials; DlHeader* hdr; float* coef;
  unsigned int* keys[2]; unsigned int* vals[2];
  int* start;
  void* cub; size_t cub_bytes;
  size_t fwd_total, total;
  int nblk, bits;
};

// with_backward = false stops behind the forward's part: no size query, nothing beyond fwd_total is valid
DlWs dl_carve(char* base, int C, int H, int W, int M, bool with_backward) {
  DlWs w{};
  Carver c(base);
  const size_t rows = (size_t)C * M, cells = (size_t)C * (H + 1) * (W + 1);
  w.nblk = (int)blocks_for((long long)rows, DL_THREADS);
  w.partials = c.take<double>((size_t)(w.nblk ? w.nblk : 1) * 2);
  w.hdr = c.take<DlHeader>(1);
  w.fwd_total = c.total();
  if (!with_backward) { w.total = c.total(); return w; }
  w.coef = c.take<float>(rows);
  w.keys[0] = c.take<unsigned int>(rows); w.keys[1] = c.take<unsigned int>(rows);
  w.vals[0] = c.take<unsigned int>(rows); w.vals[1] = c.take<unsigned int>(rows);
  w.start = c.take<int>(cells);
  w.bits = 1;
  while (w.bits < 32 && (cells >> w.bits) != 0) ++w.bits;      // the key of a row without a cell, `cells`, is the largest
  // The sort's scratch by a rule of our own, not by the library's size query: the query needs a device for all but small inputs (it fails on
  // a machine without one), and a size call must give the same number everywhere.  With both buffers of (key, row) handed over, the
  // library keeps digit histograms and one look-back word per digit and block of a few thousand pairs: well under a byte per pair.  8 bytes
  // per row + 1 MiB is several times that; the backward asks the library what it needs and refuses (hipErrorOutOfMemory) if it were more.
  w.cub_bytes = 8 * rows + ((size_t)1 << 20);
  w.cub = c.take<char>(w.cub_bytes);
  w.total = c.total();
  return w;
}

DlGeom dl_geom(const WmDepthLossArgs& a) { return DlGeom{a.C, a.H, a.W, a.M, a.strides[0], a.strides[1], a.strides[2]}; }

}  // namespace

size_t wm_depthloss_workspace_bytes(int C, int H, int W, int M, int want_backward) {
  if (!dl_sizes_ok(C, H, W, M)) return 0;
  const DlWs w = dl_carve(nullptr, C, H, W, M, want_backward != 0);
  return w.total;
}

hipError_t wm_launch_depthloss_fwd(const WmDepthLossArgs& a, int want_backward, float* out, hipStream_t s) {
  if (!dl_sizes_ok(a.C, a.H, a.W, a.M)) return hipErrorInvalidValue;
  const DlWs w = dl_carve((char*)a.workspace, a.C, a.H, a.W, a.M, want_backward != 0);
  if (a.workspace_bytes < w.total) return hipErrorInvalidValue;
  const DlGeom g = dl_geom(a);
  if (w.nblk > 0) {
    if (want_backward)
      hipLaunchKernelGGL(depthloss_fwd_kernel<true>, dim3((unsigned)w.nblk), dim3(DL_THREADS), 0, s, a.depth, g, a.points, a.depth_gt, a.valid,
                         w.partials, w.coef);
    else
      hipLaunchKernelGGL(depthloss_fwd_kernel<false>, dim3((unsigned)w.nblk), dim3(DL_THREADS), 0, s, a.depth, g, a.points, a.depth_gt, a.valid,
                         w.partials, (float*)nullptr);
  }
  hipLaunchKernelGGL(depthloss_reduce_kernel, dim3(1), dim3(DL_THREADS), 0, s, (const double*)w.partials, w.nblk, w.hdr, out);
  return hipGetLastError();
}

hipError_t wm_launch_depthloss_bwd(const WmDepthLossArgs& a, const float* gout, float* v_depth, const int64_t* v_strides, hipStream_t s) {
  if (!dl_sizes_ok(a.C, a.H, a.W, a.M)) return hipErrorInvalidValue;
  const DlWs w = dl_carve((char*)a.workspace, a.C, a.H, a.W, a.M, true);
  if (a.workspace_bytes < w.total || !v_strides) return hipErrorInvalidValue;
  DlBwdArgs k;
  k.g = DlGeom{a.C, a.H, a.W, a.M, 0, 0, 0};      // the depth image itself is not read again: the coefficients are in the workspace
  k.vc = v_strides[0]; k.vh = v_strides[1]; k.vw = v_strides[2];
  k.points = a.points; k.coef = w.coef; k.start = w.start; k.hdr = w.hdr; k.gout = gout; k.v_depth = v_depth;
  k.keys = w.keys[0]; k.vals = w.vals[0];
  k.have_lists = w.nblk > 0 ? 1 : 0;
  const long long rows = (long long)a.C * a.M;
  const size_t cells = (size_t)a.C * (a.H + 1) * (a.W + 1);
  if (k.have_lists) {
    const unsigned int none = (unsigned int)cells;
    hipLaunchKernelGGL(depthloss_keys_kernel, dim3((unsigned)w.nblk), dim3(DL_THREADS), 0, s, k.g, a.points, (const float*)w.coef, none, w.keys[0],
                       w.vals[0]);
    hipcub::DoubleBuffer<unsigned int> dk(w.keys[0], w.keys[1]), dv(w.vals[0], w.vals[1]);
    hipError_t e = sort_pairs(w.cub, w.cub_bytes, dk, dv, (int)rows, 0, w.bits, s);      // stable: a cell's rows stay in row order
    if (e != hipSuccess) return e;
    k.keys = dk.Current(); k.vals = dv.Current();
    e = hipMemsetAsync(w.start, 0xff, cells * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(depthloss_starts_kernel, dim3((unsigned)w.nblk), dim3(DL_THREADS), 0, s, k.keys, rows, none, w.start);
  }
  const long long pixels = (long long)a.C * a.H * a.W;
  hipLaunchKernelGGL(depthloss_bwd_kernel, dim3(blocks_for(pixels, DL_THREADS)), dim3(DL_THREADS), 0, s, k);
  return hipGetLastError();
}

hipError_t wm_launch_depth_project(const float* points_world, const float* camtoworlds, const float* Ks, const unsigned char* visible, int C, int P,
                                   int W, int H, float* points, float* depths, unsigned char* valid, hipStream_t s) {
  if (C < 1 || P < 0 || W < 1 || H < 1 || (long long)C * P >= (1LL << 30)) return hipErrorInvalidValue;
  if (P == 0) return hipSuccess;
  const long long rows = (long long)C * P;
  hipLaunchKernelGGL(depth_project_kernel, dim3(blocks_for(rows, DL_THREADS)), dim3(DL_THREADS), 0, s, points_world, camtoworlds,
                     Ks, visible, C, P, W, H, points, depths, valid);
  return hipGetLastError();
}
