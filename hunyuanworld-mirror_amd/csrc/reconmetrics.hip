// The reductions of a point-cloud evaluation (recon_metrics.py) around the nearest-point search of knn.hip: the statistics of one direction
// (wm_cloud_stats) and the moments and closed form of Umeyama's similarity (wm_umeyama).  The C-ABI entries are in wm_api_scene.cpp; the
// launchers are declared in wm_api.h.
//
//   sums      every sum is fp64 over a FIXED shape: at most 256 blocks of 256 threads, a thread adds its grid-strided elements in index
//             order, a wave adds its lanes by the xor butterfly, a block its four waves in order, and one thread per value adds the blocks'
//             partial sums in block order.  The shape depends on the element count alone: the same input gives the same bits.  Counts
//             (dist < tau, kept pairs) ride the same sums as doubles, which are exact below 2^53.
//   median    np.median: the order statistics of rank floor((M - 1) / 2) and floor(M / 2), found together by a most-significant-digit
//             radix select over the order-preserving image of the floats (four passes of 8 bits: a histogram of the elements that share
//             the digits chosen so far, then the digit that holds the rank); their mean in fp64.  Exact; integer atomics only.  A NaN
//             ranks above +inf.
//   normals   |n_a[i] . n_b[idx[i]]| in fp32, each operation rounded on its own; idx outside 0 .. Nb-1 (the -1 of a non-finite query) gives NaN.
//   umeyama   pass 1: the count and the two means of the pairs the mask keeps; pass 2: the centred 3 x 3 cross-covariance and the source
//             variance about those means (the differences are taken in fp64, so nothing cancels); then umeyama_solve.h on one thread.
#include "scene_common.h"
#include "umeyama_solve.h"
#include "wm_api.h"

namespace {

constexpr int RM_THREADS = 256;
constexpr unsigned RM_BLOCKS = 256;
constexpr int RM_NSTAT = 1 + WM_STATS_MAX_THRESHOLDS;

struct RmTaus { float t[WM_STATS_MAX_THRESHOLDS]; int n; };

inline unsigned rm_grid(long long n) { const unsigned b = blocks_for(n, RM_THREADS); return b < RM_BLOCKS ? (b ? b : 1u) : RM_BLOCKS; }

// v[NV] of every thread -> part[blockIdx.x][NV]; every thread calls it
template <int NV>
__device__ __forceinline__ void rm_block_sums(const double* v, double* __restrict__ part) {
  __shared__ double sW[RM_THREADS / 64][NV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double t = wave_sum(v[k]);
    if (lane == 0) sW[w][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = sW[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < RM_THREADS / 64; ++i) t += sW[i][threadIdx.x];
    part[(size_t)blockIdx.x * NV + threadIdx.x] = t;
  }
}

__device__ __forceinline__ double rm_sum_blocks(const double* __restrict__ part, unsigned nb, int nv, int k) {
  double t = 0.0;
  for (unsigned b = 0; b < nb; ++b) t += part[(size_t)b * nv + k];
  return t;
}

// ------------------------------------------------------------------ direction statistics
#pragma clang fp contract(off)      // from here on (the fp32 dot product below): no fused multiply-add
__global__ __launch_bounds__(RM_THREADS) void rm_nc_kernel(const int* __restrict__ idx, const float* __restrict__ na, const float* __restrict__ nb,
                                                           long long M, long long Nb, float* __restrict__ nc) {
  const long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x;
  if (i >= M) return;
  const long long j = idx[i];
  float v = __int_as_float(0x7fc00000);
  if (j >= 0 && j < Nb) {
    const float* a = na + 3 * i;
    const float* b = nb + 3 * j;
    v = fabsf((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);      // each operation rounded on its own
  }
  nc[i] = v;
}

__global__ __launch_bounds__(RM_THREADS) void rm_stat_sums_kernel(const float* __restrict__ x, long long M, RmTaus taus, double* __restrict__ part) {
  double v[RM_NSTAT];
#pragma unroll
  for (int k = 0; k < RM_NSTAT; ++k) v[k] = 0.0;
  for (long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x; i < M; i += (long long)gridDim.x * RM_THREADS) {
    const float d = x[i];
    v[0] += (double)d;
#pragma unroll
    for (int k = 0; k < WM_STATS_MAX_THRESHOLDS; ++k)
      if (k < taus.n && d < taus.t[k]) v[1 + k] += 1.0;
  }
  rm_block_sums<RM_NSTAT>(v, part);
}

// out_mean = sum / M; counts[k] (when counts is not null) = the k-th count
__global__ void rm_stat_finish_kernel(const double* __restrict__ part, unsigned nb, long long M, int n_taus, double* __restrict__ out_mean,
                                      double* __restrict__ counts) {
  const int k = threadIdx.x;
  if (k == 0) *out_mean = rm_sum_blocks(part, nb, RM_NSTAT, 0) / (double)M;
  else if (counts && k <= n_taus) counts[k - 1] = rm_sum_blocks(part, nb, RM_NSTAT, k);
}

// the select's state: hist [2][256], prefix [2], remain [2]
__global__ void rm_select_init_kernel(unsigned int* __restrict__ st, unsigned int M) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) st[i] = 0u;
  if (threadIdx.x == 0) { st[512] = 0u; st[513] = 0u; st[514] = (M - 1u) >> 1; st[515] = M >> 1; }
}

__global__ __launch_bounds__(RM_THREADS) void rm_select_hist_kernel(const float* __restrict__ x, long long M, int pass, unsigned int* __restrict__ st) {
  __shared__ unsigned int sh[512];
  for (int i = threadIdx.x; i < 512; i += RM_THREADS) sh[i] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned int p0 = st[512], p1 = st[513];
  for (long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x; i < M; i += (long long)gridDim.x * RM_THREADS) {
    const unsigned int key = ordered_key(x[i]);
    const unsigned int digit = (key >> shift) & 255u;
    if (pass == 0 || ((key ^ p0) >> (shift + 8)) == 0u) atomicAdd(&sh[digit], 1u);
    if (pass == 0 || ((key ^ p1) >> (shift + 8)) == 0u) atomicAdd(&sh[256 + digit], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += RM_THREADS)
    if (sh[i]) atomicAdd(&st[i], sh[i]);
}

// one block: the digit of either rank, the histograms cleared for the next pass; behind the last pass the median
__global__ void rm_select_pick_kernel(unsigned int* __restrict__ st, int pass, double* __restrict__ out) {
  if (threadIdx.x < 2) {
    const int r = threadIdx.x;
    unsigned int remain = st[514 + r], cum = 0u;
    int d = 0;
    for (; d < 255; ++d) {
      const unsigned int h = st[256 * r + d];
      if (cum + h > remain) break;
      cum += h;
    }
    st[514 + r] = remain - cum;
    st[512 + r] |= (unsigned int)d << (24 - 8 * pass);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += blockDim.x) st[i] = 0u;
  if (pass == 3 && threadIdx.x == 0) *out = 0.5 * ((double)ordered_value(st[512]) + (double)ordered_value(st[513]));
}

struct RmStatWs { double* part; unsigned int* sel; float* nc; size_t total; };

RmStatWs rm_stat_carve(char* base, size_t M) {
  RmStatWs w{};
  Carver c(base);
  w.part = c.take<double>((size_t)RM_BLOCKS * RM_NSTAT);
  w.sel = c.take<unsigned int>(516);
  w.nc = c.take<float>(M ? M : 1);
  w.total = c.total();
  return w;
}

// mean, median and counts of x [M]
void rm_stats_of(const float* x, long long M, const RmTaus& taus, const RmStatWs& w, double* out_mean, double* out_median, double* counts, hipStream_t s) {
  const unsigned nb = rm_grid(M);
  hipLaunchKernelGGL(rm_stat_sums_kernel, dim3(nb), dim3(RM_THREADS), 0, s, x, M, taus, w.part);
  hipLaunchKernelGGL(rm_stat_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)w.part, nb, M, taus.n, out_mean, counts);
  hipLaunchKernelGGL(rm_select_init_kernel, dim3(1), dim3(RM_THREADS), 0, s, w.sel, (unsigned int)M);
  const unsigned hb = blocks_for(M, RM_THREADS) < 1024u ? blocks_for(M, RM_THREADS) : 1024u;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(rm_select_hist_kernel, dim3(hb), dim3(RM_THREADS), 0, s, x, M, pass, w.sel);
    hipLaunchKernelGGL(rm_select_pick_kernel, dim3(1), dim3(RM_THREADS), 0, s, w.sel, pass, out_median);
  }
}

// ------------------------------------------------------------------ Umeyama
__device__ __forceinline__ bool rm_kept(const unsigned char* __restrict__ mask, long long i) { return !mask || mask[i] != 0; }

__global__ __launch_bounds__(RM_THREADS) void rm_um_means_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                                 const unsigned char* __restrict__ mask, long long P, double* __restrict__ part) {
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x; i < P; i += (long long)gridDim.x * RM_THREADS) {
    if (!rm_kept(mask, i)) continue;
    v[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { v[1 + a] += (double)src[3 * i + a]; v[4 + a] += (double)dst[3 * i + a]; }
  }
  rm_block_sums<7>(v, part);
}

// mom: the count, the mean of src, the mean of dst (zeros for a count of 0)
__global__ void rm_um_means_finish_kernel(const double* __restrict__ part, unsigned nb, double* __restrict__ mom) {
  __shared__ double sv[7];
  if (threadIdx.x < 7) sv[threadIdx.x] = rm_sum_blocks(part, nb, 7, threadIdx.x);
  __syncthreads();
  if (threadIdx.x < 7) mom[threadIdx.x] = threadIdx.x == 0 ? sv[0] : (sv[0] > 0.0 ? sv[threadIdx.x] / sv[0] : 0.0);
}

__global__ __launch_bounds__(RM_THREADS) void rm_um_cov_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                               const unsigned char* __restrict__ mask, long long P, const double* __restrict__ mom,
                                                               double* __restrict__ part) {
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double ms[3] = {mom[1], mom[2], mom[3]}, md[3] = {mom[4], mom[5], mom[6]};
  for (long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x; i < P; i += (long long)gridDim.x * RM_THREADS) {
    if (!rm_kept(mask, i)) continue;
    double ds[3], dd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { ds[a] = (double)src[3 * i + a] - ms[a]; dd[a] = (double)dst[3 * i + a] - md[a]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) v[3 * a + b] += dd[a] * ds[b];
      v[9] += ds[a] * ds[a];
    }
  }
  rm_block_sums<10>(v, part);
}

// out [16]: s, R [9], t [3], the count, the source variance, 0.  A count of 0 gives NaNs.
__global__ void rm_um_solve_kernel(const double* __restrict__ part, unsigned nb, const double* __restrict__ mom, int with_scale,
                                   double* __restrict__ out) {
  __shared__ double sv[10];
  if (threadIdx.x < 10) sv[threadIdx.x] = rm_sum_blocks(part, nb, 10, threadIdx.x);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = mom[0];
  double cov[9], res[13];
  for (int i = 0; i < 9; ++i) cov[i] = sv[i] / n;
  const double var = sv[9] / n;
  um_solve(cov, var, mom + 1, mom + 4, with_scale, res);
  for (int i = 0; i < 13; ++i) out[i] = res[i];
  out[13] = n;
  out[14] = var;
  out[15] = 0.0;
}

struct RmUmWs { double* part; double* mom; size_t total; };

RmUmWs rm_um_carve(char* base) {
  RmUmWs w{};
  Carver c(base);
  w.part = c.take<double>((size_t)RM_BLOCKS * 10);
  w.mom = c.take<double>(8);
  w.total = c.total();
  return w;
}

}  // namespace

size_t wm_cloud_stats_ws_bytes(long long M) {
  if (M < 1 || M >= (1LL << 31)) return 0;
  return rm_stat_carve(nullptr, (size_t)M).total;
}

hipError_t wm_launch_cloud_stats(const float* dist, const int* idx, long long M, const float* normals_a, const float* normals_b, long long Nb,
                                 const float* thresholds, int n_thresholds, void* workspace, double* out, hipStream_t s) {
  if (M < 1 || M >= (1LL << 31) || n_thresholds < 0 || n_thresholds > WM_STATS_MAX_THRESHOLDS) return hipErrorInvalidValue;
  const RmStatWs w = rm_stat_carve((char*)workspace, (size_t)M);
  RmTaus taus{};
  taus.n = n_thresholds;
  for (int k = 0; k < n_thresholds; ++k) taus.t[k] = thresholds[k];
  rm_stats_of(dist, M, taus, w, out + 0, out + 1, out + 4, s);
  if (normals_a) {
    hipLaunchKernelGGL(rm_nc_kernel, dim3(blocks_for(M, RM_THREADS)), dim3(RM_THREADS), 0, s, idx, normals_a, normals_b, M, Nb, w.nc);
    taus.n = 0;
    rm_stats_of(w.nc, M, taus, w, out + 2, out + 3, nullptr, s);
  }
  return hipGetLastError();
}

size_t wm_umeyama_ws_bytes(long long P) {
  if (P < 1 || P >= (1LL << 31)) return 0;
  return rm_um_carve(nullptr).total;
}

hipError_t wm_launch_umeyama(const float* src, const float* dst, const unsigned char* mask, long long P, int with_scale, void* workspace, double* out,
                             hipStream_t s) {
  if (P < 1 || P >= (1LL << 31)) return hipErrorInvalidValue;
  const RmUmWs w = rm_um_carve((char*)workspace);
  const unsigned nb = rm_grid(P);
  hipLaunchKernelGGL(rm_um_means_kernel, dim3(nb), dim3(RM_THREADS), 0, s, src, dst, mask, P, w.part);
  hipLaunchKernelGGL(rm_um_means_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)w.part, nb, w.mom);
  hipLaunchKernelGGL(rm_um_cov_kernel, dim3(nb), dim3(RM_THREADS), 0, s, src, dst, mask, P, (const double*)w.mom, w.part);
  hipLaunchKernelGGL(rm_um_solve_kernel, dim3(1), dim3(64), 0, s, (const double*)w.part, nb, (const double*)w.mom, with_scale, out);
  return hipGetLastError();
}
