// gsplat's MCMCStrategy (gsplat/strategy/mcmc.py, ops.py:240-369; "3D Gaussian Splatting as Markov Chain Monte Carlo",
// arXiv:2404.09591) — the other half of the strategy union of the reference's "Post 3DGS Optimization" trainer.  Five calls, no float
// atomics, every result independent of the launch order:
//   inject_noise  every step (ops.py:343-369): one thread per Gaussian, one pass, 14 floats in and 3 out.  A wave's three dword loads of
//                 a [N,3] tensor cover 768 consecutive bytes (six whole 128-byte lines, no line shared with another wave), its float4
//                 load of the quaternions 1 KiB, its opacities 256 bytes.  The gate 1 / (1 + exp(-100 (sigmoid(-o) - 0.995))) loses
//                 seven digits to the factor 100 when it is formed in fp32, so its two exponentials are fp64; everything else is fp32.
//   partition     at a refinement (mcmc.py:154-155, ops.py:258-259): dead = sigmoid(o) <= min_opacity, or a caller's byte mask; one
//                 exclusive sum (rocPRIM through hipCUB) gives every destination in both ascending lists.
//   relocation    eq. 9 of the paper (RelocationCUDA.cu:26-43) for the drawn sources: an integer histogram of the draw, then per
//                 draw the new opacity and scale in fp64, rounded once.  The double sum over (i, k) collapses by the hockey-stick
//                 identity sum_{i=k+1..n} C(i-1, k) = C(n, k+1) to one sum of n terms; the binomials come by recurrence.
//   scatter       param_fn of relocate and sample_add (ops.py:280-286, 322-328): sampled rows take their new values, dest rows a copy.
//   zero_rows     optimizer_fn of relocate (ops.py:288-290).
#include <cfloat>

#include "scene_common.h"
#include "wm_kernels.h"

namespace {

__global__ __launch_bounds__(256) void mcmc_noise_kernel(float* __restrict__ means, const float* __restrict__ quats,
                                                         const float* __restrict__ scales, const float* __restrict__ opacities,
                                                         const float* __restrict__ noise, float scaler, int N) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  const size_t g3 = (size_t)g * 3;
  const float4 q = ((const float4*)quats)[g];
  const float n0 = noise[g3], n1 = noise[g3 + 1], n2 = noise[g3 + 2];
  const float l0 = scales[g3], l1 = scales[g3 + 1], l2 = scales[g3 + 2];
  const float m0 = means[g3], m1 = means[g3 + 1], m2 = means[g3 + 2];
  // 1 - sigmoid(o) = sigmoid(-o), without the cancellation
  const double a = 1.0 / (1.0 + exp((double)opacities[g]));
  const float gate = (float)(1.0 / (1.0 + exp(-100.0 * (a - 0.995))));
  const float v0 = n0 * gate * scaler, v1 = n1 * gate * scaler, v2 = n2 * gate * scaler;
  const float qn = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);   // F.normalize
  const float w = q.x / qn, x = q.y / qn, y = q.z / qn, z = q.w / qn;
  const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - w * z), r02 = 2.f * (x * z + w * y);
  const float r10 = 2.f * (x * y + w * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - w * x);
  const float r20 = 2.f * (x * z - w * y), r21 = 2.f * (y * z + w * x), r22 = 1.f - 2.f * (x * x + y * y);
  // Sigma v = R S^2 (R^T v)
  const float s0 = expf(l0), s1 = expf(l1), s2 = expf(l2);
  const float t0 = s0 * s0 * (r00 * v0 + r10 * v1 + r20 * v2);
  const float t1 = s1 * s1 * (r01 * v0 + r11 * v1 + r21 * v2);
  const float t2 = s2 * s2 * (r02 * v0 + r12 * v1 + r22 * v2);
  means[g3] = m0 + (r00 * t0 + r01 * t1 + r02 * t2);
  means[g3 + 1] = m1 + (r10 * t0 + r11 * t1 + r12 * t2);
  means[g3 + 2] = m2 + (r20 * t0 + r21 * t1 + r22 * t2);
}

// item N is the zero tail, so that the exclusive sum leaves the number of dead Gaussians at [N]
__global__ __launch_bounds__(256) void mcmc_dead_kernel(const float* __restrict__ opacities, const unsigned char* __restrict__ mask, int N,
                                                        float min_opacity, unsigned int* __restrict__ flags) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > N) return;
  unsigned int f = 0u;
  if (g < N) f = mask ? (mask[g] != 0) : (1.0f / (1.0f + expf(-opacities[g])) <= min_opacity);
  flags[g] = f;
}

__global__ __launch_bounds__(256) void mcmc_partition_kernel(const unsigned int* __restrict__ flags, const unsigned int* __restrict__ excl, int N,
                                                             int* __restrict__ dead_idx, int* __restrict__ alive_idx,
                                                             int* __restrict__ counts_dev) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  const unsigned int e = excl[g];
  if (g == 0) { counts_dev[0] = (int)excl[N]; counts_dev[1] = N - (int)excl[N]; }
  if (flags[g]) dead_idx[e] = g;
  else alive_idx[(unsigned int)g - e] = g;
}

__global__ __launch_bounds__(256) void mcmc_hist_kernel(const int* __restrict__ sampled, int n_sampled, int N, int* __restrict__ hist) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_sampled) return;
  const int g = sampled[j];
  if ((unsigned int)g < (unsigned int)N) atomicAdd(&hist[g], 1);
}

__global__ __launch_bounds__(256) void mcmc_relocation_kernel(const float* __restrict__ opacities, const float* __restrict__ scales,
                                                              const int* __restrict__ sampled, const int* __restrict__ hist, int n_sampled,
                                                              int N, float min_opacity, float* __restrict__ new_opacities,
                                                              float* __restrict__ new_scales) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_sampled) return;
  const int g = sampled[j];
  if ((unsigned int)g >= (unsigned int)N) return;
  const int ratio = min(max(hist[g] + 1, 1), 51);
  const double o = 1.0 / (1.0 + exp(-(double)opacities[g]));
  const double x = -expm1(log1p(-o) / (double)ratio);            // 1 - (1 - o)^(1 / ratio)
  // denom = sum_{k=0..ratio-1} C(ratio, k+1) (-1)^k / sqrt(k+1) x^(k+1);  c = (-1)^k C(ratio, k+1) x^(k+1)
  double c = (double)ratio * x, denom = 0.0;
  for (int k = 0; k < ratio; ++k) {
    denom += c / sqrt((double)(k + 1));
    c *= -x * (double)(ratio - k - 1) / (double)(k + 2);
  }
  const double coeff = o / denom;
  const double xo = fmin(fmax(x, (double)min_opacity), 1.0 - (double)FLT_EPSILON);
  new_opacities[j] = (float)log(xo / (1.0 - xo));
  for (int i = 0; i < 3; ++i) new_scales[(size_t)j * 3 + i] = (float)log(coeff * exp((double)scales[(size_t)g * 3 + i]));
}

// one thread per element of the n_sampled drawn rows
__global__ __launch_bounds__(256) void mcmc_scatter_kernel(float* __restrict__ t, int rows, int R, const int* __restrict__ sampled,
                                                           const int* __restrict__ dest, const float* __restrict__ values, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t j = i / (size_t)R;
  const int col = (int)(i - j * (size_t)R);
  const int s = sampled[j], d = dest[j];
  if ((unsigned int)s >= (unsigned int)rows || (unsigned int)d >= (unsigned int)rows) return;
  float v;
  if (values) { v = values[i]; t[(size_t)s * R + col] = v; }    // a repeated source is written with the same value by every writer
  else v = t[(size_t)s * R + col];
  t[(size_t)d * R + col] = v;
}

__global__ __launch_bounds__(256) void mcmc_zero_rows_kernel(float* __restrict__ t, int rows, int R, const int* __restrict__ idx, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t j = i / (size_t)R;
  const int g = idx[j];
  if ((unsigned int)g < (unsigned int)rows) t[(size_t)g * R + (i - j * (size_t)R)] = 0.f;
}

struct PartWs { unsigned int* flags; unsigned int* excl; int* counts; void* cub; size_t cub_bytes, total; };

PartWs carve(char* base, size_t N) {
  PartWs w;
  Carver c(base);
  w.flags = c.take<unsigned int>(N + 1);
  w.excl = c.take<unsigned int>(N + 1);
  w.counts = c.take<int>(2);
  w.cub_bytes = exclusive_sum_bytes<unsigned int>((int)(N + 1));
  w.cub = c.take<char>(w.cub_bytes);
  w.total = c.total();
  return w;
}

bool grid_ok(size_t total) { return (total + 255) / 256 < (1ull << 31); }

}  // namespace

hipError_t wm_launch_mcmc_inject_noise(float* means, const float* quats, const float* scales, const float* opacities, const float* noise,
                                       float scaler, int N, hipStream_t s) {
  if (N < 0) return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, means, quats, scales, opacities, noise, scaler, N);
  return hipGetLastError();
}

size_t wm_mcmc_partition_ws_bytes(size_t N) { return carve(nullptr, N).total; }

hipError_t wm_launch_mcmc_partition(const float* opacities, const unsigned char* mask, int N, float min_opacity, int* dead_idx, int* alive_idx,
                                    int* counts_host, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (N <= 0 || (size_t)N >= (1ull << 31) - 1) return hipErrorInvalidValue;
  PartWs w = carve((char*)workspace, (size_t)N);
  if (w.total > workspace_bytes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mcmc_dead_kernel, dim3((unsigned)(((size_t)N + 1 + 255) / 256)), dim3(256), 0, s, opacities, mask, N, min_opacity, w.flags);
  hipError_t e = exclusive_sum(w.cub, w.cub_bytes, w.flags, w.excl, N + 1, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcmc_partition_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, w.flags, w.excl, N, dead_idx, alive_idx, w.counts);
  e = read_back(counts_host, w.counts, 2 * sizeof(int), s);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t wm_launch_mcmc_relocation(const float* opacities, const float* scales, const int* sampled, int n_sampled, int N, float min_opacity,
                                     float* new_opacities, float* new_scales, int* hist, hipStream_t s) {
  if (N <= 0 || n_sampled < 0) return hipErrorInvalidValue;
  if (n_sampled == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * sizeof(int), s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n_sampled + 255) / 256));
  hipLaunchKernelGGL(mcmc_hist_kernel, grid, dim3(256), 0, s, sampled, n_sampled, N, hist);
  hipLaunchKernelGGL(mcmc_relocation_kernel, grid, dim3(256), 0, s, opacities, scales, sampled, (const int*)hist, n_sampled, N, min_opacity,
                     new_opacities, new_scales);
  return hipGetLastError();
}

hipError_t wm_launch_mcmc_scatter(float* t, int rows, int R, const int* sampled, const int* dest, const float* values, int n_sampled,
                                  hipStream_t s) {
  if (rows <= 0 || R <= 0 || n_sampled < 0) return hipErrorInvalidValue;
  if (n_sampled == 0) return hipSuccess;
  const size_t total = (size_t)n_sampled * (size_t)R;
  if (!grid_ok(total)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mcmc_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t, rows, R, sampled, dest, values, total);
  return hipGetLastError();
}

hipError_t wm_launch_mcmc_zero_rows(float* t, int rows, int R, const int* idx, int n, hipStream_t s) {
  if (rows <= 0 || R <= 0 || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const size_t total = (size_t)n * (size_t)R;
  if (!grid_ok(total)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mcmc_zero_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t, rows, R, idx, total);
  return hipGetLastError();
}
