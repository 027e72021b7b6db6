// View-dependent colour for the 3D-Gaussian-splat rasteriser: real spherical harmonics of degree 1-3, forward and backward — what
// gsplat.rasterization does with sh_degree > 0 (gsplat/rendering.py:509-525: dirs = means - campos, spherical_harmonics(sh_degree,
// dirs, colors, masks = radii > 0), clamp_min(colors + 0.5, 0); the torch statement is _torch_impl.py:720-822), which the reference's
// post-3DGS trainer reaches by raising sh_degree_to_use during training (simple_trainer_worldmirror.py:613, :738-746).
//   colour    one thread per (camera, Gaussian), the grid of the projection, between projection and compositing: direction from the
//             camera position to the mean, normalised as F.normalize (d / max(|d|, 1e-12)), the (L + 1)^2 basis polynomials, the
//             coefficients of row g of [N,K,3] (K >= (L + 1)^2; higher bands are not read) -> max(colour + 0.5, 0) into the r, g, b of
//             the pair's projection record.  Culled pairs (empty tile rectangle) are left alone.
//   backward  one thread per Gaussian, cameras in order (the shape of raster_project_bwd_kernel, so every output has one writer).  Per
//             visible pair the colour cotangent is the sum of floats 6..8 of the pair's tile records, zero where the stored colour
//             channel is not > 0 (the clamp).  v_coeffs [N,K,3] accumulates in registers over the cameras (bands >= (L + 1)^2: exact
//             zeros); the direction's gradient goes back through the normalisation and is ADDED to v_means, which the projection
//             backward has written before on the same stream; its negative is the gradient of the camera position.
//   campos    with CAMPOS the three terms of a pair are summed over the wave's 64 lanes in fp64 by the fixed butterfly of the viewmats
//             gradient and stored by one lane as the wave's partial; the reducer adds the partials in a fixed order -> v_campos [C,3].
// No atomics; sums run in a fixed order everywhere.  L is a template parameter: degree 1 carries none of the degree-3 polynomials.
// Basis: sh_basis.h (the real SH polynomials in Cartesian form as published by Sloan, "Efficient Spherical Harmonic Evaluation", JCGT 2013).
#include "wm_common.h"
#include "wm_kernels.h"
#include "raster_common.h"
#include "raster_bwd_composite.h"
#include "sh_basis.h"

using namespace wm_raster;
using namespace wm_sh;

namespace {

__device__ __forceinline__ int rect_tiles(int rect) {
  return (((rect >> 16) & 255) - (rect & 255)) * (((rect >> 24) & 255) - ((rect >> 8) & 255));
}

template <int L>
__global__ __launch_bounds__(256) void raster_sh_color_kernel(const float* __restrict__ means, const float* __restrict__ coeffs, int K,
                                                              const float* __restrict__ campos, int N, G2D* __restrict__ g2d) {
  constexpr int NB = (L + 1) * (L + 1);
  const int g = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (g >= N) return;
  G2D* o = g2d + (size_t)c * N + g;
  if (rect_tiles(o->rect) <= 0) return;   // culled for this camera: no tile reads the record's colour
  const float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
  float x, y, z, den, B[NB];
  sh_direction(m, campos + 3 * c, x, y, z, den);
  sh_basis<L>(x, y, z, B);
  const float* row = coeffs + (size_t)g * K * 3;
  float col[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < NB; ++k)
#pragma unroll
    for (int i = 0; i < 3; ++i) col[i] += B[k] * row[3 * k + i];
  o->r = fmaxf(col[0] + 0.5f, 0.f); o->g = fmaxf(col[1] + 0.5f, 0.f); o->b = fmaxf(col[2] + 0.5f, 0.f);
}

// rec: floats per tile record of pair_grad (10, or 12 with absgrad).  CAMPOS: also write campos_part [C][3][waves] (fp64): per wave the
// sum over its Gaussians of minus the direction's gradient.  Lanes past N and culled pairs take part in the wave's sum with zeros.
template <int L, bool CAMPOS>
__global__ __launch_bounds__(256) void raster_sh_bwd_kernel(const float* __restrict__ means, const float* __restrict__ coeffs, int K,
                                                            const float* __restrict__ campos, int N, int C, const G2D* __restrict__ g2d,
                                                            const unsigned long long* __restrict__ pair_offs,
                                                            const float* __restrict__ pair_grad, int rec, float* __restrict__ v_means,
                                                            float* __restrict__ v_coeffs, double* __restrict__ campos_part) {
  constexpr int NB = (L + 1) * (L + 1);
  int g = blockIdx.x * 256 + threadIdx.x;
  bool live = true;
  if constexpr (CAMPOS) {
    if ((g & ~63) >= N) return;   // the whole wave is past N
    live = g < N;
    g = live ? g : N - 1;         // a lane past N reads the last Gaussian, adds zeros to the wave's sums and stores nothing
  } else {
    if (g >= N) return;
  }
  const float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
  const float* row = coeffs + (size_t)g * K * 3;
  float acc[3 * NB], a_m[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 3 * NB; ++i) acc[i] = 0.f;
  for (int c = 0; c < C; ++c) {
    const size_t idx = (size_t)c * N + g;
    const G2D* o = g2d + idx;
    const int cnt = rect_tiles(o->rect);
    float vd[3] = {0.f, 0.f, 0.f};
    if (live && cnt > 0) {
      float vc[3] = {0.f, 0.f, 0.f};
      const float* pr = pair_grad + pair_offs[idx] * (size_t)rec + 6;
      for (int t = 0; t < cnt; ++t) {
        vc[0] += pr[(size_t)t * rec]; vc[1] += pr[(size_t)t * rec + 1]; vc[2] += pr[(size_t)t * rec + 2];
      }
      vc[0] = o->r > 0.f ? vc[0] : 0.f; vc[1] = o->g > 0.f ? vc[1] : 0.f; vc[2] = o->b > 0.f ? vc[2] : 0.f;   // clamp_min(colour + 0.5, 0)
      float x, y, z, den, B[NB], w[NB], vdir[3];
      sh_direction(m, campos + 3 * c, x, y, z, den);
      sh_basis<L>(x, y, z, B);
#pragma unroll
      for (int k = 0; k < NB; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[3 * k + i] += B[k] * vc[i];
        w[k] = row[3 * k] * vc[0] + row[3 * k + 1] * vc[1] + row[3 * k + 2] * vc[2];
      }
      sh_basis_vjp<L>(x, y, z, w, vdir);
      const float dot = x * vdir[0] + y * vdir[1] + z * vdir[2];   // through d / max(|d|, 1e-12)
      vd[0] = (vdir[0] - x * dot) / den; vd[1] = (vdir[1] - y * dot) / den; vd[2] = (vdir[2] - z * dot) / den;
#pragma unroll
      for (int j = 0; j < 3; ++j) a_m[j] += vd[j];
    }
    if constexpr (CAMPOS) {
      const size_t waves = ((size_t)N + 63) / 64, wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double sum = wave_sum_hi_f64((double)-vd[j]);
        if ((threadIdx.x & 63) == 63) campos_part[((size_t)c * 3 + j) * waves + wave] = sum;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) v_means[3 * g + j] += a_m[j];
  float* out = v_coeffs + (size_t)g * K * 3;
#pragma unroll
  for (int i = 0; i < 3 * NB; ++i) out[i] = acc[i];
  for (int i = 3 * NB; i < 3 * K; ++i) out[i] = 0.f;
}

// v_campos [C,3]: one block per (component, camera), the order of raster_cam_reduce_kernel: thread t adds the partials of waves t,
// t + 256, ..., then the 256 thread sums pairwise in a fixed tree; rounded to fp32 once
__global__ __launch_bounds__(256) void raster_campos_reduce_kernel(const double* __restrict__ campos_part, size_t waves, float* __restrict__ v_campos) {
  __shared__ double sh[256];
  const int comp = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const double* part = campos_part + ((size_t)c * 3 + comp) * waves;
  double acc = 0.0;
  for (size_t w = t; w < waves; w += 256) acc += part[w];
  sh[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) v_campos[3 * c + comp] = (float)sh[0];
}

template <int L>
void launch_sh_bwd_degree(const WmRasterBwdArgs& b, const RasterWs& w, const float* pair_grad, int rec, double* campos_part, hipStream_t s) {
  const WmRasterArgs& a = b.fwd;
  const dim3 grid((unsigned)((a.N + 255) / 256));
  if (b.v_campos)
    hipLaunchKernelGGL((raster_sh_bwd_kernel<L, true>), grid, dim3(256), 0, s, a.means, a.colors, a.n_coeffs, a.campos, a.N, a.C, w.g2d, w.offsets,
                       pair_grad, rec, b.v_means, b.v_colors, campos_part);
  else
    hipLaunchKernelGGL((raster_sh_bwd_kernel<L, false>), grid, dim3(256), 0, s, a.means, a.colors, a.n_coeffs, a.campos, a.N, a.C, w.g2d, w.offsets,
                       pair_grad, rec, b.v_means, b.v_colors, nullptr);
}

}  // namespace

bool wm_raster::sh_args_valid(const WmRasterArgs& a) {
  return a.sh_degree >= 1 && a.sh_degree <= 3 && (a.sh_degree + 1) * (a.sh_degree + 1) <= a.n_coeffs && a.campos != nullptr;
}

void wm_raster::launch_sh_colors(const WmRasterArgs& a, G2D* g2d, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 255) / 256), (unsigned)a.C);
  if (a.sh_degree == 1)
    hipLaunchKernelGGL(raster_sh_color_kernel<1>, grid, dim3(256), 0, s, a.means, a.colors, a.n_coeffs, a.campos, a.N, g2d);
  else if (a.sh_degree == 2)
    hipLaunchKernelGGL(raster_sh_color_kernel<2>, grid, dim3(256), 0, s, a.means, a.colors, a.n_coeffs, a.campos, a.N, g2d);
  else
    hipLaunchKernelGGL(raster_sh_color_kernel<3>, grid, dim3(256), 0, s, a.means, a.colors, a.n_coeffs, a.campos, a.N, g2d);
}

size_t wm_raster::sh_campos_part_bytes(size_t N, size_t C) { return align256(C * 3 * ((N + 63) / 64) * sizeof(double)); }

void wm_raster::launch_sh_bwd(const WmRasterBwdArgs& b, const RasterWs& w, const float* pair_grad, int rec, double* campos_part, hipStream_t s) {
  if (b.fwd.sh_degree == 1) launch_sh_bwd_degree<1>(b, w, pair_grad, rec, campos_part, s);
  else if (b.fwd.sh_degree == 2) launch_sh_bwd_degree<2>(b, w, pair_grad, rec, campos_part, s);
  else launch_sh_bwd_degree<3>(b, w, pair_grad, rec, campos_part, s);
  if (b.v_campos)
    hipLaunchKernelGGL(raster_campos_reduce_kernel, dim3(3, (unsigned)b.fwd.C), dim3(256), 0, s, campos_part, ((size_t)b.fwd.N + 63) / 64, b.v_campos);
}
