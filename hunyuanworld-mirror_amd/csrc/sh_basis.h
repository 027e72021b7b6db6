// The real spherical-harmonics basis of degree 0-3 and its vector-Jacobian product, shared by the rasteriser's view-dependent colour
// (raster_sh.hip) and the appearance module (appearance.hip).  The polynomials in Cartesian form as published by Sloan, "Efficient
// Spherical Harmonic Evaluation", JCGT 2013 — the set gsplat evaluates in spherical_harmonics and in _eval_sh_bases_fast
// (gsplat/cuda/_torch_impl.py).
#pragma once

namespace wm_sh {

constexpr float SH_K0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.48860251190292f;
constexpr float SH_C2A = 0.5462742152960395f, SH_C2B = 1.092548430592079f, SH_C2D = 0.9461746957575601f, SH_C2E = 0.3153915652525201f;
constexpr float SH_C3A = 0.5900435899266435f, SH_C3B = 1.445305721320277f, SH_C3C = 2.285228997322329f, SH_C3D = 0.4570457994644658f;
constexpr float SH_C3E = 1.865881662950577f, SH_C3F = 1.119528997770346f;

// unit direction camera -> mean and the norm's denominator max(|d|, 1e-12)
__device__ __forceinline__ void sh_direction(const float* m, const float* __restrict__ cp, float& x, float& y, float& z, float& den) {
  const float dx = m[0] - cp[0], dy = m[1] - cp[1], dz = m[2] - cp[2];
  den = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
  x = dx / den; y = dy / den; z = dz / den;
}

// B[0 .. (L + 1)^2)
template <int L>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float* B) {
  B[0] = SH_K0;
  if constexpr (L >= 1) { B[1] = -SH_C1 * y; B[2] = SH_C1 * z; B[3] = -SH_C1 * x; }
  if constexpr (L >= 2) {
    const float z2 = z * z, c1 = x * x - y * y, s1 = 2.f * x * y;
    B[4] = SH_C2A * s1; B[5] = -SH_C2B * z * y; B[6] = SH_C2D * z2 - SH_C2E; B[7] = -SH_C2B * z * x; B[8] = SH_C2A * c1;
    if constexpr (L >= 3) {
      const float c2 = x * c1 - y * s1, s2 = x * s1 + y * c1, pz = SH_C3D - SH_C3C * z2;
      B[9] = -SH_C3A * s2; B[10] = SH_C3B * z * s1; B[11] = pz * y; B[12] = z * (SH_C3E * z2 - SH_C3F);
      B[13] = pz * x; B[14] = SH_C3B * z * c1; B[15] = -SH_C3A * c2;
    }
  }
}

// sum_k w[k] grad B_k(x, y, z), the polynomials differentiated with x, y, z independent (k = 0 is constant)
template <int L>
__device__ __forceinline__ void sh_basis_vjp(float x, float y, float z, const float* w, float* v) {
  if constexpr (L < 1) { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; return; }
  v[0] = -SH_C1 * w[3]; v[1] = -SH_C1 * w[1]; v[2] = SH_C1 * w[2];
  if constexpr (L >= 2) {
    v[0] += 2.f * SH_C2A * (y * w[4] + x * w[8]) - SH_C2B * z * w[7];
    v[1] += 2.f * SH_C2A * (x * w[4] - y * w[8]) - SH_C2B * z * w[5];
    v[2] += 2.f * SH_C2D * z * w[6] - SH_C2B * (y * w[5] + x * w[7]);
    if constexpr (L >= 3) {
      const float z2 = z * z, c1 = x * x - y * y, s1 = 2.f * x * y, pz = SH_C3D - SH_C3C * z2;
      v[0] += 2.f * SH_C3B * z * (y * w[10] + x * w[14]) - 3.f * SH_C3A * (s1 * w[9] + c1 * w[15]) + pz * w[13];
      v[1] += 2.f * SH_C3B * z * (x * w[10] - y * w[14]) - 3.f * SH_C3A * (c1 * w[9] - s1 * w[15]) + pz * w[11];
      v[2] += SH_C3B * (s1 * w[10] + c1 * w[14]) - 2.f * SH_C3C * z * (y * w[11] + x * w[13]) + (3.f * SH_C3E * z2 - SH_C3F) * w[12];
    }
  }
}

}  // namespace wm_sh
