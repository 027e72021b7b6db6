// 3D-Gaussian-splat rasteriser backward — the gradient gsplat.rasterization gives the reference's "Post 3DGS Optimization"
// through its CUDA extension (gsplat/cuda/csrc/RasterizeToPixels3DGSBwd.cu for the compositing, the torch restatement
// gsplat/cuda/_torch_impl.py:11-133,250-375 for the projection), for the configuration raster.hip renders: classic, pinhole,
// RGB + expected depth, degree-0 SH or given colours.  Gradients for means, quats, scales, opacities, colours and, on request, the
// world-to-camera matrices (gsplat: the viewmats gradient of _FullyFusedProjection.backward); none for the intrinsics.
//
// It reads what the forward left in the caller's workspace (records, sorted list, tile offsets, per-Gaussian pair offsets):
//   locate     which of the sort's two value buffers holds the sorted list (the one whose keys are in order)
//   composite  one wave per 16 x 16 tile, four pixels per lane.  The wave first walks the tile's list front to back exactly as the
//              forward does (transmittance only) to find each pixel's last blended entry and final transmittance, then walks it back
//              to front: per entry 10 per-pixel terms (2-D mean 2, conic 3, opacity 1, colour 3, depth 1) are summed over the lane's
//              pixels, then over the 64 lanes by DPP adds, and written by 10 lanes as ONE 40-byte record.  Every (Gaussian, tile)
//              pair has exactly one owner — this wave — and a slot of its own: the position the forward's emit pass gave it,
//              pair offset of its (camera, Gaussian) + index of the tile inside the Gaussian's tile rectangle.  No atomics.
//              With absgrad (gsplat's absgrad, RasterizeToPixels3DGSBwd.cu) the record is 12 floats: two more sums, of the absolute
//              value of each pixel's 2-D mean terms, taken per pixel before any sum.  The record width is a template parameter
//              (raster_bwd_composite.h); this file instantiates the 10-float kernel, raster_bwd_abs.hip the 12-float one.
//   project    one thread per Gaussian, cameras in order: sums the Gaussian's contiguous pair records, pulls the sum back through
//              conic -> 2-D covariance -> perspective projection -> camera -> world, then once through covariance -> quaternion, scale.
//              On request it also writes the summed 2-D mean terms per (camera, Gaussian) before it folds them in: the gradient of
//              the pixel-space means (and the absgrad sums) that a densification strategy reads.
//              With CAM it folds the same per-(camera, Gaussian) terms the other way as well: the 12 viewmats terms of a pair
//              (v_R 9, v_t 3) are summed over the wave's 64 lanes in fp64 and stored by one lane as the wave's partial.
//   camreduce  with CAM: per (camera, component) the waves' partials are added in a fixed order, in fp64 -> v_viewmats [C,4,4]
//   means2d    the pixel-space means the forward's projection left in its records, [C,N,2], zero where culled
//   SH 1-3     the kernels above run as for given colours (their [N,3] colour gradient goes to a scratch); raster_sh.hip then makes the
//              coefficient gradient [N,K,3], the direction's share of v_means and v_campos out of the same pair records
//   options    eps2d is the forward's.  Antialiased: the record's opacity is opacity * comp, comp = sqrt(max(det(M) / det(M + eps2d I), 0)),
//              M = the 2-D covariance before the blur, so v_opacities = sum over cameras of comp * v_opacity' and v_comp = opacity * v_opacity'
//              enters v_cov2d through d comp^2 / d M = ((1 - comp^2) adj(M + eps2d I)^T - eps2d I) / det(M + eps2d I) (gsplat's add_blur_vjp,
//              include/Utils.cuh) times 0.5 / comp.  CHOICE: the exact 0.5 / comp, which is what autograd gives the torch projection — gsplat's
//              CUDA divides by comp + 1e-6 — and exactly 0 where comp == 0 or where the determinant clamp (det < 1e-10) is active; torch's own
//              autograd gives NaN at det(M) <= 0, this kernel does not.  Backgrounds and the accumulated-depth mode change the compositing
//              backward's prologue only (raster_bwd_composite.h); v_backgrounds [C,3] is a reduction of its own over v_rgb and the forward's
//              out_alpha, which is READ here, not recomputed: fp32 terms, fp64 partials per 4096-pixel chunk, chunks added in a fixed order.
// Sums run in a fixed order everywhere, so gradients are bitwise reproducible run to run.
#include "wm_common.h"
#include "wm_kernels.h"
#include "raster_common.h"
#include "raster_bwd_composite.h"

using namespace wm_raster;

namespace {

// flag = 1 when keys0 is not in order (then the sorted list is in buffer 1).  Each radix pass is stable, so a buffer whose keys
// are in order holds the final list whatever pass wrote it.
__global__ __launch_bounds__(256) void raster_locate_sorted_kernel(const unsigned long long* __restrict__ keys0, unsigned int n,
                                                                  unsigned int* __restrict__ flag) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i + 1 < n && keys0[i] > keys0[i + 1]) *flag = 1u;
}

// _torch_impl.py:11-29,45-61 (quaternion, scale -> covariance), :250-283 (world -> camera), :78-133 (perspective), :329-355 (conic)
// is_sh = WM_COLORS_PER_CAMERA: colors_in is [C,N,3] (not read) and v_colors [C,N,3] gets every pair's summed colour terms, zeros where culled
// M2D: also write v_means2d [C,N,2] (and, with 12-float records, v_means2d_abs): the summed pair terms, zero where culled
// CAM: also write cam_part [C][12][waves] (fp64): per wave the sum over its Gaussians of the pair's viewmats terms, component 4 i + j =
//      v_R[i][j] (j < 3) or v_t[i] (j = 3).  v_t += (v_tx, v_ty, v_tz) (from mc = Rv m + t); v_R += outer(v_t, m) + (vS + vS^T) Rv cov
//      (from S = Rv cov Rv^T, cov symmetric).  Lanes past N and culled pairs take part in the wave's sum with zeros; a wave with no
//      Gaussian at all leaves, and the reducer does not read its slot.
template <int REC, bool M2D, bool CAM>
__global__ __launch_bounds__(256) void raster_project_bwd_kernel(const float* __restrict__ means, const float* __restrict__ quats,
                                                                 const float* __restrict__ scales, const float* __restrict__ colors_in, int is_sh,
                                                                 const float* __restrict__ viewmats, const float* __restrict__ Ks, int N, int C,
                                                                 int width, int height, const G2D* __restrict__ g2d,
                                                                 const unsigned long long* __restrict__ pair_offs, const float* __restrict__ pair_grad,
                                                                 float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
                                                                 float* __restrict__ v_opac, float* __restrict__ v_colors,
                                                                 float* __restrict__ v_means2d, float* __restrict__ v_means2d_abs,
                                                                 double* __restrict__ cam_part, const float* __restrict__ opac, float eps2d,
                                                                 int antialiased) {
  int g = blockIdx.x * 256 + threadIdx.x;
  bool live = true;
  if constexpr (CAM) {
    if ((g & ~63) >= N) return;   // the whole wave is past N
    live = g < N;
    g = live ? g : N - 1;         // a lane past N reads the last Gaussian, adds zeros to the wave's sums and stores nothing
  } else {
    if (g >= N) return;
  }
  const float q0 = quats[4 * g], q1 = quats[4 * g + 1], q2 = quats[4 * g + 2], q3 = quats[4 * g + 3];
  const float qn = fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12f);
  const float qw = q0 / qn, qx = q1 / qn, qy = q2 / qn, qz = q3 / qn;
  const float Rm[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                       2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                       2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)};
  const float s[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
  float M[9], cov[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = Rm[3 * i + j] * s[j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) cov[3 * i + k] = M[3 * i] * M[3 * k] + M[3 * i + 1] * M[3 * k + 1] + M[3 * i + 2] * M[3 * k + 2];
  const float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
  float a_m[3] = {0.f, 0.f, 0.f}, a_cov[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a_op = 0.f, a_col[3] = {0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const size_t idx = (size_t)c * N + g;
    const int rect = g2d[idx].rect;
    const int cnt = (((rect >> 16) & 255) - (rect & 255)) * (((rect >> 24) & 255) - ((rect >> 8) & 255));
    float cv[CAM ? 12 : 1];
    if constexpr (CAM) {
#pragma unroll
      for (int i = 0; i < 12; ++i) cv[i] = 0.f;
    }
    if (cnt <= 0) {           // culled for this camera
      if constexpr (M2D) {
        if (live) {
          v_means2d[2 * idx] = 0.f; v_means2d[2 * idx + 1] = 0.f;
          if constexpr (REC == PAIR_REC_ABS) { v_means2d_abs[2 * idx] = 0.f; v_means2d_abs[2 * idx + 1] = 0.f; }
        }
      }
      if (is_sh == WM_COLORS_PER_CAMERA && live) { v_colors[3 * idx] = 0.f; v_colors[3 * idx + 1] = 0.f; v_colors[3 * idx + 2] = 0.f; }
      if constexpr (!CAM) continue;
    }
    if (!CAM || (live && cnt > 0)) {
      float p[REC];
#pragma unroll
      for (int i = 0; i < REC; ++i) p[i] = 0.f;
      const float* rec = pair_grad + pair_offs[idx] * REC;
      for (int t = 0; t < cnt; ++t)
#pragma unroll
        for (int i = 0; i < REC; ++i) p[i] += rec[(size_t)t * REC + i];
      if constexpr (M2D) {
        v_means2d[2 * idx] = p[0]; v_means2d[2 * idx + 1] = p[1];
        if constexpr (REC == PAIR_REC_ABS) { v_means2d_abs[2 * idx] = p[10]; v_means2d_abs[2 * idx + 1] = p[11]; }
      }
      const float v_mx = p[0], v_my = p[1], v_ca = p[2], v_cb = p[3], v_cc = p[4];
      // antialiased: the pair's opacity was opac[g] * comp (comp read back from the record the forward's projection wrote):
      // v_opacities += comp * v_opacity', v_comp = opac[g] * v_opacity' goes on into the 2-D covariance below
      const float comp = antialiased ? __int_as_float(g2d[idx].pad) : 1.0f;
      a_op += antialiased ? comp * p[5] : p[5];
      a_col[0] += p[6]; a_col[1] += p[7]; a_col[2] += p[8];
      if (is_sh == WM_COLORS_PER_CAMERA) { v_colors[3 * idx] = p[6]; v_colors[3 * idx + 1] = p[7]; v_colors[3 * idx + 2] = p[8]; }   // [C,N,3]: the pair's own
      // forward, as raster_project_kernel
      const float* V = viewmats + 16 * c;
      const float Rv[9] = {V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
      const float tx = Rv[0] * m[0] + Rv[1] * m[1] + Rv[2] * m[2] + V[3];
      const float ty = Rv[3] * m[0] + Rv[4] * m[1] + Rv[5] * m[2] + V[7];
      const float tz = Rv[6] * m[0] + Rv[7] * m[1] + Rv[8] * m[2] + V[11];
      float RC[9], S[9];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) RC[3 * i + k] = Rv[3 * i] * cov[k] + Rv[3 * i + 1] * cov[3 + k] + Rv[3 * i + 2] * cov[6 + k];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int l = 0; l < 3; ++l) S[3 * i + l] = RC[3 * i] * Rv[3 * l] + RC[3 * i + 1] * Rv[3 * l + 1] + RC[3 * i + 2] * Rv[3 * l + 2];
      const float* K = Ks + 9 * c;
      const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
      const float tfx = 0.5f * width / fx, tfy = 0.5f * height / fy;
      const float lxp = (width - cx) / fx + 0.3f * tfx, lxn = cx / fx + 0.3f * tfx;
      const float lyp = (height - cy) / fy + 0.3f * tfy, lyn = cy / fy + 0.3f * tfy;
      const float rz = 1.0f / tz, rz2 = rz * rz;
      const float ux = tx * rz, uy = ty * rz;
      const bool free_x = ux >= -lxn && ux <= lxp, free_y = uy >= -lyn && uy <= lyp;   // torch.clamp: no gradient outside the limits
      const float u = fminf(fmaxf(ux, -lxn), lxp), w = fminf(fmaxf(uy, -lyn), lyp);
      const float J0 = fx * rz, J2 = -fx * u * rz, J4 = fy * rz, J5 = -fy * w * rz;   // J = [[J0 0 J2] [0 J4 J5]]
      const float a0 = J0 * S[0] + J2 * S[6], a1 = J0 * S[1] + J2 * S[7], a2 = J0 * S[2] + J2 * S[8];   // A = J S (2 x 3)
      const float b0 = J4 * S[3] + J5 * S[6], b1 = J4 * S[4] + J5 * S[7], b2 = J4 * S[5] + J5 * S[8];
      const float c00 = a0 * J0 + a2 * J2 + eps2d, c01 = a1 * J4 + a2 * J5, c10 = b0 * J0 + b2 * J2, c11 = b1 * J4 + b2 * J5 + eps2d;
      const float det_raw = c00 * c11 - c01 * c10;
      const float det = fmaxf(det_raw, 1e-10f), rdet = 1.0f / det;
      const float ka = c11 * rdet, kb = -(c01 + c10) * 0.5f * rdet, kc = c00 * rdet;
      // conic -> 2-D covariance G = d loss / d cov2d
      float g00 = v_cc * rdet, g11 = v_ca * rdet, g01 = -0.5f * v_cb * rdet, g10 = g01;
      if (det_raw >= 1e-10f) {
        const float v_det = -(v_ca * ka + v_cb * kb + v_cc * kc) * rdet;
        g00 += v_det * c11; g11 += v_det * c00; g01 -= v_det * c10; g10 -= v_det * c01;
        if (antialiased && comp > 0.f) {   // comp^2 = det(M) / det(M + eps2d I), M = cov2d before the blur (derivation: header)
          const float vsc = opac[g] * p[5] * 0.5f / comp, rest = 1.0f - comp * comp;
          g00 += vsc * (rest * c11 - eps2d) * rdet; g11 += vsc * (rest * c00 - eps2d) * rdet;
          g01 -= vsc * rest * c10 * rdet; g10 -= vsc * rest * c01 * rdet;
        }
      }
      // cov2d = J S J^T:  v_S = J^T G J,  v_J = G J S^T + G^T J S
      const float Jm[6] = {J0, 0.f, J2, 0.f, J4, J5};
      float GJ[6], vS[9];
#pragma unroll
      for (int j = 0; j < 3; ++j) { GJ[j] = g00 * Jm[j] + g01 * Jm[3 + j]; GJ[3 + j] = g10 * Jm[j] + g11 * Jm[3 + j]; }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) vS[3 * i + j] = Jm[i] * GJ[j] + Jm[3 + i] * GJ[3 + j];
      float GtJ[6];
#pragma unroll
      for (int j = 0; j < 3; ++j) { GtJ[j] = g00 * Jm[j] + g10 * Jm[3 + j]; GtJ[3 + j] = g01 * Jm[j] + g11 * Jm[3 + j]; }
      float vJ[6];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          vJ[3 * i + j] = GJ[3 * i] * S[3 * j] + GJ[3 * i + 1] * S[3 * j + 1] + GJ[3 * i + 2] * S[3 * j + 2] +
                          GtJ[3 * i] * S[j] + GtJ[3 * i + 1] * S[3 + j] + GtJ[3 * i + 2] * S[6 + j];
      // J, 2-D mean, depth -> camera-space mean
      float v_tx = 0.f, v_ty = 0.f;
      float v_tz = p[9] - (vJ[0] * fx + vJ[4] * fy) * rz2 + (vJ[2] * fx * u + vJ[5] * fy * w) * rz2;
      const float v_u = -vJ[2] * fx * rz, v_w = -vJ[5] * fy * rz;
      if (free_x) { v_tx += v_u * rz; v_tz -= v_u * tx * rz2; }
      if (free_y) { v_ty += v_w * rz; v_tz -= v_w * ty * rz2; }
      v_tx += (K[0] * v_mx + K[3] * v_my) * rz;
      v_ty += (K[1] * v_mx + K[4] * v_my) * rz;
      v_tz -= ((K[0] * tx + K[1] * ty) * v_mx + (K[3] * tx + K[4] * ty) * v_my) * rz2;
      // camera -> world
#pragma unroll
      for (int j = 0; j < 3; ++j) a_m[j] += Rv[j] * v_tx + Rv[3 + j] * v_ty + Rv[6 + j] * v_tz;
      float RtS[9];   // Rv^T vS
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) RtS[3 * i + j] = Rv[i] * vS[j] + Rv[3 + i] * vS[3 + j] + Rv[6 + i] * vS[6 + j];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a_cov[3 * i + j] += RtS[3 * i] * Rv[j] + RtS[3 * i + 1] * Rv[3 + j] + RtS[3 * i + 2] * Rv[6 + j];
      if constexpr (CAM) {      // camera -> viewmat: RC = Rv cov is still there
        const float vt[3] = {v_tx, v_ty, v_tz};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
            cv[4 * i + j] = vt[i] * m[j] + (vS[3 * i] + vS[i]) * RC[j] + (vS[3 * i + 1] + vS[3 + i]) * RC[3 + j] + (vS[3 * i + 2] + vS[6 + i]) * RC[6 + j];
          cv[4 * i + 3] = vt[i];
        }
      }
    }
    if constexpr (CAM) {
      const size_t waves = ((size_t)N + 63) / 64, wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const double sum = wave_sum_hi_f64((double)cv[i]);
        if ((threadIdx.x & 63) == 63) cam_part[((size_t)c * 12 + i) * waves + wave] = sum;
      }
    }
  }
  if (!live) return;
  // covariance = M M^T, M = R diag(s):  v_M = (v_cov + v_cov^T) M
  float vM[9], vR[9], vs[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      vM[3 * i + j] = (a_cov[3 * i] + a_cov[i]) * M[j] + (a_cov[3 * i + 1] + a_cov[3 + i]) * M[3 + j] + (a_cov[3 * i + 2] + a_cov[6 + i]) * M[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { vR[3 * i + j] = vM[3 * i + j] * s[j]; vs[j] += vM[3 * i + j] * Rm[3 * i + j]; }
  const float vw = 2.f * (-qz * vR[1] + qy * vR[2] + qz * vR[3] - qx * vR[5] - qy * vR[6] + qx * vR[7]);
  const float vx = 2.f * (qy * vR[1] + qz * vR[2] + qy * vR[3] - 2.f * qx * vR[4] - qw * vR[5] + qz * vR[6] + qw * vR[7] - 2.f * qx * vR[8]);
  const float vy = 2.f * (-2.f * qy * vR[0] + qx * vR[1] + qw * vR[2] + qx * vR[3] + qz * vR[5] - qw * vR[6] + qz * vR[7] - 2.f * qy * vR[8]);
  const float vz = 2.f * (-2.f * qz * vR[0] - qw * vR[1] + qx * vR[2] + qw * vR[3] - 2.f * qz * vR[4] + qy * vR[5] + qx * vR[6] + qy * vR[7]);
  // through q / max(|q|, 1e-12)
  const float dotq = qw * vw + qx * vx + qy * vy + qz * vz;
  v_quats[4 * g] = (vw - qw * dotq) / qn; v_quats[4 * g + 1] = (vx - qx * dotq) / qn;
  v_quats[4 * g + 2] = (vy - qy * dotq) / qn; v_quats[4 * g + 3] = (vz - qz * dotq) / qn;
  v_means[3 * g] = a_m[0]; v_means[3 * g + 1] = a_m[1]; v_means[3 * g + 2] = a_m[2];
  v_scales[3 * g] = vs[0]; v_scales[3 * g + 1] = vs[1]; v_scales[3 * g + 2] = vs[2];
  v_opac[g] = a_op;
  if (is_sh == WM_COLORS_PER_CAMERA) return;   // v_colors [C,N,3] is written per pair above
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float vc = a_col[i];
    if (is_sh) vc = SH_C0 * colors_in[3 * g + i] + 0.5f > 0.f ? SH_C0 * vc : 0.f;   // clamp_min(C0 sh + 0.5, 0) (rendering.py:919-923)
    v_colors[3 * g + i] = vc;
  }
}

// v_viewmats [C,4,4]: one block per (component, camera) adds the waves' partials, thread t those of waves t, t + 256, ... in order, then
// the 256 thread sums pairwise in a fixed tree.  The bottom row is written as zeros.
__global__ __launch_bounds__(256) void raster_cam_reduce_kernel(const double* __restrict__ cam_part, size_t waves, float* __restrict__ v_viewmats) {
  __shared__ double sh[256];
  const int comp = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const double* part = cam_part + ((size_t)c * 12 + comp) * waves;
  double acc = 0.0;
  for (size_t w = t; w < waves; w += 256) acc += part[w];
  sh[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) v_viewmats[16 * c + comp] = (float)sh[0];
  if (comp == 0 && t < 4) v_viewmats[16 * c + 12 + t] = 0.f;
}

// v_backgrounds [C,3] = sum over the camera's pixels of v_rgb (1 - alpha), alpha READ from the forward's out_alpha (not recomputed).
// Stage 1: a block takes BG_CHUNK consecutive pixels of one camera, thread t those at t, t + 256, ... in order; every term is formed in
// fp32, added in fp64, the 256 thread sums go pairwise through a fixed tree -> bg_part [C][3][chunks].  Stage 2 (raster_bg_reduce_kernel)
// adds the chunks' partials in the order of raster_cam_reduce_kernel and rounds to fp32 once.
constexpr int BG_CHUNK = 4096;
__global__ __launch_bounds__(256) void raster_bg_partial_kernel(const float* __restrict__ v_rgb, const float* __restrict__ out_alpha, size_t pixels,
                                                                size_t chunks, double* __restrict__ bg_part) {
  __shared__ double sh[3][256];
  const size_t chunk = blockIdx.x, c = blockIdx.y;
  const int t = threadIdx.x;
  const size_t lo = chunk * BG_CHUNK, hi = lo + BG_CHUNK < pixels ? lo + BG_CHUNK : pixels;
  double acc[3] = {0.0, 0.0, 0.0};
  for (size_t i = lo + t; i < hi; i += 256) {
    const size_t pix = c * pixels + i;
    const float rest = 1.0f - out_alpha[pix];
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] += (double)(v_rgb[3 * pix + j] * rest);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) sh[j][t] = acc[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int j = 0; j < 3; ++j) sh[j][t] += sh[j][t + o];
    }
    __syncthreads();
  }
  if (t < 3) bg_part[(c * 3 + t) * chunks + chunk] = sh[t][0];
}
__global__ __launch_bounds__(256) void raster_bg_reduce_kernel(const double* __restrict__ bg_part, size_t chunks, float* __restrict__ v_backgrounds) {
  __shared__ double sh[256];
  const int comp = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const double* part = bg_part + ((size_t)c * 3 + comp) * chunks;
  double acc = 0.0;
  for (size_t w = t; w < chunks; w += 256) acc += part[w];
  sh[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) v_backgrounds[3 * c + comp] = (float)sh[0];
}

// the forward's pixel-space means out of its projection records; zero where the camera culled the Gaussian (a radius of 0)
__global__ __launch_bounds__(256) void raster_means2d_kernel(const G2D* __restrict__ g2d, const int* __restrict__ radii, size_t CN,
                                                             float* __restrict__ means2d) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= CN) return;
  const bool seen = radii[2 * i] > 0 && radii[2 * i + 1] > 0;
  means2d[2 * i] = seen ? g2d[i].mx : 0.f;
  means2d[2 * i + 1] = seen ? g2d[i].my : 0.f;
}

template <int REC, bool M2D, bool CAM>
void launch_bwd_kernels(const WmRasterBwdArgs& b, const RasterWs& w, unsigned int* flag, float* pair_grad, double* cam_part, int tw, int th,
                        hipStream_t s) {
  const WmRasterArgs& a = b.fwd;
  const size_t N = a.N, C = a.C;
  if (b.n_isects > 0) {
    hipLaunchKernelGGL(raster_locate_sorted_kernel, dim3((unsigned)((b.n_isects + 255) / 256)), dim3(256), 0, s, w.keys[0], (unsigned int)b.n_isects, flag);
    const dim3 grid((unsigned)(tw * th), (unsigned)C);
    if constexpr (REC == PAIR_REC_ABS)
      wm_launch_composite_bwd_abs(grid, s, w.g2d, w.vals[0], w.vals[1], flag, w.tile_offs, w.offsets, tw, th, a.width, a.height, b.out_depth, b.v_rgb,
                                  b.v_depth, b.v_alpha, pair_grad, a.backgrounds, a.depth_mode);
    else
      hipLaunchKernelGGL(raster_composite_bwd_kernel<PAIR_REC>, grid, dim3(64), 0, s, w.g2d, w.vals[0], w.vals[1], flag, w.tile_offs, w.offsets, tw,
                         th, a.width, a.height, b.out_depth, b.v_rgb, b.v_depth, b.v_alpha, pair_grad, a.backgrounds, a.depth_mode);
  }
  hipLaunchKernelGGL((raster_project_bwd_kernel<REC, M2D, CAM>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a.means, a.quats, a.scales, a.colors,
                     a.is_sh, a.viewmats, a.Ks, a.N, a.C, a.width, a.height, w.g2d, w.offsets, pair_grad, b.v_means, b.v_quats, b.v_scales,
                     b.v_opacities, b.v_colors, b.v_means2d, b.v_means2d_abs, cam_part, a.opacities, a.eps2d, a.antialiased);
  if constexpr (CAM)
    hipLaunchKernelGGL(raster_cam_reduce_kernel, dim3(12, (unsigned)C), dim3(256), 0, s, cam_part, (N + 63) / 64, b.v_viewmats);
}

}  // namespace

size_t wm_raster_bwd_workspace_bytes(int N, int C, int width, int height, size_t n_isects, int absgrad, int cam, int sh, int campos, int bg) {
  const size_t base = align256(256) + align256(n_isects * (absgrad ? PAIR_REC_ABS : PAIR_REC) * sizeof(float));   // buffer flag | pair records
  size_t total = base;
  if (N <= 0 || C <= 0) return total;
  if (cam) total += align256((size_t)C * 12 * (((size_t)N + 63) / 64) * sizeof(double));   // | per-wave viewmats partials [C][12][waves]
  if (sh) total += align256((size_t)N * 3 * sizeof(float));                                 // | SH: the geometric pass's colour gradient (unused)
  if (sh && campos) total += sh_campos_part_bytes(N, C);                                    // | SH: per-wave campos partials [C][3][waves]
  if (bg && width > 0 && height > 0)                                                        // | backgrounds: per-chunk partials [C][3][chunks]
    total += align256((size_t)C * 3 * (((size_t)width * height + BG_CHUNK - 1) / BG_CHUNK) * sizeof(double));
  return total;
}

hipError_t wm_launch_rasterize_means2d(const void* workspace, size_t workspace_bytes, int N, int C, int width, int height, size_t max_isects,
                                       const int* radii, float* means2d, hipStream_t s) {
  const int tw = (width + TILE - 1) / TILE, th = (height + TILE - 1) / TILE;
  if (N <= 0 || C <= 0 || tw > 255 || th > 255 || (size_t)N * C >= (1ull << 31)) return hipErrorInvalidValue;
  RasterWs w = carve((char*)const_cast<void*>(workspace), N, C, tw * th, max_isects);
  if (w.total > workspace_bytes) return hipErrorInvalidValue;
  const size_t CN = (size_t)N * C;
  hipLaunchKernelGGL(raster_means2d_kernel, dim3((unsigned)((CN + 255) / 256)), dim3(256), 0, s, w.g2d, radii, CN, means2d);
  return hipGetLastError();
}

hipError_t wm_launch_rasterize_bwd(const WmRasterBwdArgs& b, hipStream_t s) {
  const WmRasterArgs& a = b.fwd;
  const int tw = (a.width + TILE - 1) / TILE, th = (a.height + TILE - 1) / TILE, tiles = tw * th;
  if (a.N <= 0 || a.C <= 0 || tw > 255 || th > 255) return hipErrorInvalidValue;
  const size_t N = a.N, C = a.C, CN = N * C;
  if (CN >= (1ull << 31) || b.n_isects > a.max_isects || b.n_isects >= (1ull << 31)) return hipErrorInvalidValue;
  if (b.absgrad && (!b.v_means2d || !b.v_means2d_abs)) return hipErrorInvalidValue;
  RasterWs w = carve((char*)a.workspace, N, C, tiles, a.max_isects);
  if (w.total > a.workspace_bytes) return hipErrorInvalidValue;
  const int cam = b.v_viewmats ? 1 : 0, sh = a.sh_degree > 0 ? 1 : 0;
  if (sh ? !sh_args_valid(a) : b.v_campos != nullptr) return hipErrorInvalidValue;
  if (!wm_raster_options_valid(a) || (b.v_backgrounds && (!a.backgrounds || !b.out_alpha))) return hipErrorInvalidValue;
  if (wm_raster_bwd_workspace_bytes(a.N, a.C, a.width, a.height, b.n_isects, b.absgrad, cam, sh, b.v_campos ? 1 : 0, b.v_backgrounds ? 1 : 0) >
      b.grad_workspace_bytes)
    return hipErrorInvalidValue;
  if (b.v_backgrounds) {   // independent of the splat gradients: its partials lie behind everything else in the workspace
    double* bg_part = (double*)((char*)b.grad_workspace + wm_raster_bwd_workspace_bytes(a.N, a.C, a.width, a.height, b.n_isects, b.absgrad, cam, sh,
                                                                                      b.v_campos ? 1 : 0));
    const size_t pixels = (size_t)a.width * a.height, chunks = (pixels + BG_CHUNK - 1) / BG_CHUNK;
    hipLaunchKernelGGL(raster_bg_partial_kernel, dim3((unsigned)chunks, (unsigned)C), dim3(256), 0, s, b.v_rgb, b.out_alpha, pixels, chunks, bg_part);
    hipLaunchKernelGGL(raster_bg_reduce_kernel, dim3(3, (unsigned)C), dim3(256), 0, s, bg_part, chunks, b.v_backgrounds);
  }
  const int rec = b.absgrad ? PAIR_REC_ABS : PAIR_REC;
  unsigned int* flag = (unsigned int*)b.grad_workspace;
  float* pair_grad = (float*)((char*)b.grad_workspace + align256(256));
  double* cam_part = (double*)((char*)pair_grad + align256(b.n_isects * rec * sizeof(float)));   // every slot the reducer reads is written
  if (sh) {
    // SH degree 1-3: the geometric part through the kernels below as for given colours, their [N,3] colour gradient into a scratch of the
    // workspace; then raster_sh.hip turns the pairs' colour terms into v_colors [N,K,3], its share of v_means and v_campos
    char* sh_ws = (char*)b.grad_workspace + wm_raster_bwd_workspace_bytes(a.N, a.C, a.width, a.height, b.n_isects, b.absgrad, cam);
    WmRasterBwdArgs geo = b;
    geo.fwd.sh_degree = 0; geo.fwd.is_sh = 0; geo.v_campos = nullptr; geo.v_backgrounds = nullptr;
    geo.v_colors = (float*)sh_ws;
    geo.grad_workspace_bytes = (size_t)(sh_ws - (char*)b.grad_workspace);
    const hipError_t e = wm_launch_rasterize_bwd(geo, s);
    if (e != hipSuccess) return e;
    launch_sh_bwd(b, w, pair_grad, rec, (double*)(sh_ws + align256(N * 3 * sizeof(float))), s);
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(b.grad_workspace, 0, align256(256) + b.n_isects * rec * sizeof(float), s);
  if (e != hipSuccess) return e;
  if (cam) {
    if (b.absgrad) launch_bwd_kernels<PAIR_REC_ABS, true, true>(b, w, flag, pair_grad, cam_part, tw, th, s);
    else if (b.v_means2d) launch_bwd_kernels<PAIR_REC, true, true>(b, w, flag, pair_grad, cam_part, tw, th, s);
    else launch_bwd_kernels<PAIR_REC, false, true>(b, w, flag, pair_grad, cam_part, tw, th, s);
  } else if (b.absgrad) launch_bwd_kernels<PAIR_REC_ABS, true, false>(b, w, flag, pair_grad, nullptr, tw, th, s);
  else if (b.v_means2d) launch_bwd_kernels<PAIR_REC, true, false>(b, w, flag, pair_grad, nullptr, tw, th, s);
  else launch_bwd_kernels<PAIR_REC, false, false>(b, w, flag, pair_grad, nullptr, tw, th, s);
  return hipGetLastError();
}
