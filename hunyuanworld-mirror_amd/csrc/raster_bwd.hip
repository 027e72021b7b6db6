// 3D-Gaussian-splat rasteriser backward — the gradient gsplat.rasterization gives the reference's "Post 3DGS Optimization"
// through its CUDA extension (gsplat/cuda/csrc/RasterizeToPixels3DGSBwd.cu for the compositing, the torch restatement
// gsplat/cuda/_torch_impl.py:11-133,250-375 for the projection), for the configuration raster.hip renders: classic, pinhole,
// RGB + expected depth, degree-0 SH or given colours.  Gradients for means, quats, scales, opacities, colours; none for cameras.
//
// It reads what the forward left in the caller's workspace (records, sorted list, tile offsets, per-Gaussian pair offsets):
//   locate     which of the sort's two value buffers holds the sorted list (the one whose keys are in order)
//   composite  one wave per 16 x 16 tile, four pixels per lane.  The wave first walks the tile's list front to back exactly as the
//              forward does (transmittance only) to find each pixel's last blended entry and final transmittance, then walks it back
//              to front: per entry 10 per-pixel terms (2-D mean 2, conic 3, opacity 1, colour 3, depth 1) are summed over the lane's
//              pixels, then over the 64 lanes by DPP adds, and written by 10 lanes as ONE 40-byte record.  Every (Gaussian, tile)
//              pair has exactly one owner — this wave — and a slot of its own: the position the forward's emit pass gave it,
//              pair offset of its (camera, Gaussian) + index of the tile inside the Gaussian's tile rectangle.  No atomics.
//   project    one thread per Gaussian, cameras in order: sums the Gaussian's contiguous pair records, pulls the sum back through
//              conic -> 2-D covariance -> perspective projection -> camera -> world, then once through covariance -> quaternion, scale.
// Sums run in a fixed order everywhere, so gradients are bitwise reproducible run to run.
#include "wm_common.h"
#include "wm_kernels.h"
#include "raster_common.h"

using namespace wm_raster;

namespace {

constexpr int PAIR_REC = 10;   // floats per (Gaussian, tile) pair: v_mx v_my | v_ca v_cb v_cc | v_opacity | v_r v_g v_b | v_depth

// flag = 1 when keys0 is not in order (then the sorted list is in buffer 1).  Each radix pass is stable, so a buffer whose keys
// are in order holds the final list whatever pass wrote it.
__global__ __launch_bounds__(256) void raster_locate_sorted_kernel(const unsigned long long* __restrict__ keys0, unsigned int n,
                                                                  unsigned int* __restrict__ flag) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i + 1 < n && keys0[i] > keys0[i + 1]) *flag = 1u;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_of(float x) {   // lanes the row mask leaves out read 0
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}
// sum over the 64 lanes; the total is valid in lanes 48-63
__device__ __forceinline__ float wave_sum_hi(float v) {
  v += dpp_of<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
  v += dpp_of<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
  v += dpp_of<0x141, 0xf>(v);   // row_half_mirror
  v += dpp_of<0x140, 0xf>(v);   // row_mirror: every lane holds its row's sum
  v += dpp_of<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += dpp_of<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}

// Blending rules: raster.hip raster_composite_kernel (RasterizeToPixels3DGSFwd.cu:118-184); backward terms:
// RasterizeToPixels3DGSBwd.cu (per pixel, last blended Gaussian to first).
__global__ __launch_bounds__(64) void raster_composite_bwd_kernel(const G2D* __restrict__ g2d, const unsigned int* __restrict__ vals0,
                                                                  const unsigned int* __restrict__ vals1, const unsigned int* __restrict__ which,
                                                                  const unsigned int* __restrict__ offs, const unsigned long long* __restrict__ pair_offs,
                                                                  int tw, int th, int width, int height, const float* __restrict__ out_depth,
                                                                  const float* __restrict__ v_rgb, const float* __restrict__ v_depth,
                                                                  const float* __restrict__ v_alpha, float* __restrict__ pair_grad) {
  constexpr int PX = 2, PY = 2, NP = 4;
  const int tile = blockIdx.x, cam = blockIdx.y;
  const int ty = tile / tw, tx = tile - ty * tw;
  const int lane = threadIdx.x;
  const int i0 = ty * TILE + (lane >> 3) * PY, j0 = tx * TILE + (lane & 7) * PX;
  const unsigned int begin = offs[cam * tw * th + tile], end = offs[cam * tw * th + tile + 1];
  if (begin >= end) return;
  const unsigned int* __restrict__ vals = __builtin_amdgcn_readfirstlane((int)*which) ? vals1 : vals0;
  float px[NP], py[NP], T[NP];
  int last[NP];
  bool inimg[NP], open[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int i = i0 + q / PX, j = j0 + q % PX;
    px[q] = (float)j + 0.5f; py[q] = (float)i + 0.5f;
    inimg[q] = i < height && j < width;
    open[q] = inimg[q];
    T[q] = 1.0f; last[q] = -1;
  }
  // ---- front to back: the forward's decisions, transmittance only
  unsigned int k = begin;
  for (; k < end; ++k) {
    const unsigned int v = __builtin_amdgcn_readfirstlane(vals[k]);
    const G2D* __restrict__ rp = g2d + v;
    const float mx = rp->mx, my = rp->my, ca = rp->ca, cb = rp->cb, cc = rp->cc, op = rp->opacity;
    bool still = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const float dx = mx - px[q], dy = my - py[q];
      const float sigma = 0.5f * (ca * dx * dx + cc * dy * dy) + cb * dx * dy;
      const float alpha = fminf(0.999f, op * __expf(-sigma));
      const bool hit = open[q] && !(sigma < 0.f) && !(alpha < ALPHA_THRESHOLD);
      const float nT = T[q] * (1.0f - alpha);
      const bool stop = hit && nT <= 1e-4f;
      const bool blend = hit && !stop;
      T[q] = blend ? nT : T[q];
      last[q] = blend ? (int)k : last[q];
      open[q] = open[q] && !stop;
      still |= open[q];
    }
    if (__builtin_amdgcn_ballot_w64(still) == 0ull) { ++k; break; }
  }
  const unsigned int walked = k;   // entries [begin, walked) were looked at by the forward
  // ---- cotangents of the four composited channels and of alpha; the expected-depth division D / max(alpha, 1e-10) is undone here
  float vr[NP], vg[NP], vb[NP], vd[NP], tfv[NP], br[NP], bg[NP], bb[NP], bd[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int i = i0 + q / PX, j = j0 + q % PX;
    vr[q] = vg[q] = vb[q] = vd[q] = tfv[q] = 0.f;
    br[q] = bg[q] = bb[q] = bd[q] = 0.f;
    if (inimg[q]) {
      const size_t pix = ((size_t)cam * height + i) * width + j;
      const float al = 1.0f - T[q];
      const float inv = 1.0f / fmaxf(al, 1e-10f);
      const float ved = v_depth[pix];
      vr[q] = v_rgb[3 * pix]; vg[q] = v_rgb[3 * pix + 1]; vb[q] = v_rgb[3 * pix + 2];
      vd[q] = ved * inv;
      const float val = v_alpha[pix] - (al > 1e-10f ? ved * out_depth[pix] * inv : 0.f);
      tfv[q] = T[q] * val;
    }
  }
  // ---- back to front
  for (k = walked; k-- > begin;) {
    const unsigned int v = __builtin_amdgcn_readfirstlane(vals[k]);
    const G2D* __restrict__ rp = g2d + v;
    const float mx = rp->mx, my = rp->my, ca = rp->ca, cb = rp->cb, cc = rp->cc, op = rp->opacity, depth = rp->depth;
    const float cr = rp->r, cg = rp->g, cbl = rp->b;
    float alpha[NP], vis[NP], dx[NP], dy[NP];
    bool blend[NP], any = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      dx[q] = mx - px[q]; dy[q] = my - py[q];
      const float sigma = 0.5f * (ca * dx[q] * dx[q] + cc * dy[q] * dy[q]) + cb * dx[q] * dy[q];
      vis[q] = __expf(-sigma);
      alpha[q] = fminf(0.999f, op * vis[q]);
      blend[q] = inimg[q] && !(sigma < 0.f) && !(alpha[q] < ALPHA_THRESHOLD) && (int)k <= last[q];
      any |= blend[q];
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;   // nobody in the tile blended this Gaussian: its record stays zero
    float s_mx = 0.f, s_my = 0.f, s_ca = 0.f, s_cb = 0.f, s_cc = 0.f, s_op = 0.f, s_r = 0.f, s_g = 0.f, s_b = 0.f, s_d = 0.f;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const float ra = __builtin_amdgcn_rcpf(1.0f - alpha[q]);
      const float Tb = T[q] * ra;                       // transmittance in front of this Gaussian
      const float fac = blend[q] ? alpha[q] * Tb : 0.f;
      s_r += fac * vr[q]; s_g += fac * vg[q]; s_b += fac * vb[q]; s_d += fac * vd[q];
      float va = (cr * Tb - br[q] * ra) * vr[q] + (cg * Tb - bg[q] * ra) * vg[q] + (cbl * Tb - bb[q] * ra) * vb[q] +
                 (depth * Tb - bd[q] * ra) * vd[q] + tfv[q] * ra;
      va = blend[q] ? va : 0.f;
      br[q] += cr * fac; bg[q] += cg * fac; bb[q] += cbl * fac; bd[q] += depth * fac;
      T[q] = blend[q] ? Tb : T[q];
      const float ov = op * vis[q];
      const float vs = ov <= 0.999f ? -ov * va : 0.f;   // the 0.999 cap passes no gradient
      s_op += ov <= 0.999f ? vis[q] * va : 0.f;
      s_ca += 0.5f * vs * dx[q] * dx[q]; s_cb += vs * dx[q] * dy[q]; s_cc += 0.5f * vs * dy[q] * dy[q];
      s_mx += vs * (ca * dx[q] + cb * dy[q]); s_my += vs * (cb * dx[q] + cc * dy[q]);
    }
    s_mx = wave_sum_hi(s_mx); s_my = wave_sum_hi(s_my); s_ca = wave_sum_hi(s_ca); s_cb = wave_sum_hi(s_cb); s_cc = wave_sum_hi(s_cc);
    s_op = wave_sum_hi(s_op); s_r = wave_sum_hi(s_r); s_g = wave_sum_hi(s_g); s_b = wave_sum_hi(s_b); s_d = wave_sum_hi(s_d);
    // slot of this pair: where the forward's emit pass wrote it
    const int rect = rp->rect;
    const int x0 = rect & 255, y0 = (rect >> 8) & 255, x1 = (rect >> 16) & 255;
    const unsigned long long slot = pair_offs[v] + (unsigned long long)((ty - y0) * (x1 - x0) + (tx - x0));
    float o = s_mx;
    o = lane == 49 ? s_my : o; o = lane == 50 ? s_ca : o; o = lane == 51 ? s_cb : o; o = lane == 52 ? s_cc : o; o = lane == 53 ? s_op : o;
    o = lane == 54 ? s_r : o; o = lane == 55 ? s_g : o; o = lane == 56 ? s_b : o; o = lane == 57 ? s_d : o;
    if (lane >= 48 && lane < 48 + PAIR_REC) pair_grad[slot * PAIR_REC + (lane - 48)] = o;
  }
}

// _torch_impl.py:11-29,45-61 (quaternion, scale -> covariance), :250-283 (world -> camera), :78-133 (perspective), :329-355 (conic)
__global__ __launch_bounds__(256) void raster_project_bwd_kernel(const float* __restrict__ means, const float* __restrict__ quats,
                                                                 const float* __restrict__ scales, const float* __restrict__ colors_in, int is_sh,
                                                                 const float* __restrict__ viewmats, const float* __restrict__ Ks, int N, int C,
                                                                 int width, int height, const G2D* __restrict__ g2d,
                                                                 const unsigned long long* __restrict__ pair_offs, const float* __restrict__ pair_grad,
                                                                 float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
                                                                 float* __restrict__ v_opac, float* __restrict__ v_colors) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
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
    if (cnt <= 0) continue;   // culled for this camera
    float p[PAIR_REC];
#pragma unroll
    for (int i = 0; i < PAIR_REC; ++i) p[i] = 0.f;
    const float* rec = pair_grad + pair_offs[idx] * PAIR_REC;
    for (int t = 0; t < cnt; ++t)
#pragma unroll
      for (int i = 0; i < PAIR_REC; ++i) p[i] += rec[(size_t)t * PAIR_REC + i];
    const float v_mx = p[0], v_my = p[1], v_ca = p[2], v_cb = p[3], v_cc = p[4];
    a_op += p[5]; a_col[0] += p[6]; a_col[1] += p[7]; a_col[2] += p[8];
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
    const float c00 = a0 * J0 + a2 * J2 + 0.3f, c01 = a1 * J4 + a2 * J5, c10 = b0 * J0 + b2 * J2, c11 = b1 * J4 + b2 * J5 + 0.3f;
    const float det_raw = c00 * c11 - c01 * c10;
    const float det = fmaxf(det_raw, 1e-10f), rdet = 1.0f / det;
    const float ka = c11 * rdet, kb = -(c01 + c10) * 0.5f * rdet, kc = c00 * rdet;
    // conic -> 2-D covariance G = d loss / d cov2d
    float g00 = v_cc * rdet, g11 = v_ca * rdet, g01 = -0.5f * v_cb * rdet, g10 = g01;
    if (det_raw >= 1e-10f) {
      const float v_det = -(v_ca * ka + v_cb * kb + v_cc * kc) * rdet;
      g00 += v_det * c11; g11 += v_det * c00; g01 -= v_det * c10; g10 -= v_det * c01;
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
  }
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
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float vc = a_col[i];
    if (is_sh) vc = SH_C0 * colors_in[3 * g + i] + 0.5f > 0.f ? SH_C0 * vc : 0.f;   // clamp_min(C0 sh + 0.5, 0) (rendering.py:919-923)
    v_colors[3 * g + i] = vc;
  }
}

}  // namespace

size_t wm_raster_bwd_workspace_bytes(int N, int C, int width, int height, size_t n_isects) {
  (void)N; (void)C; (void)width; (void)height;
  return align256(256) + align256(n_isects * PAIR_REC * sizeof(float));   // buffer flag | pair records
}

hipError_t wm_launch_rasterize_bwd(const WmRasterBwdArgs& b, hipStream_t s) {
  const WmRasterArgs& a = b.fwd;
  const int tw = (a.width + TILE - 1) / TILE, th = (a.height + TILE - 1) / TILE, tiles = tw * th;
  if (a.N <= 0 || a.C <= 0 || tw > 255 || th > 255) return hipErrorInvalidValue;
  const size_t N = a.N, C = a.C, CN = N * C;
  if (CN >= (1ull << 31) || b.n_isects > a.max_isects || b.n_isects >= (1ull << 31)) return hipErrorInvalidValue;
  RasterWs w = carve((char*)a.workspace, N, C, tiles, a.max_isects);
  if (w.total > a.workspace_bytes) return hipErrorInvalidValue;
  if (wm_raster_bwd_workspace_bytes(a.N, a.C, a.width, a.height, b.n_isects) > b.grad_workspace_bytes) return hipErrorInvalidValue;
  unsigned int* flag = (unsigned int*)b.grad_workspace;
  float* pair_grad = (float*)((char*)b.grad_workspace + align256(256));
  hipError_t e = hipMemsetAsync(b.grad_workspace, 0, align256(256) + b.n_isects * PAIR_REC * sizeof(float), s);
  if (e != hipSuccess) return e;
  if (b.n_isects > 0) {
    hipLaunchKernelGGL(raster_locate_sorted_kernel, dim3((unsigned)((b.n_isects + 255) / 256)), dim3(256), 0, s, w.keys[0], (unsigned int)b.n_isects, flag);
    hipLaunchKernelGGL(raster_composite_bwd_kernel, dim3((unsigned)tiles, (unsigned)C), dim3(64), 0, s, w.g2d, w.vals[0], w.vals[1], flag, w.tile_offs,
                       w.offsets, tw, th, a.width, a.height, b.out_depth, b.v_rgb, b.v_depth, b.v_alpha, pair_grad);
  }
  hipLaunchKernelGGL(raster_project_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a.means, a.quats, a.scales, a.colors, a.is_sh,
                     a.viewmats, a.Ks, a.N, a.C, a.width, a.height, w.g2d, w.offsets, pair_grad, b.v_means, b.v_quats, b.v_scales, b.v_opacities,
                     b.v_colors);
  return hipGetLastError();
}
