// The compositing backward of the rasteriser, as a template over the pair record's width.  Each width is instantiated in a file of its
// own: the 10-float kernel in raster_bwd.hip stays the one compositing-backward kernel of that file, compiled as it was before the
// record width became a parameter; the 12-float (absgrad) kernel lives in raster_bwd_abs.hip.
#pragma once
#include "wm_common.h"
#include "raster_common.h"

namespace {

using namespace wm_raster;

constexpr int PAIR_REC = 10;       // floats per (Gaussian, tile) pair: v_mx v_my | v_ca v_cb v_cc | v_opacity | v_r v_g v_b | v_depth
constexpr int PAIR_REC_ABS = 12;   // ... | sum |v_mx of a pixel|  sum |v_my of a pixel|   (absgrad)

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
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_of_f64(double x) {   // as dpp_of, on both halves
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sum over the 64 lanes in the order of wave_sum_hi; the total is valid in lanes 48-63
__device__ __forceinline__ double wave_sum_hi_f64(double v) {
  v += dpp_of_f64<0xB1, 0xf>(v);
  v += dpp_of_f64<0x4E, 0xf>(v);
  v += dpp_of_f64<0x141, 0xf>(v);
  v += dpp_of_f64<0x140, 0xf>(v);
  v += dpp_of_f64<0x142, 0xa>(v);
  v += dpp_of_f64<0x143, 0xc>(v);
  return v;
}

// Blending rules: raster.hip raster_composite_kernel (RasterizeToPixels3DGSFwd.cu:118-184); backward terms:
// RasterizeToPixels3DGSBwd.cu (per pixel, last blended Gaussian to first).
// REC: floats per pair record: PAIR_REC (instantiated in raster_bwd.hip) or PAIR_REC_ABS with the two absgrad sums (raster_bwd_abs.hip)
template <int REC>
__global__ __launch_bounds__(64) void raster_composite_bwd_kernel(const G2D* __restrict__ g2d, const unsigned int* __restrict__ vals0,
                                              const unsigned int* __restrict__ vals1, const unsigned int* __restrict__ which,
                                              const unsigned int* __restrict__ offs, const unsigned long long* __restrict__ pair_offs,
                                              int tw, int th, int width, int height, const float* __restrict__ out_depth,
                                              const float* __restrict__ v_rgb, const float* __restrict__ v_depth,
                                              const float* __restrict__ v_alpha, float* __restrict__ pair_grad,
                                              const float* __restrict__ backgrounds, int depth_mode) {
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
  // ---- cotangents of the four composited channels and of alpha; the expected-depth division D / max(alpha, 1e-10) is undone here.
  // Prologue options (wave-uniform, as the forward's epilogue): depth_mode 1 (accumulated depth): the depth cotangent is that of D
  // itself and alpha's has no depth term; backgrounds [C,3]: rgb = composited + bg (1 - alpha) gives alpha's cotangent - v_rgb . bg[cam].
  float bgr = 0.f, bgg = 0.f, bgb = 0.f;
  if (backgrounds) { bgr = backgrounds[3 * cam]; bgg = backgrounds[3 * cam + 1]; bgb = backgrounds[3 * cam + 2]; }
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
      vd[q] = depth_mode ? ved : ved * inv;
      float val = v_alpha[pix];
      if (!depth_mode) val -= al > 1e-10f ? ved * out_depth[pix] * inv : 0.f;
      if (backgrounds) val -= vr[q] * bgr + vg[q] * bgg + vb[q] * bgb;
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
    float s_ax = 0.f, s_ay = 0.f;
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
      if constexpr (REC == PAIR_REC_ABS) { s_ax += fabsf(vs * (ca * dx[q] + cb * dy[q])); s_ay += fabsf(vs * (cb * dx[q] + cc * dy[q])); }
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
    if constexpr (REC == PAIR_REC_ABS) {
      s_ax = wave_sum_hi(s_ax); s_ay = wave_sum_hi(s_ay);
      o = lane == 58 ? s_ax : o; o = lane == 59 ? s_ay : o;
    }
    if (lane >= 48 && lane < 48 + REC) pair_grad[slot * REC + (lane - 48)] = o;
  }
}

}  // namespace

// the 12-float instantiation (raster_bwd_abs.hip): same grid, block and arguments as the 10-float launch in raster_bwd.hip
void wm_launch_composite_bwd_abs(dim3 grid, hipStream_t s, const wm_raster::G2D* g2d, const unsigned int* vals0, const unsigned int* vals1,
                                 const unsigned int* which, const unsigned int* offs, const unsigned long long* pair_offs, int tw, int th, int width,
                                 int height, const float* out_depth, const float* v_rgb, const float* v_depth, const float* v_alpha, float* pair_grad,
                                 const float* backgrounds, int depth_mode);
