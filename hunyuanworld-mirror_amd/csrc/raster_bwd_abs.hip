// The absgrad instantiation of the rasteriser's compositing backward (raster_bwd_composite.h): 12-float pair records, the two extra
// sums being the per-pixel absolute values of the 2-D mean terms (gsplat's absgrad, RasterizeToPixels3DGSBwd.cu).
#include "raster_bwd_composite.h"

void wm_launch_composite_bwd_abs(dim3 grid, hipStream_t s, const wm_raster::G2D* g2d, const unsigned int* vals0, const unsigned int* vals1,
                                 const unsigned int* which, const unsigned int* offs, const unsigned long long* pair_offs, int tw, int th, int width,
                                 int height, const float* out_depth, const float* v_rgb, const float* v_depth, const float* v_alpha, float* pair_grad,
                                 const float* backgrounds, int depth_mode) {
  hipLaunchKernelGGL(raster_composite_bwd_kernel<PAIR_REC_ABS>, grid, dim3(64), 0, s, g2d, vals0, vals1, which, offs, pair_offs, tw, th, width, height,
                     out_depth, v_rgb, v_depth, v_alpha, pair_grad, backgrounds, depth_mode);
}
