// Shared between the rasteriser's forward (raster.hip) and backward (raster_bwd.hip): the per-(camera, Gaussian) record the
// projection writes, and the layout of the caller's workspace.  The backward reads what the forward left there.
#pragma once
#include "scene_common.h"
#include "wm_kernels.h"

namespace wm_raster {

constexpr int TILE = 16;
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float ALPHA_THRESHOLD = 1.0f / 255.0f;

struct __attribute__((aligned(16))) G2D {  // per (camera, Gaussian): 48 B = three 16-byte scalar loads of the compositing pass
  float mx, my;         // pixel-space mean
  float ca, cb;         // conic
  float cc, opacity;
  float depth;
  float r, g, b;        // colour: degree-0 SH or given colours (the same for every camera), or SH degree 1-3 along the pair's direction (raster_sh.hip)
  int rect;             // x0 | y0 << 8 | x1 << 16 | y1 << 24 in tiles (tile grids up to 255 x 255); the compositing pass reads words 0-9 only
  int pad;
};
static_assert(sizeof(G2D) == 48, "G2D is read as three dwordx4");

struct RasterWs {
  G2D* g2d; unsigned long long* counts; unsigned long long* offsets; float4* rgb;
  unsigned long long* keys[2]; unsigned int* vals[2]; unsigned int* tile_offs; void* cub; size_t cub_bytes; size_t total;
};

// the forward's carving of the caller's workspace (raster.hip; base may be null: sizes only)
RasterWs carve(char* base, size_t N, size_t C, int tiles, size_t max_isects);

// view-dependent colour, SH degree 1-3 (raster_sh.hip).  sh_args_valid: 1 <= sh_degree <= 3, (sh_degree + 1)^2 <= n_coeffs, campos given
bool sh_args_valid(const WmRasterArgs& a);
// after the projection: max(SH colour + 0.5, 0) into the r, g, b of every record with a tile rectangle
void launch_sh_colors(const WmRasterArgs& a, G2D* g2d, hipStream_t s);
// after the projection backward: v_colors [N,K,3] written, the direction's term added to v_means, v_campos [C,3] where asked for
// (campos_part: sh_campos_part_bytes of workspace); pair_grad: the compositing backward's tile records of rec floats
size_t sh_campos_part_bytes(size_t N, size_t C);
void launch_sh_bwd(const WmRasterBwdArgs& b, const RasterWs& w, const float* pair_grad, int rec, double* campos_part, hipStream_t s);

}  // namespace wm_raster
