// Shared between the rasteriser's forward (raster.hip) and backward (raster_bwd.hip): the per-(camera, Gaussian) record the
// projection writes, and the layout of the caller's workspace.  The backward reads what the forward left there.
#pragma once
#include "wm_common.h"

namespace wm_raster {

constexpr int TILE = 16;
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float ALPHA_THRESHOLD = 1.0f / 255.0f;

struct __attribute__((aligned(16))) G2D {  // per (camera, Gaussian): 48 B = three 16-byte scalar loads of the compositing pass
  float mx, my;         // pixel-space mean
  float ca, cb;         // conic
  float cc, opacity;
  float depth;
  float r, g, b;        // colour (view-independent: degree-0 SH or given colours)
  int rect;             // x0 | y0 << 8 | x1 << 16 | y1 << 24 in tiles (tile grids up to 255 x 255); the compositing pass reads words 0-9 only
  int pad;
};
static_assert(sizeof(G2D) == 48, "G2D is read as three dwordx4");

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RasterWs {
  G2D* g2d; unsigned long long* counts; unsigned long long* offsets; float4* rgb;
  unsigned long long* keys[2]; unsigned int* vals[2]; unsigned int* tile_offs; void* cub; size_t cub_bytes; size_t total;
};

// the forward's carving of the caller's workspace (raster.hip; base may be null: sizes only)
RasterWs carve(char* base, size_t N, size_t C, int tiles, size_t max_isects);

}  // namespace wm_raster
