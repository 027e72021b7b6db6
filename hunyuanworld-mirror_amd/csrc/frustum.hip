// Target-view validity mask of the novel-view protocol (reference: src/models/utils/frustum.py:26-89 calculate_in_frustum_mask,
// called through calculate_unprojected_mask :7-23 from the renderer, rasterization.py:11): which pixels of the V1 target views did some
// of the V2 context views actually see?
//
//   for target pixel (x, y) of view (b, i), depth d, and every context view j:
//     c  = Kinv1[b,i] (x, y, 1) d                       unproject_depth :168-196 (Kinv1 = K1^-1, taken once on the host side in fp64)
//     p  = R[b,i,j] c + t[b,i,j]                        [R | t] = c2w_2[b,j]^-1 c2w_1[b,i], rows 0..2 (:152-165, once, fp64)
//     n  = p / p.z  (no z > 0 test: :97-99, 147)        q = K2[b,j] n, (px, py) = q.xy (:136-149)
//     in_j    = 0 < px < W && 0 < py < H                :60-65
//     s       = grid_sample(depth_2[b,j], align_corners=False) at pixel coordinates (px - 0.5, py - 0.5): bilinear, zero padding :74-83
//     match_j = isclose(p.z, s, atol = 0.1, rtol = 1e-5) :84 = (p.z == s) || (|p.z - s| finite and <= 0.1 + |1e-5 s|); NaN -> false
//   mask = any_j(in_j) && d > 1e-6 && any_j(match_j)    :66, 69, 86-88 (the two any are independent)
//
// The reference materialises six [b, v1, v2, h, w, 3] fp32 tensors and samples in a triple Python loop.  Here one lane owns one target
// pixel and keeps everything in registers: it reads its depth once, loops over the context views with the four bilinear taps gathered
// straight from depth_2 (a view is 1 MB at 518^2: L2 traffic after the first touch), stops with its wave as soon as no later view can
// change the wave's bits, and writes one byte.  A block never crosses a
// target view, so the block's view index comes from blockIdx alone and the 3 + 7 V2 matrix rows it needs are wave-uniform: the compiler
// fetches them with scalar loads into SGPRs.  No atomics, no shared memory: the bits are the same on every run.
#include "wm_common.h"
#include "wm_kernels.h"

namespace {

constexpr int FR_BLOCK = 256;

// address of one tap of the zero-padded bilinear sample, clamped into the image (NaN -> 0): every tap is loaded, in-range or not
__device__ __forceinline__ int fr_addr(float xf, float yf, int H, int W) {
  return (int)fminf(fmaxf(yf, 0.f), (float)(H - 1)) * W + (int)fminf(fmaxf(xf, 0.f), (float)(W - 1));   // H W < 2^31 (checked by the entry)
}
// ... and dropped by a select when out of range.  The range test is made on the floats, so that a NaN or infinite coordinate (a point
// in the camera's plane) selects no tap, as the reference's out-of-range integer does
__device__ __forceinline__ float fr_acc(float acc, float v, float wgt, float xf, float yf, int H, int W) {
  const bool in = (xf >= 0.f) & (xf <= (float)(W - 1)) & (yf >= 0.f) & (yf <= (float)(H - 1));
  return in ? acc + v * wgt : acc;
}

__global__ __launch_bounds__(FR_BLOCK) void in_frustum_mask_kernel(const float* __restrict__ depth_1, const float* __restrict__ depth_2,
                                                                   const float* __restrict__ kinv_1, const float* __restrict__ rel,
                                                                   const float* __restrict__ k_2, int V1, int V2, int H, int W,
                                                                   unsigned int tiles, unsigned char* __restrict__ mask) {
  const unsigned int bi = blockIdx.x / tiles;                 // (b, i) flattened: wave-uniform
  const unsigned int tile = blockIdx.x - bi * tiles;
  const unsigned int b = bi / (unsigned int)V1;
  const size_t hw = (size_t)H * W;
  const size_t r = (size_t)tile * FR_BLOCK + threadIdx.x;
  if (r >= hw) return;
  const int y = (int)(r / (size_t)W), x = (int)(r - (size_t)y * W);
  const float d = depth_1[(size_t)bi * hw + r];
  const float* Ki = kinv_1 + (size_t)bi * 9;
  const float xf = (float)x, yf = (float)y;
  const float cx = (Ki[0] * xf + Ki[1] * yf + Ki[2]) * d;
  const float cy = (Ki[3] * xf + Ki[4] * yf + Ki[5]) * d;
  const float cz = (Ki[6] * xf + Ki[7] * yf + Ki[8]) * d;
  bool any_in = false, any_match = false;
  for (int j = 0; j < V2; ++j) {
    const float* M = rel + ((size_t)bi * V2 + j) * 12;
    const float* K = k_2 + ((size_t)b * V2 + j) * 9;
    const float* img = depth_2 + ((size_t)b * V2 + j) * hw;
    const float px3 = M[0] * cx + M[1] * cy + M[2] * cz + M[3];
    const float py3 = M[4] * cx + M[5] * cy + M[6] * cz + M[7];
    const float z = M[8] * cx + M[9] * cy + M[10] * cz + M[11];
    // one hardware reciprocal (1 ulp) instead of three divisions: px moves by at most 2 ulp of itself, 2^-15 px at 518, far inside
    // the 2^-10 px that no comparison against another arithmetic order can resolve anyway; z / z stays 1 or, for z = 0, inf, NaN, NaN
    const float rz = __builtin_amdgcn_rcpf(z);
    const float nx = px3 * rz, ny = py3 * rz, nz = z * rz;
    const float px = K[0] * nx + K[1] * ny + K[2] * nz;
    const float py = K[3] * nx + K[4] * ny + K[5] * nz;
    any_in |= px > 0.f && px < (float)W && py > 0.f && py < (float)H;
    // grid_sample, align_corners = False: ((2 px / W - 1 + 1) W - 1) / 2 = px - 0.5
    const float ix = px - 0.5f, iy = py - 0.5f;
    const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
    float v00 = img[fr_addr(x0, y0, H, W)], v10 = img[fr_addr(x1, y0, H, W)], v01 = img[fr_addr(x0, y1, H, W)], v11 = img[fr_addr(x1, y1, H, W)];
    // (an empty statement that owns the four values: without it hipcc moves each load under its tap's range test, four dependent
    // branches with a full wait each; with it the four gathers are in flight together)
    asm volatile("" : "+v"(v00), "+v"(v10), "+v"(v01), "+v"(v11));
    float s = 0.f;
    s = fr_acc(s, v00, (x1 - ix) * (y1 - iy), x0, y0, H, W);
    s = fr_acc(s, v10, (ix - x0) * (y1 - iy), x1, y0, H, W);
    s = fr_acc(s, v01, (x1 - ix) * (iy - y0), x0, y1, H, W);
    s = fr_acc(s, v11, (ix - x0) * (iy - y0), x1, y1, H, W);
    const float err = fabsf(z - s);
    any_match |= z == s || (err <= 0.1f + fabsf(1e-5f * s) && err < INFINITY);
    // both any are monotone: once every lane of the wave is settled (true in both, or false for good by its depth), later views cannot
    // change a bit.  Wave-uniform, so nobody waits for anybody
    if (__all((any_in && any_match) || !(d > 1e-6f))) break;
  }
  mask[(size_t)bi * hw + r] = (any_in && d > 1e-6f && any_match) ? 1 : 0;
}

}  // namespace

hipError_t wm_launch_in_frustum_mask(const float* depth_1, const float* depth_2, const float* kinv_1, const float* rel, const float* k_2, int B,
                                     int V1, int V2, int H, int W, unsigned char* mask, hipStream_t s) {
  const size_t hw = (size_t)H * W, tiles = (hw + FR_BLOCK - 1) / FR_BLOCK, blocks = tiles * (size_t)B * V1;
  if (B < 1 || V1 < 1 || V2 < 1 || H < 1 || W < 1 || blocks >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(in_frustum_mask_kernel, dim3((unsigned int)blocks), dim3(FR_BLOCK), 0, s, depth_1, depth_2, kinv_1, rel, k_2, V1, V2, H, W,
                     (unsigned int)tiles, mask);
  return hipGetLastError();
}
