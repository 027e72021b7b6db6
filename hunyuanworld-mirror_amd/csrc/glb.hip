// GLB scene hand-off: the per-view image meshes of src/utils/visual_util.py:109-205 (create_image_mesh with a mask and triangulate=True), the
// masked point cloud of :273-298 and the order statistics behind the scene scale of :306-309 (np.percentile at 5 and 95), on the device in the
// layout of the glTF BIN chunk.  The host (glb.py) writes the JSON, the camera solids and the container, and copies the finished body once.
// The C-ABI entries are in wm_api_scene.cpp; the launchers are declared in wm_api.h.
//
// image mesh (wm_launch_image_mesh_count, wm_launch_image_mesh_pack)
//   A quad at pixel p = y W + x is valid when p, p + W, p + W + 1 and p + 1 are all masked in; a pixel is a vertex when it is a corner of a
//   valid quad (np.unique over the kept faces), so both flags come from the 3 x 3 mask neighbourhood of the pixel.  Vertices come in ascending
//   pixel index and faces in raster order of the quads, (a, b, c), (a, c, d) for the quad (p, p + W, p + W + 1, p + 1), local to the view:
//     count    per block, the vertices and the valid quads                                             -> blk_v, blk_q (as counts)
//     scan     one block: the exclusive scans of both, the per-view counts and the totals             -> blk_v, blk_q, res
//     (the host reads res: the ONE stream synchronisation, to size the output)
//     vertex   per block: the flags again, an ordered in-block rank by wave ballots; position, RGBA and normal of each vertex written at
//              blk_v[block] + rank, its view-local index into remap[pixel], the block's coordinate bounds into blk_bounds
//     faces    per block: the quad flags, the rank, and the two triangles of each valid quad through remap at blk_q[block] + rank
//     bounds   one block per view: min / max of its blocks' bounds
//   A block owns GL_CHUNK consecutive pixels of ONE view, so a view's count is a difference of two block offsets.  Positions come from the
//   scans alone: no atomics, no floating-point accumulation (min and max are exact in any order), the output is a function of the input.
//   The vertices of all views are concatenated (view-major), and so are the faces; a view's rows start at the sum of the earlier counts.
//
// point cloud (wm_launch_glb_points): the same count / scan / vertex / bounds kernels over a flat list (one "view" of N items, the flag
//   being the mask byte), colours as uint8(trunc(fl32(x 255))).  positions go to out[0, 12 n) and RGBA to out[12 n, 16 n), n read on the
//   device from the scan, so one call and one synchronisation (to tell the host n) produce the BIN body.
//
// percentile neighbours (wm_launch_percentile_neighbours): for each of three columns and each quantile q, the order statistics of rank
//   floor((n - 1) q) and that + 1 (clipped to n - 1) of the masked rows, n being their number: what np.percentile's linear method
//   interpolates between.  All selections share four 8-bit radix passes; the only atomics are the integer histogram adds.
#include <vector>

#include "scene_common.h"
#include "wm_api.h"

namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_ROUNDS = 2;
constexpr int GL_CHUNK = GL_THREADS * GL_ROUNDS;      // items of one view per block

unsigned gl_bpv(long long hw) { return (unsigned)((hw + GL_CHUNK - 1) / GL_CHUNK); }

struct GlWs {
  unsigned int* blk_v; unsigned int* blk_q; float* blk_bounds; long long* res; int* remap;
  size_t total;
};

// S views of hw items; remap only for meshes
GlWs gl_carve(char* base, int S, long long hw, bool mesh) {
  GlWs w{};
  Carver c(base);
  const size_t nblk = (size_t)S * gl_bpv(hw);
  w.blk_v = c.take<unsigned int>(nblk + 1);
  w.blk_q = c.take<unsigned int>(nblk + 1);
  w.blk_bounds = c.take<float>(nblk * 6);
  w.res = c.take<long long>(2 * (size_t)S + 2);
  w.remap = mesh ? c.take<int>((size_t)S * (size_t)hw) : nullptr;
  w.total = c.total();
  return w;
}

// the mask of pixel (y, x) of one view; outside the image: false; no mask: every pixel
__device__ __forceinline__ bool gl_in(const unsigned char* __restrict__ m, int H, int W, int y, int x) {
  if (y < 0 || x < 0 || y >= H || x >= W) return false;
  return m ? m[(size_t)y * W + x] != 0 : true;
}

// the quad whose first corner is (y, x): corners (y, x), (y + 1, x), (y + 1, x + 1), (y, x + 1); gl_in refuses what lies outside
__device__ __forceinline__ bool gl_quad(const unsigned char* __restrict__ m, int H, int W, int y, int x) {
  return gl_in(m, H, W, y, x) && gl_in(m, H, W, y + 1, x) && gl_in(m, H, W, y + 1, x + 1) && gl_in(m, H, W, y, x + 1);
}

// item p of a view: MESH: (vertex, valid quad) of the pixel; else (mask byte, false).  m: the view's mask or null
template <bool MESH>
__device__ __forceinline__ void gl_flags(const unsigned char* __restrict__ m, int H, int W, long long hw, long long p, bool& used, bool& quad) {
  used = quad = false;
  if (p >= hw) return;
  if (!MESH) { used = m ? m[p] != 0 : true; return; }
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  if (!gl_in(m, H, W, y, x)) return;
  quad = gl_quad(m, H, W, y, x);
  used = quad || gl_quad(m, H, W, y - 1, x) || gl_quad(m, H, W, y, x - 1) || gl_quad(m, H, W, y - 1, x - 1);
}

template <bool MESH>
__global__ __launch_bounds__(GL_THREADS) void gl_count_kernel(const unsigned char* __restrict__ mask, int H, int W, long long hw, unsigned int bpv,
                                                              unsigned int* __restrict__ blk_v, unsigned int* __restrict__ blk_q) {
  __shared__ unsigned int sW[GL_THREADS / 64];
  const unsigned int v = blockIdx.x / bpv, c = blockIdx.x - v * bpv;
  const unsigned char* m = mask ? mask + (size_t)v * hw : nullptr;
  unsigned int nv = 0, nq = 0, tot;
#pragma unroll
  for (int r = 0; r < GL_ROUNDS; ++r) {
    const long long p = (long long)c * GL_CHUNK + r * GL_THREADS + threadIdx.x;
    bool used, quad;
    gl_flags<MESH>(m, H, W, hw, p, used, quad);
    block_rank<GL_THREADS>(used, sW, tot);
    nv += tot;
    if (MESH) {
      block_rank<GL_THREADS>(quad, sW, tot);
      nq += tot;
    }
  }
  if (threadIdx.x == 0) { blk_v[blockIdx.x] = nv; blk_q[blockIdx.x] = nq; }
}

// one block: both scans, then res[0 .. S) vertices per view, res[S .. 2S) quads per view, res[2S], res[2S + 1] the totals
__global__ __launch_bounds__(GL_THREADS) void gl_scan_kernel(unsigned int* blk_v, unsigned int* blk_q, unsigned int nblk, unsigned int bpv, int S,
                                                             long long* __restrict__ res) {
  __shared__ unsigned int part[GL_THREADS];
  block_scan_in_place<GL_THREADS>(blk_v, nblk, part);
  block_scan_in_place<GL_THREADS>(blk_q, nblk, part);
  for (int v = threadIdx.x; v < S; v += GL_THREADS) {
    res[v] = (long long)blk_v[(size_t)(v + 1) * bpv] - (long long)blk_v[(size_t)v * bpv];
    res[S + v] = (long long)blk_q[(size_t)(v + 1) * bpv] - (long long)blk_q[(size_t)v * bpv];
  }
  if (threadIdx.x == 0) { res[2 * S] = blk_v[nblk]; res[2 * S + 1] = blk_q[nblk]; }
}

// min of lo[3] and max of hi[3] over the block -> out[6]; every lane calls it
__device__ __forceinline__ void gl_block_bounds(float* lo, float* hi, float (*sB)[6] /* 4 */, float* __restrict__ out) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      lo[j] = fminf(lo[j], __shfl_xor(lo[j], o));
      hi[j] = fmaxf(hi[j], __shfl_xor(hi[j], o));
    }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { sB[w][j] = lo[j]; sB[w][3 + j] = hi[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float r = sB[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < GL_THREADS / 64; ++i) r = threadIdx.x < 3 ? fminf(r, sB[i][threadIdx.x]) : fmaxf(r, sB[i][threadIdx.x]);
    out[threadIdx.x] = r;
  }
}

// the three fp32 roundings of the reference's mesh colours (visual_util.py:400 / :416 / :428): x * 255, / 255, * 255, truncated
__device__ __forceinline__ unsigned char gl_mesh_byte(float x) {
  return (unsigned char)(int)__fmul_rn(__fdiv_rn(__fmul_rn(x, 255.f), 255.f), 255.f);
}
// the point cloud's (visual_util.py:281): one product, truncated
__device__ __forceinline__ unsigned char gl_point_byte(float x) { return (unsigned char)(int)__fmul_rn(x, 255.f); }

// rgba == null (the point cloud): RGBA follows the positions, at positions + 3 blk_v[nblk] floats.  limit: the rows the outputs hold
template <bool MESH>
__global__ __launch_bounds__(GL_THREADS) void gl_vertex_kernel(const float* __restrict__ points, const float* __restrict__ colors,
                                                               const float* __restrict__ normals, const unsigned char* __restrict__ mask, int H, int W,
                                                               long long hw, unsigned int bpv, unsigned int nblk,
                                                               const unsigned int* __restrict__ blk_v, long long limit, float* __restrict__ positions,
                                                               unsigned char* __restrict__ rgba, float* __restrict__ normals_out,
                                                               int* __restrict__ remap, float* __restrict__ blk_bounds) {
  __shared__ unsigned int sW[GL_THREADS / 64];
  __shared__ float sB[GL_THREADS / 64][6];
  const unsigned int v = blockIdx.x / bpv, c = blockIdx.x - v * bpv;
  const unsigned char* m = mask ? mask + (size_t)v * hw : nullptr;
  const unsigned int view_base = blk_v[(size_t)v * bpv];
  if (!rgba) rgba = (unsigned char*)(positions + 3 * (size_t)blk_v[nblk]);
  unsigned int run = blk_v[blockIdx.x], tot;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int r = 0; r < GL_ROUNDS; ++r) {
    const long long p = (long long)c * GL_CHUNK + r * GL_THREADS + threadIdx.x;
    bool used, quad;
    gl_flags<MESH>(m, H, W, hw, p, used, quad);
    const unsigned int pos = run + block_rank<GL_THREADS>(used, sW, tot);
    run += tot;
    if (used && (long long)pos < limit) {
      const size_t idx = (size_t)v * hw + (size_t)p;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float x = points[3 * idx + j];
        positions[3 * (size_t)pos + j] = x;
        lo[j] = fminf(lo[j], x);
        hi[j] = fmaxf(hi[j], x);
        const float col = colors[3 * idx + j];
        rgba[4 * (size_t)pos + j] = MESH ? gl_mesh_byte(col) : gl_point_byte(col);
        if (normals_out) normals_out[3 * (size_t)pos + j] = normals[3 * idx + j];
      }
      rgba[4 * (size_t)pos + 3] = 255;
      if (MESH) remap[idx] = (int)(pos - view_base);
    }
  }
  gl_block_bounds(lo, hi, sB, blk_bounds + 6 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(GL_THREADS) void gl_faces_kernel(const unsigned char* __restrict__ mask, int H, int W, long long hw, unsigned int bpv,
                                                              const unsigned int* __restrict__ blk_q, const int* __restrict__ remap, long long total_q,
                                                              int* __restrict__ faces) {
  __shared__ unsigned int sW[GL_THREADS / 64];
  const unsigned int v = blockIdx.x / bpv, c = blockIdx.x - v * bpv;
  const unsigned char* m = mask ? mask + (size_t)v * hw : nullptr;
  const int* rm = remap + (size_t)v * hw;
  unsigned int run = blk_q[blockIdx.x], tot;
#pragma unroll
  for (int r = 0; r < GL_ROUNDS; ++r) {
    const long long p = (long long)c * GL_CHUNK + r * GL_THREADS + threadIdx.x;
    bool quad = false;
    if (p < hw) {
      const int y = (int)(p / W), x = (int)(p - (long long)y * W);
      quad = gl_quad(m, H, W, y, x);
    }
    const unsigned int pos = run + block_rank<GL_THREADS>(quad, sW, tot);
    run += tot;
    if (quad && (long long)pos < total_q) {      // a valid quad has x + 1 < W and y + 1 < H: p + W + 1 < hw
      const int a = rm[p], b = rm[p + W], cc = rm[p + W + 1], d = rm[p + 1];
      int* f = faces + 6 * (size_t)pos;
      f[0] = a; f[1] = b; f[2] = cc;
      f[3] = a; f[4] = cc; f[5] = d;
    }
  }
}

// one block per view: the bounds of its bpv blocks -> bounds[view][6] (min xyz, max xyz; +inf / -inf for a view without vertices)
__global__ __launch_bounds__(GL_THREADS) void gl_bounds_kernel(const float* __restrict__ blk_bounds, unsigned int bpv, float* __restrict__ bounds) {
  __shared__ float sB[GL_THREADS / 64][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (unsigned int i = threadIdx.x; i < bpv; i += GL_THREADS) {
    const float* b = blk_bounds + 6 * ((size_t)blockIdx.x * bpv + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) { lo[j] = fminf(lo[j], b[j]); hi[j] = fmaxf(hi[j], b[3 + j]); }
  }
  gl_block_bounds(lo, hi, sB, bounds + 6 * (size_t)blockIdx.x);
}

bool gl_mesh_sizes_ok(int S, int H, int W) { return S >= 1 && H >= 1 && W >= 1 && (long long)S * H * W < (1LL << 31); }

// ---------------------------------------------------------------- percentile neighbours
constexpr int PN_MAXQ = 4;                  // quantiles per call
constexpr int PN_MAXSEL = 3 * 2 * PN_MAXQ;  // columns x (lower, upper) x quantiles
constexpr unsigned PN_MAXBLK = 2048;

struct PnQ { double q[PN_MAXQ]; };      // the quantiles, by value

struct PnState {
  unsigned int prefix[PN_MAXSEL], remaining[PN_MAXSEL];
  unsigned int n, pad;
  unsigned int hist[PN_MAXSEL][256];
};

__global__ __launch_bounds__(GL_THREADS) void pn_count_kernel(const unsigned char* __restrict__ mask, long long N, unsigned int* __restrict__ blk_cnt) {
  __shared__ unsigned int sW[GL_THREADS / 64];
  unsigned int cnt = 0, tot;
  const long long per = (N + gridDim.x - 1) / gridDim.x, lo = (long long)blockIdx.x * per, hi = lo + per < N ? lo + per : N;
  for (long long i0 = lo; i0 < hi; i0 += GL_THREADS) {      // uniform trip count within the block
    const long long i = i0 + threadIdx.x;
    block_rank<GL_THREADS>(i < hi && (mask ? mask[i] != 0 : true), sW, tot);
    cnt += tot;
  }
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}

// one block: n, the ranks of every selection (sel = (col * nq + j) * 2 + upper), the histograms zeroed
__global__ __launch_bounds__(GL_THREADS) void pn_setup_kernel(const unsigned int* __restrict__ blk_cnt, unsigned int nblk, PnQ qs, int nq,
                                                              PnState* st, long long* __restrict__ count_out) {
  __shared__ unsigned int part[GL_THREADS];
  unsigned int s = 0;
  for (unsigned int i = threadIdx.x; i < nblk; i += GL_THREADS) s += blk_cnt[i];
  part[threadIdx.x] = s;
  for (int i = threadIdx.x; i < PN_MAXSEL * 256; i += GL_THREADS) (&st->hist[0][0])[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int n = 0;
    for (int i = 0; i < GL_THREADS; ++i) n += part[i];
    st->n = n;
    st->pad = 0;
    *count_out = n;
    for (int sel = 0; sel < PN_MAXSEL; ++sel) {
      const int j = (sel >> 1) % (nq > 0 ? nq : 1);
      unsigned int rank = 0;
      if (n > 0 && sel < 6 * nq) {
        const double pos = (double)(n - 1) * qs.q[j];      // numpy's virtual index, in double
        double fl = floor(pos);
        fl = fl < 0.0 ? 0.0 : (fl > (double)(n - 1) ? (double)(n - 1) : fl);
        rank = (unsigned int)fl + (sel & 1);
        if (rank > n - 1) rank = n - 1;
      }
      st->prefix[sel] = 0;
      st->remaining[sel] = rank + 1;      // the (rank + 1)-th smallest
    }
  }
}

__global__ __launch_bounds__(GL_THREADS) void pn_hist_kernel(const float* __restrict__ points, const unsigned char* __restrict__ mask, long long N, int nq,
                                                             PnState* st, int shift) {
  __shared__ unsigned int lh[PN_MAXSEL][256];
  __shared__ unsigned int sPrefix[PN_MAXSEL];
  const int nsel = 6 * nq, per_col = 2 * nq;
  for (int i = threadIdx.x; i < nsel * 256; i += GL_THREADS) (&lh[0][0])[i] = 0;
  if ((int)threadIdx.x < nsel) sPrefix[threadIdx.x] = st->prefix[threadIdx.x];
  __syncthreads();
  const unsigned int himask = shift == 24 ? 0u : ~0u << (shift + 8);
  for (long long i = (long long)blockIdx.x * GL_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * GL_THREADS) {
    if (mask && !mask[i]) continue;
    for (int col = 0; col < 3; ++col) {
      const unsigned int key = ordered_key(points[3 * i + col]);
      for (int s = col * per_col; s < (col + 1) * per_col; ++s)
        if ((key & himask) == sPrefix[s]) atomicAdd(&lh[s][(key >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nsel * 256; i += GL_THREADS) {
    const unsigned int c = (&lh[0][0])[i];
    if (c) atomicAdd(&(&st->hist[0][0])[i], c);
  }
}

// one block, one lane per selection: walk the bins from the bottom; after the last digit the value goes to out[sel]
__global__ __launch_bounds__(GL_THREADS) void pn_pick_kernel(PnState* st, int nq, int shift, float* __restrict__ out) {
  const int nsel = 6 * nq;
  if ((int)threadIdx.x < nsel && st->n > 0) {
    const int s = threadIdx.x;
    unsigned int rem = st->remaining[s], bin = 255;
    for (unsigned int b = 0; b < 256; ++b) {
      const unsigned int h = st->hist[s][b];
      if (h >= rem) { bin = b; break; }
      rem -= h;
    }
    const unsigned int prefix = st->prefix[s] | (bin << shift);
    st->prefix[s] = prefix;
    st->remaining[s] = rem;
    if (shift == 0) out[s] = ordered_value(prefix);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nsel * 256; i += GL_THREADS) (&st->hist[0][0])[i] = 0;
}

unsigned pn_blocks(long long N) {
  const unsigned b = blocks_for(N, GL_THREADS);
  return b < 1 ? 1 : (b > PN_MAXBLK ? PN_MAXBLK : b);
}

bool pn_sizes_ok(long long N, int nq) { return N >= 0 && N < (1LL << 31) / 3 && nq >= 1 && nq <= PN_MAXQ; }

}  // namespace

// ------------------------------------------------------------------ launchers (wm_api.h)
size_t wm_image_mesh_ws_bytes(int S, int H, int W) {
  if (!gl_mesh_sizes_ok(S, H, W)) return 0;
  return gl_carve(nullptr, S, (long long)H * W, true).total;
}

hipError_t wm_launch_image_mesh_count(const unsigned char* mask, int S, int H, int W, void* workspace, long long* n_vertices, long long* n_quads,
                                      hipStream_t s) {
  if (!gl_mesh_sizes_ok(S, H, W)) return hipErrorInvalidValue;
  const long long hw = (long long)H * W;
  const GlWs w = gl_carve((char*)workspace, S, hw, true);
  const unsigned bpv = gl_bpv(hw), nblk = (unsigned)S * bpv;
  hipLaunchKernelGGL(gl_count_kernel<true>, dim3(nblk), dim3(GL_THREADS), 0, s, mask, H, W, hw, bpv, w.blk_v, w.blk_q);
  hipLaunchKernelGGL(gl_scan_kernel, dim3(1), dim3(GL_THREADS), 0, s, w.blk_v, w.blk_q, nblk, bpv, S, w.res);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  std::vector<long long> res(2 * (size_t)S + 2);
  e = read_back(res.data(), w.res, res.size() * 8, s);      // the one synchronisation: the caller sizes its outputs by the counts
  if (e != hipSuccess) return e;
  for (int v = 0; v < S; ++v) { n_vertices[v] = res[v]; n_quads[v] = res[(size_t)S + v]; }
  n_vertices[S] = res[2 * (size_t)S];
  n_quads[S] = res[2 * (size_t)S + 1];
  return hipSuccess;
}

hipError_t wm_launch_image_mesh_pack(const float* points, const float* colors, const float* normals, const unsigned char* mask, int S, int H, int W,
                                     void* workspace, long long total_v, long long total_q, float* positions, unsigned char* rgba, float* normals_out,
                                     int* faces, float* bounds, hipStream_t s) {
  if (!gl_mesh_sizes_ok(S, H, W) || total_v < 0 || total_q < 0 || total_v > (long long)S * H * W || total_q > (long long)S * H * W)
    return hipErrorInvalidValue;
  const long long hw = (long long)H * W;
  const GlWs w = gl_carve((char*)workspace, S, hw, true);
  const unsigned bpv = gl_bpv(hw), nblk = (unsigned)S * bpv;
  hipLaunchKernelGGL(gl_vertex_kernel<true>, dim3(nblk), dim3(GL_THREADS), 0, s, points, colors, normals, mask, H, W, hw, bpv, nblk,
                     (const unsigned int*)w.blk_v, total_v, positions, rgba, normals ? normals_out : nullptr, w.remap, w.blk_bounds);
  if (total_q > 0)
    hipLaunchKernelGGL(gl_faces_kernel, dim3(nblk), dim3(GL_THREADS), 0, s, mask, H, W, hw, bpv, (const unsigned int*)w.blk_q, (const int*)w.remap,
                       total_q, faces);
  hipLaunchKernelGGL(gl_bounds_kernel, dim3(S), dim3(GL_THREADS), 0, s, (const float*)w.blk_bounds, bpv, bounds);
  return hipGetLastError();
}

size_t wm_glb_points_ws_bytes(long long N) {
  if (N < 1 || N >= (1LL << 31)) return 0;
  return gl_carve(nullptr, 1, N, false).total;
}

hipError_t wm_launch_glb_points(const float* points, const float* colors, const unsigned char* mask, long long N, void* workspace, void* out,
                                long long* n_kept, float* bounds, hipStream_t s) {
  if (N < 1 || N >= (1LL << 31)) return hipErrorInvalidValue;
  const GlWs w = gl_carve((char*)workspace, 1, N, false);
  const unsigned bpv = gl_bpv(N), nblk = bpv;
  hipLaunchKernelGGL(gl_count_kernel<false>, dim3(nblk), dim3(GL_THREADS), 0, s, mask, 1, 1, N, bpv, w.blk_v, w.blk_q);
  hipLaunchKernelGGL(gl_scan_kernel, dim3(1), dim3(GL_THREADS), 0, s, w.blk_v, w.blk_q, nblk, bpv, 1, w.res);
  hipLaunchKernelGGL(gl_vertex_kernel<false>, dim3(nblk), dim3(GL_THREADS), 0, s, points, colors, (const float*)nullptr, mask, 1, 1, N, bpv, nblk,
                     (const unsigned int*)w.blk_v, N, (float*)out, (unsigned char*)nullptr, (float*)nullptr, (int*)nullptr, w.blk_bounds);
  hipLaunchKernelGGL(gl_bounds_kernel, dim3(1), dim3(GL_THREADS), 0, s, (const float*)w.blk_bounds, bpv, bounds);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  long long total = 0;
  e = read_back(&total, w.res + 2, 8, s);
  if (e != hipSuccess) return e;
  if (total < 0 || total > N) return hipErrorUnknown;
  *n_kept = total;
  return hipSuccess;
}

size_t wm_percentile_neighbours_ws_bytes(long long N, int nq) {
  if (!pn_sizes_ok(N, nq)) return 0;
  return align256(sizeof(PnState)) + align256((size_t)PN_MAXBLK * 4);
}

hipError_t wm_launch_percentile_neighbours(const float* points, const unsigned char* mask, long long N, const double* q, int nq, void* workspace,
                                           float* out, long long* count_out, hipStream_t s) {
  if (!pn_sizes_ok(N, nq)) return hipErrorInvalidValue;
  PnQ qs{};
  for (int j = 0; j < nq; ++j) {
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return hipErrorInvalidValue;
    qs.q[j] = q[j];
  }
  PnState* st = (PnState*)workspace;
  unsigned int* blk_cnt = (unsigned int*)((char*)workspace + align256(sizeof(PnState)));
  const unsigned nblk = pn_blocks(N);
  hipLaunchKernelGGL(pn_count_kernel, dim3(nblk), dim3(GL_THREADS), 0, s, mask, N, blk_cnt);
  hipLaunchKernelGGL(pn_setup_kernel, dim3(1), dim3(GL_THREADS), 0, s, (const unsigned int*)blk_cnt, nblk, qs, nq, st, count_out);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(pn_hist_kernel, dim3(nblk), dim3(GL_THREADS), 0, s, points, mask, N, nq, st, shift);
    hipLaunchKernelGGL(pn_pick_kernel, dim3(1), dim3(GL_THREADS), 0, s, st, nq, shift, out);
  }
  return hipGetLastError();
}
