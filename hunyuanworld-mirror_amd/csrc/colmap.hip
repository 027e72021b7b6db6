// COLMAP hand-off: the point selection of infer.py:296-335 (--save_colmap), the per-point bodies of images.bin and points3D.bin that
// pycolmap's Reconstruction.write produces from src/utils/build_pycolmap_recon.py:36-51, 76-77, and the coloured point-cloud PLY rows of
// src/utils/save_utils.py:81-130 (save_scene_ply, save_points_ply), all on the device in the byte order of the files.  The host writes the
// headers and copies each finished body once.  The C-ABI entries are in wm_api_scene.cpp; the launchers are declared in wm_api.h.
//
// selection (wm_launch_colmap_select, wm_launch_colmap_gather)
//   A pixel is a candidate when depth > eps (depth_to_world_coords_points' mask, elementwise.hip).  Candidates are ordered view-major and
//   row-major inside a view.  Of the N_valid candidates the K = max(1, ceil(N_valid (100 - p) / 100)) highest confidences are kept (p <= 0:
//   all of them), conf <= 1e-5 counting as -inf (conf_key, scene_common.h) and ties at the K-th value going to the lowest candidate
//   index: select.hip's rules, restated here because K depends on N_valid, which only the device knows.  Nothing of [S,H,W,3] is
//   materialised and no index list is formed:
//     count    per block, the number of candidates                                                  -> blk_off (as counts)
//     setup    one block: N_valid, K, the select state
//     hist / pick  4 x (8-bit histogram of the candidates' keys under the fixed prefix; walk the bins from the top): the K-th largest key
//     count2   per block, the candidates above the K-th key and the candidates equal to it        -> blk_gt, blk_eq
//     scan     one block: exclusive scan of blk_eq (the tie ranks), kept per block = gt + clamp(need_eq - ties before, 0, eq), exclusive scan of
//              that (the output positions), the per-view counts and the total                        -> blk_eq, blk_off, res
//     (the host reads res: the ONE stream synchronisation)
//     gather   per block: the flags again, an ordered in-block rank by wave ballots, and the kept pixels' world point, colour and (x, y, view)
//              written at blk_off[block] + rank
//   A block owns CM_CHUNK consecutive pixels of ONE view, so a view's count is a difference of two block offsets.  Positions come from the
//   two scans alone: the order does not depend on block scheduling.  The only atomics are the integer histogram adds.
//
// packing (wm_launch_colmap_pack, wm_launch_point_ply)
//   points3D.bin: 59-byte records, points3D.ply: 15-byte rows.  Neither is a multiple of 4, so a block stages its 256 records in LDS (256
//   records are a whole number of dwords) and writes them out as consecutive dwords, the last block's remainder as bytes.  images.bin's
//   per-point part is 3 x 8 bytes (x, y as f64, point3D_id): one lane per 8-byte word.  The view of a point and its index inside the view
//   come from the exclusive prefix of `counts` (the order is view-major), found by a search over the S + 1 offsets.
#include <vector>

#include "scene_common.h"
#include "wm_api.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_ROUNDS = 2;
constexpr int CM_CHUNK = CM_THREADS * CM_ROUNDS;      // pixels of one view per block

struct CmState {
  unsigned int prefix, remaining, kth, need_eq, total_eq, nvalid, K, pad;
  unsigned int hist[256];
};

struct CmWs {
  CmState* st; unsigned int* blk_gt; unsigned int* blk_eq; unsigned int* blk_off; long long* res;
  size_t total;
};

unsigned cm_bpv(int H, int W) { return (unsigned)(((size_t)H * W + CM_CHUNK - 1) / CM_CHUNK); }

CmWs cm_carve(char* base, int S, int H, int W) {
  CmWs w{};
  Carver c(base);
  const size_t nblk = (size_t)S * cm_bpv(H, W);
  w.st = c.take<CmState>(1);
  w.blk_gt = c.take<unsigned int>(nblk + 1);
  w.blk_eq = c.take<unsigned int>(nblk + 1);
  w.blk_off = c.take<unsigned int>(nblk + 1);
  w.res = c.take<long long>((size_t)S + 1);
  w.total = c.total();
  return w;
}

struct CmPix { bool valid; unsigned int key; size_t idx; int p; };

// pixel `round * 256 + tid` of this block's chunk: its view-local index p, the flat index, the candidate rule and the key
__device__ __forceinline__ CmPix cm_pixel(const float* __restrict__ depth, const float* __restrict__ conf, int hw, unsigned int bpv, float eps, int round) {
  CmPix px;
  const unsigned int v = blockIdx.x / bpv, c = blockIdx.x - v * bpv;
  const long long p = (long long)c * CM_CHUNK + round * CM_THREADS + threadIdx.x;
  px.p = (int)p;
  px.idx = (size_t)v * hw + (size_t)p;
  px.valid = p < hw && depth[px.idx] > eps;      // NaN compares false
  px.key = px.valid ? conf_key(conf[px.idx]) : 0u;
  return px;
}

__global__ __launch_bounds__(CM_THREADS) void cm_valid_count_kernel(const float* __restrict__ depth, int hw, unsigned int bpv, float eps,
                                                                    unsigned int* __restrict__ blk_cnt) {
  __shared__ unsigned int sW[CM_THREADS / 64];
  const unsigned int v = blockIdx.x / bpv, c = blockIdx.x - v * bpv;
  unsigned int cnt = 0, tot;
#pragma unroll
  for (int r = 0; r < CM_ROUNDS; ++r) {
    const long long p = (long long)c * CM_CHUNK + r * CM_THREADS + threadIdx.x;
    const bool ok = p < hw && depth[(size_t)v * hw + (size_t)p] > eps;
    block_rank<CM_THREADS>(ok, sW, tot);
    cnt += tot;
  }
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}

// one block: N_valid and K (infer.py:44-50 in double, as numpy), the select state zeroed
__global__ __launch_bounds__(CM_THREADS) void cm_setup_kernel(const unsigned int* __restrict__ blk_cnt, unsigned int nblk, double percent, CmState* st) {
  __shared__ unsigned int part[CM_THREADS];
  unsigned int s = 0;
  for (unsigned int i = threadIdx.x; i < nblk; i += CM_THREADS) s += blk_cnt[i];
  part[threadIdx.x] = s;
  st->hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int n = 0;
    for (int i = 0; i < CM_THREADS; ++i) n += part[i];
    unsigned int K = 0;
    if (n) {
      double keep = (double)n;
      if (percent > 0.0) keep = ceil((double)n * (100.0 - percent) / 100.0);
      K = keep < 1.0 ? 1u : (keep > (double)n ? n : (unsigned int)keep);
    }
    st->prefix = 0; st->remaining = K; st->kth = 0; st->need_eq = 0; st->total_eq = 0; st->nvalid = n; st->K = K; st->pad = 0;
  }
}

__global__ __launch_bounds__(CM_THREADS) void cm_hist_kernel(const float* __restrict__ depth, const float* __restrict__ conf, int hw, unsigned int bpv,
                                                             float eps, CmState* st, int shift) {
  __shared__ unsigned int lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const unsigned int prefix = st->prefix;
  const unsigned int himask = shift == 24 ? 0u : ~0u << (shift + 8);
#pragma unroll
  for (int r = 0; r < CM_ROUNDS; ++r) {
    const CmPix px = cm_pixel(depth, conf, hw, bpv, eps, r);
    if (px.valid && (px.key & himask) == prefix) atomicAdd(&lh[(px.key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], lh[threadIdx.x]);
}

__global__ __launch_bounds__(CM_THREADS) void cm_pick_kernel(CmState* st, int shift) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = st->hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int rem = st->remaining, bin = 0;
    for (int b = 255; b >= 0; --b) {
      if (h[b] >= rem) { bin = (unsigned int)b; break; }
      rem -= h[b];
    }
    st->prefix |= bin << shift;
    st->remaining = rem;
    if (shift == 0) { st->kth = st->prefix; st->need_eq = rem; st->total_eq = h[bin]; }
  }
  __syncthreads();
  st->hist[threadIdx.x] = 0;
}

__global__ __launch_bounds__(CM_THREADS) void cm_count_kernel(const float* __restrict__ depth, const float* __restrict__ conf, int hw, unsigned int bpv,
                                                              float eps, const CmState* st, unsigned int* __restrict__ blk_gt,
                                                              unsigned int* __restrict__ blk_eq) {
  __shared__ unsigned int sW[CM_THREADS / 64];
  const unsigned int kth = st->kth;
  unsigned int gt = 0, eq = 0, tot;
#pragma unroll
  for (int r = 0; r < CM_ROUNDS; ++r) {
    const CmPix px = cm_pixel(depth, conf, hw, bpv, eps, r);
    block_rank<CM_THREADS>(px.valid && px.key > kth, sW, tot);
    gt += tot;
    block_rank<CM_THREADS>(px.valid && px.key == kth, sW, tot);
    eq += tot;
  }
  if (threadIdx.x == 0) { blk_gt[blockIdx.x] = gt; blk_eq[blockIdx.x] = eq; }
}

// one block: tie ranks, kept per block, output offsets, per-view counts and the total (res[0 .. S) and res[S])
__global__ __launch_bounds__(CM_THREADS) void cm_scan_kernel(const unsigned int* __restrict__ blk_gt, unsigned int* blk_eq, unsigned int* blk_off,
                                                             unsigned int nblk, unsigned int bpv, int S, const CmState* st, long long* __restrict__ res) {
  __shared__ unsigned int part[CM_THREADS];
  const unsigned int need = st->nvalid ? st->need_eq : 0u;
  const unsigned int per = (nblk + CM_THREADS - 1) / CM_THREADS, lo = threadIdx.x * per, hi = lo + per < nblk ? lo + per : nblk;
  for (unsigned int i = lo; i < hi; ++i) blk_off[i] = blk_eq[i];      // the tie counts themselves: the scan below overwrites blk_eq
  block_scan_in_place<CM_THREADS>(blk_eq, nblk, part);
  for (unsigned int i = lo; i < hi; ++i) {
    const unsigned int before = blk_eq[i], eq = blk_off[i];
    const unsigned int left = need > before ? need - before : 0u;
    blk_off[i] = blk_gt[i] + (left < eq ? left : eq);
  }
  block_scan_in_place<CM_THREADS>(blk_off, nblk, part);
  for (int v = threadIdx.x; v <= S; v += CM_THREADS)
    res[v] = v < S ? (long long)blk_off[(size_t)(v + 1) * bpv] - (long long)blk_off[(size_t)v * bpv] : (long long)blk_off[nblk];
}

__global__ __launch_bounds__(CM_THREADS) void cm_gather_kernel(const float* __restrict__ depth, const float* __restrict__ conf,
                                                               const float* __restrict__ images, const float* __restrict__ c2w,
                                                               const float* __restrict__ intr, int H, int W, unsigned int bpv, float eps, double scale_x,
                                                               double scale_y, const CmState* st, const unsigned int* __restrict__ blk_eq,
                                                               const unsigned int* __restrict__ blk_off, unsigned int n_kept, float* __restrict__ points,
                                                               unsigned char* __restrict__ colors, int* __restrict__ xyf) {
  __shared__ unsigned int sW[CM_THREADS / 64];
  const int hw = H * W;
  const unsigned int kth = st->kth, need = st->nvalid ? st->need_eq : 0u;
  const unsigned int view = blockIdx.x / bpv;
  unsigned int eq_run = blk_eq[blockIdx.x], out_run = blk_off[blockIdx.x], tot;
#pragma unroll
  for (int r = 0; r < CM_ROUNDS; ++r) {
    const CmPix px = cm_pixel(depth, conf, hw, bpv, eps, r);
    const bool is_eq = px.valid && px.key == kth;
    const unsigned int eq_rank = eq_run + block_rank<CM_THREADS>(is_eq, sW, tot);
    eq_run += tot;
    const bool keep = px.valid && (px.key > kth || (is_eq && eq_rank < need));
    const unsigned int pos = out_run + block_rank<CM_THREADS>(keep, sW, tot);
    out_run += tot;
    if (keep && pos < n_kept) {
      const int y = px.p / W, x = px.p - y * W;
      const float* K = intr + view * 9;
      const float* E = c2w + view * 16;
      // depth_to_world_kernel's expressions (elementwise.hip): (u - cx) z / fx, then R cam + t
      const float z = depth[px.idx];
      const float cx_ = __fdiv_rn(__fmul_rn((float)x - K[2], z), K[0]);
      const float cy_ = __fdiv_rn(__fmul_rn((float)y - K[5], z), K[4]);
#pragma unroll
      for (int j = 0; j < 3; ++j) points[3 * (size_t)pos + j] = E[4 * j] * cx_ + E[4 * j + 1] * cy_ + E[4 * j + 2] * z + E[4 * j + 3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float c = images[((size_t)view * 3 + ch) * hw + px.p];
        colors[3 * (size_t)pos + ch] = (unsigned char)(int)__fmul_rn(fminf(fmaxf(c, 0.f), 1.f), 255.f);      // NaN -> 0; the cast truncates
      }
      xyf[3 * (size_t)pos] = (int)((double)x * scale_x);
      xyf[3 * (size_t)pos + 1] = (int)((double)y * scale_y);
      xyf[3 * (size_t)pos + 2] = (int)view;
    }
  }
}

// ---------------------------------------------------------------- packing
__device__ __forceinline__ void cm_put(unsigned char* p, unsigned long long v, int nbytes) {
#pragma unroll
  for (int j = 0; j < nbytes; ++j) p[j] = (unsigned char)(v >> (8 * j));
}
__device__ __forceinline__ unsigned long long cm_f64(double v) { return (unsigned long long)__double_as_longlong(v); }

// a block's staged records (n_rec of REC bytes, in sRec) to out + block * 256 * REC: dwords, then the last 0..3 bytes
template <int REC>
__device__ __forceinline__ void cm_flush(const unsigned int* sRec, int n_rec, unsigned char* __restrict__ out) {
  const size_t base = (size_t)blockIdx.x * CM_THREADS * REC;      // a multiple of 4
  const int nbytes = n_rec * REC, ndw = nbytes >> 2;
  unsigned int* out32 = (unsigned int*)(out + base);
  for (int i = threadIdx.x; i < ndw; i += CM_THREADS) out32[i] = sRec[i];
  const int tail = nbytes & 3;
  if ((int)threadIdx.x < tail) out[base + 4 * (size_t)ndw + threadIdx.x] = ((const unsigned char*)sRec)[4 * ndw + threadIdx.x];
}

__global__ void cm_offsets_kernel(const long long* __restrict__ counts, int S, long long* __restrict__ offs) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    long long run = 0;
    for (int v = 0; v < S; ++v) { offs[v] = run; run += counts[v] > 0 ? counts[v] : 0; }
    offs[S] = run;
  }
}

// the view that holds global point r: the last v in [0, S) with offs[v] <= r (views without points share an offset with their successor)
__device__ __forceinline__ int cm_view_of(const long long* __restrict__ offs, int S, long long r) {
  int lo = 0, hi = S;      // first v in (0, S] with offs[v] > r, minus one
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// points3D.bin: u64 id | 3 f64 xyz | 3 u8 rgb | f64 error = -1 | u64 track length = 1 | u32 image_id | u32 point2D_idx
__global__ __launch_bounds__(CM_THREADS) void cm_pack_points3d_kernel(const float* __restrict__ points, const unsigned char* __restrict__ colors,
                                                                      const long long* __restrict__ offs, int S, long long P,
                                                                      unsigned char* __restrict__ out) {
  constexpr int REC = 59;
  __shared__ unsigned int sRec[CM_THREADS * REC / 4];
  const long long r = (long long)blockIdx.x * CM_THREADS + threadIdx.x;
  if (r < P) {
    unsigned char* p = (unsigned char*)sRec + threadIdx.x * REC;
    const int v = cm_view_of(offs, S, r);
    cm_put(p, (unsigned long long)(r + 1), 8);
#pragma unroll
    for (int j = 0; j < 3; ++j) cm_put(p + 8 + 8 * j, cm_f64((double)points[3 * r + j]), 8);
#pragma unroll
    for (int j = 0; j < 3; ++j) p[32 + j] = colors[3 * r + j];
    cm_put(p + 35, cm_f64(-1.0), 8);
    cm_put(p + 43, 1ull, 8);
    cm_put(p + 51, (unsigned long long)(v + 1), 4);
    cm_put(p + 55, (unsigned long long)(r - offs[v]), 4);
  }
  __syncthreads();
  const long long left = P - (long long)blockIdx.x * CM_THREADS;
  cm_flush<REC>(sRec, (int)(left < CM_THREADS ? left : CM_THREADS), out);
}

// images.bin, per kept point: f64 x | f64 y | u64 point3D_id; one lane per 8-byte word
__global__ __launch_bounds__(CM_THREADS) void cm_pack_points2d_kernel(const int* __restrict__ xyf, long long P, unsigned long long* __restrict__ out) {
  const long long e = (long long)blockIdx.x * CM_THREADS + threadIdx.x;
  if (e >= 3 * P) return;
  const long long r = e / 3;
  const int w = (int)(e - 3 * r);
  out[e] = w == 2 ? (unsigned long long)(r + 1) : cm_f64((double)xyf[3 * r + w]);
}

// ---- point-cloud PLY rows: 3 f32 | 3 u8
__device__ __forceinline__ bool cm_ply_keep(const float* __restrict__ points, const unsigned char* __restrict__ keep, int filter_finite, long long N) {
  const long long i = (long long)blockIdx.x * CM_THREADS + threadIdx.x;
  if (i >= N) return false;
  if (keep) return keep[i] != 0;
  if (filter_finite) return finite_f32(points[3 * i]) && finite_f32(points[3 * i + 1]) && finite_f32(points[3 * i + 2]);
  return true;
}

__global__ __launch_bounds__(CM_THREADS) void cm_ply_count_kernel(const float* __restrict__ points, const unsigned char* __restrict__ keep, int filter_finite,
                                                                  long long N, unsigned int* __restrict__ blk_cnt) {
  __shared__ unsigned int sW[CM_THREADS / 64];
  unsigned int tot;
  block_rank<CM_THREADS>(cm_ply_keep(points, keep, filter_finite, N), sW, tot);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(CM_THREADS) void cm_scan1_kernel(unsigned int* blk, unsigned int nblk) {
  __shared__ unsigned int part[CM_THREADS];
  block_scan_in_place<CM_THREADS>(blk, nblk, part);
}

__global__ __launch_bounds__(CM_THREADS) void cm_ply_scatter_kernel(const float* __restrict__ points, const unsigned char* __restrict__ keep, int filter_finite,
                                                                    long long N, const unsigned int* __restrict__ blk_off, unsigned int* __restrict__ kept) {
  __shared__ unsigned int sW[CM_THREADS / 64];
  unsigned int tot;
  const bool k = cm_ply_keep(points, keep, filter_finite, N);
  const unsigned int pos = blk_off[blockIdx.x] + block_rank<CM_THREADS>(k, sW, tot);
  if (k) kept[pos] = (unsigned int)((long long)blockIdx.x * CM_THREADS + threadIdx.x);
}

// kept == null: rows 0 .. n in order
__global__ __launch_bounds__(CM_THREADS) void cm_pack_ply_kernel(const float* __restrict__ points, const unsigned char* __restrict__ colors,
                                                                 const unsigned int* __restrict__ kept, long long n, unsigned char* __restrict__ out) {
  constexpr int REC = 15;
  __shared__ unsigned int sRec[CM_THREADS * REC / 4];
  const long long r = (long long)blockIdx.x * CM_THREADS + threadIdx.x;
  if (r < n) {
    const long long i = kept ? (long long)kept[r] : r;
    unsigned char* p = (unsigned char*)sRec + threadIdx.x * REC;
#pragma unroll
    for (int j = 0; j < 3; ++j) cm_put(p + 4 * j, __float_as_uint(points[3 * i + j]), 4);
#pragma unroll
    for (int j = 0; j < 3; ++j) p[12 + j] = colors[3 * i + j];
  }
  __syncthreads();
  const long long left = n - (long long)blockIdx.x * CM_THREADS;
  cm_flush<REC>(sRec, (int)(left < CM_THREADS ? left : CM_THREADS), out);
}

bool cm_select_sizes_ok(int S, int H, int W) { return S >= 1 && H >= 1 && W >= 1 && (long long)S * H * W < (1LL << 31); }

}  // namespace

// ------------------------------------------------------------------ launchers (wm_api.h)
size_t wm_colmap_select_ws_bytes(int S, int H, int W) {
  if (!cm_select_sizes_ok(S, H, W)) return 0;
  return cm_carve(nullptr, S, H, W).total;
}

hipError_t wm_launch_colmap_select(const float* depth, const float* conf, int S, int H, int W, float eps, double percent, void* workspace,
                                   long long* n_kept, long long* counts, hipStream_t s) {
  if (!cm_select_sizes_ok(S, H, W)) return hipErrorInvalidValue;
  const CmWs w = cm_carve((char*)workspace, S, H, W);
  const unsigned bpv = cm_bpv(H, W), nblk = (unsigned)S * bpv;
  const int hw = H * W;
  hipLaunchKernelGGL(cm_valid_count_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, depth, hw, bpv, eps, w.blk_off);
  hipLaunchKernelGGL(cm_setup_kernel, dim3(1), dim3(CM_THREADS), 0, s, (const unsigned int*)w.blk_off, nblk, percent, w.st);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(cm_hist_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, depth, conf, hw, bpv, eps, w.st, shift);
    hipLaunchKernelGGL(cm_pick_kernel, dim3(1), dim3(CM_THREADS), 0, s, w.st, shift);
  }
  hipLaunchKernelGGL(cm_count_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, depth, conf, hw, bpv, eps, (const CmState*)w.st, w.blk_gt, w.blk_eq);
  hipLaunchKernelGGL(cm_scan_kernel, dim3(1), dim3(CM_THREADS), 0, s, (const unsigned int*)w.blk_gt, w.blk_eq, w.blk_off, nblk, bpv, S,
                     (const CmState*)w.st, w.res);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  std::vector<long long> res((size_t)S + 1);
  e = read_back(res.data(), w.res, res.size() * 8, s);      // the one synchronisation: the caller sizes its outputs by *n_kept
  if (e != hipSuccess) return e;
  for (int v = 0; v < S; ++v) counts[v] = res[v];
  *n_kept = res[S];
  return hipSuccess;
}

hipError_t wm_launch_colmap_gather(const float* depth, const float* conf, const float* images, const float* c2w, const float* intr, int S, int H, int W,
                                   float eps, double scale_x, double scale_y, const void* workspace, long long n_kept, float* points,
                                   unsigned char* colors, int* xyf, hipStream_t s) {
  if (!cm_select_sizes_ok(S, H, W) || n_kept < 0 || n_kept > (long long)S * H * W) return hipErrorInvalidValue;
  if (n_kept == 0) return hipSuccess;
  const CmWs w = cm_carve((char*)workspace, S, H, W);
  const unsigned bpv = cm_bpv(H, W), nblk = (unsigned)S * bpv;
  hipLaunchKernelGGL(cm_gather_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, depth, conf, images, c2w, intr, H, W, bpv, eps, scale_x, scale_y,
                     (const CmState*)w.st, (const unsigned int*)w.blk_eq, (const unsigned int*)w.blk_off, (unsigned int)n_kept, points, colors, xyf);
  return hipGetLastError();
}

size_t wm_colmap_pack_ws_bytes(long long P, int S) {
  if (P < 0 || P >= (1LL << 31) || S < 1) return 0;
  return align256(((size_t)S + 1) * 8);
}

hipError_t wm_launch_colmap_pack(const float* points, const unsigned char* colors, const int* xyf, const long long* counts, int S, long long P,
                                 void* workspace, void* points3d, void* points2d, hipStream_t s) {
  if (P < 0 || P >= (1LL << 31) || S < 1) return hipErrorInvalidValue;
  if (P == 0) return hipSuccess;
  long long* offs = (long long*)workspace;
  if (points3d) {
    hipLaunchKernelGGL(cm_offsets_kernel, dim3(1), dim3(64), 0, s, counts, S, offs);
    hipLaunchKernelGGL(cm_pack_points3d_kernel, dim3(blocks_for(P, CM_THREADS)), dim3(CM_THREADS), 0, s, points, colors, (const long long*)offs, S, P,
                       (unsigned char*)points3d);
  }
  if (points2d)
    hipLaunchKernelGGL(cm_pack_points2d_kernel, dim3(blocks_for(3 * P, CM_THREADS)), dim3(CM_THREADS), 0, s, xyf, P, (unsigned long long*)points2d);
  return hipGetLastError();
}

size_t wm_point_ply_ws_bytes(long long N) {
  if (N < 0 || N >= (1LL << 31)) return 0;
  const size_t rows = (size_t)(N > 0 ? N : 1);
  return align256(((size_t)blocks_for((long long)rows, CM_THREADS) + 1) * 4) + align256(rows * 4);
}

hipError_t wm_launch_point_ply(const float* points, const unsigned char* colors, const unsigned char* keep, int filter_finite, long long N,
                               void* workspace, void* out, long long* n_kept, hipStream_t s) {
  if (N < 0 || N >= (1LL << 31)) return hipErrorInvalidValue;
  *n_kept = 0;
  if (N == 0) return hipSuccess;
  const unsigned nblk = blocks_for(N, CM_THREADS);
  const unsigned int* kept = nullptr;
  long long n = N;
  if (keep || filter_finite) {
    unsigned int* blk = (unsigned int*)workspace;
    unsigned int* list = (unsigned int*)((char*)workspace + align256(((size_t)nblk + 1) * 4));
    hipLaunchKernelGGL(cm_ply_count_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, points, keep, filter_finite, N, blk);
    hipLaunchKernelGGL(cm_scan1_kernel, dim3(1), dim3(CM_THREADS), 0, s, blk, nblk);
    hipLaunchKernelGGL(cm_ply_scatter_kernel, dim3(nblk), dim3(CM_THREADS), 0, s, points, keep, filter_finite, N, (const unsigned int*)blk, list);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    unsigned int total = 0;
    e = read_back(&total, blk + nblk, 4, s);
    if (e != hipSuccess) return e;
    if ((long long)total > N) return hipErrorUnknown;
    n = total;
    kept = list;
  }
  *n_kept = n;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(cm_pack_ply_kernel, dim3(blocks_for(n, CM_THREADS)), dim3(CM_THREADS), 0, s, points, colors, kept, n, (unsigned char*)out);
  return hipGetLastError();
}
