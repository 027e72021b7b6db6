// Exact k nearest neighbours of a 3-D cloud within itself: the reference's knn (submodules/gsplat/examples/utils.py:141-145, scikit-learn's
// kd-tree on the host) as the trainer's create_splats_with_optimizers uses it (simple_trainer_worldmirror.py:334-337), on the device.
// The C-ABI entries are in wm_api_scene.cpp; the launchers are declared in wm_api.h.
//
//   init / bbox   the bounding box (integer atomic min / max of the order-preserving image of the floats) and the non-finite flag
//   keys          t = x - min per axis, q = floor(t * scale) clamped to 21 bits, ONE scale for the three axes (2^21 / the largest extent:
//                 cubic cells, so a flat or thin cloud keeps cubic neighbourhoods), 63-bit Morton key; value = the row
//   sort          hipcub::DeviceRadixSort::SortPairs (stable)
//   gather        the points in sorted order, (x, y, z, row) as one 16-byte record
//   query         one query per lane, queries in sorted order (the lanes of a wave walk the same cells).  A level-L cell is 2^L finest
//                 cells wide: all keys with the same top 63 - 3L bits, a contiguous run of the sorted keys found by two binary searches.
//                   start level  the finer of the two cells that hold the query and its K-th sorted neighbour to the left / to the right
//                                (common Morton prefix): at least K + 1 points, sized by the local density and not by the bounding box
//                   a pass       the 3 x 3 x 3 cells of the level, the query's own first; a cell whose box is farther than the current
//                                K-th distance is stepped over, a cell of more than 48 points is taken apart into its finer cells under
//                                the same rule (kn_walk: the sorted order is the octree's depth-first order, so no stack is kept); the
//                                candidates go through a K-slot insertion list in registers, ordered by (distance, row)
//                   accept       when the K-th distance is no larger than the distance from the query to the faces of the 3 x 3 x 3 block.
//                                Otherwise the list is emptied and the pass repeated at the finest coarser level whose block faces are at
//                                least the K-th distance away (with fewer than K candidates: one level coarser).  The blocks are nested,
//                                so that second pass is accepted; level 21 is the whole cloud and accepts unconditionally.
//                   a full list whose K-th distance is 0 ends the search at once: nothing is nearer than a duplicate.
//                 The result goes to the query's input row.
//
// Exactness.  A distance is sqrt(dx dx + dy dy + dz dz) in fp32 with dx = xi - xj, every operation rounded on its own (no fused
// multiply-add); the list keeps the squares and the root is taken once (sqrt is monotone).  The structure only prunes, and every pruning
// comparison is conservative in fp32: q is a monotone function of x (a subtraction of a constant, a product with a positive constant, a
// truncation, a clamp), so the points whose q lies beyond a cell boundary b lie beyond the plane min + b * cell up to the roundings of
// x - min (2u ext for the two points), of scale and cell against each other and of the products (5u ext) and of the final subtraction
// (u ext), u = 2^-24: 8u ext in all.  Every face distance is reduced by slack = 16u ext = 2^-20 ext and then by the factor 1 - 2^-20
// (a pruned point's fp32 distance is within 3.5u of its real one); a comparison then accepts or skips only when it holds with that margin.
// A bounding box that is empty, below 1e-30 or above 1e38 in extent has no usable cells: every query scans the cloud (with the duplicate
// shortcut, which is what makes N identical points cheap).
//
// Determinism.  The K smallest distances of a row do not depend on the order the candidates are met in; the sort is stable and nothing
// else is order-dependent (the only atomics are integer min / max / or).
//
// Worst case.  A pass costs the points of its 27 cells that are not farther than the K-th candidate.  A cloud whose dense part is smaller
// than 2^-21 of its bounding box falls into one finest cell and every query of it scans that cell: towards N per query.  A far outlier
// starts at a coarse level; what it scans is what lies within its K-th distance of its cells' boxes, which for an outlier whose
// neighbours are farther away than the dense part is, is the dense part: many such outliers cost N each.  Both stay exact.
#include "scene_common.h"
#include "wm_api.h"

namespace {

typedef unsigned long long u64;

constexpr int KN_THREADS = 256;
constexpr int KN_BITS = 21;                         // per axis
constexpr unsigned int KN_QMAX = (1u << KN_BITS) - 1u;
constexpr int KN_NONE = 0x7fffffff;                 // the row of an empty list slot: behind every real row (N < 2^31)

// bb: [0..3) min, [3..6) max, as order-preserving unsigned images
struct KnFrame { float mn[3]; float scale, cell, slack; int degenerate; };

__device__ __forceinline__ KnFrame kn_frame(const unsigned int* __restrict__ bb) {
  KnFrame f;
  float ext = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f.mn[a] = ordered_value(bb[a]);
    ext = fmaxf(ext, __fsub_rn(ordered_value(bb[3 + a]), f.mn[a]));
  }
  f.degenerate = !(ext >= 1e-30f && ext <= 1e38f);
  f.scale = f.degenerate ? 0.f : __fdiv_rn(2097152.f, ext);
  f.cell = f.degenerate ? 0.f : __fmul_rn(ext, 1.f / 2097152.f);
  f.slack = f.degenerate ? 0.f : __fmul_rn(ext, 1.f / 1048576.f);
  return f;
}

// monotone in t; t >= 0
__device__ __forceinline__ unsigned int kn_quant(float t, float scale) {
  const float v = __fmul_rn(t, scale);
  return v >= 1.f ? (v < 2097151.f ? (unsigned int)v : KN_QMAX) : 0u;
}

// 21 bits -> every third bit of 63
__device__ __forceinline__ u64 kn_spread(unsigned int q) {
  u64 x = q & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__global__ void kn_init_kernel(unsigned int* __restrict__ bb, int* __restrict__ flag) {
  if (blockIdx.x == 0 && threadIdx.x < 6) bb[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 6) *flag = 0;
}

__global__ __launch_bounds__(KN_THREADS) void kn_bbox_kernel(const float* __restrict__ pts, long long N, unsigned int* __restrict__ bb,
                                                             int* __restrict__ flag) {
  unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  int bad = 0;
  for (long long i = (long long)blockIdx.x * KN_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * KN_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = pts[3 * i + a];
      bad |= !finite_f32(v);      // NaN or infinite
      const unsigned int k = ordered_key(v);
      lo[a] = k < lo[a] ? k : lo[a];
      hi[a] = k > hi[a] ? k : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned int l2 = (unsigned int)__shfl_xor((int)lo[a], o), h2 = (unsigned int)__shfl_xor((int)hi[a], o);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&bb[a], lo[a]); atomicMax(&bb[3 + a], hi[a]); }
  }
  if (bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(KN_THREADS) void kn_keys_kernel(const float* __restrict__ pts, long long N, const unsigned int* __restrict__ bb,
                                                             const int* __restrict__ flag, u64* __restrict__ keys, unsigned int* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * KN_THREADS + threadIdx.x;
  if (i >= N) return;
  rows[i] = (unsigned int)i;
  if (*flag) { keys[i] = 0; return; }      // a non-finite input: nothing below looks at the cloud, the sort still gets defined keys
  const KnFrame f = kn_frame(bb);
  u64 key = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) key |= kn_spread(kn_quant(__fsub_rn(pts[3 * i + a], f.mn[a]), f.scale)) << a;
  keys[i] = key;
}

__global__ __launch_bounds__(KN_THREADS) void kn_gather_kernel(const float* __restrict__ pts, long long N, const unsigned int* __restrict__ rows,
                                                               const int* __restrict__ flag, float4* __restrict__ sp) {
  const long long p = (long long)blockIdx.x * KN_THREADS + threadIdx.x;
  if (p >= N || *flag) return;
  const unsigned int r = rows[p];
  sp[p] = make_float4(pts[3 * (size_t)r], pts[3 * (size_t)r + 1], pts[3 * (size_t)r + 2], __int_as_float((int)r));
}

// every third bit of 63 -> 21 bits (the inverse of kn_spread)
__device__ __forceinline__ unsigned int kn_compact(u64 x) {
  x &= 0x1249249249249249ull;
  x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
  x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
  x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
  x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
  x = (x ^ (x >> 32)) & 0x1fffffull;
  return (unsigned int)x;
}

// first position in keys[lo .. hi) whose key is >= v (hi when there is none)
__device__ __forceinline__ unsigned int kn_lower_bound(const u64* __restrict__ keys, unsigned int lo, unsigned int hi, u64 v) {
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the conservative distance from the query (cells q, offsets t) to the nearest face of its 3 x 3 x 3 block of level L < 21 behind which
// a point can lie; +inf when the block covers the grid
__device__ __forceinline__ float kn_face_bound(int L, const unsigned int* q, const float* t, const KnFrame& f) {
  float b = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const unsigned int c = q[a] >> L;
    if (c >= 2u) b = fminf(b, __fsub_rn(__fsub_rn(t[a], __fmul_rn((float)((c - 1u) << L), f.cell)), f.slack));      // points with q < (c - 1) << L
    const unsigned int hq = (c + 2u) << L;
    if (hq <= KN_QMAX) b = fminf(b, __fsub_rn(__fsub_rn(__fmul_rn((float)hq, f.cell), t[a]), f.slack));             // points with q >= (c + 2) << L
  }
  return b > 0.f ? __fmul_rn(b, 0.99999905f) : b;
}

template <int KM>
struct KnList {
  float d[KM];
  int r[KM];
  // slots [0, KM - K) are held by entries nothing displaces, so the K-th smallest is always the last slot
  __device__ __forceinline__ void reset(int K) {
#pragma unroll
    for (int s = 0; s < KM; ++s) {
      const bool real = s >= KM - K;
      d[s] = real ? INFINITY : -1.f;
      r[s] = real ? KN_NONE : -1;
    }
  }
  __device__ __forceinline__ bool full() const { return r[KM - 1] != KN_NONE; }
  __device__ __forceinline__ bool takes(float d2, int row) const { return d2 < d[KM - 1] || (d2 == d[KM - 1] && row < r[KM - 1]); }
  __device__ __forceinline__ void insert(float d2, int row) {
#pragma unroll
    for (int s = 0; s < KM; ++s) {
      const bool sw = d2 < d[s] || (d2 == d[s] && row < r[s]);
      const float td = d[s];
      const int tr = r[s];
      d[s] = sw ? d2 : td;
      r[s] = sw ? row : tr;
      d2 = sw ? td : d2;
      row = sw ? tr : row;
    }
  }
};

// candidates sp[lo .. hi); true when the list is full with a K-th distance of 0 (the search is over)
template <int KM>
__device__ __forceinline__ bool kn_scan(const float4* __restrict__ sp, unsigned int lo, unsigned int hi, float xi, float yi, float zi, KnList<KM>& list) {
  for (unsigned int j = lo; j < hi; ++j) {
    const float4 s = sp[j];
    const float dx = __fsub_rn(xi, s.x), dy = __fsub_rn(yi, s.y), dz = __fsub_rn(zi, s.z);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    const int row = __float_as_int(s.w);
    if (list.takes(d2, row)) {
      list.insert(d2, row);
      if (list.d[KM - 1] == 0.f && list.full()) return true;
    }
  }
  return false;
}

constexpr unsigned int KN_LEAF = 48;      // a cell with no more points than this is scanned, a larger one is taken apart

// the conservative squared distance from the query (offsets t) to the box of the cells qlo <= q < qlo + 2^l
__device__ __forceinline__ float kn_cell_dmin2(const unsigned int* qlo, int l, const float* t, const KnFrame& f) {
  float d2 = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float below = __fsub_rn(__fsub_rn(__fmul_rn((float)qlo[a], f.cell), t[a]), f.slack);
    const float above = __fsub_rn(__fsub_rn(t[a], __fmul_rn((float)(qlo[a] + (1u << l)), f.cell)), f.slack);
    const float da = fmaxf(below, above);
    if (da > 0.f) d2 = __fadd_rn(d2, __fmul_rn(da, da));
  }
  return __fmul_rn(d2, 0.9999f);
}

// The points of ONE cell of level L (keys[lo .. hi), L <= 21; not for a degenerate frame) without a stack: the sorted keys are the depth-first
// order of the octree, so the state is a position j and a level l.  The cell of level l at j is stepped over when its box is farther than
// the K-th candidate, scanned when it is small, and otherwise looked at one level finer; behind a cell, l returns to the coarsest level
// at which position j starts a cell.  Every step lowers l or advances j.  true: the search is over (kn_scan).
template <int KM>
__device__ __forceinline__ bool kn_walk(const float4* __restrict__ sp, const u64* __restrict__ keys, unsigned int lo, unsigned int hi, int L,
                                        const float* x, const float* t, const KnFrame& f, KnList<KM>& list) {
  unsigned int j = lo, cap = hi;      // cap: the end of the enclosing cell already known
  int l = L;
  while (j < hi) {
    const u64 key = keys[j];
    const u64 k0 = (key >> (3 * l)) << (3 * l);
    const unsigned int end = (l == L) ? hi : kn_lower_bound(keys, j + 1u, cap, k0 + (1ull << (3 * l)));
    bool skip = false;
    if (list.full()) {
      const unsigned int qlo[3] = {kn_compact(k0), kn_compact(k0 >> 1), kn_compact(k0 >> 2)};
      skip = kn_cell_dmin2(qlo, l, t, f) > list.d[KM - 1];
    }
    if (!skip && end - j > KN_LEAF && l > 0) { --l; cap = end; continue; }
    if (!skip && kn_scan<KM>(sp, j, end, x[0], x[1], x[2], list)) return true;
    j = end;
    cap = hi;
    if (j < hi) {
      const int top = 63 - __clzll((long long)(keys[j] ^ keys[j - 1u]));      // the keys differ: j starts another cell of level l
      l = top / 3 < L ? top / 3 : L;
    }
  }
  return false;
}

template <int KM>
__global__ __launch_bounds__(KN_THREADS) void kn_query_kernel(const float4* __restrict__ sp, const u64* __restrict__ keys, unsigned int N, int K,
                                                              const unsigned int* __restrict__ bb, const int* __restrict__ flag,
                                                              float* __restrict__ dist, int* __restrict__ idx) {
  const long long pl = (long long)blockIdx.x * KN_THREADS + threadIdx.x;
  if (pl >= (long long)N || *flag) return;
  const unsigned int p = (unsigned int)pl;
  const KnFrame f = kn_frame(bb);
  const float4 me = sp[p];
  const float x[3] = {me.x, me.y, me.z};
  float t[3];
  unsigned int q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { t[a] = __fsub_rn(x[a], f.mn[a]); q[a] = kn_quant(t[a], f.scale); }

  // start level: the finer of the cells shared with the K-th sorted neighbour on either side
  int L = KN_BITS;
  if (!f.degenerate) {
    const u64 key = keys[p];
    int common = -1;
    if (p >= (unsigned int)K) {
      const u64 d = key ^ keys[p - (unsigned int)K];
      common = d ? __clzll((long long)d) - 1 : 63;
    }
    if ((u64)p + (u64)K < (u64)N) {
      const u64 d = key ^ keys[p + (unsigned int)K];
      const int c2 = d ? __clzll((long long)d) - 1 : 63;
      common = c2 > common ? c2 : common;
    }
    if (common >= 0) L = (63 - common + 2) / 3;
  }

  KnList<KM> list;
  for (;;) {      // at most 22 passes: L grows in every one
    list.reset(K);
    if (L >= KN_BITS) {
      if (f.degenerate) kn_scan<KM>(sp, 0u, N, x[0], x[1], x[2], list);
      else kn_walk<KM>(sp, keys, 0u, N, KN_BITS, x, t, f, list);
      break;
    }
    const unsigned int ncell = 1u << (KN_BITS - L);
    const unsigned int c[3] = {q[0] >> L, q[1] >> L, q[2] >> L};
    bool done = false;
    for (int o = 0; o < 27 && !done; ++o) {
      const int code = o + 13 < 27 ? o + 13 : o - 14;      // the query's own cell first
      const int dc[3] = {code % 3 - 1, (code / 3) % 3 - 1, code / 9 - 1};
      bool inside = true;
      unsigned int cc[3], qlo[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long v = (long long)c[a] + dc[a];
        inside = inside && v >= 0 && v < (long long)ncell;
        cc[a] = (unsigned int)v;
        qlo[a] = cc[a] << L;      // the cell's points have qlo <= q < qlo + 2^L
      }
      if (!inside) continue;
      if (list.full() && kn_cell_dmin2(qlo, L, t, f) > list.d[KM - 1]) continue;      // the whole cell is farther than the K-th candidate
      const u64 k0 = (kn_spread(cc[0]) | kn_spread(cc[1]) << 1 | kn_spread(cc[2]) << 2) << (3 * L);
      const unsigned int lo = kn_lower_bound(keys, 0u, N, k0);
      const unsigned int hi = kn_lower_bound(keys, lo, N, k0 + (1ull << (3 * L)));
      done = kn_walk<KM>(sp, keys, lo, hi, L, x, t, f, list);
    }
    if (done) break;
    if (!list.full()) { ++L; continue; }
    const float kth = __fsqrt_rn(list.d[KM - 1]);
    if (kth <= kn_face_bound(L, q, t, f)) break;
    do { ++L; } while (L < KN_BITS && !(kth <= kn_face_bound(L, q, t, f)));
  }

  const size_t out = (size_t)(unsigned int)__float_as_int(me.w) * (size_t)K;
#pragma unroll
  for (int s = 0; s < KM; ++s) {
    const int o = s - (KM - K);
    if (o >= 0) {
      dist[out + o] = __fsqrt_rn(list.d[s]);
      if (idx) idx[out + o] = list.r[s];
    }
  }
}

struct KnWs { unsigned int* bb; u64* keys[2]; unsigned int* rows[2]; float4* sp; void* cub; size_t cub_bytes, total; };

KnWs kn_carve(char* base, size_t N) {
  KnWs w{};
  Carver c(base);
  w.bb = c.take<unsigned int>(8);
  w.keys[0] = c.take<u64>(N); w.keys[1] = c.take<u64>(N);
  w.rows[0] = c.take<unsigned int>(N); w.rows[1] = c.take<unsigned int>(N);
  w.sp = c.take<float4>(N);
  w.cub_bytes = sort_pairs_bytes<u64, unsigned int>((int)N, 0, 63);
  w.cub = c.take<char>(w.cub_bytes ? w.cub_bytes : 4);
  w.total = c.total();
  return w;
}

bool kn_sizes_ok(long long N, int K) { return K >= 1 && K <= 16 && N >= (long long)K && N < (1LL << 31); }

}  // namespace

size_t wm_knn_ws_bytes(long long N, int K) {
  if (!kn_sizes_ok(N, K)) return 0;
  return kn_carve(nullptr, (size_t)N).total;
}

// bbox, keys, stable sort, gather: the index both searches walk.  keys_out: the buffer the sorted keys ended in.
static hipError_t kn_build(const float* points, long long N, const KnWs& w, int* nonfinite_flag, const u64** keys_out, hipStream_t s) {
  const unsigned nb = blocks_for(N, KN_THREADS);
  hipLaunchKernelGGL(kn_init_kernel, dim3(1), dim3(64), 0, s, w.bb, nonfinite_flag);
  hipLaunchKernelGGL(kn_bbox_kernel, dim3(nb < 2048u ? nb : 2048u), dim3(KN_THREADS), 0, s, points, N, w.bb, nonfinite_flag);
  hipLaunchKernelGGL(kn_keys_kernel, dim3(nb), dim3(KN_THREADS), 0, s, points, N, (const unsigned int*)w.bb, (const int*)nonfinite_flag, w.keys[0],
                     w.rows[0]);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipcub::DoubleBuffer<u64> dk(w.keys[0], w.keys[1]);
  hipcub::DoubleBuffer<unsigned int> dv(w.rows[0], w.rows[1]);
  e = sort_pairs(w.cub, w.cub_bytes, dk, dv, (int)N, 0, 63, s);      // stable: equal keys stay in row order
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kn_gather_kernel, dim3(nb), dim3(KN_THREADS), 0, s, points, N, (const unsigned int*)dv.Current(), (const int*)nonfinite_flag, w.sp);
  *keys_out = dk.Current();
  return hipGetLastError();
}

hipError_t wm_launch_knn(const float* points, long long N, int K, void* workspace, float* dist, int* idx, int* nonfinite_flag, hipStream_t s) {
  if (!kn_sizes_ok(N, K)) return hipErrorInvalidValue;
  const KnWs w = kn_carve((char*)workspace, (size_t)N);
  const unsigned nb = blocks_for(N, KN_THREADS);
  const u64* keys = nullptr;
  const hipError_t e = kn_build(points, N, w, nonfinite_flag, &keys, s);
  if (e != hipSuccess) return e;
  const float4* sp = w.sp;
  const unsigned int* bb = w.bb;
  const int* flag = nonfinite_flag;
  if (K <= 4)
    hipLaunchKernelGGL(kn_query_kernel<4>, dim3(nb), dim3(KN_THREADS), 0, s, sp, keys, (unsigned int)N, K, bb, flag, dist, idx);
  else if (K <= 8)
    hipLaunchKernelGGL(kn_query_kernel<8>, dim3(nb), dim3(KN_THREADS), 0, s, sp, keys, (unsigned int)N, K, bb, flag, dist, idx);
  else
    hipLaunchKernelGGL(kn_query_kernel<16>, dim3(nb), dim3(KN_THREADS), 0, s, sp, keys, (unsigned int)N, K, bb, flag, dist, idx);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the nearest point of ANOTHER cloud (wm_nearest_build / wm_nearest_query)
// The index is the one above (bbox, keys, stable sort, 16-byte records), built once over ref [N,3] and left in the caller's index memory;
// a query call keys the queries [M,3] in the reference's frame (clamped to the grid), sorts them so that the lanes of a wave walk the same
// cells, and runs one query per lane:
//   seed    the 8 sorted records around the position of the query's key (a finite best distance before the walk starts)
//   walk    nn_walk, the stackless octree walk of kn_walk from level 21 (the whole cloud) with a one-slot best in registers: a cell whose
//           box is farther than the best is stepped over, a cell of at most 48 points is scanned, a larger one is taken apart.
// There is no acceptance rule: the walk covers the whole cloud and only prunes, so it is exact wherever the query lies.
//
// Exactness.  dist = sqrt(min_j fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz))), dx = fl(q.x - r.x), every operation rounded on its own; idx is
// the lowest row that attains the minimum square (the best is ordered by (square, row), and no search ends early on a zero: a lower row
// with the same square may follow).  A cell is stepped over only when its conservative box distance exceeds the best square, strictly.
// The box distance per axis is fl(fl(qlo cell) - t) - slack_q with t = fl(q - min): beside the 8u ext of the structure (see the top of
// this file) t carries u |t| and the product u ext, which for a query far outside the box is NOT small against ext, so
// slack_q = 16u ext + 8u max|t| (u = 2^-24); the relative error of the last subtraction, of the squares and of their sum (< 4u) and of a
// pruned point's own fp32 square (< 3.5u) are covered by the factor 0.9999.  A bound below 1e-30 counts as 0 (nothing is pruned by it):
// squares that small are denormal in fp32 and carry no relative accuracy.  An overflowing distance is +inf on both sides of a comparison
// and prunes nothing.
// A frame without usable cells (all of ref in one point, extent below 1e-30 or above 1e38) scans the cloud for every query.
//
// Determinism.  The minimum over (square, row) does not depend on the order the candidates are met in; both sorts are stable; the only
// atomics are the integer min / max / or of the bounding box.
//
// Worst case.  A query costs the points of the cells its best-distance ball touches.  All of ref inside one finest cell (a dense part
// below 2^-21 of the extent): N per query.  A query much farther from the cloud than the cloud is wide sees every cell at nearly the same
// distance, and pruning by a 1e-4 margin fails once the cloud's extent is below 1e-4 of that distance: towards N per such query.  Both
// stay exact.
// One rounding per operation, for the rest of this file: the compiler's default for device code is to contract a product and a sum into a
// fused multiply-add wherever it can, and the __f*_rn functions of this toolchain are plain operators that take part in that.  The
// candidate squares below are therefore written with plain operators under this pragma (the pruning bounds, which are only conservative,
// may be rounded either way).
#pragma clang fp contract(off)
namespace {

__device__ __forceinline__ void nn_scan(const float4* __restrict__ sp, unsigned int lo, unsigned int hi, float xi, float yi, float zi, float& bd,
                                        int& br) {
  for (unsigned int j = lo; j < hi; ++j) {
    const float4 s = sp[j];
    const float dx = xi - s.x, dy = yi - s.y, dz = zi - s.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;      // three products and two sums, each rounded (contract off)
    const int row = __float_as_int(s.w);
    if (d2 < bd || (d2 == bd && row < br)) { bd = d2; br = row; }
  }
}

// kn_cell_dmin2 with the query's own slack
__device__ __forceinline__ float nn_cell_dmin2(const unsigned int* qlo, int l, const float* t, float cell, float slack) {
  float d2 = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float below = __fsub_rn(__fsub_rn(__fmul_rn((float)qlo[a], cell), t[a]), slack);
    const float above = __fsub_rn(__fsub_rn(t[a], __fmul_rn((float)(qlo[a] + (1u << l)), cell)), slack);
    const float da = fmaxf(below, above);
    if (da > 0.f) d2 = __fadd_rn(d2, __fmul_rn(da, da));
  }
  return d2 > 1e-30f ? __fmul_rn(d2, 0.9999f) : 0.f;
}

// kn_walk over the whole cloud keys[0 .. N) from level 21, one-slot best (bd, br), no early end
__device__ __forceinline__ void nn_walk(const float4* __restrict__ sp, const u64* __restrict__ keys, unsigned int N, const float* x, const float* t,
                                        float cell, float slack, float& bd, int& br) {
  unsigned int j = 0u, cap = N;
  int l = KN_BITS;
  while (j < N) {
    const u64 key = keys[j];
    const u64 k0 = (key >> (3 * l)) << (3 * l);
    const unsigned int end = (l == KN_BITS) ? N : kn_lower_bound(keys, j + 1u, cap, k0 + (1ull << (3 * l)));
    bool skip = false;
    if (br != KN_NONE) {
      const unsigned int qlo[3] = {kn_compact(k0), kn_compact(k0 >> 1), kn_compact(k0 >> 2)};
      skip = nn_cell_dmin2(qlo, l, t, cell, slack) > bd;
    }
    if (!skip && end - j > KN_LEAF && l > 0) { --l; cap = end; continue; }
    if (!skip) nn_scan(sp, j, end, x[0], x[1], x[2], bd, br);
    j = end;
    cap = N;
    if (j < N) {
      const int top = 63 - __clzll((long long)(keys[j] ^ keys[j - 1u]));      // the keys differ: j starts another cell of level l
      l = top / 3 < KN_BITS ? top / 3 : KN_BITS;
    }
  }
}

// bb[6]: the non-finite flag of the build, bb[7]: N
__global__ void nn_seal_kernel(unsigned int* __restrict__ bb, const int* __restrict__ flag, unsigned int N) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { bb[6] = (unsigned int)*flag; bb[7] = N; }
}

__global__ __launch_bounds__(KN_THREADS) void nn_query_kernel(const float4* __restrict__ sp, const u64* __restrict__ keys, unsigned int N,
                                                              const unsigned int* __restrict__ bb, const float* __restrict__ queries,
                                                              const unsigned int* __restrict__ qrows, unsigned int M, float* __restrict__ dist,
                                                              int* __restrict__ idx) {
  const long long pl = (long long)blockIdx.x * KN_THREADS + threadIdx.x;
  if (pl >= (long long)M || bb[6]) return;
  const size_t row = qrows[pl];
  const float x[3] = {queries[3 * row], queries[3 * row + 1], queries[3 * row + 2]};
  if (!(finite_f32(x[0]) && finite_f32(x[1]) && finite_f32(x[2]))) {
    dist[row] = __int_as_float(0x7fc00000);
    if (idx) idx[row] = -1;
    return;
  }
  const KnFrame f = kn_frame(bb);
  float bd = INFINITY;
  int br = KN_NONE;
  if (f.degenerate) {
    nn_scan(sp, 0u, N, x[0], x[1], x[2], bd, br);
  } else {
    float t[3], tmax = 0.f;
    u64 key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = __fsub_rn(x[a], f.mn[a]);
      tmax = fmaxf(tmax, fabsf(t[a]));
      key |= kn_spread(kn_quant(t[a], f.scale)) << a;      // a negative t gives cell 0, one beyond the box the last cell
    }
    const unsigned int p = kn_lower_bound(keys, 0u, N, key);
    const unsigned int lo = p >= 4u ? p - 4u : 0u, hi = lo + 8u < N ? lo + 8u : N;
    nn_scan(sp, lo, hi, x[0], x[1], x[2], bd, br);
    nn_walk(sp, keys, N, x, t, f.cell, __fadd_rn(f.slack, __fmul_rn(tmax, 1.f / 2097152.f)), bd, br);
  }
  dist[row] = (float)sqrt((double)bd);      // the correctly rounded fp32 root: an fp64 root rounded once more is exact for fp32 inputs
  if (idx) idx[row] = br;
}

struct NnQueryWs { u64* keys[2]; unsigned int* rows[2]; void* cub; size_t cub_bytes, total; };

NnQueryWs nn_carve(char* base, size_t M) {
  NnQueryWs w{};
  Carver c(base);
  const size_t m = M ? M : 1;
  w.keys[0] = c.take<u64>(m); w.keys[1] = c.take<u64>(m);
  w.rows[0] = c.take<unsigned int>(m); w.rows[1] = c.take<unsigned int>(m);
  w.cub_bytes = sort_pairs_bytes<u64, unsigned int>((int)m, 0, 63);
  w.cub = c.take<char>(w.cub_bytes ? w.cub_bytes : 4);
  w.total = c.total();
  return w;
}

}  // namespace

size_t wm_nearest_index_bytes(long long N) {
  if (N < 1 || N >= (1LL << 31)) return 0;
  return kn_carve(nullptr, (size_t)N).total;
}

size_t wm_nearest_query_ws_bytes(long long M) {
  if (M < 0 || M >= (1LL << 31)) return 0;
  return nn_carve(nullptr, (size_t)M).total;
}

hipError_t wm_launch_nearest_build(const float* ref, long long N, void* index, int* nonfinite_flag, hipStream_t s) {
  if (N < 1 || N >= (1LL << 31)) return hipErrorInvalidValue;
  const KnWs w = kn_carve((char*)index, (size_t)N);
  const u64* keys = nullptr;
  hipError_t e = kn_build(ref, N, w, nonfinite_flag, &keys, s);
  if (e != hipSuccess) return e;
  if (keys != w.keys[0]) {      // a query finds the sorted keys in the first buffer
    e = hipMemcpyAsync(w.keys[0], keys, (size_t)N * sizeof(u64), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(nn_seal_kernel, dim3(1), dim3(64), 0, s, w.bb, (const int*)nonfinite_flag, (unsigned int)N);
  return hipGetLastError();
}

hipError_t wm_launch_nearest_query(const void* index, long long N, const float* queries, long long M, void* workspace, float* dist, int* idx,
                                   hipStream_t s) {
  if (N < 1 || N >= (1LL << 31) || M < 0 || M >= (1LL << 31)) return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  const KnWs ix = kn_carve((char*)index, (size_t)N);
  const NnQueryWs w = nn_carve((char*)workspace, (size_t)M);
  const unsigned nb = blocks_for(M, KN_THREADS);
  const unsigned int* bb = ix.bb;
  hipLaunchKernelGGL(kn_keys_kernel, dim3(nb), dim3(KN_THREADS), 0, s, queries, M, bb, (const int*)(bb + 6), w.keys[0], w.rows[0]);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipcub::DoubleBuffer<u64> dk(w.keys[0], w.keys[1]);
  hipcub::DoubleBuffer<unsigned int> dv(w.rows[0], w.rows[1]);
  e = sort_pairs(w.cub, w.cub_bytes, dk, dv, (int)M, 0, 63, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nn_query_kernel, dim3(nb), dim3(KN_THREADS), 0, s, (const float4*)ix.sp, (const u64*)ix.keys[0], (unsigned int)N, bb, queries,
                     (const unsigned int*)dv.Current(), (unsigned int)M, dist, idx);
  return hipGetLastError();
}
