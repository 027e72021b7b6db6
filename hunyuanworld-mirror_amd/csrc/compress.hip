// PNG compression of trained splats: the device side of gsplat.compression.PngCompression (gsplat/compression/png_compression.py) as the
// trainer's Runner.run_compression calls it (simple_trainer_worldmirror.py:1293-1307).  The C-ABI entries are in wm_api_compress.cpp; the
// launchers are declared in wm_api.h.  Plain HIP C++, every global write an ordinary vector store.
//
//   minmax        per-channel min and max of x [rows, C] and a non-finite flag: a two-level block reduction, no atomics.  Level 1 gives every
//                 block a fixed run of rows, level 2 is one block over the partials.  NaN does not enter a min or a max (fminf / fmaxf), it
//                 sets the flag; the flag is only ever set, the caller zeroes it.
//   quantise      :169-172 / :241-246 in fp32: q = rint(((x - min) / (max - min)) * (2^b - 1)), IEEE division, the product rounded to fp32
//                 before rint (half to even, as numpy.round), one u8 plane (b <= 8) or the low and high byte planes (b = 16).  A channel with
//                 max == min encodes as 0 (the reference divides 0 by 0).
//   dequantise    :203-208 / :287-291 / :412-416, which run in fp64 (numpy's img / 255 is a double and torch promotes the rest):
//                 double(code) / (2^b - 1) * double(float(max - min)) + double(min), every operation rounded on its own, then once to fp32.
//   gather        out_f[r, :] = in_f[idx[r], :] for up to 16 fields in one launch (the crop, the grid order, centroids[labels]).
//   kmeans        Lloyd's algorithm under L1 distance, semantics in include/wm_hip.h (wm_kmeans_l1).
//     assign      the hot kernel.  One row per lane, the row's D values in registers (D a template parameter: 9, 24, 45).  Every lane of a
//                 wave needs the same centroid value at the same time, so the [K, D] table is read through wave-uniform addresses (scalar
//                 loads; the table is at most 11.8 MB and stays in the L2 / Infinity Cache) and a term costs one subtract with a scalar operand
//                 and one add with the |.| source modifier.  Each distance is one fp32 chain in the order d = 0 .. D-1, so the same row and
//                 centroid give the same bits wherever they are computed; a strict < keeps the lowest index among ties.  No [N, K] array.
//                 Packed fp32 adds are not used: the library keeps v_pk_*_f32 out of every kernel but the GELU GEMM
//                 (tests/test_kernel_resources_cpu.py), and |.| is no source modifier of a packed add anyway.
//     error       sum of the assigned distances in fp64: every block a fixed run of rows and a fixed tree, then one block over the partials.
//     update      stable hipCUB radix sort of (label, row), the segment starts by binary search, one lane per (centroid, d) summing its
//                 members in row order in fp64, divided by the count in fp64 and rounded once to fp32; an empty centroid is left alone.
//     stop        the stop rule is evaluated on the device by the error kernel, which records the iteration it fired in; every kernel of a
//                 later iteration returns at once.  (The radix sort of such an iteration still runs, on labels nobody reads.)
//   grid order    30-bit Morton codes of the means (per-axis bounding box, 10 bits per axis: floor((x - min) / (max - min) * 1024) held to
//                 0 .. 1023, an axis of zero extent divides by 1), stable sort; 2-D Morton codes (row, col) of the n x n cells, same sort;
//                 perm[cell of rank i] = row of rank i.
#include <climits>

#include "scene_common.h"
#include "wm_api.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned char u8;

constexpr int CP_THREADS = 256;
constexpr int CP_WAVES = CP_THREADS / 64;
constexpr int CP_MAX_BLOCKS = 1024;      // level-1 blocks of the two-level reductions

// ------------------------------------------------------------------ minmax
// partials: per block 2 C + 1 floats (C mins, C maxs, 1.0 when a value was NaN or infinite).  Every lane of the block calls cp_block_out.
__device__ __forceinline__ void cp_block_out(float lo, float hi, float* sLo, float* sHi, float* out_lo, float* out_hi) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sLo[tid >> 6] = lo; sHi[tid >> 6] = hi; }
  __syncthreads();
  if (tid == 0) {
    float a = sLo[0], b = sHi[0];
    for (int w = 1; w < CP_WAVES; ++w) { a = fminf(a, sLo[w]); b = fmaxf(b, sHi[w]); }
    *out_lo = a;
    *out_hi = b;
  }
  __syncthreads();
}

__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void cp_minmax_kernel(const float* __restrict__ x, long long rows, int C, long long rows_per_block,
                                                                                 float* __restrict__ partials) {
  __shared__ float sLo[CP_WAVES], sHi[CP_WAVES];
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  float* out = partials + (size_t)blockIdx.x * (size_t)(2 * C + 1);
  float bad = 0.f;
  for (int c = 0; c < C; ++c) {
    float lo = INFINITY, hi = -INFINITY;
    for (long long r = r0 + threadIdx.x; r < r1; r += CP_THREADS) {
      const float v = x[r * C + c];
      if (!finite_f32(v)) bad = 1.f;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    cp_block_out(lo, hi, sLo, sHi, out + c, out + C + c);
  }
  float unused;
  cp_block_out(0.f, bad, sLo, sHi, &unused, out + 2 * C);
}

__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void cp_minmax_final_kernel(const float* __restrict__ partials, int nblk, int C, float* __restrict__ mm,
                                                                                       int* __restrict__ flag) {
  __shared__ float sLo[CP_WAVES], sHi[CP_WAVES];
  __shared__ float sBad;
  const int stride = 2 * C + 1;
  for (int c = 0; c < C; ++c) {
    float lo = INFINITY, hi = -INFINITY;
    for (int b = threadIdx.x; b < nblk; b += CP_THREADS) {
      lo = fminf(lo, partials[(size_t)b * stride + c]);
      hi = fmaxf(hi, partials[(size_t)b * stride + C + c]);
    }
    cp_block_out(lo, hi, sLo, sHi, mm + c, mm + C + c);
  }
  float bad = 0.f, unused;
  for (int b = threadIdx.x; b < nblk; b += CP_THREADS) bad = fmaxf(bad, partials[(size_t)b * stride + 2 * C]);
  cp_block_out(0.f, bad, sLo, sHi, &unused, &sBad);
  if (threadIdx.x == 0 && sBad != 0.f) *flag = 1;
}

// ------------------------------------------------------------------ quantise / dequantise
__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void cp_quantise_kernel(const float* __restrict__ x, long long total, int C, const float* __restrict__ mm,
                                                                                   float maxcode, u8* __restrict__ lo, u8* __restrict__ hi) {
  const long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const float mn = mm[c], mx = mm[C + c];
  float q = 0.f;
  if (mx != mn) q = rintf(__fmul_rn(__fdiv_rn(__fsub_rn(x[e], mn), __fsub_rn(mx, mn)), maxcode));
  q = fminf(fmaxf(q, 0.f), maxcode);      // finite input is inside already; NaN -> 0
  const unsigned int code = (unsigned int)q;
  lo[e] = (u8)(code & 0xffu);
  if (hi) hi[e] = (u8)(code >> 8);
}

__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void cp_dequantise_kernel(const u8* __restrict__ lo, const u8* __restrict__ hi, long long total, int C,
                                                                                     const float* __restrict__ mm, double maxcode, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const unsigned int code = (unsigned int)lo[e] | (hi ? (unsigned int)hi[e] << 8 : 0u);
  const double range = (double)__fsub_rn(mm[C + c], mm[c]);
  out[e] = (float)__dadd_rn(__dmul_rn(__ddiv_rn((double)code, maxcode), range), (double)mm[c]);
}

// ------------------------------------------------------------------ row gather
constexpr int CP_MAX_FIELDS = 16;
struct CpFields {
  const char* src[CP_MAX_FIELDS];
  char* dst[CP_MAX_FIELDS];
  int units[CP_MAX_FIELDS];      // per row: dwords (wide) or bytes
  int wide[CP_MAX_FIELDS];
};

// blockIdx.y: the field; a grid-stride walk over its rows x units
__global__ __launch_bounds__(CP_THREADS) void cp_gather_kernel(CpFields f, const int* __restrict__ idx, long long rows) {
  const int fi = blockIdx.y;
  const int units = f.units[fi];
  const long long total = rows * units;
  for (long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CP_THREADS) {
    const long long r = e / units;
    const int u = (int)(e - r * units);
    const long long s = (long long)idx[r] * units + u;
    if (f.wide[fi]) ((unsigned int*)f.dst[fi])[e] = ((const unsigned int*)f.src[fi])[s];
    else f.dst[fi][e] = f.src[fi][s];
  }
}

// ------------------------------------------------------------------ k-means under L1
struct KmState { int stop_iter; int iters; int bad_init; int pad; double prev_err; };

__global__ __launch_bounds__(CP_THREADS) void km_init_kernel(const float* __restrict__ x, long long N, int D, const long long* __restrict__ init, int K,
                                                             float* __restrict__ cent, unsigned int* __restrict__ rows, KmState* __restrict__ st) {
  const long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e == 0) { st->stop_iter = INT_MAX; st->iters = 0; st->pad = 0; st->prev_err = 0.0; }
  if (e < N) rows[e] = (unsigned int)e;
  if (e < (long long)K * D) {
    const int k = (int)(e / D);
    const int d = (int)(e - (long long)k * D);
    long long r = init[k];
    if (r < 0 || r >= N) { st->bad_init = 1; r = 0; }      // every writer stores the same 1; zeroed by the launcher's memset
    cent[e] = x[r * D + d];
  }
}

template <int D>
__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void km_assign_kernel(const float* __restrict__ x, int N, const float* __restrict__ cent, int K, int t,
                                                                                 const KmState* __restrict__ st, int* __restrict__ labels,
                                                                                 float* __restrict__ dist) {
  if (st && t > st->stop_iter) return;      // st null: the assignment on its own
  const int i = blockIdx.x * CP_THREADS + threadIdx.x;
  const size_t r = (size_t)(i < N ? i : N - 1);      // the lanes behind the last row repeat it and store nothing
  float v[D];
#pragma unroll
  for (int d = 0; d < D; ++d) v[d] = x[r * D + d];
  float best = INFINITY;
  int bi = 0;
#pragma unroll 2
  for (int k = 0; k < K; ++k) {
    const float* __restrict__ c = cent + (size_t)k * D;      // wave-uniform: scalar loads
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) acc = __fadd_rn(acc, fabsf(__fsub_rn(v[d], c[d])));
    if (acc < best) { best = acc; bi = k; }
  }
  if (i < N) { labels[i] = bi; dist[i] = best; }
}

// every lane of the block calls it; the sum of the block's 256 values by a fixed tree, valid in lane 0
__device__ __forceinline__ double km_block_sum(double v, double* sD) {
  sD[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = CP_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sD[threadIdx.x] = __dadd_rn(sD[threadIdx.x], sD[threadIdx.x + s]);
    __syncthreads();
  }
  return sD[0];
}

__global__ __launch_bounds__(CP_THREADS) void km_err1_kernel(const float* __restrict__ dist, long long N, long long per_block, int t, const KmState* __restrict__ st,
                                                             double* __restrict__ part) {
  __shared__ double sD[CP_THREADS];
  if (t > st->stop_iter) return;
  const long long r0 = (long long)blockIdx.x * per_block;
  const long long r1 = r0 + per_block < N ? r0 + per_block : N;
  double a = 0.0;
  for (long long r = r0 + threadIdx.x; r < r1; r += CP_THREADS) a = __dadd_rn(a, (double)dist[r]);
  const double s = km_block_sum(a, sD);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(CP_THREADS) void km_err2_kernel(const double* __restrict__ part, int nblk, long long N, int t, double tol, KmState* __restrict__ st,
                                                             double* __restrict__ errors) {
  __shared__ double sD[CP_THREADS];
  if (t > st->stop_iter) return;      // read by every lane before the barriers of km_block_sum, written by lane 0 behind them
  double a = 0.0;
  for (int b = threadIdx.x; b < nblk; b += CP_THREADS) a = __dadd_rn(a, part[b]);
  const double s = km_block_sum(a, sD);
  if (threadIdx.x == 0) {
    const double e = __ddiv_rn(s, (double)N);
    errors[t] = e;
    st->iters = t + 1;
    if (t > 0 && fabs(__dsub_rn(st->prev_err, e)) <= __dmul_rn(tol, st->prev_err)) st->stop_iter = t;      // this iteration's update still runs
    st->prev_err = e;
  }
}

// off[k] = the first position of the sorted labels that holds a label >= k, for k = 0 .. K (off[K] = N)
__global__ __launch_bounds__(CP_THREADS) void km_offsets_kernel(const unsigned int* __restrict__ keys, int N, int K, int t, const KmState* __restrict__ st,
                                                                int* __restrict__ off) {
  if (t > st->stop_iter) return;
  const int k = blockIdx.x * CP_THREADS + threadIdx.x;
  if (k > K) return;
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < (unsigned int)k) lo = mid + 1; else hi = mid;
  }
  off[k] = lo;
}

__global__ __launch_bounds__(CP_THREADS) void km_update_kernel(const float* __restrict__ x, int D, int K, const unsigned int* __restrict__ rows,
                                                               const int* __restrict__ off, int t, const KmState* __restrict__ st, float* __restrict__ cent) {
  if (t > st->stop_iter) return;
  const long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e >= (long long)K * D) return;
  const int k = (int)(e / D);
  const int d = (int)(e - (long long)k * D);
  const int s0 = off[k], s1 = off[k + 1];
  if (s1 <= s0) return;      // no members: the centroid keeps its value
  double sum = 0.0;
  for (int j = s0; j < s1; ++j) sum = __dadd_rn(sum, (double)x[(size_t)rows[j] * D + d]);      // the sort is stable: row order
  cent[e] = (float)__ddiv_rn(sum, (double)(s1 - s0));
}

struct KmWs { KmState* st; float* dist; int* labels; unsigned int* keys_sorted; unsigned int* rows; unsigned int* rows_sorted; int* off; double* part;
              void* cub; size_t cub_bytes, total; };

KmWs km_carve(char* base, size_t N, size_t K) {
  KmWs w{};
  Carver c(base);
  w.st = c.take<KmState>(1);
  w.dist = c.take<float>(N);
  w.labels = c.take<int>(N);
  w.keys_sorted = c.take<unsigned int>(N);
  w.rows = c.take<unsigned int>(N);
  w.rows_sorted = c.take<unsigned int>(N);
  w.off = c.take<int>(K + 1);
  w.part = c.take<double>(CP_MAX_BLOCKS);
  w.cub_bytes = sort_pairs_copy_bytes<unsigned int, unsigned int>((int)N, 0, 16);
  w.cub = c.take<char>(w.cub_bytes ? w.cub_bytes : 4);
  w.total = c.total();
  return w;
}

bool km_sizes_ok(long long N, int D, int K) { return (D == 9 || D == 24 || D == 45) && K >= 1 && K <= 65536 && N >= (long long)K && N <= (1LL << 30); }

template <int D>
void km_assign(const float* x, int N, const float* cent, int K, int t, const KmState* st, int* labels, float* dist, hipStream_t s) {
  hipLaunchKernelGGL(km_assign_kernel<D>, dim3(blocks_for(N, CP_THREADS)), dim3(CP_THREADS), 0, s, x, N, cent, K, t, st, labels, dist);
}
void km_assign_any(int D, const float* x, int N, const float* cent, int K, int t, const KmState* st, int* labels, float* dist, hipStream_t s) {
  if (D == 9) km_assign<9>(x, N, cent, K, t, st, labels, dist, s);
  else if (D == 24) km_assign<24>(x, N, cent, K, t, st, labels, dist, s);
  else km_assign<45>(x, N, cent, K, t, st, labels, dist, s);
}

// ------------------------------------------------------------------ grid order
__global__ __launch_bounds__(CP_THREADS) WM_NO_PACKED_FP32 void cp_morton3_kernel(const float* __restrict__ means, long long N, const float* __restrict__ mm,
                                                                                  unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (i >= N) return;
  unsigned int q[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float lo = mm[j];
    float len = __fsub_rn(mm[3 + j], lo);
    if (!(len > 0.f)) len = 1.f;
    const float s = floorf(__fmul_rn(__fdiv_rn(__fsub_rn(means[3 * i + j], lo), len), 1024.f));
    q[j] = (unsigned int)fminf(fmaxf(s, 0.f), 1023.f);      // the maximum itself gives 1024; NaN -> 0
  }
  keys[i] = (part1by2_10(q[2]) << 2) | (part1by2_10(q[1]) << 1) | part1by2_10(q[0]);
  vals[i] = (unsigned int)i;
}

__global__ __launch_bounds__(CP_THREADS) void cp_morton2_kernel(int n, long long N, unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
  const long long c = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (c >= N) return;
  const unsigned int row = (unsigned int)(c / n), col = (unsigned int)(c - (long long)row * n);
  keys[c] = (part1by1_16(row) << 1) | part1by1_16(col);
  vals[c] = (unsigned int)c;
}

// cells: a permutation of 0 .. N-1, so every perm entry is written once
__global__ __launch_bounds__(CP_THREADS) void cp_place_kernel(const unsigned int* __restrict__ order, const unsigned int* __restrict__ cells, long long N,
                                                              int* __restrict__ perm) {
  const long long i = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (i >= N) return;
  const unsigned int c = cells[i];
  if ((long long)c < N) perm[c] = (int)order[i];
}

size_t cp_minmax_partial_bytes(int C) { return (size_t)CP_MAX_BLOCKS * (size_t)(2 * C + 1) * 4; }

struct GoWs { float* mm; float* partials; unsigned int* keys[2]; unsigned int* vals[2]; unsigned int* ckeys[2]; unsigned int* cvals[2]; void* cub;
              size_t cub_bytes, total; };

GoWs go_carve(char* base, size_t N) {
  GoWs w{};
  Carver c(base);
  w.mm = c.take<float>(6);
  w.partials = (float*)c.take<char>(cp_minmax_partial_bytes(3));
  for (int b = 0; b < 2; ++b) { w.keys[b] = c.take<unsigned int>(N); w.vals[b] = c.take<unsigned int>(N); }
  for (int b = 0; b < 2; ++b) { w.ckeys[b] = c.take<unsigned int>(N); w.cvals[b] = c.take<unsigned int>(N); }
  const size_t tb32 = sort_pairs_bytes<unsigned int, unsigned int>((int)N, 0, 32), tb30 = sort_pairs_bytes<unsigned int, unsigned int>((int)N, 0, 30);
  w.cub_bytes = tb32 > tb30 ? tb32 : tb30;
  w.cub = c.take<char>(w.cub_bytes ? w.cub_bytes : 4);
  w.total = c.total();
  return w;
}

hipError_t cp_minmax(const float* x, long long rows, int C, float* partials, float* mm, int* flag, hipStream_t s) {
  long long nb = (rows + CP_THREADS - 1) / CP_THREADS;
  if (nb > CP_MAX_BLOCKS) nb = CP_MAX_BLOCKS;
  const long long per = (rows + nb - 1) / nb;
  nb = (rows + per - 1) / per;      // no empty block
  hipLaunchKernelGGL(cp_minmax_kernel, dim3((unsigned)nb), dim3(CP_THREADS), 0, s, x, rows, C, per, partials);
  hipLaunchKernelGGL(cp_minmax_final_kernel, dim3(1), dim3(CP_THREADS), 0, s, (const float*)partials, (int)nb, C, mm, flag);
  return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t wm_compress_minmax_ws_bytes(long long rows, int C) {
  if (rows < 1 || C < 1 || C > 16 || rows > (1LL << 40) / C) return 0;
  return cp_minmax_partial_bytes(C);
}
hipError_t wm_launch_compress_minmax(const float* x, long long rows, int C, void* workspace, float* mm, int* nonfinite_flag, hipStream_t s) {
  if (wm_compress_minmax_ws_bytes(rows, C) == 0) return hipErrorInvalidValue;
  return cp_minmax(x, rows, C, (float*)workspace, mm, nonfinite_flag, s);
}

hipError_t wm_launch_compress_quantise(const float* x, long long rows, int C, const float* mm, int bits, unsigned char* lo, unsigned char* hi, hipStream_t s) {
  if (rows < 1 || C < 1 || C > 16 || rows > (1LL << 40) / C || bits < 1 || bits > 16 || (bits > 8) != (hi != nullptr)) return hipErrorInvalidValue;
  const long long total = rows * C;
  hipLaunchKernelGGL(cp_quantise_kernel, dim3(blocks_for(total, CP_THREADS)), dim3(CP_THREADS), 0, s, x, total, C, mm, (float)((1 << bits) - 1), lo, hi);
  return hipGetLastError();
}
hipError_t wm_launch_compress_dequantise(const unsigned char* lo, const unsigned char* hi, long long rows, int C, const float* mm, int bits, float* out,
                                         hipStream_t s) {
  if (rows < 1 || C < 1 || C > 16 || rows > (1LL << 40) / C || bits < 1 || bits > 16 || (bits > 8) != (hi != nullptr)) return hipErrorInvalidValue;
  const long long total = rows * C;
  hipLaunchKernelGGL(cp_dequantise_kernel, dim3(blocks_for(total, CP_THREADS)), dim3(CP_THREADS), 0, s, lo, hi, total, C, mm, (double)((1 << bits) - 1), out);
  return hipGetLastError();
}

hipError_t wm_launch_gather_rows(const void* const* src, void* const* dst, const int* row_bytes, int n_fields, const int* idx, long long rows, hipStream_t s) {
  if (n_fields < 1 || n_fields > CP_MAX_FIELDS || rows < 1 || rows >= (1LL << 31)) return hipErrorInvalidValue;
  CpFields f{};
  long long most = 0;
  for (int i = 0; i < n_fields; ++i) {
    if (!src[i] || !dst[i] || row_bytes[i] < 1) return hipErrorInvalidValue;
    const bool wide = row_bytes[i] % 4 == 0 && ((size_t)src[i] & 3) == 0 && ((size_t)dst[i] & 3) == 0;
    f.src[i] = (const char*)src[i];
    f.dst[i] = (char*)dst[i];
    f.wide[i] = wide ? 1 : 0;
    f.units[i] = wide ? row_bytes[i] / 4 : row_bytes[i];
    if (rows * f.units[i] > most) most = rows * f.units[i];
  }
  long long nb = (most + CP_THREADS - 1) / CP_THREADS;
  if (nb > 65536) nb = 65536;
  hipLaunchKernelGGL(cp_gather_kernel, dim3((unsigned)nb, (unsigned)n_fields), dim3(CP_THREADS), 0, s, f, idx, rows);
  return hipGetLastError();
}

size_t wm_kmeans_l1_ws_bytes(long long N, int D, int K) {
  if (!km_sizes_ok(N, D, K)) return 0;
  return km_carve(nullptr, (size_t)N, (size_t)K).total;
}

hipError_t wm_launch_kmeans_l1(const float* x, long long N, int D, int K, const long long* init, int max_iter, double tol, void* workspace, int* labels,
                               int* labels_last, float* centroids, double* errors, int* info, hipStream_t s) {
  if (!km_sizes_ok(N, D, K) || max_iter < 1 || max_iter > 65536 || !(tol >= 0.0)) return hipErrorInvalidValue;
  const KmWs w = km_carve((char*)workspace, (size_t)N, (size_t)K);
  int* last = labels_last ? labels_last : w.labels;
  const int n = (int)N;
  hipError_t e = hipMemsetAsync(w.st, 0, sizeof(KmState), s);
  if (e != hipSuccess) return e;
  const long long most = N > (long long)K * D ? N : (long long)K * D;
  hipLaunchKernelGGL(km_init_kernel, dim3(blocks_for(most, CP_THREADS)), dim3(CP_THREADS), 0, s, x, N, D, init, K, centroids, w.rows, w.st);
  long long nb = (N + CP_THREADS - 1) / CP_THREADS;
  if (nb > CP_MAX_BLOCKS) nb = CP_MAX_BLOCKS;
  const long long per = (N + nb - 1) / nb;
  nb = (N + per - 1) / per;
  for (int t = 0; t < max_iter; ++t) {
    km_assign_any(D, x, n, centroids, K, t, w.st, last, w.dist, s);
    hipLaunchKernelGGL(km_err1_kernel, dim3((unsigned)nb), dim3(CP_THREADS), 0, s, (const float*)w.dist, N, per, t, (const KmState*)w.st, w.part);
    hipLaunchKernelGGL(km_err2_kernel, dim3(1), dim3(CP_THREADS), 0, s, (const double*)w.part, (int)nb, N, t, tol, w.st, errors);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = sort_pairs(w.cub, w.cub_bytes, (const unsigned int*)last, w.keys_sorted, (const unsigned int*)w.rows, w.rows_sorted, n, 0, 16, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(km_offsets_kernel, dim3(blocks_for(K + 1, CP_THREADS)), dim3(CP_THREADS), 0, s, (const unsigned int*)w.keys_sorted, n, K, t, (const KmState*)w.st, w.off);
    hipLaunchKernelGGL(km_update_kernel, dim3(blocks_for((long long)K * D, CP_THREADS)), dim3(CP_THREADS), 0, s, x, D, K, (const unsigned int*)w.rows_sorted,
                       (const int*)w.off, t, (const KmState*)w.st, centroids);
  }
  km_assign_any(D, x, n, centroids, K, -1, w.st, labels, w.dist, s);      // the returned labels belong to the returned centroids
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(info, &w.st->iters, 2 * sizeof(int), hipMemcpyDeviceToDevice, s);      // iterations run, bad_init
}

hipError_t wm_launch_kmeans_l1_assign(const float* x, long long N, int D, const float* centroids, int K, int* labels, float* dist, hipStream_t s) {
  if (!km_sizes_ok(N > K ? N : K, D, K) || N < 1) return hipErrorInvalidValue;
  km_assign_any(D, x, (int)N, centroids, K, -1, nullptr, labels, dist, s);
  return hipGetLastError();
}

size_t wm_grid_order_ws_bytes(int n_side) {
  if (n_side < 1 || n_side > 46340) return 0;
  return go_carve(nullptr, (size_t)n_side * (size_t)n_side).total;
}

hipError_t wm_launch_grid_order(const float* means, int n_side, void* workspace, int* perm, int* nonfinite_flag, hipStream_t s) {
  if (wm_grid_order_ws_bytes(n_side) == 0) return hipErrorInvalidValue;
  const long long N = (long long)n_side * n_side;
  const GoWs w = go_carve((char*)workspace, (size_t)N);
  hipError_t e = cp_minmax(means, N, 3, w.partials, w.mm, nonfinite_flag, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cp_morton3_kernel, dim3(blocks_for(N, CP_THREADS)), dim3(CP_THREADS), 0, s, means, N, (const float*)w.mm, w.keys[0], w.vals[0]);
  hipLaunchKernelGGL(cp_morton2_kernel, dim3(blocks_for(N, CP_THREADS)), dim3(CP_THREADS), 0, s, n_side, N, w.ckeys[0], w.cvals[0]);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipcub::DoubleBuffer<unsigned int> dk(w.keys[0], w.keys[1]), dv(w.vals[0], w.vals[1]);
  e = sort_pairs(w.cub, w.cub_bytes, dk, dv, (int)N, 0, 30, s);      // stable: equal codes stay in row order
  if (e != hipSuccess) return e;
  hipcub::DoubleBuffer<unsigned int> ck(w.ckeys[0], w.ckeys[1]), cv(w.cvals[0], w.cvals[1]);
  e = sort_pairs(w.cub, w.cub_bytes, ck, cv, (int)N, 0, 32, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cp_place_kernel, dim3(blocks_for(N, CP_THREADS)), dim3(CP_THREADS), 0, s, (const unsigned int*)dv.Current(), (const unsigned int*)cv.Current(), N, perm);
  return hipGetLastError();
}
