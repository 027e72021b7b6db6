// Splat export: the file BODIES of gsplat's export_splats (gsplat/exporter.py:194-553: "ply", "splat", "ply_compressed") and of the
// feed-forward hand-off file save_gs_ply (src/utils/save_utils.py:133-188), produced on the device in the byte order of the file.  The
// host writes the text header and copies the finished body once.  The C ABI entries are at the end of this file.
//
// stages
//   keep      one lane per input row: the row is kept when every one of its numbers is finite (14 + 3K of them) and, for
//             ply_compressed, 1 / (1 + exp(-opacity)) > opacity_threshold.  The flags go through an exclusive scan (hipcub) and
//             a scatter: kept rows stay in input order.  The number kept is the one value the host waits for.
//   morton    (splat, ply_compressed) min / max of the kept means per axis by a two-level block reduction (no atomics),
//             q = int(floor((c - min) / len * 1024)) with len == 0 -> 1, the low 10 bits per axis (1024 wraps to 0, as the reference's
//             mask does), bits interleaved z<<2 | y<<1 | x, then a STABLE 30-bit radix sort of (code, row): equal codes stay in row order.
//   ply       one lane per output float, rows [x y z | f_dc | f_rest (channel-major: column c K + k reads shN[i, k, c]) | opacity |
//             scale | rot], the parameters as given.  The kernel is a generic row packer: a list of columns (base pointer, row stride,
//             transform none / log; a null base is a column of zeros) gathered through the kept-row list.  save_gs_ply is the same
//             kernel with another column list and a keep mask handed in by the caller.
//   splat     one lane per splat of the Morton order, a 32-byte record by two 16-byte stores: mean, exp(scale),
//             u8 trunc(clamp(255 [0.5 + C0 sh0, sigmoid(opacity)], 0, 255)), u8 trunc(clamp(q / |q| 128 + 128, 0, 255)).
//   ply_compressed   one 256-lane block per chunk of 256 consecutive splats of the Morton order, one lane per splat.  A block min / max
//             gives the 18 chunk floats (means; log-scales, clamped to +-20 AFTER the reduction; 0.5 + C0 sh0); every lane packs
//             position 11-10-11, rotation (index of the largest component, 3 x 10 bits), scale 11-10-11 and colour + opacity 8-8-8-8 and
//             writes the four words with one 16-byte store.  pack_unorm(v, b) = clamp(floor(v (2^b - 1) + 0.5), 0, 2^b - 1).  A second
//             kernel writes the 3K sh bytes per splat, trunc(clamp((x / 8 + 0.5) 256, 0, 255)), one lane per byte.
//             Body: [18 floats per chunk | 4 words per splat | 3K bytes per splat].
//
// arithmetic.  The bytes are the contract, so every value is formed in fp32 in the reference's operation order, each operation rounded
// on its own: `#pragma clang fp contract(off)` below covers the whole file (hipcc contracts a * b + c into one fma by default).
// Divisions are `/` and the norm is sqrtf, both correctly rounded in hipcc's default mode (-fhip-fp32-correctly-rounded-divide-sqrt); exp
// and log are the library's expf / logf, not the fast intrinsics.  C0 and sqrt(2) / 2 are doubles rounded to fp32 once, as torch rounds
// a Python scalar that meets an fp32 tensor.  Sigmoid is 1 / (1 + exp(-x)).  No floating-point atomics anywhere.
//
// where the reference leaves the answer undefined, it is defined here:
//   * a chunk quantity with max == min (0 / 0 = NaN and an undefined integer cast in the reference): the packed field is 0; likewise a
//     NaN that reaches a pack (a quaternion of norm 0) packs as 0
//   * no row kept (torch.min of an empty tensor raises in the reference): n_kept = 0, nothing is written, the file has zero elements
//   * a min / max over values that hold both -0.0 and +0.0 (the reference's result depends on the order of the elements): the sign of a zero
//     chunk bound is whatever fminf / fmaxf give and is not pinned; nothing else of the file depends on it ((v - min) is 0 either way)
//   * a non-finite opacity (the reference's `.any(dim=0)` on the 1-D opacities is one scalar for all rows, so a single NaN empties the
//     file): here that row alone is dropped
#include "scene_common.h"
#include "wm_api.h"

#pragma clang fp contract(off)

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_CHUNK = 256;          // splats per chunk of ply_compressed; one lane each
constexpr int EX_MAX_COLS = 64;        // 14 + 3 * 15 = 59 columns for the ply of degree-3 splats
constexpr float EX_C0 = (float)0.28209479177387814;
constexpr float EX_HALF_SQRT2 = (float)(1.4142135623730951 * 0.5);

struct ExIn {
  const float* means; const float* scales; const float* quats; const float* opac; const float* sh0; const float* shN;
  int N, K;
};

struct ExCol { const float* base; int stride; int xf; };      // base null: zeros; xf 0 none, 1 log
struct ExCols { ExCol c[EX_MAX_COLS]; int n; };

__device__ __forceinline__ float ex_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- keep flags
__global__ __launch_bounds__(EX_THREADS) WM_NO_PACKED_FP32 void export_flags_kernel(ExIn a, int use_threshold, float threshold, int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= a.N) return;
  bool ok = finite_f32(a.opac[i]);
#pragma unroll
  for (int j = 0; j < 3; ++j) ok = ok && finite_f32(a.means[3 * i + j]) && finite_f32(a.scales[3 * i + j]) && finite_f32(a.sh0[3 * i + j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) ok = ok && finite_f32(a.quats[4 * i + j]);
  const int nr = 3 * a.K;
  for (int j = 0; j < nr; ++j) ok = ok && finite_f32(a.shN[(long long)nr * i + j]);
  if (ok && use_threshold) ok = ex_sigmoid(a.opac[i]) > threshold;
  flags[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(EX_THREADS) void export_mask_flags_kernel(const unsigned char* __restrict__ mask, int N, int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i < N) flags[i] = (!mask || mask[i]) ? 1 : 0;
}

// kept rows in input order; the last lane leaves the count
__global__ __launch_bounds__(EX_THREADS) void export_scatter_kernel(const int* __restrict__ flags, const int* __restrict__ offs, int N,
                                                                    int* __restrict__ kept, int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= N) return;
  if (flags[i]) kept[offs[i]] = (int)i;
  if (i == N - 1) *count = offs[i] + flags[i];
}

// ---- min / max of the kept means
// block min / max of NQ quantities; every lane of the block calls it; the results are in sOut[0 .. NQ) (min) and sOut[NQ .. 2 NQ) (max)
template <int NQ>
__device__ __forceinline__ void ex_block_minmax(const float (&lo)[NQ], const float (&hi)[NQ], float* sRed /* 2 NQ waves */, float* sOut /* 2 NQ */) {
  constexpr int WAVES = EX_THREADS / 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float a = wave_min(lo[q]), b = wave_max(hi[q]);
    if ((tid & 63) == 0) { sRed[q * WAVES + (tid >> 6)] = a; sRed[(NQ + q) * WAVES + (tid >> 6)] = b; }
  }
  __syncthreads();
  if (tid < 2 * NQ) {
    float v = sRed[tid * WAVES];
    for (int w = 1; w < WAVES; ++w) v = tid < NQ ? fminf(v, sRed[tid * WAVES + w]) : fmaxf(v, sRed[tid * WAVES + w]);
    sOut[tid] = v;
  }
  __syncthreads();
}

// level 1: rows of `kept` (means gathered through it); level 2 (kept == null, stride 6): the partials themselves, one block
__global__ __launch_bounds__(EX_THREADS) void export_minmax_kernel(const float* __restrict__ means, const int* __restrict__ kept, int n,
                                                                   float* __restrict__ partials) {
  __shared__ float sRed[6 * (EX_THREADS / 64)], sOut[6];
  const long long r = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  float lo[3], hi[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { lo[j] = INFINITY; hi[j] = -INFINITY; }
  if (r < n) {
    const long long i = kept[r];
#pragma unroll
    for (int j = 0; j < 3; ++j) lo[j] = hi[j] = means[3 * i + j];
  }
  ex_block_minmax<3>(lo, hi, sRed, sOut);
  if (threadIdx.x < 6) partials[6 * (size_t)blockIdx.x + threadIdx.x] = sOut[threadIdx.x];
}
__global__ __launch_bounds__(EX_THREADS) void export_minmax_final_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ mm) {
  __shared__ float sRed[6 * (EX_THREADS / 64)], sOut[6];
  float lo[3], hi[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { lo[j] = INFINITY; hi[j] = -INFINITY; }
  for (int b = threadIdx.x; b < nblk; b += EX_THREADS) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { lo[j] = fminf(lo[j], partials[6 * (size_t)b + j]); hi[j] = fmaxf(hi[j], partials[6 * (size_t)b + 3 + j]); }
  }
  ex_block_minmax<3>(lo, hi, sRed, sOut);
  if (threadIdx.x < 6) mm[threadIdx.x] = sOut[threadIdx.x];
}

__global__ __launch_bounds__(EX_THREADS) WM_NO_PACKED_FP32 void export_morton_kernel(const float* __restrict__ means, const int* __restrict__ kept, int n,
                                                                                     const float* __restrict__ mm, unsigned int* __restrict__ keys,
                                                                                     unsigned int* __restrict__ vals) {
  const long long r = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (r >= n) return;
  const long long i = kept[r];
  unsigned int q[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float lo = mm[j];
    float len = mm[3 + j] - lo;
    if (len == 0.f) len = 1.f;
    const float s = floorf((means[3 * i + j] - lo) / len * 1024.f);      // 0 .. 1024 for finite kept means
    q[j] = (unsigned int)(int)s;
  }
  keys[r] = (part1by2_10(q[2]) << 2) + (part1by2_10(q[1]) << 1) + part1by2_10(q[0]);
  vals[r] = (unsigned int)i;
}

// ---- generic row packer: out[r, c] = xf_c(col_c[kept[r]])
__global__ __launch_bounds__(EX_THREADS) WM_NO_PACKED_FP32 void export_pack_rows_kernel(ExCols cols, const int* __restrict__ kept, long long total,
                                                                                        float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long r = e / cols.n;
  const int c = (int)(e - r * cols.n);
  const ExCol col = cols.c[c];
  float v = 0.f;
  if (col.base) {
    v = col.base[(long long)kept[r] * col.stride];
    if (col.xf == 1) v = logf(v);
  }
  out[e] = v;
}

// ---- .splat
__device__ __forceinline__ unsigned int ex_u8(float v) { return (unsigned int)(int)fminf(fmaxf(v, 0.f), 255.f); }      // NaN -> 0; the cast truncates

__global__ __launch_bounds__(EX_THREADS) WM_NO_PACKED_FP32 void export_splat_kernel(ExIn a, const unsigned int* __restrict__ order, int n,
                                                                                    uint4* __restrict__ out) {
  const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (p >= n) return;
  const long long i = order[p];
  uint4 w0, w1;
  w0.x = __float_as_uint(a.means[3 * i]); w0.y = __float_as_uint(a.means[3 * i + 1]); w0.z = __float_as_uint(a.means[3 * i + 2]);
  w0.w = __float_as_uint(expf(a.scales[3 * i]));
  w1.x = __float_as_uint(expf(a.scales[3 * i + 1]));
  w1.y = __float_as_uint(expf(a.scales[3 * i + 2]));
  unsigned int col = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) col |= ex_u8((a.sh0[3 * i + j] * EX_C0 + 0.5f) * 255.f) << (8 * j);
  col |= ex_u8(ex_sigmoid(a.opac[i]) * 255.f) << 24;
  w1.z = col;
  float q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = a.quats[4 * i + j];
  const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  unsigned int rot = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) rot |= ex_u8(q[j] / nrm * 128.f + 128.f) << (8 * j);
  w1.w = rot;
  out[2 * p] = w0;
  out[2 * p + 1] = w1;
}

// ---- ply_compressed
__device__ __forceinline__ unsigned int ex_pack_unorm(float v, int bits) {
  const float t = (float)((1 << bits) - 1);
  return (unsigned int)(int)fminf(fmaxf(floorf(v * t + 0.5f), 0.f), t);      // NaN -> 0
}
__device__ __forceinline__ float ex_normalise(float v, float lo, float hi) { return hi == lo ? 0.f : (v - lo) / (hi - lo); }

struct __attribute__((packed, aligned(4))) ExWords { unsigned int w[4]; };      // the vertex section starts on an 8-byte boundary only

__global__ __launch_bounds__(EX_CHUNK) WM_NO_PACKED_FP32 void export_compressed_kernel(ExIn a, const unsigned int* __restrict__ order, int n,
                                                                                       float* __restrict__ chunks, ExWords* __restrict__ verts) {
  __shared__ float sRed[18 * (EX_THREADS / 64)], sOut[18];
  const long long p = (long long)blockIdx.x * EX_CHUNK + threadIdx.x;
  const bool live = p < n;
  float v[9], lo[9], hi[9];
  long long i = 0;
  if (live) {
    i = order[p];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v[j] = a.means[3 * i + j];
      v[3 + j] = a.scales[3 * i + j];
      v[6 + j] = a.sh0[3 * i + j] * EX_C0 + 0.5f;
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) { lo[j] = live ? v[j] : INFINITY; hi[j] = live ? v[j] : -INFINITY; }
  ex_block_minmax<9>(lo, hi, sRed, sOut);
  // chunk floats: [min means, max means, min scales, max scales, min colours, max colours], the scale bounds clamped
  float mn[9], mx[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) { mn[j] = sOut[j]; mx[j] = sOut[9 + j]; }
#pragma unroll
  for (int j = 3; j < 6; ++j) { mn[j] = fminf(fmaxf(mn[j], -20.f), 20.f); mx[j] = fminf(fmaxf(mx[j], -20.f), 20.f); }
  if (threadIdx.x < 18) {
    const int t = threadIdx.x, g = t / 6, w = t % 6;      // group (means / scales / colours), slot in the group: 0..2 min, 3..5 max
    float val = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (j == g * 3 + (w % 3)) val = w < 3 ? mn[j] : mx[j];
    }
    chunks[18 * (size_t)blockIdx.x + t] = val;
  }
  if (!live) return;
  ExWords o;
  o.w[0] = (ex_pack_unorm(ex_normalise(v[0], mn[0], mx[0]), 11) << 21) | (ex_pack_unorm(ex_normalise(v[1], mn[1], mx[1]), 10) << 11) |
           ex_pack_unorm(ex_normalise(v[2], mn[2], mx[2]), 11);
  o.w[2] = (ex_pack_unorm(ex_normalise(v[3], mn[3], mx[3]), 11) << 21) | (ex_pack_unorm(ex_normalise(v[4], mn[4], mx[4]), 10) << 11) |
           ex_pack_unorm(ex_normalise(v[5], mn[5], mx[5]), 11);
  o.w[3] = (ex_pack_unorm(ex_normalise(v[6], mn[6], mx[6]), 8) << 24) | (ex_pack_unorm(ex_normalise(v[7], mn[7], mx[7]), 8) << 16) |
           (ex_pack_unorm(ex_normalise(v[8], mn[8], mx[8]), 8) << 8) | ex_pack_unorm(ex_sigmoid(a.opac[i]), 8);
  // rotation: normalise, the first largest |component|, its sign made positive, the other three in order
  float q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = a.quats[4 * i + j];
  const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = q[j] / nrm;
  int big = 0;
  float best = fabsf(q[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (fabsf(q[j]) > best) { best = fabsf(q[j]); big = j; }
  }
  float lead = q[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) lead = big == j ? q[j] : lead;
  const bool flip = lead < 0.f;
  unsigned int rot = (unsigned int)big;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j != big) {
      const float c = flip ? -q[j] : q[j];
      rot = (rot << 10) | ex_pack_unorm(c * EX_HALF_SQRT2 + 0.5f, 10);
    }
  }
  o.w[1] = rot;
  verts[p] = o;
}

// sh bytes of ply_compressed: byte j = c K + k of splat p reads shN[i, k, c]
__global__ __launch_bounds__(EX_THREADS) WM_NO_PACKED_FP32 void export_sh_bytes_kernel(const float* __restrict__ shN, int K,
                                                                                       const unsigned int* __restrict__ order, long long total,
                                                                                       unsigned char* __restrict__ out) {
  const long long e = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
  if (e >= total) return;
  const int nr = 3 * K;
  const long long p = e / nr;
  const int j = (int)(e - p * nr), c = j / K, k = j - c * K;
  const float x = shN[(long long)order[p] * nr + 3 * k + c];
  out[e] = (unsigned char)ex_u8((x / 8.f + 0.5f) * 256.f);
}

// ------------------------------------------------------------------ host side
struct ExWs {
  int* flags; int* offs; int* kept; int* count;
  float* partials; float* mm;
  unsigned int* keys[2]; unsigned int* vals[2];
  void* cub; size_t cub_bytes;
  size_t total;
};

// The library scan's and sort's scratch by a rule of our own (8 bytes per row + 1 MiB, as the depth loss counts its sort): a size call gives
// the same number on every machine, with or without a device; the launchers ask the library what it needs and refuse if it were more.
ExWs ex_carve(char* base, long long N, bool with_sort) {
  ExWs w{};
  Carver c(base);
  const size_t rows = (size_t)(N > 0 ? N : 1);
  w.flags = c.take<int>(rows); w.offs = c.take<int>(rows); w.kept = c.take<int>(rows); w.count = c.take<int>(1);
  if (with_sort) {
    w.partials = c.take<float>((size_t)blocks_for((long long)rows, EX_THREADS) * 6); w.mm = c.take<float>(6);
    w.keys[0] = c.take<unsigned int>(rows); w.keys[1] = c.take<unsigned int>(rows);
    w.vals[0] = c.take<unsigned int>(rows); w.vals[1] = c.take<unsigned int>(rows);
  }
  w.cub_bytes = 8 * rows + ((size_t)1 << 20);
  w.cub = c.take<char>(w.cub_bytes);
  w.total = c.total();
  return w;
}

// flags (already written) -> kept list and *n_kept on the host; the one stream synchronisation of an export
hipError_t ex_compact(const ExWs& w, int N, int* n_kept, hipStream_t s) {
  hipError_t e = exclusive_sum(w.cub, w.cub_bytes, w.flags, w.offs, N, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(export_scatter_kernel, dim3(blocks_for(N, EX_THREADS)), dim3(EX_THREADS), 0, s, (const int*)w.flags, (const int*)w.offs, N, w.kept, w.count);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return read_back(n_kept, w.count, sizeof(int), s);
}

// kept rows -> Morton order (original row indices) in *order
hipError_t ex_morton_order(const ExWs& w, const float* means, int n, const unsigned int** order, hipStream_t s) {
  const unsigned nb = blocks_for(n, EX_THREADS);
  hipLaunchKernelGGL(export_minmax_kernel, dim3(nb), dim3(EX_THREADS), 0, s, means, (const int*)w.kept, n, w.partials);
  hipLaunchKernelGGL(export_minmax_final_kernel, dim3(1), dim3(EX_THREADS), 0, s, (const float*)w.partials, (int)nb, w.mm);
  hipLaunchKernelGGL(export_morton_kernel, dim3(nb), dim3(EX_THREADS), 0, s, means, (const int*)w.kept, n, (const float*)w.mm, w.keys[0], w.vals[0]);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipcub::DoubleBuffer<unsigned int> dk(w.keys[0], w.keys[1]), dv(w.vals[0], w.vals[1]);
  e = sort_pairs(w.cub, w.cub_bytes, dk, dv, n, 0, 30, s);      // stable: equal codes stay in row order
  if (e != hipSuccess) return e;
  *order = dv.Current();
  return hipSuccess;
}

hipError_t ex_pack_rows(const ExCols& cols, const int* kept, int n, float* out, hipStream_t s) {
  const long long total = (long long)n * cols.n;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(export_pack_rows_kernel, dim3(blocks_for(total, EX_THREADS)), dim3(EX_THREADS), 0, s, cols, kept, total, out);
  return hipGetLastError();
}

size_t ex_payload(long long n, int K, int format) {
  switch (format) {
    case WM_EXPORT_PLY: return (size_t)n * (size_t)(14 + 3 * K) * 4;
    case WM_EXPORT_SPLAT: return (size_t)n * 32;
    default: return (size_t)((n + EX_CHUNK - 1) / EX_CHUNK) * 72 + (size_t)n * 16 + (size_t)n * 3 * (size_t)K;
  }
}

bool ex_sizes_ok(long long N, int K, int format) {
  return N >= 0 && N < (1LL << 31) && K >= 0 && K <= 15 && format >= WM_EXPORT_PLY && format <= WM_EXPORT_PLY_COMPRESSED;
}

}  // namespace

// ------------------------------------------------------------------ C ABI (include/wm_hip.h)
extern "C" size_t wm_export_splats_workspace_bytes(int64_t N, int K, int format) {
  if (!ex_sizes_ok(N, K, format)) return 0;
  return ex_carve(nullptr, N, format != WM_EXPORT_PLY).total;
}

extern "C" size_t wm_export_splats_payload_bytes(int64_t n_kept, int K, int format) {
  if (!ex_sizes_ok(n_kept, K, format)) return 0;
  return ex_payload(n_kept, K, format);
}

// replaces gsplat/exporter.py:501-547 (the finite filter and the dispatch), :363-417 (ply), :420-472 (splat), :194-360 (ply_compressed)
// and :56-85 (the Morton order)
extern "C" wm_status wm_export_splats(const float* means, const float* scales, const float* quats, const float* opacities, const float* sh0,
                                      const float* shN, int64_t N, int K, int format, float opacity_threshold, void* workspace,
                                      size_t workspace_bytes, void* out, size_t out_bytes, int* n_kept, void* stream) {
  if (!ex_sizes_ok(N, K, format) || !n_kept || !workspace) return WM_ERR_INVALID;
  if (N > 0 && (!means || !scales || !quats || !opacities || !sh0 || !out || (K > 0 && !shN))) return WM_ERR_INVALID;
  const ExWs w = ex_carve((char*)workspace, N, format != WM_EXPORT_PLY);
  if (workspace_bytes < w.total || out_bytes < ex_payload(N, K, format)) return WM_ERR_INVALID;
  *n_kept = 0;
  if (N == 0) return WM_OK;
  hipStream_t s = (hipStream_t)stream;
  const ExIn a{means, scales, quats, opacities, sh0, shN, (int)N, K};
  hipLaunchKernelGGL(export_flags_kernel, dim3(blocks_for(N, EX_THREADS)), dim3(EX_THREADS), 0, s, a, format == WM_EXPORT_PLY_COMPRESSED ? 1 : 0,
                     opacity_threshold, w.flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return wm_status_of(e);
  int n = 0;
  e = ex_compact(w, (int)N, &n, s);
  if (e != hipSuccess) return WM_ERR_HIP;
  if (n < 0 || n > N) return WM_ERR_HIP;
  *n_kept = n;
  if (n == 0) return WM_OK;
  if (format == WM_EXPORT_PLY) {
    ExCols cols{};
    int c = 0;
    auto add = [&](const float* base, int stride) { cols.c[c].base = base; cols.c[c].stride = stride; cols.c[c].xf = 0; ++c; };
    for (int j = 0; j < 3; ++j) add(means + j, 3);
    for (int j = 0; j < 3; ++j) add(sh0 + j, 3);
    for (int ch = 0; ch < 3; ++ch)
      for (int k = 0; k < K; ++k) add(shN + 3 * k + ch, 3 * K);      // channel-major: the reference permutes [N,K,3] -> [N,3,K]
    add(opacities, 1);
    for (int j = 0; j < 3; ++j) add(scales + j, 3);
    for (int j = 0; j < 4; ++j) add(quats + j, 4);
    cols.n = c;
    return wm_status_of(ex_pack_rows(cols, w.kept, n, (float*)out, s));
  }
  const unsigned int* order = nullptr;
  e = ex_morton_order(w, means, n, &order, s);
  if (e != hipSuccess) return WM_ERR_HIP;
  if (format == WM_EXPORT_SPLAT) {
    hipLaunchKernelGGL(export_splat_kernel, dim3(blocks_for(n, EX_THREADS)), dim3(EX_THREADS), 0, s, a, order, n, (uint4*)out);
    return wm_status_of(hipGetLastError());
  }
  const int nchunks = (n + EX_CHUNK - 1) / EX_CHUNK;
  char* body = (char*)out;
  float* chunks = (float*)body;
  ExWords* verts = (ExWords*)(body + (size_t)nchunks * 72);
  unsigned char* shb = (unsigned char*)(body + (size_t)nchunks * 72 + (size_t)n * 16);
  hipLaunchKernelGGL(export_compressed_kernel, dim3((unsigned)nchunks), dim3(EX_CHUNK), 0, s, a, order, n, chunks, verts);
  if (K > 0) {
    const long long total = (long long)n * 3 * K;
    hipLaunchKernelGGL(export_sh_bytes_kernel, dim3(blocks_for(total, EX_THREADS)), dim3(EX_THREADS), 0, s, shN, K, order, total, shb);
  }
  return wm_status_of(hipGetLastError());
}

extern "C" size_t wm_pack_rows_workspace_bytes(int64_t N) {
  if (N < 0 || N >= (1LL << 31)) return 0;
  return ex_carve(nullptr, N, false).total;
}

// replaces src/utils/save_utils.py:154-185 (the masked gathers, the zero normals, scales.log(), the concatenation) for any column list
extern "C" wm_status wm_pack_rows(const float* const* col_ptrs, const int* col_strides, const int* col_transforms, int n_cols,
                                  const unsigned char* keep, int64_t N, void* workspace, size_t workspace_bytes, float* out, size_t out_bytes,
                                  int* n_kept, void* stream) {
  if (!col_ptrs || !col_strides || !col_transforms || n_cols < 1 || n_cols > EX_MAX_COLS || N < 0 || N >= (1LL << 31) || !n_kept || !workspace)
    return WM_ERR_INVALID;
  ExCols cols{};
  for (int c = 0; c < n_cols; ++c) {
    if (col_strides[c] < 0 || col_transforms[c] < WM_PACK_NONE || col_transforms[c] > WM_PACK_LOG) return WM_ERR_INVALID;
    cols.c[c].base = col_ptrs[c]; cols.c[c].stride = col_strides[c]; cols.c[c].xf = col_transforms[c];
  }
  cols.n = n_cols;
  const ExWs w = ex_carve((char*)workspace, N, false);
  if (workspace_bytes < w.total || out_bytes < (size_t)N * (size_t)n_cols * 4 || (N > 0 && !out)) return WM_ERR_INVALID;
  *n_kept = 0;
  if (N == 0) return WM_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(export_mask_flags_kernel, dim3(blocks_for(N, EX_THREADS)), dim3(EX_THREADS), 0, s, keep, (int)N, w.flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return wm_status_of(e);
  int n = 0;
  e = ex_compact(w, (int)N, &n, s);
  if (e != hipSuccess || n < 0 || n > N) return WM_ERR_HIP;
  *n_kept = n;
  return wm_status_of(ex_pack_rows(cols, w.kept, n, out, s));
}
