// What the kernels either side of the forward (export, COLMAP, GLB, k-NN, video, compression, MCMC, densify, the losses, the rasteriser's
// host side) share: workspace carving, the hipCUB sort / scan calls with their size check, the one-synchronisation read-back, and the small
// device helpers (finite test, order-preserving float keys, wave reductions, in-block rank and scan, Morton bit spreading).  One copy each;
// the radix-select state machines and the quantisation in front of a Morton code stay with their kernels.
#pragma once
#include <hipcub/hipcub.hpp>

#include "wm_common.h"

// ------------------------------------------------------------------ host side
constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// Carves a caller's workspace into 256-byte aligned pieces in the order of the take calls.  base may be null: a size-only pass, every piece
// null.  A workspace layout is ABI (a later call reads what an earlier one carved): neither the order nor the size of a take may change.
class Carver {
 public:
  explicit Carver(char* base) : base_(base) {}
  template <typename T>
  T* take(size_t count) {
    char* p = base_ ? base_ + o_ : nullptr;
    o_ += align256(count * sizeof(T));
    return (T*)p;
  }
  size_t total() const { return o_; }

 private:
  char* base_;
  size_t o_ = 0;
};

// device -> host copy and the ONE stream synchronisation of a call whose output size only the device knows
inline hipError_t read_back(void* host, const void* device, size_t bytes, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// hipCUB scratch sizes for the carvers; 0 where the library cannot answer (a large input on a machine without a device).
// sort_pairs_bytes: both buffers of keys and values handed over; sort_pairs_copy_bytes: separate input and output arrays.
template <typename K, typename V>
size_t sort_pairs_bytes(int n, int begin_bit, int end_bit) {
  size_t b = 0;
  hipcub::DoubleBuffer<K> dk((K*)nullptr, (K*)nullptr);
  hipcub::DoubleBuffer<V> dv((V*)nullptr, (V*)nullptr);
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, dk, dv, n, begin_bit, end_bit);
  return b;
}
template <typename K, typename V>
size_t sort_pairs_copy_bytes(int n, int begin_bit, int end_bit) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const K*)nullptr, (K*)nullptr, (const V*)nullptr, (V*)nullptr, n, begin_bit, end_bit);
  return b;
}
template <typename T>
size_t exclusive_sum_bytes(int n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (T*)nullptr, (T*)nullptr, n);
  return b;
}
template <typename T, typename Op>
size_t exclusive_scan_bytes(Op op, T init, int n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveScan(nullptr, b, (T*)nullptr, (T*)nullptr, op, init, n);
  return b;
}

// The library calls themselves: ask the size, refuse (hipErrorOutOfMemory) when it is more than the caller carved, run.  All sorts are stable.
template <typename K, typename V>
hipError_t sort_pairs(void* scratch, size_t capacity, hipcub::DoubleBuffer<K>& keys, hipcub::DoubleBuffer<V>& vals, int n, int begin_bit, int end_bit,
                      hipStream_t s) {
  size_t tb = 0;
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, vals, n, begin_bit, end_bit, s);      // the size alone: nothing is launched
  if (e != hipSuccess) return e;
  if (tb > capacity) return hipErrorOutOfMemory;
  return hipcub::DeviceRadixSort::SortPairs(scratch, tb, keys, vals, n, begin_bit, end_bit, s);
}
template <typename K, typename V>
hipError_t sort_pairs(void* scratch, size_t capacity, const K* keys_in, K* keys_out, const V* vals_in, V* vals_out, int n, int begin_bit, int end_bit,
                      hipStream_t s) {
  size_t tb = 0;
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s);
  if (e != hipSuccess) return e;
  if (tb > capacity) return hipErrorOutOfMemory;
  return hipcub::DeviceRadixSort::SortPairs(scratch, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s);
}
template <typename T>
hipError_t exclusive_sum(void* scratch, size_t capacity, T* in, T* out, int n, hipStream_t s) {
  size_t tb = 0;
  const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, n, s);
  if (e != hipSuccess) return e;
  if (tb > capacity) return hipErrorOutOfMemory;
  return hipcub::DeviceScan::ExclusiveSum(scratch, tb, in, out, n, s);
}
template <typename T, typename Op>
hipError_t exclusive_scan(void* scratch, size_t capacity, T* in, T* out, Op op, T init, int n, hipStream_t s) {
  size_t tb = 0;
  const hipError_t e = hipcub::DeviceScan::ExclusiveScan(nullptr, tb, in, out, op, init, n, s);
  if (e != hipSuccess) return e;
  if (tb > capacity) return hipErrorOutOfMemory;
  return hipcub::DeviceScan::ExclusiveScan(scratch, tb, in, out, op, init, n, s);
}

// ------------------------------------------------------------------ device side
__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN

// the order-preserving uint32 image of a float (smaller float <=> smaller key; -0 below +0, NaNs outside the infinities) and its inverse
__device__ __forceinline__ unsigned int ordered_key(float v) {
  const unsigned int u = __builtin_bit_cast(unsigned int, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned int k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// the confidence rule of create_confidence_mask (infer.py:25-59): conf <= 1e-5 counts as -inf, larger float <=> larger key
__device__ __forceinline__ unsigned int conf_key(float c) {
  if (c != c) return 0xFFFFFFFFu;  // any NaN, either sign, any payload: the one top key, above +inf like torch.topk's NaN-largest
  return ordered_key(c <= 1e-5f ? -INFINITY : c);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ordered rank of the lanes of a THREADS-wide block whose flag is set, and the number set; every lane calls it
template <int THREADS>
__device__ __forceinline__ unsigned int block_rank(bool f, unsigned int* sW /* THREADS / 64 */, unsigned int& total) {
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned int r = (unsigned int)__popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();      // sW may still be read from the call before
  if (lane == 0) sW[w] = (unsigned int)__popcll(b);
  __syncthreads();
  unsigned int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    if (i < w) base += sW[i];
    total += sW[i];
  }
  return base + r;
}

// in-place exclusive scan of v[0 .. n) by ONE THREADS-wide block; v[n] receives the total
template <int THREADS>
__device__ void block_scan_in_place(unsigned int* v, unsigned int n, unsigned int* part /* THREADS, shared */) {
  const unsigned int per = (n + THREADS - 1) / THREADS, lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  unsigned int s = 0;
  for (unsigned int i = lo; i < hi; ++i) s += v[i];
  __syncthreads();
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int run = 0;
    for (int i = 0; i < THREADS; ++i) { const unsigned int t = part[i]; part[i] = run; run += t; }
    v[n] = run;
  }
  __syncthreads();
  unsigned int run = part[threadIdx.x];
  for (unsigned int i = lo; i < hi; ++i) { const unsigned int t = v[i]; v[i] = run; run += t; }
  __syncthreads();
}

// Morton bit spreading: the low 10 bits to every third bit of 30, the low 16 bits to every second bit of 32
__device__ __forceinline__ unsigned int part1by2_10(unsigned int x) {
  x &= 0x000003ffu;
  x = (x ^ (x << 16)) & 0xff0000ffu;
  x = (x ^ (x << 8)) & 0x0300f00fu;
  x = (x ^ (x << 4)) & 0x030c30c3u;
  x = (x ^ (x << 2)) & 0x09249249u;
  return x;
}
__device__ __forceinline__ unsigned int part1by1_16(unsigned int x) {
  x &= 0x0000ffffu;
  x = (x ^ (x << 8)) & 0x00ff00ffu;
  x = (x ^ (x << 4)) & 0x0f0f0f0fu;
  x = (x ^ (x << 2)) & 0x33333333u;
  x = (x ^ (x << 1)) & 0x55555555u;
  return x;
}
