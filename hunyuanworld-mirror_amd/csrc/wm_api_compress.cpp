// C-ABI entries of the splat compression (include/wm_hip.h; kernels and launchers in compress.hip): what gsplat's PngCompression
// (gsplat/compression/png_compression.py) runs on the host with numpy, torchpq and PLAS, as the trainer's run_compression calls it.  Each
// entry checks its arguments, launches on the caller's stream and maps the hipError_t; none synchronises.
#include <hip/hip_runtime.h>

#include "wm_api.h"

extern "C" size_t wm_compress_minmax_workspace_bytes(int64_t rows, int C) { return wm_compress_minmax_ws_bytes(rows, C); }
// replaces png_compression.py:167-168 / :239-240 / :367-368 (torch.amin / amax over the grid, torch.min / max over the centroids)
extern "C" wm_status wm_compress_minmax(const float* x, int64_t rows, int C, void* workspace, size_t workspace_bytes, float* mm, int32_t* nonfinite_flag,
                                        void* stream) {
  const size_t need = wm_compress_minmax_ws_bytes(rows, C);
  if (need == 0 || !x || !workspace || workspace_bytes < need || !mm || !nonfinite_flag) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_compress_minmax(x, rows, C, workspace, mm, nonfinite_flag, (hipStream_t)stream));
}
// replaces png_compression.py:169-172 / :241-246 / :369-373 (normalise, scale, numpy's round, the byte split)
extern "C" wm_status wm_compress_quantise(const float* x, int64_t rows, int C, const float* mm, int bits, unsigned char* lo, unsigned char* hi, void* stream) {
  if (!x || !mm || !lo) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_compress_quantise(x, rows, C, mm, bits, lo, hi, (hipStream_t)stream));
}
// replaces png_compression.py:203-208 / :285-291 / :412-416 (the fp64 decoders)
extern "C" wm_status wm_compress_dequantise(const unsigned char* lo, const unsigned char* hi, int64_t rows, int C, const float* mm, int bits, float* out,
                                            void* stream) {
  if (!lo || !mm || !out) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_compress_dequantise(lo, hi, rows, C, mm, bits, out, (hipStream_t)stream));
}
// replaces png_compression.py:138-139 (the crop), sort.py's index_select over the fields and png_compression.py:418 (centroids[labels])
extern "C" wm_status wm_gather_rows(const void* const* src, void* const* dst, const int32_t* row_bytes, int n_fields, const int32_t* idx, int64_t rows,
                                    void* stream) {
  if (!src || !dst || !row_bytes || !idx) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_gather_rows(src, dst, row_bytes, n_fields, idx, rows, (hipStream_t)stream));
}
extern "C" size_t wm_kmeans_l1_workspace_bytes(int64_t N, int D, int K) { return wm_kmeans_l1_ws_bytes(N, D, K); }
// replaces png_compression.py:361-365 (torchpq's KMeans(distance="manhattan").fit)
extern "C" wm_status wm_kmeans_l1(const float* x, int64_t N, int D, int K, const int64_t* init, int max_iter, double tol, void* workspace,
                                  size_t workspace_bytes, int32_t* labels, int32_t* labels_last, float* centroids, double* errors, int32_t* info,
                                  void* stream) {
  const size_t need = wm_kmeans_l1_ws_bytes(N, D, K);
  if (need == 0 || !x || !init || !workspace || workspace_bytes < need || !labels || !centroids || !errors || !info) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_kmeans_l1(x, N, D, K, (const long long*)init, max_iter, tol, workspace, labels, labels_last, centroids, errors, info,
                                          (hipStream_t)stream));
}
// step (1) of an iteration on its own: new rows against a given table
extern "C" wm_status wm_kmeans_l1_assign(const float* x, int64_t N, int D, const float* centroids, int K, int32_t* labels, float* dist, void* stream) {
  if (!x || !centroids || !labels || !dist) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_kmeans_l1_assign(x, N, D, centroids, K, labels, dist, (hipStream_t)stream));
}
extern "C" size_t wm_grid_order_workspace_bytes(int n_side) { return wm_grid_order_ws_bytes(n_side); }
// stands where gsplat/compression/sort.py (sort_splats: PLAS) stands in the reference; the order itself is this library's own
extern "C" wm_status wm_grid_order(const float* means, int n_side, void* workspace, size_t workspace_bytes, int32_t* perm, int32_t* nonfinite_flag,
                                   void* stream) {
  const size_t need = wm_grid_order_ws_bytes(n_side);
  if (need == 0 || !means || !workspace || workspace_bytes < need || !perm || !nonfinite_flag) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_grid_order(means, n_side, workspace, perm, nonfinite_flag, (hipStream_t)stream));
}
