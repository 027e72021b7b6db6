// What the C-ABI entry files (wm_api_ops.cpp, wm_api_scene.cpp, wm_api_compress.cpp) share: the public header, the launcher interface and the status mapping.
#pragma once
#include "../../include/wm_hip.h"
#include "wm_kernels.h"

// For entries whose launcher checks sizes itself and answers hipErrorInvalidValue: that is the caller's mistake, not a HIP failure.
// Entries that report every launcher error as WM_ERR_HIP write `== hipSuccess ? WM_OK : WM_ERR_HIP` out and do not come through here.
static inline wm_status wm_status_of(hipError_t e) { return e == hipSuccess ? WM_OK : e == hipErrorInvalidValue ? WM_ERR_INVALID : WM_ERR_HIP; }

// ------------------------------------------------------------------ COLMAP hand-off (colmap.hip), entries in wm_api_scene.cpp
// select: candidates (depth > eps) of [S,H,W], the top K confidences among them; leaves its state in the workspace, synchronises the stream once and
// writes *n_kept and counts[S] (host).  gather: reads that state and writes the kept points in candidate order.  Sizes: S H W < 2^31.
size_t wm_colmap_select_ws_bytes(int S, int H, int W);      // 0 for sizes the launchers refuse
hipError_t wm_launch_colmap_select(const float* depth, const float* conf, int S, int H, int W, float eps, double percent, void* workspace,
                                   long long* n_kept, long long* counts, hipStream_t s);
hipError_t wm_launch_colmap_gather(const float* depth, const float* conf, const float* images, const float* c2w, const float* intr, int S, int H, int W,
                                   float eps, double scale_x, double scale_y, const void* workspace, long long n_kept, float* points,
                                   unsigned char* colors, int* xyf, hipStream_t s);
// the per-point bodies of points3D.bin (59 P bytes) and images.bin (24 P bytes); either may be null; counts [S] int64 on the device
size_t wm_colmap_pack_ws_bytes(long long P, int S);
hipError_t wm_launch_colmap_pack(const float* points, const unsigned char* colors, const int* xyf, const long long* counts, int S, long long P,
                                 void* workspace, void* points3d, void* points2d, hipStream_t s);
// 15-byte rows (3 f32, 3 u8) of the rows with keep != 0, or with finite coordinates (filter_finite), or of every row; synchronises only to count
size_t wm_point_ply_ws_bytes(long long N);
hipError_t wm_launch_point_ply(const float* points, const unsigned char* colors, const unsigned char* keep, int filter_finite, long long N,
                               void* workspace, void* out, long long* n_kept, hipStream_t s);

// ------------------------------------------------------------------ k nearest neighbours (knn.hip), entries in wm_api_scene.cpp
// dist [N,K] (ascending, the point itself included) and, when idx is not null, the rows idx [N,K] of the K nearest points of points [N,3] within
// the cloud itself; exact.  *nonfinite_flag (device) is written 0, or 1 for a NaN / infinite coordinate, and then nothing else is written.
// No synchronisation.  1 <= K <= 16, K <= N < 2^31.
size_t wm_knn_ws_bytes(long long N, int K);      // 0 for sizes the launcher refuses
hipError_t wm_launch_knn(const float* points, long long N, int K, void* workspace, float* dist, int* idx, int* nonfinite_flag, hipStream_t s);

// The nearest point of another cloud (knn.hip): build leaves the index of ref [N,3] in `index` (wm_nearest_index_bytes) and writes
// *nonfinite_flag (device) as wm_launch_knn does; query writes dist [M] and, when idx is not null, idx [M] for queries [M,3] against an index
// built for the same N (nothing when the build met a non-finite coordinate; NaN and -1 for a non-finite query row).  No synchronisation.
// 1 <= N < 2^31, 0 <= M < 2^31.
size_t wm_nearest_index_bytes(long long N);         // 0 for sizes the launchers refuse
size_t wm_nearest_query_ws_bytes(long long M);      // 0 for sizes the launchers refuse
hipError_t wm_launch_nearest_build(const float* ref, long long N, void* index, int* nonfinite_flag, hipStream_t s);
hipError_t wm_launch_nearest_query(const void* index, long long N, const float* queries, long long M, void* workspace, float* dist, int* idx,
                                   hipStream_t s);

// ------------------------------------------------------------------ point-cloud evaluation (reconmetrics.hip), entries in wm_api_scene.cpp
// out (device, 4 + WM_STATS_MAX_THRESHOLDS doubles): the mean and the median of dist [M], the mean and the median of |n_a[i] . n_b[idx[i]]|
// (written only with normals_a), then the counts of dist < thresholds[k] (host array).  No synchronisation.  1 <= M < 2^31.
size_t wm_cloud_stats_ws_bytes(long long M);      // 0 for sizes the launcher refuses
hipError_t wm_launch_cloud_stats(const float* dist, const int* idx, long long M, const float* normals_a, const float* normals_b, long long Nb,
                                 const float* thresholds, int n_thresholds, void* workspace, double* out, hipStream_t s);
// out (device, 16 doubles): s, R [9] row-major, t [3], the count of kept pairs, the source variance, 0.  mask [P] bytes or null.  1 <= P < 2^31.
size_t wm_umeyama_ws_bytes(long long P);      // 0 for sizes the launcher refuses
hipError_t wm_launch_umeyama(const float* src, const float* dst, const unsigned char* mask, long long P, int with_scale, void* workspace, double* out,
                             hipStream_t s);

// ------------------------------------------------------------------ PNG compression of splats (compress.hip), entries in wm_api_compress.cpp
// None of these synchronises.  mm [2 C]: C minima, then C maxima.  *nonfinite_flag (device) is set to 1 for a NaN or infinite value and
// otherwise left as it is: the caller zeroes it once and reads it once.
size_t wm_compress_minmax_ws_bytes(long long rows, int C);      // 0 for sizes the launcher refuses (C in 1..16)
hipError_t wm_launch_compress_minmax(const float* x, long long rows, int C, void* workspace, float* mm, int* nonfinite_flag, hipStream_t s);
// bits <= 8: one plane lo (hi null); bits 9..16: the low and the high bytes
hipError_t wm_launch_compress_quantise(const float* x, long long rows, int C, const float* mm, int bits, unsigned char* lo, unsigned char* hi, hipStream_t s);
hipError_t wm_launch_compress_dequantise(const unsigned char* lo, const unsigned char* hi, long long rows, int C, const float* mm, int bits, float* out,
                                         hipStream_t s);
// dst_f[r, :] = src_f[idx[r], :] for n_fields <= 16 fields of row_bytes[f] bytes per row (host arrays), rows < 2^31; idx values are the caller's to bound
hipError_t wm_launch_gather_rows(const void* const* src, void* const* dst, const int* row_bytes, int n_fields, const int* idx, long long rows, hipStream_t s);
// Lloyd under L1 distance (semantics: include/wm_hip.h).  D in {9, 24, 45}, 1 <= K <= 65536, K <= N <= 2^30.  info (device, 2 ints): the
// iterations run, and 1 when an init row was outside 0 .. N-1 (row 0 was taken in its place).  labels_last may be null.
size_t wm_kmeans_l1_ws_bytes(long long N, int D, int K);      // 0 for sizes the launcher refuses
hipError_t wm_launch_kmeans_l1(const float* x, long long N, int D, int K, const long long* init, int max_iter, double tol, void* workspace, int* labels,
                               int* labels_last, float* centroids, double* errors, int* info, hipStream_t s);
// one assignment on its own: labels [N] and dist [N] (the fp32 L1 distance to the chosen centroid) of x [N, D] against centroids [K, D]; N >= 1
hipError_t wm_launch_kmeans_l1_assign(const float* x, long long N, int D, const float* centroids, int K, int* labels, float* dist, hipStream_t s);
// perm [n^2]: the row of means [n^2, 3] that goes to every cell of the n x n grid.  1 <= n_side <= 46340.
size_t wm_grid_order_ws_bytes(int n_side);      // 0 for sizes the launcher refuses
hipError_t wm_launch_grid_order(const float* means, int n_side, void* workspace, int* perm, int* nonfinite_flag, hipStream_t s);

// ------------------------------------------------------------------ fly-through video (video.hip), entries in wm_api_scene.cpp
// GSEffects.apply_effect, effect_type 2, on (means - shift) * inv_scale, scales * inv_scale and rgb or degree-0 SH colours; shift [3] on the
// device or null.  stats (device, 2 doubles): the count of flag < 0.99 and the sum of flag.  No synchronisation.  N < 2^31.
size_t wm_gs_effect_ws_bytes(long long N);      // 0 for sizes the launcher refuses
hipError_t wm_launch_gs_effect_spread(const float* means, const float* scales, const float* opacities, const float* colors, const float* random_vals,
                                      long long N, double t_n, int ignore_scale, const float* shift, float inv_scale, int colors_are_sh0,
                                      float* out_means, float* out_scales, float* out_opacities, float* out_colors, float* flag, double* stats,
                                      void* workspace, hipStream_t s);
// rgbs [F,H,W,3] -> rgb_out u8 and / or depths [F,H,W] -> depth_out [F,H,W,3] u8 (turbo) + near_far [F,2]; either input may be null
size_t wm_video_frames_ws_bytes(int F, int H, int W);      // 0 for sizes the launcher refuses
hipError_t wm_launch_video_frames(const float* rgbs, const float* depths, int F, int H, int W, unsigned char* rgb_out, unsigned char* depth_out,
                                  float* near_far, void* workspace, hipStream_t s);
void wm_turbo_lut_bytes(unsigned char* out);      // host: the 256 x 3 table

// ------------------------------------------------------------------ GLB scene hand-off (glb.hip), entries in wm_api_scene.cpp
// count: the vertices and valid quads of every view's image mesh (mask [S,H,W] bytes or null = all); leaves its scans in the workspace, synchronises
// the stream once and writes n_vertices[S + 1], n_quads[S + 1] (host; the totals last).  pack: reads those scans and writes the views' vertices
// (positions, RGBA, normals when given) and faces, concatenated, and bounds [S,6].  Sizes: S H W < 2^31.
size_t wm_image_mesh_ws_bytes(int S, int H, int W);      // 0 for sizes the launchers refuse
hipError_t wm_launch_image_mesh_count(const unsigned char* mask, int S, int H, int W, void* workspace, long long* n_vertices, long long* n_quads,
                                      hipStream_t s);
hipError_t wm_launch_image_mesh_pack(const float* points, const float* colors, const float* normals, const unsigned char* mask, int S, int H, int W,
                                     void* workspace, long long total_v, long long total_q, float* positions, unsigned char* rgba, float* normals_out,
                                     int* faces, float* bounds, hipStream_t s);
// the masked rows of points / colors [N,3] in order: out[0, 12 n) positions, out[12 n, 16 n) RGBA; bounds [6]; synchronises once for *n_kept
size_t wm_glb_points_ws_bytes(long long N);
hipError_t wm_launch_glb_points(const float* points, const float* colors, const unsigned char* mask, long long N, void* workspace, void* out,
                                long long* n_kept, float* bounds, hipStream_t s);
// out [3][nq][2] (device): per column and quantile the order statistics of rank floor((n - 1) q) and the next; *count_out (device) = n
size_t wm_percentile_neighbours_ws_bytes(long long N, int nq);
hipError_t wm_launch_percentile_neighbours(const float* points, const unsigned char* mask, long long N, const double* q, int nq, void* workspace,
                                           float* out, long long* count_out, hipStream_t s);

// ------------------------------------------------------------------ trainer evaluation (evalmetrics.hip), entries in wm_api_scene.cpp
// colors / pixels [B,H,W,3] by element strides (B, H, W, C); clamped [B,H,W,3], canvas [B,H,2W,3] u8, psnr_all, psnr_each [B]: each may be null.
// No synchronisation.  Sizes: B <= 65535, 6 H W < 2^31.
size_t wm_eval_frame_ws_bytes(int B, int H, int W);      // 0 for sizes the launcher refuses
hipError_t wm_launch_eval_frame(const float* colors, const long long* cs, const float* pixels, const long long* ps, int B, int H, int W, int clamp,
                                double data_range, float* clamped, unsigned char* canvas, float* psnr_all, float* psnr_each, void* workspace,
                                hipStream_t s);
// img, ref, out: contiguous [nsys][P][3]; out must not overlap img.  No synchronisation.  nsys <= 65535, P < 2^31.
size_t wm_color_correct_ws_bytes(int nsys, long long P);      // 0 for sizes the launcher refuses
hipError_t wm_launch_color_correct(const float* img, const float* ref, int nsys, long long P, int num_iters, double eps, float* out, void* workspace,
                                   hipStream_t s);
