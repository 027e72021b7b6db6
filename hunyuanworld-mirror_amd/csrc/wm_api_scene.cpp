// Scene-level entries of the C ABI (include/wm_hip.h): the caller's steps on either side of the forward, each with its *_workspace_bytes.
// In file order: splat pruning, the rasteriser, densification, MCMC, the photometric loss, the bilateral grid, the appearance module, the
// depth loss and point projection, then image ingest and the point masks (with the novel-view path's select and validity mask), the COLMAP hand-off, the nearest neighbours, the point-cloud evaluation, the fly-through video, the GLB scene and the trainer evaluation.  Each entry
// checks its arguments, fills its launcher's args struct, launches on the caller's stream and maps the hipError_t.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "wm_api.h"

extern "C" size_t wm_prune_gs_workspace_bytes(size_t n) { return wm_prune_workspace_bytes(n); }
extern "C" wm_status wm_prune_gs(const float* means, const float* quats, const float* scales, const float* opacities, const float* sh,
                                 const float* weights, int n, float voxel_size, float* out_means, float* out_quats, float* out_scales,
                                 float* out_opacities, float* out_sh, int* n_voxels, void* workspace, size_t workspace_bytes, void* stream) {
  if (n < 0 || !(voxel_size > 0.f) || !n_voxels) return WM_ERR_INVALID;
  if (n > 0 && (!means || !quats || !scales || !sh || !weights || !out_means || !out_quats || !out_scales || !out_opacities || !out_sh || !workspace))
    return WM_ERR_INVALID;
  const hipError_t e = wm_launch_prune_gs(means, quats, scales, opacities, sh, weights, n, voxel_size, out_means, out_quats, out_scales,
                                          out_opacities, out_sh, n_voxels, workspace, workspace_bytes, (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" size_t wm_rasterize_workspace_bytes(int n_gaussians, int n_cameras, int width, int height, size_t max_isects) {
  return wm_raster_workspace_bytes(n_gaussians, n_cameras, width, height, max_isects);
}
// ---- the rasteriser's entries: wm_rasterize_splats_opt / wm_rasterize_splats_backward_opt do everything; the entries without options are
// thin wrappers that keep their own argument checks and pass default options (null)
static bool raster_fill(WmRasterArgs& a, const float* means, const float* quats, const float* scales, const float* opacities, const float* colors,
                        int colors_are_sh0, int n_coeffs, int sh_degree, const float* campos, int n_gaussians, const float* viewmats,
                        const float* Ks, int n_cameras, int width, int height, const wm_raster_options* opt) {
  memset(&a, 0, sizeof(a));
  wm_raster_default_options(a);
  if (opt) {
    a.antialiased = opt->antialiased; a.depth_mode = opt->depth_mode; a.eps2d = opt->eps2d; a.near_plane = opt->near_plane;
    a.far_plane = opt->far_plane; a.radius_clip = opt->radius_clip; a.backgrounds = opt->backgrounds;
  }
  a.means = means; a.quats = quats; a.scales = scales; a.opacities = opacities; a.colors = colors;
  if (sh_degree == 0) a.is_sh = colors_are_sh0;
  else { a.sh_degree = sh_degree; a.n_coeffs = n_coeffs; a.campos = campos; }
  a.N = n_gaussians; a.viewmats = viewmats; a.Ks = Ks; a.C = n_cameras; a.width = width; a.height = height;
  // checked here, in front of the first HIP call
  if (sh_degree < 0 || sh_degree > 3 || (sh_degree > 0 && ((sh_degree + 1) * (sh_degree + 1) > n_coeffs || !campos))) return false;
  if (colors_are_sh0 < 0 || colors_are_sh0 > WM_COLORS_PER_CAMERA || (colors_are_sh0 == WM_COLORS_PER_CAMERA && sh_degree > 0)) return false;
  return wm_raster_options_valid(a);
}
extern "C" wm_status wm_rasterize_splats_opt(const float* means, const float* quats, const float* scales, const float* opacities,
                                             const float* colors, int colors_are_sh0, int n_coeffs, int sh_degree, const float* campos,
                                             int n_gaussians, const float* viewmats, const float* Ks, int n_cameras, int width, int height,
                                             const wm_raster_options* options, float* out_rgb, float* out_depth, float* out_alpha,
                                             int* radii_out, void* workspace, size_t workspace_bytes, size_t max_isects,
                                             unsigned long long* n_isects, void* stream) {
  if (!means || !quats || !scales || !opacities || !colors || !viewmats || !Ks || !out_rgb || !out_depth || !out_alpha || !workspace)
    return WM_ERR_INVALID;
  WmRasterArgs a;
  if (!raster_fill(a, means, quats, scales, opacities, colors, colors_are_sh0, n_coeffs, sh_degree, campos, n_gaussians, viewmats, Ks, n_cameras,
                   width, height, options))
    return WM_ERR_INVALID;
  a.out_rgb = out_rgb; a.out_depth = out_depth; a.out_alpha = out_alpha; a.radii_out = radii_out;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.max_isects = max_isects;
  unsigned long long n = 0;
  const hipError_t e = wm_launch_rasterize(a, (hipStream_t)stream, &n);
  if (n_isects) *n_isects = n;
  if (e != hipSuccess) return wm_status_of(e);
  return n > max_isects ? WM_ERR_STATE : WM_OK;  // WM_ERR_STATE: the workspace is too small for *n_isects pairs, nothing was rendered
}
extern "C" size_t wm_rasterize_backward_workspace_bytes_opt(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad,
                                                            int want_viewmats, int sh_degree, int want_campos, int want_backgrounds) {
  return wm_raster_bwd_workspace_bytes(n_gaussians, n_cameras, width, height, n_isects, want_absgrad ? 1 : 0, want_viewmats ? 1 : 0,
                                       sh_degree > 0 ? 1 : 0, sh_degree > 0 && want_campos ? 1 : 0, want_backgrounds ? 1 : 0);
}
extern "C" wm_status wm_rasterize_splats_backward_opt(const float* means, const float* quats, const float* scales, const float* opacities,
                                                      const float* colors, int colors_are_sh0, int n_coeffs, int sh_degree, const float* campos,
                                                      int n_gaussians, const float* viewmats, const float* Ks, int n_cameras, int width,
                                                      int height, const wm_raster_options* options, const void* workspace,
                                                      size_t workspace_bytes, size_t max_isects, size_t n_isects, const float* out_rgb,
                                                      const float* out_depth, const float* out_alpha, const float* v_rgb, const float* v_depth,
                                                      const float* v_alpha, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                                      float* v_colors, float* v_means2d, float* v_means2d_abs, int want_absgrad,
                                                      float* v_viewmats, float* v_campos, float* v_backgrounds, void* grad_workspace,
                                                      size_t grad_workspace_bytes, void* stream) {
  (void)out_rgb;   // the kernels rebuild the transmittance themselves; the expected depth is read back, and out_alpha for v_backgrounds only
  if (!means || !quats || !scales || !opacities || !colors || !viewmats || !Ks || !workspace || !out_depth || !v_rgb || !v_depth || !v_alpha ||
      !v_means || !v_quats || !v_scales || !v_opacities || !v_colors || !grad_workspace)
    return WM_ERR_INVALID;
  if (want_absgrad && (!v_means2d || !v_means2d_abs)) return WM_ERR_INVALID;
  if (v_backgrounds && (!options || !options->backgrounds || !out_alpha)) return WM_ERR_INVALID;
  if (v_campos && sh_degree <= 0) return WM_ERR_INVALID;
  WmRasterBwdArgs b;
  memset(&b, 0, sizeof(b));
  if (!raster_fill(b.fwd, means, quats, scales, opacities, colors, colors_are_sh0, n_coeffs, sh_degree, campos, n_gaussians, viewmats, Ks,
                   n_cameras, width, height, options))
    return WM_ERR_INVALID;
  if (n_isects > max_isects) return WM_ERR_STATE;   // that forward rendered nothing: there is no state to differentiate
  WmRasterArgs& a = b.fwd;
  a.workspace = const_cast<void*>(workspace); a.workspace_bytes = workspace_bytes; a.max_isects = max_isects;
  b.n_isects = n_isects; b.out_depth = out_depth; b.out_alpha = out_alpha; b.v_rgb = v_rgb; b.v_depth = v_depth; b.v_alpha = v_alpha;
  b.v_means = v_means; b.v_quats = v_quats; b.v_scales = v_scales; b.v_opacities = v_opacities; b.v_colors = v_colors;
  b.v_means2d = v_means2d; b.v_means2d_abs = want_absgrad ? v_means2d_abs : nullptr; b.absgrad = want_absgrad ? 1 : 0;
  b.v_viewmats = v_viewmats; b.v_campos = v_campos; b.v_backgrounds = v_backgrounds;
  b.grad_workspace = grad_workspace; b.grad_workspace_bytes = grad_workspace_bytes;
  const hipError_t e = wm_launch_rasterize_bwd(b, (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" wm_status wm_rasterize_splats(const float* means, const float* quats, const float* scales, const float* opacities,
                                         const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                                         int n_cameras, int width, int height, float* out_rgb, float* out_depth, float* out_alpha,
                                         int* radii_out, void* workspace, size_t workspace_bytes, size_t max_isects,
                                         unsigned long long* n_isects, void* stream) {
  return wm_rasterize_splats_opt(means, quats, scales, opacities, colors, colors_are_sh0, 0, 0, nullptr, n_gaussians, viewmats, Ks, n_cameras, width,
                                 height, nullptr, out_rgb, out_depth, out_alpha, radii_out, workspace, workspace_bytes, max_isects, n_isects, stream);
}
extern "C" size_t wm_rasterize_backward_workspace_bytes(int n_gaussians, int n_cameras, int width, int height, size_t n_isects) {
  return wm_raster_bwd_workspace_bytes(n_gaussians, n_cameras, width, height, n_isects);
}
extern "C" wm_status wm_rasterize_splats_backward(const float* means, const float* quats, const float* scales, const float* opacities,
                                                  const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                                                  int n_cameras, int width, int height, const void* workspace, size_t workspace_bytes,
                                                  size_t max_isects, size_t n_isects, const float* out_rgb, const float* out_depth,
                                                  const float* out_alpha, const float* v_rgb, const float* v_depth, const float* v_alpha,
                                                  float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                                                  void* grad_workspace, size_t grad_workspace_bytes, void* stream) {
  return wm_rasterize_splats_backward_opt(means, quats, scales, opacities, colors, colors_are_sh0, 0, 0, nullptr, n_gaussians, viewmats, Ks, n_cameras,
                                          width, height, nullptr, workspace, workspace_bytes, max_isects, n_isects, out_rgb, out_depth, out_alpha, v_rgb,
                                          v_depth, v_alpha, v_means, v_quats, v_scales, v_opacities, v_colors, nullptr, nullptr, 0, nullptr, nullptr,
                                          nullptr, grad_workspace, grad_workspace_bytes, stream);
}
extern "C" size_t wm_rasterize_backward_workspace_bytes_ex(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad) {
  return wm_raster_bwd_workspace_bytes(n_gaussians, n_cameras, width, height, n_isects, want_absgrad ? 1 : 0);
}
extern "C" wm_status wm_rasterize_splats_backward_ex(const float* means, const float* quats, const float* scales, const float* opacities,
                                                     const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats,
                                                     const float* Ks, int n_cameras, int width, int height, const void* workspace,
                                                     size_t workspace_bytes, size_t max_isects, size_t n_isects, const float* out_rgb,
                                                     const float* out_depth, const float* out_alpha, const float* v_rgb, const float* v_depth,
                                                     const float* v_alpha, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                                     float* v_colors, float* v_means2d, float* v_means2d_abs, int want_absgrad,
                                                     void* grad_workspace, size_t grad_workspace_bytes, void* stream) {
  return wm_rasterize_splats_backward_opt(means, quats, scales, opacities, colors, colors_are_sh0, 0, 0, nullptr, n_gaussians, viewmats, Ks, n_cameras,
                                          width, height, nullptr, workspace, workspace_bytes, max_isects, n_isects, out_rgb, out_depth, out_alpha, v_rgb,
                                          v_depth, v_alpha, v_means, v_quats, v_scales, v_opacities, v_colors, v_means2d, v_means2d_abs, want_absgrad,
                                          nullptr, nullptr, nullptr, grad_workspace, grad_workspace_bytes, stream);
}
extern "C" size_t wm_rasterize_backward_workspace_bytes_cam(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad) {
  return wm_raster_bwd_workspace_bytes(n_gaussians, n_cameras, width, height, n_isects, want_absgrad ? 1 : 0, 1);
}
extern "C" wm_status wm_rasterize_splats_backward_cam(const float* means, const float* quats, const float* scales, const float* opacities,
                                                      const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats,
                                                      const float* Ks, int n_cameras, int width, int height, const void* workspace,
                                                      size_t workspace_bytes, size_t max_isects, size_t n_isects, const float* out_rgb,
                                                      const float* out_depth, const float* out_alpha, const float* v_rgb, const float* v_depth,
                                                      const float* v_alpha, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                                      float* v_colors, float* v_means2d, float* v_means2d_abs, int want_absgrad,
                                                      float* v_viewmats, void* grad_workspace, size_t grad_workspace_bytes, void* stream) {
  if (!v_viewmats) return WM_ERR_INVALID;
  return wm_rasterize_splats_backward_opt(means, quats, scales, opacities, colors, colors_are_sh0, 0, 0, nullptr, n_gaussians, viewmats, Ks, n_cameras,
                                          width, height, nullptr, workspace, workspace_bytes, max_isects, n_isects, out_rgb, out_depth, out_alpha, v_rgb,
                                          v_depth, v_alpha, v_means, v_quats, v_scales, v_opacities, v_colors, v_means2d, v_means2d_abs, want_absgrad,
                                          v_viewmats, nullptr, nullptr, grad_workspace, grad_workspace_bytes, stream);
}
extern "C" wm_status wm_rasterize_splats_sh(const float* means, const float* quats, const float* scales, const float* opacities,
                                            const float* sh_coeffs, int n_coeffs, int sh_degree, const float* campos, int n_gaussians,
                                            const float* viewmats, const float* Ks, int n_cameras, int width, int height, float* out_rgb,
                                            float* out_depth, float* out_alpha, int* radii_out, void* workspace, size_t workspace_bytes,
                                            size_t max_isects, unsigned long long* n_isects, void* stream) {
  if (sh_degree < 1) return WM_ERR_INVALID;
  return wm_rasterize_splats_opt(means, quats, scales, opacities, sh_coeffs, 0, n_coeffs, sh_degree, campos, n_gaussians, viewmats, Ks, n_cameras, width,
                                 height, nullptr, out_rgb, out_depth, out_alpha, radii_out, workspace, workspace_bytes, max_isects, n_isects, stream);
}
extern "C" size_t wm_rasterize_backward_workspace_bytes_sh(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad,
                                                           int want_viewmats, int want_campos) {
  return wm_raster_bwd_workspace_bytes(n_gaussians, n_cameras, width, height, n_isects, want_absgrad ? 1 : 0, want_viewmats ? 1 : 0, 1,
                                       want_campos ? 1 : 0);
}
extern "C" wm_status wm_rasterize_splats_backward_sh(const float* means, const float* quats, const float* scales, const float* opacities,
                                                     const float* sh_coeffs, int n_coeffs, int sh_degree, const float* campos, int n_gaussians,
                                                     const float* viewmats, const float* Ks, int n_cameras, int width, int height,
                                                     const void* workspace, size_t workspace_bytes, size_t max_isects, size_t n_isects,
                                                     const float* out_rgb, const float* out_depth, const float* out_alpha, const float* v_rgb,
                                                     const float* v_depth, const float* v_alpha, float* v_means, float* v_quats, float* v_scales,
                                                     float* v_opacities, float* v_sh_coeffs, float* v_means2d, float* v_means2d_abs,
                                                     int want_absgrad, float* v_viewmats, float* v_campos, void* grad_workspace,
                                                     size_t grad_workspace_bytes, void* stream) {
  if (sh_degree < 1) return WM_ERR_INVALID;
  return wm_rasterize_splats_backward_opt(means, quats, scales, opacities, sh_coeffs, 0, n_coeffs, sh_degree, campos, n_gaussians, viewmats, Ks,
                                          n_cameras, width, height, nullptr, workspace, workspace_bytes, max_isects, n_isects, out_rgb, out_depth,
                                          out_alpha, v_rgb, v_depth, v_alpha, v_means, v_quats, v_scales, v_opacities, v_sh_coeffs, v_means2d,
                                          v_means2d_abs, want_absgrad, v_viewmats, v_campos, nullptr, grad_workspace, grad_workspace_bytes, stream);
}
extern "C" wm_status wm_rasterize_means2d(const void* workspace, size_t workspace_bytes, int n_gaussians, int n_cameras, int width, int height,
                                          size_t max_isects, const int* radii, float* means2d, void* stream) {
  if (!workspace || !radii || !means2d) return WM_ERR_INVALID;
  const hipError_t e = wm_launch_rasterize_means2d(workspace, workspace_bytes, n_gaussians, n_cameras, width, height, max_isects, radii, means2d,
                                                   (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" wm_status wm_densify_accumulate(const float* v_means2d, const int* radii, int n_gaussians, int n_cameras, int width, int height,
                                           float* grad2d, float* count, float* radii_state, void* stream) {
  if (!v_means2d || !radii || !grad2d || !count) return WM_ERR_INVALID;
  const hipError_t e = wm_launch_densify_accumulate(v_means2d, radii, n_gaussians, n_cameras, width, height, grad2d, count, radii_state,
                                                    (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" size_t wm_densify_plan_workspace_bytes(size_t n_gaussians) { return wm_densify_plan_ws_bytes(n_gaussians); }
extern "C" wm_status wm_densify_plan(const float* grad2d, const float* count, const float* radii_state, const float* scales,
                                     const float* opacities, int n_gaussians, float grow_grad2d, float grow_scale3d, float grow_scale2d,
                                     float prune_opa, float prune_scale3d, float prune_scale2d, int use_scale2d, int prune_big,
                                     int revised_opacity, int* src, int* kind, int* rank, int* counts, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!grad2d || !count || !scales || !opacities || !src || !kind || !rank || !counts || !workspace) return WM_ERR_INVALID;
  WmDensifyPlanArgs a;
  memset(&a, 0, sizeof(a));
  a.grad2d = grad2d; a.count = count; a.radii_state = radii_state; a.scales = scales; a.opacities = opacities; a.N = n_gaussians;
  a.grow_grad2d = grow_grad2d; a.grow_scale3d = grow_scale3d; a.grow_scale2d = grow_scale2d;
  a.prune_opa = prune_opa; a.prune_scale3d = prune_scale3d; a.prune_scale2d = prune_scale2d;
  a.use_scale2d = use_scale2d ? 1 : 0; a.prune_big = prune_big ? 1 : 0; a.revised_opacity = revised_opacity ? 1 : 0;
  a.src = src; a.kind = kind; a.rank = rank; a.counts = counts; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  const hipError_t e = wm_launch_densify_plan(a, (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" wm_status wm_densify_gather(const float* in, float* out, int n_gaussians, int row, int mode, const int* src, const int* kind,
                                       const int* rank, int n_out, const float* quats, const float* scales, const float* noise, void* stream) {
  if (n_out > 0 && (!src || !kind || !rank || !in || !out)) return WM_ERR_INVALID;   // an empty result has no rows to point at
  const hipError_t e = wm_launch_densify_gather(in, out, n_gaussians, row, mode, src, kind, rank, n_out, quats, scales, noise, (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" wm_status wm_mcmc_inject_noise(float* means, const float* quats, const float* scales, const float* opacities, const float* noise,
                                          float scaler, int n_gaussians, void* stream) {
  if (n_gaussians > 0 && (!means || !quats || !scales || !opacities || !noise)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_mcmc_inject_noise(means, quats, scales, opacities, noise, scaler, n_gaussians, (hipStream_t)stream));
}
extern "C" size_t wm_mcmc_partition_workspace_bytes(size_t n_gaussians) { return wm_mcmc_partition_ws_bytes(n_gaussians); }
extern "C" wm_status wm_mcmc_partition(const float* opacities, const unsigned char* mask, int n_gaussians, float min_opacity, int* dead_idx,
                                       int* alive_idx, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if ((!opacities && !mask) || !dead_idx || !alive_idx || !counts || !workspace) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_mcmc_partition(opacities, mask, n_gaussians, min_opacity, dead_idx, alive_idx, counts, workspace, workspace_bytes,
                                              (hipStream_t)stream));
}
extern "C" wm_status wm_mcmc_relocation(const float* opacities, const float* scales, const int* sampled, int n_sampled, int n_gaussians,
                                        float min_opacity, float* new_opacities, float* new_scales, int* hist, void* stream) {
  if (n_sampled > 0 && (!opacities || !scales || !sampled || !new_opacities || !new_scales || !hist)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_mcmc_relocation(opacities, scales, sampled, n_sampled, n_gaussians, min_opacity, new_opacities, new_scales, hist,
                                               (hipStream_t)stream));
}
extern "C" wm_status wm_mcmc_scatter(float* t, int rows, int row, const int* sampled, const int* dest, const float* values, int n_sampled,
                                     void* stream) {
  if (n_sampled > 0 && (!t || !sampled || !dest)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_mcmc_scatter(t, rows, row, sampled, dest, values, n_sampled, (hipStream_t)stream));
}
extern "C" wm_status wm_mcmc_zero_rows(float* t, int rows, int row, const int* idx, int n, void* stream) {
  if (n > 0 && (!t || !idx)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_mcmc_zero_rows(t, rows, row, idx, n, (hipStream_t)stream));
}
extern "C" size_t wm_photometric_loss_workspace_bytes(int B, int C, int H, int W) { return wm_photoloss_workspace_bytes(B, C, H, W); }
extern "C" size_t wm_photometric_loss_forward_workspace_bytes(int B, int C, int H, int W) {
  return C > 0 ? wm_photoloss_forward_only_bytes(B, H, W) : 0;
}
static bool photo_args(WmPhotoLossArgs& a, const float* img1, const int64_t* strides1, const float* img2, const int64_t* strides2, int B, int C,
                       int H, int W, int padding_valid, void* workspace, size_t workspace_bytes, bool maps) {
  if (!img1 || !img2 || !strides1 || !strides2 || !workspace || B <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
  if (padding_valid && (H < 11 || W < 11)) return false;                 // fused_ssim would take the mean of an empty map
  if (workspace_bytes < (maps ? wm_photoloss_workspace_bytes(B, C, H, W) : wm_photoloss_forward_only_bytes(B, H, W))) return false;
  memset(&a, 0, sizeof(a));
  a.img1 = img1; a.img2 = img2; a.strides1 = strides1; a.strides2 = strides2; a.B = B; a.C = C; a.H = H; a.W = W;
  a.padding_valid = padding_valid; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return true;
}
extern "C" wm_status wm_photometric_loss(const float* img1, const int64_t* strides1, const float* img2, const int64_t* strides2, int B, int C,
                                         int H, int W, int padding_valid, int want_backward, float* out_ssim, float* out_l1,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  WmPhotoLossArgs a;
  if (!out_ssim || !out_l1 ||
      !photo_args(a, img1, strides1, img2, strides2, B, C, H, W, padding_valid, workspace, workspace_bytes, want_backward != 0))
    return WM_ERR_INVALID;
  const hipError_t e = wm_launch_photoloss_fwd(a, want_backward, out_ssim, out_l1, (hipStream_t)stream);
  return wm_status_of(e);
}
extern "C" wm_status wm_photometric_loss_backward(const float* img1, const int64_t* strides1, const float* img2, const int64_t* strides2, int B,
                                                  int C, int H, int W, int padding_valid, const float* g_ssim, const float* g_l1,
                                                  float* grad_img1, const void* workspace, size_t workspace_bytes, void* stream) {
  WmPhotoLossArgs a;
  if (!g_ssim || !g_l1 || !grad_img1 ||
      !photo_args(a, img1, strides1, img2, strides2, B, C, H, W, padding_valid, const_cast<void*>(workspace), workspace_bytes, true))
    return WM_ERR_INVALID;
  const hipError_t e = wm_launch_photoloss_bwd(a, g_ssim, g_l1, grad_img1, (hipStream_t)stream);
  return wm_status_of(e);
}
static bool bilagrid_args(WmBilagridArgs& a, const float* grids, int G, int L, int Hg, int Wg, const int* grid_idx, const float* xy, const float* rgb,
                          int B, int n) {
  if (!grids || !grid_idx || !xy || !rgb) return false;
  a.grids = grids; a.grid_idx = grid_idx; a.xy = xy; a.rgb = rgb; a.G = G; a.L = L; a.Hg = Hg; a.Wg = Wg; a.B = B; a.n = n;
  return true;       // the sizes are checked by the launcher, before it launches anything
}
extern "C" wm_status wm_bilagrid_slice(const float* grids, int G, int L, int Hg, int Wg, const int* grid_idx, const float* xy, const float* rgb,
                                       int B, int n, float* out, void* stream) {
  WmBilagridArgs a;
  if (!out || !bilagrid_args(a, grids, G, L, Hg, Wg, grid_idx, xy, rgb, B, n)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilagrid_slice(a, out, (hipStream_t)stream));
}
extern "C" size_t wm_bilagrid_slice_backward_workspace_bytes(int G, int L, int Hg, int Wg, int B, int n) {
  return wm_bilagrid_bwd_workspace_bytes(G, L, Hg, Wg, B, n);
}
extern "C" wm_status wm_bilagrid_slice_backward(const float* grids, int G, int L, int Hg, int Wg, const int* grid_idx, const float* xy,
                                                const float* rgb, int B, int n, const float* v_out, float* v_grids, float* v_rgb,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  WmBilagridArgs a;
  if (!v_out || !bilagrid_args(a, grids, G, L, Hg, Wg, grid_idx, xy, rgb, B, n)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilagrid_slice_bwd(a, v_out, v_grids, v_rgb, workspace, workspace_bytes, (hipStream_t)stream));
}
extern "C" size_t wm_bilagrid_tv_workspace_bytes(int B, int C, int L, int H, int W) { return wm_bilagrid_tv_ws_bytes(B, C, L, H, W); }
extern "C" wm_status wm_bilagrid_tv(const float* x, int B, int C, int L, int H, int W, float* out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!x || !out) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilagrid_tv(x, B, C, L, H, W, out, workspace, workspace_bytes, (hipStream_t)stream));
}
extern "C" wm_status wm_bilagrid_tv_backward(const float* x, int B, int C, int L, int H, int W, const float* g, float* v_x, void* stream) {
  if (!x || !g || !v_x) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilagrid_tv_bwd(x, B, C, L, H, W, g, v_x, (hipStream_t)stream));
}
// ---- appearance module (appearance.hip)
static bool appearance_fill(WmAppearanceArgs& a, const float* features, const float* embeds, int n_embeds, const int* embed_ids, const float* dirs,
                            const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3, int n_gaussians,
                            int n_cameras, int module_sh_degree, int sh_degree) {
  memset(&a, 0, sizeof(a));
  if (!features || !dirs || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || n_gaussians <= 0 || n_cameras <= 0) return false;
  if (module_sh_degree < 0 || module_sh_degree > 3 || sh_degree < 0 || sh_degree > module_sh_degree) return false;
  if (embed_ids && (!embeds || n_embeds <= 0)) return false;
  if ((size_t)n_gaussians * n_cameras >= (1ull << 29)) return false;
  a.features = features; a.embeds = embeds; a.embed_ids = embed_ids; a.dirs = dirs; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3;
  a.N = n_gaussians; a.C = n_cameras; a.n_embeds = n_embeds; a.n_bases = (module_sh_degree + 1) * (module_sh_degree + 1); a.degree = sh_degree;
  return true;
}
extern "C" wm_status wm_appearance_forward(const float* features, const float* embeds, int n_embeds, const int* embed_ids, const float* dirs,
                                           const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                                           int n_gaussians, int n_cameras, int module_sh_degree, int sh_degree, float* out, void* stream) {
  WmAppearanceArgs a;
  if (!out || !appearance_fill(a, features, embeds, n_embeds, embed_ids, dirs, W1, b1, W2, b2, W3, b3, n_gaussians, n_cameras, module_sh_degree, sh_degree))
    return WM_ERR_INVALID;
  return wm_status_of(wm_launch_appearance_fwd(a, out, (hipStream_t)stream));
}
extern "C" size_t wm_appearance_backward_workspace_bytes(int n_gaussians, int n_cameras) {
  return wm_appearance_bwd_workspace_bytes(n_gaussians, n_cameras);
}
extern "C" wm_status wm_appearance_backward(const float* features, const float* embeds, int n_embeds, const int* embed_ids, const float* dirs,
                                            const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                                            int n_gaussians, int n_cameras, int module_sh_degree, int sh_degree, const float* v_out,
                                            float* v_features, float* v_dirs, float* v_embeds, float* v_W1, float* v_b1, float* v_W2, float* v_b2,
                                            float* v_W3, float* v_b3, void* workspace, size_t workspace_bytes, void* stream) {
  WmAppearanceArgs a;
  if (!appearance_fill(a, features, embeds, n_embeds, embed_ids, dirs, W1, b1, W2, b2, W3, b3, n_gaussians, n_cameras, module_sh_degree, sh_degree))
    return WM_ERR_INVALID;
  if (!v_out || !v_features || !v_dirs || !v_W1 || !v_b1 || !v_W2 || !v_b2 || !v_W3 || !v_b3 || !workspace) return WM_ERR_INVALID;
  if (v_embeds && (!embeds || n_embeds <= 0)) return WM_ERR_INVALID;
  if (workspace_bytes < wm_appearance_bwd_workspace_bytes(n_gaussians, n_cameras)) return WM_ERR_INVALID;
  WmAppearanceGrads v;
  v.v_out = v_out; v.v_features = v_features; v.v_dirs = v_dirs; v.v_embeds = v_embeds; v.v_W1 = v_W1; v.v_b1 = v_b1; v.v_W2 = v_W2; v.v_b2 = v_b2;
  v.v_W3 = v_W3; v.v_b3 = v_b3;
  return wm_status_of(wm_launch_appearance_bwd(a, v, workspace, workspace_bytes, (hipStream_t)stream));
}
// ---- sparse disparity loss and point projection (depthloss.hip)
extern "C" size_t wm_depth_loss_workspace_bytes(int C, int H, int W, int M, int want_backward) {
  return wm_depthloss_workspace_bytes(C, H, W, M, want_backward);
}
static bool depth_loss_args(WmDepthLossArgs& a, const float* depth, const int64_t* strides, int C, int H, int W, const float* points,
                            const float* depth_gt, const unsigned char* valid, int M, void* workspace, size_t workspace_bytes, bool backward) {
  if (!depth || !strides || !workspace || C < 1 || H < 2 || W < 2 || M < 0) return false;      // the reference divides by W - 1 and H - 1
  if (M > 0 && (!points || !depth_gt)) return false;
  const size_t need = wm_depthloss_workspace_bytes(C, H, W, M, backward ? 1 : 0);
  if (need == 0 || workspace_bytes < need) return false;
  memset(&a, 0, sizeof(a));
  a.depth = depth; a.strides = strides; a.points = points; a.depth_gt = depth_gt; a.valid = valid; a.C = C; a.H = H; a.W = W; a.M = M;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return true;
}
extern "C" wm_status wm_depth_loss(const float* depth, const int64_t* strides, int C, int H, int W, const float* points, const float* depth_gt,
                                   const unsigned char* valid, int M, int want_backward, float* out_loss, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  WmDepthLossArgs a;
  if (!out_loss || !depth_loss_args(a, depth, strides, C, H, W, points, depth_gt, valid, M, workspace, workspace_bytes, want_backward != 0))
    return WM_ERR_INVALID;
  return wm_status_of(wm_launch_depthloss_fwd(a, want_backward, out_loss, (hipStream_t)stream));
}
extern "C" wm_status wm_depth_loss_backward(int C, int H, int W, const float* points, int M, const float* g, float* v_depth,
                                            const int64_t* v_strides, void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !v_depth || !v_strides || !workspace || C < 1 || H < 2 || W < 2 || M < 0 || (M > 0 && !points)) return WM_ERR_INVALID;
  const size_t need = wm_depthloss_workspace_bytes(C, H, W, M, 1);
  if (need == 0 || workspace_bytes < need) return WM_ERR_INVALID;
  WmDepthLossArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points; a.C = C; a.H = H; a.W = W; a.M = M; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return wm_status_of(wm_launch_depthloss_bwd(a, g, v_depth, v_strides, (hipStream_t)stream));
}
extern "C" wm_status wm_project_depth_points(const float* points_world, const float* camtoworlds, const float* Ks, const unsigned char* visible,
                                             int C, int P, int width, int height, float* points, float* depths, unsigned char* valid,
                                             void* stream) {
  if (!camtoworlds || !Ks || C < 1 || P < 0 || width < 1 || height < 1) return WM_ERR_INVALID;
  if (P > 0 && (!points_world || !points || !depths || !valid)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_depth_project(points_world, camtoworlds, Ks, visible, C, P, width, height, points, depths, valid, (hipStream_t)stream));
}
// ---------------------------------------------------------------- image ingest
// Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for the BICUBIC filter, in double
// precision with contraction off so that every rounding matches Pillow's C build (and oracle/ingest_ref.py).
#pragma clang fp contract(off)
static double wm_bicubic(double x) {
  const double a = -0.5;
  if (x < 0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static int wm_resample_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  bounds.assign((size_t)out_size * 2, 0);
  kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> w((size_t)ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = wm_bicubic((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    for (int x = 0; x < xmax; ++x) {
      double v = w[x];
      if (ww != 0.0) v /= ww;
      kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}
// inference_utils.py:70-83; Python's round() is half-to-even = nearbyint in the default rounding mode
static void wm_ingest_dims(int H, int W, int mode, int target, int* sw, int* sh, int* hf, int* wf, int* ry0, int* rx0) {
#pragma clang fp contract(off)
  if (mode == 1) {  // pad
    if (W >= H) { *sw = target; *sh = (int)std::nearbyint((double)H * ((double)target / (double)W) / 14.0) * 14; }
    else { *sh = target; *sw = (int)std::nearbyint((double)W * ((double)target / (double)H) / 14.0) * 14; }
    *hf = target > *sh ? target : *sh; *wf = target > *sw ? target : *sw;           // pad up to the square; never crops
    *ry0 = -((*hf - *sh) / 2); *rx0 = -((*wf - *sw) / 2);
  } else {          // crop
    *sw = target; *sh = (int)std::nearbyint((double)H * ((double)target / (double)W) / 14.0) * 14;
    *wf = *sw; *hf = *sh > target ? target : *sh;
    *ry0 = *sh > target ? (*sh - target) / 2 : 0; *rx0 = 0;
  }
}
extern "C" wm_status wm_preprocess_image_size(int H, int W, int mode, int output_size, int* out_h, int* out_w) {
  if (H <= 0 || W <= 0 || (mode != 0 && mode != 1) || output_size <= 0 || !out_h || !out_w) return WM_ERR_INVALID;
  int sw, sh, ry0, rx0;
  wm_ingest_dims(H, W, mode, output_size, &sw, &sh, out_h, out_w, &ry0, &rx0);
  return (sw > 0 && sh > 0) ? WM_OK : WM_ERR_INVALID;
}
extern "C" size_t wm_preprocess_image_workspace_bytes(int H, int W, int mode, int output_size) {
  int sw, sh, hf, wf, ry0, rx0;
  if (H <= 0 || W <= 0) return 0;
  wm_ingest_dims(H, W, mode, output_size, &sw, &sh, &hf, &wf, &ry0, &rx0);
  if (sw <= 0 || sh <= 0) return 0;
  auto ks = [](int in, int out) { const double sc = (double)in / out; return (int)std::ceil(2.0 * (sc < 1.0 ? 1.0 : sc)) * 2 + 1; };
  const size_t tabs = ((size_t)sw * (2 + ks(W, sw)) + (size_t)sh * (2 + ks(H, sh))) * sizeof(int);
  return (size_t)H * sw * 3 + 256 + tabs + 256;
}
extern "C" wm_status wm_preprocess_image(const unsigned char* rgb, int H, int W, int mode, int output_size, float* out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  if (!rgb || !out || !workspace || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return WM_ERR_INVALID;
  if (workspace_bytes < wm_preprocess_image_workspace_bytes(H, W, mode, output_size)) return WM_ERR_INVALID;
  int sw, sh, hf, wf, ry0, rx0;
  wm_ingest_dims(H, W, mode, output_size, &sw, &sh, &hf, &wf, &ry0, &rx0);
  if (sw <= 0 || sh <= 0) return WM_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> bh, kh, bv, kv;
  const int ksh = sw != W ? wm_resample_coeffs(W, sw, bh, kh) : 0;
  const int ksv = sh != H ? wm_resample_coeffs(H, sh, bv, kv) : 0;
  char* ws = (char*)workspace;
  unsigned char* tmp = (unsigned char*)ws;
  size_t off = ((size_t)H * sw * 3 + 255) / 256 * 256;
  int* d_bh = (int*)(ws + off); off += bh.size() * 4;
  int* d_kh = (int*)(ws + off); off += kh.size() * 4;
  int* d_bv = (int*)(ws + off); off += bv.size() * 4;
  int* d_kv = (int*)(ws + off); off += kv.size() * 4;
  // the tables are small (a few hundred KB at most); pageable copies are synchronous with respect to the host, which
  // keeps the vectors alive long enough
  if (ksh) {
    if (hipMemcpyAsync(d_bh, bh.data(), bh.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return WM_ERR_HIP;
    if (hipMemcpyAsync(d_kh, kh.data(), kh.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return WM_ERR_HIP;
  }
  if (ksv) {
    if (hipMemcpyAsync(d_bv, bv.data(), bv.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return WM_ERR_HIP;
    if (hipMemcpyAsync(d_kv, kv.data(), kv.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return WM_ERR_HIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess) return WM_ERR_HIP;
  const unsigned char* hsrc = rgb;
  if (ksh) {
    if (wm_launch_resample_h(rgb, tmp, H, W, sw, d_bh, d_kh, ksh, s) != hipSuccess) return WM_ERR_HIP;
    hsrc = tmp;
  }
  if (wm_launch_resample_v_tensor(hsrc, out, H, sw, sh, hf, wf, ry0, rx0, ksv ? d_bv : nullptr, ksv ? d_kv : nullptr, ksv, s) != hipSuccess)
    return WM_ERR_HIP;
  return WM_OK;
}

extern "C" size_t wm_confidence_mask_workspace_bytes(size_t n) { return wm_confidence_mask_workspace(n); }
extern "C" wm_status wm_confidence_mask(const float* conf, size_t n, double conf_threshold_percent, unsigned char* mask, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (!conf || !mask || !workspace || workspace_bytes < wm_confidence_mask_workspace(n)) return WM_ERR_INVALID;
  if (n == 0) return WM_OK;
  // infer.py:44-48: keep the top ceil(N (100 - p) / 100), at least one; p <= 0 keeps everything.  p is the caller's Python float and
  // the arithmetic is the reference's, in double: an fp32 image of p (33.3f > 33.3) moves K by one at n = 1000
  double keep = (double)n;
  if (conf_threshold_percent > 0.0) keep = std::ceil((double)n * (100.0 - conf_threshold_percent) / 100.0);
  size_t K = keep < 1.0 ? 1 : (size_t)keep;
  if (K > n) K = n;
  return wm_launch_confidence_mask(conf, n, (unsigned int)K, mask, workspace, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// the select of wm_confidence_mask with the count given: GaussianSplatRenderer.apply_confidence_filter (rasterization.py:248-299) caps its
// count with max_gaussians, which no percentage expresses
extern "C" wm_status wm_confidence_mask_count(const float* conf, size_t n, size_t k, unsigned char* mask, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  if (!conf || !mask || !workspace || workspace_bytes < wm_confidence_mask_workspace(n)) return WM_ERR_INVALID;
  if (n < 1 || k < 1 || k > n || n >= ((size_t)1 << 32)) return WM_ERR_INVALID;
  return wm_launch_confidence_mask(conf, n, (unsigned int)k, mask, workspace, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// replaces calculate_in_frustum_mask (src/models/utils/frustum.py:26-89) behind the two matrix inverses, which the caller takes once
extern "C" wm_status wm_in_frustum_mask(const float* depth_1, const float* depth_2, const float* kinv_1, const float* rel, const float* k_2, int B,
                                        int V1, int V2, int H, int W, unsigned char* mask, void* stream) {
  if (!depth_1 || !depth_2 || !kinv_1 || !rel || !k_2 || !mask || B < 1 || V1 < 1 || V2 < 1 || H < 1 || W < 1) return WM_ERR_INVALID;
  if ((long long)B * V1 * H * W >= (1LL << 31) || (long long)B * V2 * H * W >= (1LL << 31) || (long long)B * V1 * V2 >= (1LL << 24))
    return WM_ERR_INVALID;
  return wm_status_of(wm_launch_in_frustum_mask(depth_1, depth_2, kinv_1, rel, k_2, B, V1, V2, H, W, mask, (hipStream_t)stream));
}
extern "C" wm_status wm_depth_edge(const float* depth, const unsigned char* mask, int S, int H, int W, int k, int has_atol, float atol,
                                   int has_rtol, float rtol, unsigned char* out, void* stream) {
  if (!depth || !out || S < 0 || H < 0 || W < 0 || (k != 3 && k != 5 && k != 7) || (long long)S * H * W >= (1LL << 31)) return WM_ERR_INVALID;
  return wm_launch_depth_edge(depth, mask, S, H, W, k, has_atol, atol, has_rtol, rtol, out, (hipStream_t)stream) == hipSuccess ? WM_OK
                                                                                                                           : WM_ERR_HIP;
}
extern "C" wm_status wm_normals_edge(const float* normals, const unsigned char* mask, int S, int H, int W, int k, double tol_deg,
                                     unsigned char* out, void* stream) {
  if (!normals || !out || S < 0 || H < 0 || W < 0 || (k != 3 && k != 5 && k != 7) || (long long)S * H * W >= (1LL << 31)) return WM_ERR_INVALID;
  return wm_launch_normals_edge(normals, mask, S, H, W, k, tol_deg, out, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" size_t wm_point_filter_mask_workspace_bytes(int S, int H, int W) { return wm_point_filter_mask_workspace(S, H, W); }
extern "C" wm_status wm_point_filter_mask(const float* conf, const float* depth, const float* normals, int S, int H, int W, int apply_conf,
                                          double percentile, int apply_edge, double normal_tol_deg, float depth_rtol, float* thresholds_out,
                                          unsigned char* mask_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mask_out || S < 0 || H < 0 || W < 0 || (long long)S * H * W >= (1LL << 31)) return WM_ERR_INVALID;
  if ((apply_conf && !conf) || (apply_edge && (!depth || !normals))) return WM_ERR_INVALID;
  if (apply_conf && !(percentile >= 0.0 && percentile <= 100.0)) return WM_ERR_INVALID;
  if (!workspace || workspace_bytes < wm_point_filter_mask_workspace(S, H, W)) return WM_ERR_INVALID;
  return wm_launch_point_filter_mask(conf, depth, normals, S, H, W, apply_conf, percentile, apply_edge, normal_tol_deg, depth_rtol,
                                     thresholds_out, mask_out, nullptr, nullptr, workspace, (hipStream_t)stream) == hipSuccess ? WM_OK
                                                                                                                               : WM_ERR_HIP;
}
extern "C" wm_status wm_depth_to_world(const float* depth, const float* extrinsic, const float* intrinsic, float* world, float* cam,
                                       unsigned char* mask, int B, int H, int W, float eps, void* stream) {
  if (!depth || !extrinsic || !intrinsic || B < 0 || H < 0 || W < 0) return WM_ERR_INVALID;
  return wm_launch_depth_to_world(depth, extrinsic, intrinsic, world, cam, mask, B, H, W, eps, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}

// ---------------------------------------------------------------- COLMAP hand-off (colmap.hip)
extern "C" size_t wm_colmap_select_workspace_bytes(int S, int H, int W) { return wm_colmap_select_ws_bytes(S, H, W); }
// replaces infer.py:296-324 (the per-view unprojection mask, the boolean indexing, the concatenation and the global confidence top-k)
extern "C" wm_status wm_colmap_select(const float* depth, const float* conf, int S, int H, int W, float eps, double conf_threshold_percent,
                                      void* workspace, size_t workspace_bytes, int64_t* n_kept, int64_t* counts, void* stream) {
  const size_t need = wm_colmap_select_ws_bytes(S, H, W);
  if (!depth || !conf || !workspace || !n_kept || !counts || need == 0 || workspace_bytes < need) return WM_ERR_INVALID;
  static_assert(sizeof(long long) == sizeof(int64_t), "int64_t is long long here");
  return wm_status_of(wm_launch_colmap_select(depth, conf, S, H, W, eps, conf_threshold_percent, workspace, (long long*)n_kept, (long long*)counts,
                                              (hipStream_t)stream));
}
// replaces infer.py:303-313, 329-335 (the kept rows of the world points, the colours and the pixel grid, and the rescaling of x and y)
extern "C" wm_status wm_colmap_gather(const float* depth, const float* conf, const float* images, const float* camtoworlds, const float* intrinsics,
                                      int S, int H, int W, float eps, double scale_x, double scale_y, const void* workspace, size_t workspace_bytes,
                                      int64_t n_kept, float* points, unsigned char* colors, int32_t* xyf, void* stream) {
  const size_t need = wm_colmap_select_ws_bytes(S, H, W);
  if (!depth || !conf || !images || !camtoworlds || !intrinsics || !workspace || need == 0 || workspace_bytes < need) return WM_ERR_INVALID;
  if (n_kept < 0 || (n_kept > 0 && (!points || !colors || !xyf))) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_colmap_gather(depth, conf, images, camtoworlds, intrinsics, S, H, W, eps, scale_x, scale_y, workspace, n_kept, points,
                                              colors, xyf, (hipStream_t)stream));
}
extern "C" size_t wm_colmap_pack_workspace_bytes(int64_t P, int S) { return wm_colmap_pack_ws_bytes(P, S); }
// replaces src/utils/build_pycolmap_recon.py:36-51, 76-77 (add_point3D, Point2D and track.add_element per point) and the per-point part of
// pycolmap's Reconstruction.write (infer.py:356)
extern "C" wm_status wm_colmap_pack(const float* points, const unsigned char* colors, const int32_t* xyf, const int64_t* counts, int S, int64_t P,
                                    void* workspace, size_t workspace_bytes, void* points3d, size_t points3d_bytes, void* points2d,
                                    size_t points2d_bytes, void* stream) {
  const size_t need = wm_colmap_pack_ws_bytes(P, S);
  if (need == 0 || !workspace || workspace_bytes < need) return WM_ERR_INVALID;
  if (P > 0 && ((points3d && (!points || !colors || !counts)) || (points2d && !xyf))) return WM_ERR_INVALID;
  if ((points3d && points3d_bytes < (size_t)P * 59) || (points2d && points2d_bytes < (size_t)P * 24)) return WM_ERR_INVALID;
  if (((size_t)points3d & 3) || ((size_t)points2d & 7)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_colmap_pack(points, colors, xyf, (const long long*)counts, S, P, workspace, points3d, points2d, (hipStream_t)stream));
}
extern "C" size_t wm_pack_point_ply_workspace_bytes(int64_t N) { return wm_point_ply_ws_bytes(N); }
// replaces src/utils/save_utils.py:86-111 and :119-127 (the finite filter or the mask, and the structured array of x y z red green blue)
extern "C" wm_status wm_pack_point_ply(const float* points, const unsigned char* colors, const unsigned char* keep, int filter_finite, int64_t N,
                                       void* workspace, size_t workspace_bytes, void* out, size_t out_bytes, int64_t* n_kept, void* stream) {
  const size_t need = wm_point_ply_ws_bytes(N);
  if (need == 0 || !workspace || workspace_bytes < need || !n_kept) return WM_ERR_INVALID;
  if (N > 0 && (!points || !colors || !out)) return WM_ERR_INVALID;
  if (out_bytes < (size_t)N * 15 || ((size_t)out & 3)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_point_ply(points, colors, keep, filter_finite, N, workspace, out, (long long*)n_kept, (hipStream_t)stream));
}

// ---------------------------------------------------------------- k nearest neighbours (knn.hip)
extern "C" size_t wm_knn_workspace_bytes(int64_t N, int K) { return wm_knn_ws_bytes(N, K); }
// replaces submodules/gsplat/examples/utils.py:141-145 (knn: the copy to the host and scikit-learn's kd-tree) as
// simple_trainer_worldmirror.py:334-337 calls it
extern "C" wm_status wm_knn(const float* points, int64_t N, int K, void* workspace, size_t workspace_bytes, float* dist, int32_t* idx,
                            int32_t* nonfinite_flag, void* stream) {
  const size_t need = wm_knn_ws_bytes(N, K);
  if (need == 0 || !points || !workspace || workspace_bytes < need || !dist || !nonfinite_flag) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_knn(points, N, K, workspace, dist, idx, nonfinite_flag, (hipStream_t)stream));
}

// the nearest point of another cloud: the index once, the queries many times (the kd-tree of a host-side accuracy / completeness evaluation)
extern "C" size_t wm_nearest_build_workspace_bytes(int64_t N) { return wm_nearest_index_bytes(N); }
extern "C" wm_status wm_nearest_build(const float* ref, int64_t N, void* index, size_t index_bytes, int32_t* nonfinite_flag, void* stream) {
  const size_t need = wm_nearest_index_bytes(N);
  if (need == 0 || !ref || !index || index_bytes < need || !nonfinite_flag) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_nearest_build(ref, N, index, nonfinite_flag, (hipStream_t)stream));
}
extern "C" size_t wm_nearest_query_workspace_bytes(int64_t M) { return wm_nearest_query_ws_bytes(M); }
extern "C" wm_status wm_nearest_query(const void* index, size_t index_bytes, int64_t N, const float* queries, int64_t M, void* workspace,
                                      size_t workspace_bytes, float* dist, int32_t* idx, void* stream) {
  const size_t need_index = wm_nearest_index_bytes(N), need = wm_nearest_query_ws_bytes(M);
  if (need_index == 0 || need == 0 || !index || index_bytes < need_index || !workspace || workspace_bytes < need) return WM_ERR_INVALID;
  if (M > 0 && (!queries || !dist)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_nearest_query(index, N, queries, M, workspace, dist, idx, (hipStream_t)stream));
}

// ---------------------------------------------------------------- point-cloud evaluation (reconmetrics.hip)
extern "C" size_t wm_cloud_stats_workspace_bytes(int64_t M) { return wm_cloud_stats_ws_bytes(M); }
extern "C" wm_status wm_cloud_stats(const float* dist, const int32_t* idx, int64_t M, const float* normals_a, const float* normals_b, int64_t Nb,
                                    const float* thresholds, int n_thresholds, void* workspace, size_t workspace_bytes, double* out, void* stream) {
  const size_t need = wm_cloud_stats_ws_bytes(M);
  if (need == 0 || !dist || !out || !workspace || workspace_bytes < need) return WM_ERR_INVALID;
  if (n_thresholds < 0 || n_thresholds > WM_STATS_MAX_THRESHOLDS || (n_thresholds > 0 && !thresholds)) return WM_ERR_INVALID;
  if (normals_a && (!normals_b || !idx || Nb < 1)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_cloud_stats(dist, idx, M, normals_a, normals_b, Nb, thresholds, n_thresholds, workspace, out, (hipStream_t)stream));
}
extern "C" size_t wm_umeyama_workspace_bytes(int64_t P) { return wm_umeyama_ws_bytes(P); }
extern "C" wm_status wm_umeyama(const float* src, const float* dst, const unsigned char* mask, int64_t P, int with_scale, void* workspace,
                                size_t workspace_bytes, double* out, void* stream) {
  const size_t need = wm_umeyama_ws_bytes(P);
  if (need == 0 || !src || !dst || !out || !workspace || workspace_bytes < need) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_umeyama(src, dst, mask, P, with_scale, workspace, out, (hipStream_t)stream));
}

// ---------------------------------------------------------------- fly-through video (video.hip)
extern "C" size_t wm_gs_effect_spread_workspace_bytes(int64_t N) { return wm_gs_effect_ws_bytes(N); }
// replaces src/utils/gs_effects.py:162-242 (apply_effect, effect_type 2) with src/utils/render_utils.py:230-234 around it (the shift and
// scale of the pruned splats, SH2RGB / RGB2SH) and the two reductions of :228 and :281
extern "C" wm_status wm_gs_effect_spread(const float* means, const float* scales, const float* opacities, const float* colors,
                                         const float* random_vals, int64_t N, double t_n, int ignore_scale, const float* shift, float inv_scale,
                                         int colors_are_sh0, float* out_means, float* out_scales, float* out_opacities, float* out_colors,
                                         float* flag, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t need = wm_gs_effect_ws_bytes(N);
  if (need == 0 || !workspace || workspace_bytes < need || !stats || !(t_n == t_n)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_gs_effect_spread(means, scales, opacities, colors, random_vals, N, t_n, ignore_scale, shift, inv_scale, colors_are_sh0,
                                                 out_means, out_scales, out_opacities, out_colors, flag, stats, workspace, (hipStream_t)stream));
}
extern "C" size_t wm_video_frames_workspace_bytes(int F, int H, int W) { return wm_video_frames_ws_bytes(F, H, W); }
// replaces src/utils/render_utils.py:326-357 (depth_vis per frame with src/utils/color_map.py:11-29, and _make_video's clamp * 255 -> uint8)
extern "C" wm_status wm_video_frames(const float* rgbs, const float* depths, int F, int H, int W, unsigned char* rgb_out, unsigned char* depth_out,
                                     float* near_far, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t need = wm_video_frames_ws_bytes(F, H, W);
  if (need == 0 || (!rgbs && !depths)) return WM_ERR_INVALID;
  if (depths && (!workspace || workspace_bytes < need)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_video_frames(rgbs, depths, F, H, W, rgb_out, depth_out, near_far, workspace, (hipStream_t)stream));
}
extern "C" void wm_turbo_lut(unsigned char out[768]) {
  if (out) wm_turbo_lut_bytes(out);
}

// ---------------------------------------------------------------- GLB scene hand-off (glb.hip)
extern "C" size_t wm_image_mesh_workspace_bytes(int S, int H, int W) { return wm_image_mesh_ws_bytes(S, H, W); }
// replaces the mask part of src/utils/visual_util.py:168-179 (valid_quads and np.unique's count) for every view
extern "C" wm_status wm_image_mesh_count(const unsigned char* mask, int S, int H, int W, void* workspace, size_t workspace_bytes,
                                         int64_t* n_vertices, int64_t* n_quads, void* stream) {
  const size_t need = wm_image_mesh_ws_bytes(S, H, W);
  if (need == 0 || !workspace || workspace_bytes < need || !n_vertices || !n_quads) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_image_mesh_count(mask, S, H, W, workspace, (long long*)n_vertices, (long long*)n_quads, (hipStream_t)stream));
}
// replaces visual_util.py:172-190 (the kept faces, the triangles, np.unique's remap and the gathers) and the uint8 colours of :378 / :428
extern "C" wm_status wm_image_mesh_pack(const float* points, const float* colors, const float* normals, const unsigned char* mask, int S, int H,
                                        int W, const void* workspace, size_t workspace_bytes, int64_t total_vertices, int64_t total_quads,
                                        float* positions, unsigned char* rgba, float* normals_out, int32_t* faces, float* bounds, void* stream) {
  const size_t need = wm_image_mesh_ws_bytes(S, H, W);
  if (need == 0 || !workspace || workspace_bytes < need || !points || !colors || !bounds) return WM_ERR_INVALID;
  if (total_vertices < 0 || total_quads < 0) return WM_ERR_INVALID;
  if (total_vertices > 0 && (!positions || !rgba || (normals && !normals_out))) return WM_ERR_INVALID;
  if (total_quads > 0 && !faces) return WM_ERR_INVALID;
  if (((size_t)positions & 3) || ((size_t)normals_out & 3) || ((size_t)faces & 3)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_image_mesh_pack(points, colors, normals, mask, S, H, W, (void*)workspace, total_vertices, total_quads, positions,
                                                rgba, normals_out, faces, bounds, (hipStream_t)stream));
}
extern "C" size_t wm_glb_pack_points_workspace_bytes(int64_t N) { return wm_glb_points_ws_bytes(N); }
// replaces visual_util.py:274-298 (the uint8 colours and the boolean indexing of the flattened points)
extern "C" wm_status wm_glb_pack_points(const float* points, const float* colors, const unsigned char* mask, int64_t N, void* workspace,
                                        size_t workspace_bytes, void* out, size_t out_bytes, int64_t* n_kept, float* bounds, void* stream) {
  const size_t need = wm_glb_points_ws_bytes(N);
  if (need == 0 || !workspace || workspace_bytes < need || !points || !colors || !out || !n_kept || !bounds) return WM_ERR_INVALID;
  if (out_bytes < (size_t)N * 16 || ((size_t)out & 3)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_glb_points(points, colors, mask, N, workspace, out, (long long*)n_kept, bounds, (hipStream_t)stream));
}
extern "C" size_t wm_masked_percentile_neighbours_workspace_bytes(int64_t N, int n_quantiles) {
  return wm_percentile_neighbours_ws_bytes(N, n_quantiles);
}
// replaces the selection inside np.percentile of visual_util.py:307-308 (a partition of the filtered points per axis)
extern "C" wm_status wm_masked_percentile_neighbours(const float* points, const unsigned char* mask, int64_t N, const double* quantiles,
                                                     int n_quantiles, void* workspace, size_t workspace_bytes, float* out, int64_t* count_out,
                                                     void* stream) {
  const size_t need = wm_percentile_neighbours_ws_bytes(N, n_quantiles);
  if (need == 0 || !workspace || workspace_bytes < need || !quantiles || !out || !count_out || (N > 0 && !points)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_percentile_neighbours(points, mask, N, quantiles, n_quantiles, workspace, out, (long long*)count_out,
                                                      (hipStream_t)stream));
}
extern "C" size_t wm_eval_frame_workspace_bytes(int B, int H, int W) { return wm_eval_frame_ws_bytes(B, H, W); }
// replaces simple_trainer_worldmirror.py:1040-1054: the clamp, the canvas bytes and the PSNR of one batch of renders
extern "C" wm_status wm_eval_frame(const float* colors, const int64_t* color_strides, const float* pixels, const int64_t* pixel_strides, int B, int H,
                                   int W, int clamp_colors, double data_range, float* clamped_out, unsigned char* canvas_out, float* psnr_out,
                                   float* psnr_per_image, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t need = wm_eval_frame_ws_bytes(B, H, W);
  if (need == 0 || !workspace || workspace_bytes < need || !colors || !pixels || !color_strides || !pixel_strides) return WM_ERR_INVALID;
  if (!(data_range > 0.0) || (canvas_out && !clamp_colors)) return WM_ERR_INVALID;   // the canvas shows the clamped render
  if (((size_t)workspace & 7) || ((size_t)clamped_out & 3)) return WM_ERR_INVALID;
  long long cs[4], ps[4];
  for (int i = 0; i < 4; ++i) { cs[i] = color_strides[i]; ps[i] = pixel_strides[i]; }
  return wm_status_of(wm_launch_eval_frame(colors, cs, pixels, ps, B, H, W, clamp_colors, data_range, clamped_out, canvas_out, psnr_out,
                                           psnr_per_image, workspace, (hipStream_t)stream));
}
extern "C" size_t wm_color_correct_workspace_bytes(int n_systems, int64_t n_pixels) { return wm_color_correct_ws_bytes(n_systems, n_pixels); }
// replaces lib_bilagrid.py:56-126 (color_correct): per iteration one accumulation pass and one solve, no [P,10] matrix, no host round trip
extern "C" wm_status wm_color_correct(const float* img, const float* ref, int n_systems, int64_t n_pixels, int num_iters, double eps, float* out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const size_t need = wm_color_correct_ws_bytes(n_systems, n_pixels);
  if (need == 0 || !workspace || workspace_bytes < need || ((size_t)workspace & 7) || !img || !ref || !out) return WM_ERR_INVALID;
  if (num_iters < 0 || !(eps > 0.0) || !(eps < 0.5)) return WM_ERR_INVALID;
  const size_t bytes = (size_t)n_systems * (size_t)n_pixels * 3 * sizeof(float);
  if ((const char*)out < (const char*)img + bytes && (const char*)img < (const char*)out + bytes) return WM_ERR_INVALID;   // mask0 reads img throughout
  return wm_status_of(wm_launch_color_correct(img, ref, n_systems, n_pixels, num_iters, eps, out, workspace, (hipStream_t)stream));
}
