"""ctypes binding of libwm_hip.so (the C ABI declared in include/wm_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing
this module's ``lib()`` raises.  ``import torch`` must come first so that this library binds to the
HIP runtime / RCCL already loaded by torch-ROCm (same sonames) and device pointers are shared.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (loads libamdhip64.so.7 / librccl.so.1 first)

_HERE = os.path.dirname(os.path.abspath(__file__))
# WM_HIP_LIB: a diagnostic build of the same library (tools only, e.g. the in-kernel stamp build of csrc/Makefile "stamps")
LIB_PATH = os.environ.get("WM_HIP_LIB") or os.path.join(_HERE, "libwm_hip.so")

WM_DT = {"bf16": 0, "f16": 1, "fp16": 1, "float16": 1, "bfloat16": 0}
EPI_F32, EPI_T16, EPI_GELU_T16, EPI_RESID = 0, 1, 2, 3


class wm_config(C.Structure):
    _fields_ = [
        ("img_size", C.c_int32), ("patch_size", C.c_int32), ("embed_dim", C.c_int32), ("gs_dim", C.c_int32),
        ("enable_cond", C.c_int32), ("enable_cam", C.c_int32), ("enable_pts", C.c_int32), ("enable_depth", C.c_int32),
        ("enable_norm", C.c_int32), ("enable_gs", C.c_int32),
        ("depth", C.c_int32), ("num_heads", C.c_int32), ("mlp_ratio", C.c_int32), ("num_register_tokens", C.c_int32),
        ("intermediate_idxs", C.c_int32 * 4),
        ("rope_freq", C.c_float),
        ("dino_depth", C.c_int32), ("dino_heads", C.c_int32),
        ("cam_trunk_depth", C.c_int32), ("cam_heads", C.c_int32), ("cam_steps", C.c_int32),
        ("dpt_features", C.c_int32),
        ("dpt_out_channels", C.c_int32 * 4),
        ("backbone_dtype", C.c_int32), ("head_dtype", C.c_int32),
    ]


_FP = C.c_void_p  # device float*


class wm_outputs(C.Structure):
    _fields_ = [(n, _FP) for n in (
        "camera_params", "camera_poses", "camera_intrs", "depth", "depth_conf", "pts3d", "pts3d_conf",
        "normals", "normals_conf", "gs_depth", "gs_depth_conf", "splat_means", "splat_quats", "splat_scales",
        "splat_opacities", "splat_sh", "splat_weights")] + [("taps", _FP * 4)]


class wm_raster_options(C.Structure):
    """include/wm_hip.h wm_raster_options: gsplat.rasterization's options as the _opt rasteriser entries take them"""
    _fields_ = [("antialiased", C.c_int), ("depth_mode", C.c_int), ("eps2d", C.c_float), ("near_plane", C.c_float), ("far_plane", C.c_float),
                ("radius_clip", C.c_float), ("backgrounds", C.c_void_p)]


EXPORTS = [
    "wm_create", "wm_destroy", "wm_last_error", "wm_set_weight", "wm_finalize_weights", "wm_host_resample_pos",
    "wm_workspace_bytes", "wm_reserve", "wm_set_workspace", "wm_missing_name", "wm_share_weights", "wm_forward", "wm_forward_sharded", "wm_rccl_unique_id", "wm_comm_init_rccl",
    "wm_local_group_create", "wm_local_group_destroy", "wm_comm_init_local", "wm_allgather", "wm_profile_enable", "wm_profile_read",
    "wm_op_gemm", "wm_op_gemm_resid_ln", "wm_op_gemm_qkv", "wm_op_attention", "wm_op_layernorm", "wm_op_qkv_post", "wm_op_conv", "wm_op_bilinear",
    "wm_op_linear_f32", "wm_host_to_16", "wm_set_tuning", "wm_op_attention_split", "wm_op_attention_ex", "wm_op_attention_flag_count", "wm_op_gs_splat", "wm_op_conv3x3_up", "wm_depth_to_world", "wm_confidence_mask", "wm_confidence_mask_workspace_bytes", "wm_preprocess_image", "wm_preprocess_image_size",
    "wm_preprocess_image_workspace_bytes", "wm_rasterize_splats", "wm_rasterize_workspace_bytes", "wm_rasterize_splats_backward", "wm_rasterize_backward_workspace_bytes", "wm_prune_gs", "wm_prune_gs_workspace_bytes", "wm_op_up_conv_n32", "wm_op_conv3x3_gemm16", "wm_op_conv_ex", "wm_op_upconv3x3_tap", "wm_op_tconv", "wm_op_upconv_gather",
    "wm_depth_edge", "wm_normals_edge", "wm_point_filter_mask_workspace_bytes", "wm_point_filter_mask",
    "wm_op_im2col", "wm_op_im2col7", "wm_op_dino_tokens", "wm_op_vgt_special", "wm_op_gemm_rowmap", "wm_op_gemm_convt", "wm_op_layernorm_rows",
    "wm_op_bilinear_add", "wm_op_bilinear16", "wm_op_copy2d", "wm_op_small_attention", "wm_op_adaln", "wm_op_cam_update", "wm_op_cam_matrices",
    "wm_op_linear_f32_ex", "wm_op_dpt_tail", "wm_op_up_conv_n32_tail", "wm_op_dpt_tap_front",
    "wm_photometric_loss_workspace_bytes", "wm_photometric_loss_forward_workspace_bytes", "wm_photometric_loss", "wm_photometric_loss_backward",
    "wm_rasterize_backward_workspace_bytes_ex", "wm_rasterize_splats_backward_ex", "wm_rasterize_means2d",
    "wm_rasterize_backward_workspace_bytes_cam", "wm_rasterize_splats_backward_cam",
    "wm_rasterize_splats_sh", "wm_rasterize_backward_workspace_bytes_sh", "wm_rasterize_splats_backward_sh",
    "wm_rasterize_splats_opt", "wm_rasterize_backward_workspace_bytes_opt", "wm_rasterize_splats_backward_opt",
    "wm_densify_accumulate", "wm_densify_plan_workspace_bytes", "wm_densify_plan", "wm_densify_gather",
    "wm_mcmc_inject_noise", "wm_mcmc_partition_workspace_bytes", "wm_mcmc_partition", "wm_mcmc_relocation", "wm_mcmc_scatter", "wm_mcmc_zero_rows",
    "wm_bilagrid_slice", "wm_bilagrid_slice_backward_workspace_bytes", "wm_bilagrid_slice_backward", "wm_bilagrid_tv_workspace_bytes",
    "wm_bilagrid_tv", "wm_bilagrid_tv_backward",
    "wm_appearance_forward", "wm_appearance_backward_workspace_bytes", "wm_appearance_backward",
    "wm_depth_loss_workspace_bytes", "wm_depth_loss", "wm_depth_loss_backward", "wm_project_depth_points",
    "wm_export_splats_workspace_bytes", "wm_export_splats_payload_bytes", "wm_export_splats", "wm_pack_rows_workspace_bytes", "wm_pack_rows",
    "wm_colmap_select_workspace_bytes", "wm_colmap_select", "wm_colmap_gather", "wm_colmap_pack_workspace_bytes", "wm_colmap_pack",
    "wm_pack_point_ply_workspace_bytes", "wm_pack_point_ply",
    "wm_knn_workspace_bytes", "wm_knn",
    "wm_nearest_build_workspace_bytes", "wm_nearest_build", "wm_nearest_query_workspace_bytes", "wm_nearest_query",
    "wm_cloud_stats_workspace_bytes", "wm_cloud_stats", "wm_umeyama_workspace_bytes", "wm_umeyama",
    "wm_gs_effect_spread_workspace_bytes", "wm_gs_effect_spread", "wm_video_frames_workspace_bytes", "wm_video_frames", "wm_turbo_lut",
    "wm_image_mesh_workspace_bytes", "wm_image_mesh_count", "wm_image_mesh_pack", "wm_glb_pack_points_workspace_bytes", "wm_glb_pack_points",
    "wm_masked_percentile_neighbours_workspace_bytes", "wm_masked_percentile_neighbours",
    "wm_eval_frame_workspace_bytes", "wm_eval_frame", "wm_color_correct_workspace_bytes", "wm_color_correct",
    "wm_confidence_mask_count", "wm_in_frustum_mask",
    "wm_compress_minmax_workspace_bytes", "wm_compress_minmax", "wm_compress_quantise", "wm_compress_dequantise", "wm_gather_rows",
    "wm_kmeans_l1_workspace_bytes", "wm_kmeans_l1", "wm_kmeans_l1_assign", "wm_grid_order_workspace_bytes", "wm_grid_order",
]

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    # restype is set only where it is not ctypes' default c_int (wm_status / int); tests/test_cabi_cpu.py holds every entry's
    # argtypes and restype against its prototype in include/wm_hip.h
    L.wm_create.argtypes = [C.POINTER(wm_config), i32, C.POINTER(vp)]
    L.wm_destroy.argtypes = [vp]
    L.wm_destroy.restype = None
    L.wm_last_error.argtypes = [vp]
    L.wm_last_error.restype = C.c_char_p
    L.wm_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), i32]
    L.wm_finalize_weights.argtypes = [vp, C.POINTER(i32)]
    L.wm_host_resample_pos.argtypes = [vp, i32, i32, i32, i32, vp]
    L.wm_host_resample_pos.restype = None
    L.wm_workspace_bytes.argtypes = [vp, i32, i32, i32, i32]
    L.wm_workspace_bytes.restype = C.c_size_t
    L.wm_reserve.argtypes = [vp, i32, i32, i32, i32]
    L.wm_set_workspace.argtypes = [vp, vp, C.c_size_t]
    L.wm_share_weights.argtypes = [vp, vp]
    L.wm_missing_name.argtypes = [vp, i32]
    L.wm_missing_name.restype = C.c_char_p
    L.wm_forward.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(wm_outputs), vp]
    L.wm_forward_sharded.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_int32),
                                     C.POINTER(wm_outputs), vp]
    L.wm_rccl_unique_id.argtypes = [vp]
    L.wm_comm_init_rccl.argtypes = [vp, vp, i32, i32]
    L.wm_local_group_create.argtypes = [i32]
    L.wm_local_group_create.restype = vp
    L.wm_local_group_destroy.argtypes = [vp]
    L.wm_local_group_destroy.restype = None
    L.wm_comm_init_local.argtypes = [vp, vp, i32]
    L.wm_allgather.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.wm_profile_enable.argtypes = [vp, i32]
    L.wm_profile_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.wm_op_gemm.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.wm_op_gemm_resid_ln.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, C.POINTER(i32), vp]
    L.wm_op_gemm_qkv.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    L.wm_op_attention.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.wm_op_attention_split.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_op_attention_ex.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.wm_op_attention_flag_count.argtypes = [i32, i32, i32]
    L.wm_op_attention_flag_count.restype = C.c_size_t
    L.wm_op_layernorm.argtypes = [vp, vp, vp, vp, i32, i32, f32, i32, i32, vp]
    L.wm_op_qkv_post.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    L.wm_op_conv.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_bilinear.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_linear_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.wm_host_to_16.argtypes = [vp, vp, C.c_size_t, i32]
    L.wm_host_to_16.restype = None
    L.wm_depth_to_world.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp]
    L.wm_confidence_mask_workspace_bytes.argtypes = [C.c_size_t]
    L.wm_confidence_mask_workspace_bytes.restype = C.c_size_t
    L.wm_confidence_mask.argtypes = [vp, C.c_size_t, C.c_double, vp, vp, C.c_size_t, vp]
    L.wm_confidence_mask_count.argtypes = [vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t, vp]
    L.wm_in_frustum_mask.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    L.wm_depth_edge.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, i32, f32, vp, vp]
    L.wm_normals_edge.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, vp, vp]
    L.wm_point_filter_mask_workspace_bytes.argtypes = [i32, i32, i32]
    L.wm_point_filter_mask_workspace_bytes.restype = C.c_size_t
    L.wm_point_filter_mask.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_double, i32, C.c_double, f32, vp, vp, vp, C.c_size_t, vp]
    L.wm_op_up_conv_n32.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    L.wm_op_conv3x3_gemm16.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    L.wm_op_conv3x3_up.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_op_conv_ex.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_upconv3x3_tap.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_op_tconv.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.wm_op_upconv_gather.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.wm_prune_gs_workspace_bytes.argtypes = [C.c_size_t]
    L.wm_prune_gs_workspace_bytes.restype = C.c_size_t
    L.wm_prune_gs.argtypes = [vp, vp, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp, vp, C.POINTER(i32), vp, C.c_size_t, vp]
    L.wm_rasterize_workspace_bytes.argtypes = [i32, i32, i32, i32, C.c_size_t]
    L.wm_rasterize_workspace_bytes.restype = C.c_size_t
    L.wm_rasterize_splats.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t,
                                      C.POINTER(C.c_ulonglong), vp]
    L.wm_rasterize_backward_workspace_bytes.argtypes = [i32, i32, i32, i32, C.c_size_t]
    L.wm_rasterize_backward_workspace_bytes.restype = C.c_size_t
    L.wm_rasterize_splats_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                               vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_rasterize_backward_workspace_bytes_ex.argtypes = [i32, i32, i32, i32, C.c_size_t, i32]
    L.wm_rasterize_backward_workspace_bytes_ex.restype = C.c_size_t
    L.wm_rasterize_splats_backward_ex.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, C.c_size_t, vp]
    L.wm_rasterize_backward_workspace_bytes_cam.argtypes = [i32, i32, i32, i32, C.c_size_t, i32]
    L.wm_rasterize_backward_workspace_bytes_cam.restype = C.c_size_t
    L.wm_rasterize_splats_backward_cam.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                   vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.c_size_t, vp]
    L.wm_rasterize_splats_sh.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t,
                                         C.POINTER(C.c_ulonglong), vp]
    L.wm_rasterize_backward_workspace_bytes_sh.argtypes = [i32, i32, i32, i32, C.c_size_t, i32, i32, i32]
    L.wm_rasterize_backward_workspace_bytes_sh.restype = C.c_size_t
    L.wm_rasterize_splats_backward_sh.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, i32, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, C.c_size_t, vp]
    optp = C.POINTER(wm_raster_options)
    L.wm_rasterize_splats_opt.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, i32, optp, vp, vp, vp, vp, vp, C.c_size_t,
                                          C.c_size_t, C.POINTER(C.c_ulonglong), vp]
    L.wm_rasterize_backward_workspace_bytes_opt.argtypes = [i32, i32, i32, i32, C.c_size_t, i32, i32, i32, i32, i32]
    L.wm_rasterize_backward_workspace_bytes_opt.restype = C.c_size_t
    L.wm_rasterize_splats_backward_opt.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, i32, optp, vp, C.c_size_t, C.c_size_t,
                                                   C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_rasterize_means2d.argtypes = [vp, C.c_size_t, i32, i32, i32, i32, C.c_size_t, vp, vp, vp]
    L.wm_densify_accumulate.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.wm_densify_plan_workspace_bytes.argtypes = [C.c_size_t]
    L.wm_densify_plan_workspace_bytes.restype = C.c_size_t
    L.wm_densify_plan.argtypes = [vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, f32, f32, i32, i32, i32, vp, vp, vp, C.POINTER(i32 * 4), vp,
                                  C.c_size_t, vp]
    L.wm_densify_gather.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.wm_mcmc_inject_noise.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp]
    L.wm_mcmc_partition_workspace_bytes.argtypes = [C.c_size_t]
    L.wm_mcmc_partition_workspace_bytes.restype = C.c_size_t
    L.wm_mcmc_partition.argtypes = [vp, vp, i32, f32, vp, vp, C.POINTER(i32 * 2), vp, C.c_size_t, vp]
    L.wm_mcmc_relocation.argtypes = [vp, vp, vp, i32, i32, f32, vp, vp, vp, vp]
    L.wm_mcmc_scatter.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp]
    L.wm_mcmc_zero_rows.argtypes = [vp, i32, i32, vp, i32, vp]
    i64p = C.POINTER(C.c_int64)
    L.wm_photometric_loss_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.wm_photometric_loss_workspace_bytes.restype = C.c_size_t
    L.wm_photometric_loss_forward_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.wm_photometric_loss_forward_workspace_bytes.restype = C.c_size_t
    L.wm_photometric_loss.argtypes = [vp, i64p, vp, i64p, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.c_size_t, vp]
    L.wm_photometric_loss_backward.argtypes = [vp, i64p, vp, i64p, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_bilagrid_slice.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp]
    L.wm_bilagrid_slice_backward_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32]
    L.wm_bilagrid_slice_backward_workspace_bytes.restype = C.c_size_t
    L.wm_bilagrid_slice_backward.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_bilagrid_tv_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    L.wm_bilagrid_tv_workspace_bytes.restype = C.c_size_t
    L.wm_bilagrid_tv.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, C.c_size_t, vp]
    L.wm_bilagrid_tv_backward.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_depth_loss_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    L.wm_depth_loss_workspace_bytes.restype = C.c_size_t
    L.wm_depth_loss.argtypes = [vp, i64p, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, C.c_size_t, vp]
    L.wm_depth_loss_backward.argtypes = [i32, i32, i32, vp, i32, vp, vp, i64p, vp, C.c_size_t, vp]
    L.wm_project_depth_points.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    i64 = C.c_int64
    L.wm_export_splats_workspace_bytes.argtypes = [i64, i32, i32]
    L.wm_export_splats_workspace_bytes.restype = C.c_size_t
    L.wm_export_splats_payload_bytes.argtypes = [i64, i32, i32]
    L.wm_export_splats_payload_bytes.restype = C.c_size_t
    L.wm_export_splats.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, f32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(i32), vp]
    L.wm_pack_rows_workspace_bytes.argtypes = [i64]
    L.wm_pack_rows_workspace_bytes.restype = C.c_size_t
    L.wm_pack_rows.argtypes = [C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32, vp, i64, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(i32), vp]
    f64 = C.c_double
    L.wm_colmap_select_workspace_bytes.argtypes = [i32, i32, i32]
    L.wm_colmap_select_workspace_bytes.restype = C.c_size_t
    L.wm_colmap_select.argtypes = [vp, vp, i32, i32, i32, f32, f64, vp, C.c_size_t, i64p, i64p, vp]
    L.wm_colmap_gather.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, f64, f64, vp, C.c_size_t, i64, vp, vp, vp, vp]
    L.wm_colmap_pack_workspace_bytes.argtypes = [i64, i32]
    L.wm_colmap_pack_workspace_bytes.restype = C.c_size_t
    L.wm_colmap_pack.argtypes = [vp, vp, vp, vp, i32, i64, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.wm_pack_point_ply_workspace_bytes.argtypes = [i64]
    L.wm_pack_point_ply_workspace_bytes.restype = C.c_size_t
    L.wm_pack_point_ply.argtypes = [vp, vp, vp, i32, i64, vp, C.c_size_t, vp, C.c_size_t, i64p, vp]
    L.wm_knn_workspace_bytes.argtypes = [i64, i32]
    L.wm_knn_workspace_bytes.restype = C.c_size_t
    L.wm_knn.argtypes = [vp, i64, i32, vp, C.c_size_t, vp, vp, vp, vp]
    L.wm_nearest_build_workspace_bytes.argtypes = [i64]
    L.wm_nearest_build_workspace_bytes.restype = C.c_size_t
    L.wm_nearest_build.argtypes = [vp, i64, vp, C.c_size_t, vp, vp]
    L.wm_nearest_query_workspace_bytes.argtypes = [i64]
    L.wm_nearest_query_workspace_bytes.restype = C.c_size_t
    L.wm_nearest_query.argtypes = [vp, C.c_size_t, i64, vp, i64, vp, C.c_size_t, vp, vp, vp]
    L.wm_cloud_stats_workspace_bytes.argtypes = [i64]
    L.wm_cloud_stats_workspace_bytes.restype = C.c_size_t
    L.wm_cloud_stats.argtypes = [vp, vp, i64, vp, vp, i64, C.POINTER(f32), i32, vp, C.c_size_t, vp, vp]
    L.wm_umeyama_workspace_bytes.argtypes = [i64]
    L.wm_umeyama_workspace_bytes.restype = C.c_size_t
    L.wm_umeyama.argtypes = [vp, vp, vp, i64, i32, vp, C.c_size_t, vp, vp]
    L.wm_gs_effect_spread_workspace_bytes.argtypes = [i64]
    L.wm_gs_effect_spread_workspace_bytes.restype = C.c_size_t
    L.wm_gs_effect_spread.argtypes = [vp, vp, vp, vp, vp, i64, f64, i32, vp, f32, i32, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_video_frames_workspace_bytes.argtypes = [i32, i32, i32]
    L.wm_video_frames_workspace_bytes.restype = C.c_size_t
    L.wm_video_frames.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_turbo_lut.argtypes = [vp]
    L.wm_turbo_lut.restype = None
    L.wm_image_mesh_workspace_bytes.argtypes = [i32, i32, i32]
    L.wm_image_mesh_workspace_bytes.restype = C.c_size_t
    L.wm_image_mesh_count.argtypes = [vp, i32, i32, i32, vp, C.c_size_t, i64p, i64p, vp]
    L.wm_image_mesh_pack.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, C.c_size_t, i64, i64, vp, vp, vp, vp, vp, vp]
    L.wm_glb_pack_points_workspace_bytes.argtypes = [i64]
    L.wm_glb_pack_points_workspace_bytes.restype = C.c_size_t
    L.wm_glb_pack_points.argtypes = [vp, vp, vp, i64, vp, C.c_size_t, vp, C.c_size_t, i64p, vp, vp]
    L.wm_masked_percentile_neighbours_workspace_bytes.argtypes = [i64, i32]
    L.wm_masked_percentile_neighbours_workspace_bytes.restype = C.c_size_t
    L.wm_masked_percentile_neighbours.argtypes = [vp, vp, i64, C.POINTER(f64), i32, vp, C.c_size_t, vp, vp, vp]
    L.wm_eval_frame_workspace_bytes.argtypes = [i32, i32, i32]
    L.wm_eval_frame_workspace_bytes.restype = C.c_size_t
    L.wm_eval_frame.argtypes = [vp, i64p, vp, i64p, i32, i32, i32, i32, f64, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.wm_color_correct_workspace_bytes.argtypes = [i32, i64]
    L.wm_color_correct_workspace_bytes.restype = C.c_size_t
    L.wm_color_correct.argtypes = [vp, vp, i32, i64, i32, f64, vp, vp, C.c_size_t, vp]
    L.wm_compress_minmax_workspace_bytes.argtypes = [i64, i32]
    L.wm_compress_minmax_workspace_bytes.restype = C.c_size_t
    L.wm_compress_minmax.argtypes = [vp, i64, i32, vp, C.c_size_t, vp, vp, vp]
    L.wm_compress_quantise.argtypes = [vp, i64, i32, vp, i32, vp, vp, vp]
    L.wm_compress_dequantise.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp]
    L.wm_gather_rows.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), i32, vp, i64, vp]
    L.wm_kmeans_l1_workspace_bytes.argtypes = [i64, i32, i32]
    L.wm_kmeans_l1_workspace_bytes.restype = C.c_size_t
    L.wm_kmeans_l1.argtypes = [vp, i64, i32, i32, vp, i32, f64, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.wm_kmeans_l1_assign.argtypes = [vp, i64, i32, vp, i32, vp, vp, vp]
    L.wm_grid_order_workspace_bytes.argtypes = [i32]
    L.wm_grid_order_workspace_bytes.restype = C.c_size_t
    L.wm_grid_order.argtypes = [vp, i32, vp, C.c_size_t, vp, vp, vp]
    L.wm_appearance_forward.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.wm_appearance_backward_workspace_bytes.argtypes = [i32, i32]
    L.wm_appearance_backward_workspace_bytes.restype = C.c_size_t
    L.wm_appearance_backward.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                         C.c_size_t, vp]
    L.wm_preprocess_image_size.argtypes = [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.wm_preprocess_image_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.wm_preprocess_image_workspace_bytes.restype = C.c_size_t
    L.wm_preprocess_image.argtypes = [vp, i32, i32, i32, i32, vp, vp, C.c_size_t, vp]
    L.wm_op_im2col.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_im2col7.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp]
    L.wm_op_dino_tokens.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.wm_op_vgt_special.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_gemm_rowmap.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_gemm_convt.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_layernorm_rows.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.wm_op_bilinear_add.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_op_bilinear16.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wm_op_copy2d.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.wm_op_small_attention.argtypes = [vp, vp, i32, i32, i32, vp]
    L.wm_op_adaln.argtypes = [vp, vp, vp, i32, i32, f32, vp]
    L.wm_op_cam_update.argtypes = [vp, vp, vp, i32, i32, vp]
    L.wm_op_cam_matrices.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.wm_op_linear_f32_ex.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp]
    L.wm_op_gs_splat.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.wm_op_dpt_tail.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, i32, i32, vp]
    L.wm_op_up_conv_n32_tail.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.wm_op_dpt_tap_front.argtypes = [i32, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, i32, i32,
                                      C.POINTER(vp), C.POINTER(i32), vp]
    L.wm_set_tuning.argtypes = [C.c_char_p, i32]
    _lib = L
    return L


def make_config(cfg, backbone_dtype="bf16", head_dtype="f16") -> wm_config:
    c = wm_config()
    for k in ("img_size", "patch_size", "embed_dim", "gs_dim", "depth", "num_heads", "mlp_ratio",
              "num_register_tokens", "dino_depth", "dino_heads", "cam_trunk_depth", "cam_heads", "cam_steps",
              "dpt_features"):
        setattr(c, k, int(getattr(cfg, k)))
    for k in ("enable_cond", "enable_cam", "enable_pts", "enable_depth", "enable_norm", "enable_gs"):
        setattr(c, k, 1 if getattr(cfg, k) else 0)
    c.rope_freq = float(cfg.rope_freq)
    for i in range(4):
        c.intermediate_idxs[i] = int(cfg.intermediate_idxs[i])
        c.dpt_out_channels[i] = int(cfg.dpt_out_channels[i])
    c.backbone_dtype = WM_DT[backbone_dtype]
    c.head_dtype = WM_DT[head_dtype]
    return c


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev):
    """The current torch stream of device `dev`, as the entries take it."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check(st, name):
    """Raise for a non-zero status of the entry `name`."""
    if st != 0:
        raise RuntimeError(f"{name} failed with status {st}")
