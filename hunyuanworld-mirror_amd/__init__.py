"""MI355X-native WorldMirror forward pass (hand-written HIP kernels behind a C ABI)."""
from .config import WMConfig, param_spec  # noqa: F401
from .worldmirror import WorldMirror, extract_priors  # noqa: F401
from .geometry import (create_confidence_mask, depth_edge, depth_to_world_coords_points, filter_points_mask,  # noqa: F401
                       normals_edge)
from .ingest import load_and_preprocess_images, preprocess_rgb  # noqa: F401
from .rasterization import Rasterizer, rasterization  # noqa: F401
from .losses import depth_loss, fused_ssim, photometric_loss, project_depth_points  # noqa: F401
from .bilagrid import BilateralGrid, slice, total_variation_loss  # noqa: F401
from .appearance import AppearanceOptModule  # noqa: F401
from .strategy import DefaultStrategy  # noqa: F401
from .strategy_mcmc import MCMCStrategy  # noqa: F401
from .pose import CameraOptModule  # noqa: F401
from .exporter import export_splats, load_gaussian_ply, process_ply_to_splat, save_gs_ply, splats_from_ply  # noqa: F401
from .colmap import colmap_points_from_depth, load_colmap, save_colmap, save_points_ply, save_scene_ply  # noqa: F401
from .splat_init import create_splats_with_optimizers, knn, knn_scales, rgb_to_sh  # noqa: F401
from .video import (GSEffects, depth_frames, interpolate_trajectory, quaternion_to_rotation_matrix, render_interpolated_frames,  # noqa: F401
                    render_interpolated_video, rgb_frames, rotation_matrix_to_quaternion, slerp_quaternions, wobble_trajectory)
from .metrics import (Evaluator, PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure, color_correct, eval_metrics, psnr,  # noqa: F401
                      ssim)
from .glb import (GLBScene, convert_predictions_to_glb_scene, image_mesh, load_glb, save_camera_params)  # noqa: F401
from .nvs import apply_confidence_filter, calculate_in_frustum_mask, calculate_unprojected_mask  # noqa: F401
from .compression import PngCompression, kmeans_l1, sort_splats  # noqa: F401
from .recon_metrics import (NearestIndex, accuracy_completeness, apply_transform, direction_statistics, evaluate_pointmaps, icp,  # noqa: F401
                            nearest, umeyama)
