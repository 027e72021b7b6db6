"""Novel-view path (the reference's README table "Novel view synthesis"): the target-view validity mask, the confidence filter in front
of prune_gs and the render step of GaussianSplatRenderer.

Reference: src/models/utils/frustum.py (calculate_unprojected_mask :7-23, calculate_in_frustum_mask :26-89) and
src/models/models/rasterization.py (render :166-246, apply_confidence_filter :248-299, prepare_splats :469-484).  The mask is one HIP
kernel (csrc/frustum.hip), the filter's select is the exact radix select of csrc/select.hip followed by the stable row packer of
csrc/export.hip, the rendering is the package's rasteriser; torch carries device memory, the two small matrix inverses (fp64) and the
concatenation of the rendered chunks.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream

SPLAT_KEYS = ("means", "quats", "scales", "opacities", "sh", "weights")   # rasterization.py:282


# ------------------------------------------------------------------------------------------------ validity mask (frustum.py)
def _check_set(depth, intrinsics, c2w, name):
    if depth.dim() != 4:
        raise ValueError(f"depth_{name}: expected [b, v, h, w], got {tuple(depth.shape)}")
    b, v = depth.shape[:2]
    if tuple(intrinsics.shape) != (b, v, 3, 3):
        raise ValueError(f"intrinsics_{name}: expected {(b, v, 3, 3)}, got {tuple(intrinsics.shape)}")
    if tuple(c2w.shape) != (b, v, 4, 4):
        raise ValueError(f"c2w_{name}: expected {(b, v, 4, 4)}, got {tuple(c2w.shape)}")


def frustum_matrices(intrinsics_1: torch.Tensor, c2w_1: torch.Tensor, c2w_2: torch.Tensor):
    """What the kernel takes instead of the reference's per-pixel inverses, in fp64 on the host (a few 4x4): K1^-1 [b,v1,3,3] and
    rows 0..2 of c2w_2[b,j]^-1 c2w_1[b,i] [b,v1,v2,3,4].  The reference keeps xyz of the world point and appends a new 1
    (frustum.py:131-133, 163), so the last row of c2w_1 counts as (0, 0, 0, 1) whatever it holds."""
    kinv = torch.linalg.inv(intrinsics_1.detach().to("cpu", torch.float64))
    a1 = c2w_1.detach().to("cpu", torch.float64).clone()
    a1[..., 3, :] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    w2c_2 = torch.linalg.inv(c2w_2.detach().to("cpu", torch.float64))
    rel = torch.einsum("bjrk,bikc->bijrc", w2c_2, a1)[..., :3, :]
    return kinv, rel


def calculate_in_frustum_mask(depth_1: torch.Tensor, intrinsics_1: torch.Tensor, c2w_1: torch.Tensor, depth_2: torch.Tensor,
                              intrinsics_2: torch.Tensor, c2w_2: torch.Tensor) -> torch.Tensor:
    """Drop-in for frustum.py:26-89: which pixels of the first set of views (depth_1 [b,v1,h,w], intrinsics_1 [b,v1,3,3], c2w_1
    [b,v1,4,4]) have a matching pixel in any view of the second set ([b,v2,...])?  Returns bool [b,v1,h,w] (what the reference's code
    returns; its docstring names another shape).  GPU tensors only; the inverses are taken once in fp64, the per-pixel arithmetic is fp32
    in one kernel (csrc/frustum.hip) without any [b,v1,v2,h,w] intermediate."""
    _check_set(depth_1, intrinsics_1, c2w_1, "1")
    _check_set(depth_2, intrinsics_2, c2w_2, "2")
    b, v1, h, w = depth_1.shape
    v2 = depth_2.shape[1]
    if depth_2.shape[0] != b or tuple(depth_2.shape[2:]) != (h, w):
        raise ValueError(f"depth_2 {tuple(depth_2.shape)} does not match depth_1 {tuple(depth_1.shape)} in batch, height and width")
    if min(b, v1, v2, h, w) < 1:
        raise ValueError(f"empty input: depth_1 {tuple(depth_1.shape)}, depth_2 {tuple(depth_2.shape)}")
    dev = depth_1.device
    if dev.type != "cuda" or depth_2.device != dev:
        raise RuntimeError("calculate_in_frustum_mask runs in libwm_hip.so: both depth tensors must be on one HIP device")
    kinv, rel = frustum_matrices(intrinsics_1, c2w_1, c2w_2)
    d1, d2 = depth_1.detach().contiguous().float(), depth_2.detach().contiguous().float()
    kinv, rel = kinv.to(dev, torch.float32).contiguous(), rel.to(dev, torch.float32).contiguous()
    k2 = intrinsics_2.detach().to(dev, torch.float32).contiguous()
    mask = torch.empty((b, v1, h, w), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        st = _lib.lib().wm_in_frustum_mask(ptr(d1), ptr(d2), ptr(kinv), ptr(rel), ptr(k2), b, v1, v2, h, w, ptr(mask), stream(dev))
    check(st, "wm_in_frustum_mask")
    return mask.bool()


def check_context_nums(context_nums, n_views: int, allow_all: bool = False) -> int:
    """context_nums as an int with 1 <= S < n_views (<= with allow_all); anything else is a ValueError"""
    if isinstance(context_nums, bool) or not isinstance(context_nums, int):
        raise ValueError(f"context_nums must be an int, got {type(context_nums).__name__}")
    hi = n_views if allow_all else n_views - 1
    if not 1 <= context_nums <= hi:
        raise ValueError(f"context_nums = {context_nums} is outside 1..{hi} for {n_views} views")
    return context_nums


def calculate_unprojected_mask(views: Dict[str, torch.Tensor], context_nums: int) -> torch.Tensor:
    """Drop-in for frustum.py:7-23: the loss mask of the target views views[...][:, context_nums:] against the context views
    [:, :context_nums], from views["depthmap"] [b,n,h,w], ["camera_intrinsics"] [b,n,>=3,>=3] (cut to 3x3 as the reference does) and
    ["camera_pose"] [b,n,4,4] (camera to world).  Returns bool [b, n - context_nums, h, w]."""
    for k in ("depthmap", "camera_intrinsics", "camera_pose"):
        if k not in views:
            raise ValueError(f"views has no {k!r}")
    depth, K, c2w = views["depthmap"], views["camera_intrinsics"], views["camera_pose"]
    if depth.dim() != 4:
        raise ValueError(f"views['depthmap']: expected [b, n, h, w], got {tuple(depth.shape)}")
    if K.dim() != 4 or K.shape[-2] < 3 or K.shape[-1] < 3:
        raise ValueError(f"views['camera_intrinsics']: expected [b, n, 3, 3], got {tuple(K.shape)}")
    S = check_context_nums(context_nums, int(depth.shape[1]))
    K = K[..., :3, :3]
    return calculate_in_frustum_mask(depth[:, S:], K[:, S:], c2w[:, S:], depth[:, :S], K[:, :S], c2w[:, :S])


# ------------------------------------------------------------------------------------------------ confidence filter (rasterization.py:248-299)
def filter_keep_count(n: int, conf_threshold_percent: float, max_gaussians: int) -> int:
    """rasterization.py:272-276: K = max(1, min(max_gaussians, ceil(N (100 - p) / 100))) (p <= 0: N), the arithmetic in double"""
    keep = int(math.ceil(n * (100.0 - conf_threshold_percent) / 100.0)) if conf_threshold_percent > 0 else n
    return max(1, min(int(max_gaussians), keep))


def _pack(x: torch.Tensor, keep: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """the kept rows of x [n, ...] in input order (wm_pack_rows: prefix sums, no atomics)"""
    from .exporter import _pack_rows
    row = x[0].numel() if x.dim() > 1 else 1
    out, kept = _pack_rows([(x, c, row, 0) for c in range(row)], keep, n, x.device)
    if kept != k:
        raise RuntimeError(f"confidence filter: {kept} rows kept where the select chose {k}")
    return out[:k * row * 4].view(torch.float32).reshape((k,) + tuple(x.shape[1:]))


def apply_confidence_filter(splats: Dict[str, torch.Tensor], conf: Optional[torch.Tensor], conf_threshold_percent: float = 30.0,
                            max_gaussians: int = 5_000_000) -> Dict[str, torch.Tensor]:
    """rasterization.py:248-299: per batch element keep the K highest confidences (filter_keep_count; conf <= 1e-5 counts as -inf) of
    splats [B, N, ...] with conf [B, ...] flattening to [B, N].  Two rules the reference's topk(sorted=False) leaves open are fixed:
    ties at the K-th value go to the lowest indices and NaN ranks above +inf (wm_confidence_mask's rules), and the kept rows stay in
    input order (prune_gs sums in row order).  Keys outside means, quats, scales, opacities, sh, weights pass through untouched."""
    if conf is None:
        return splats
    means = splats["means"]
    if means.dim() != 3:
        raise ValueError(f"splats['means']: expected [B, N, 3], got {tuple(means.shape)}")
    B, N = int(means.shape[0]), int(means.shape[1])
    if conf.shape[0] != B or conf.numel() != B * N:
        raise ValueError(f"confidences {tuple(conf.shape)} do not flatten to the splats' [B, N] = {(B, N)}")
    if N < 1:
        raise ValueError("confidence filter: no splats")
    dev = means.device
    if dev.type != "cuda" or conf.device != dev:
        raise RuntimeError("apply_confidence_filter runs in libwm_hip.so: the splats and their confidences must be on one HIP device")
    K = filter_keep_count(N, conf_threshold_percent, max_gaussians)
    L = _lib.lib()
    c = conf.detach().reshape(B, N).contiguous().float()
    wsb = L.wm_confidence_mask_workspace_bytes(N)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    keep = torch.empty((B, N), device=dev, dtype=torch.uint8)
    out = {k: ([] if k in SPLAT_KEYS else v) for k, v in splats.items()}
    for b in range(B):
        with torch.cuda.device(dev):
            check(L.wm_confidence_mask_count(ptr(c[b]), N, K, ptr(keep[b]), ptr(ws), wsb, stream(dev)), "wm_confidence_mask_count")
        for k in SPLAT_KEYS:
            if k in splats:
                out[k].append(_pack(splats[k][b].detach().contiguous().float(), keep[b], N, K))
    for k in SPLAT_KEYS:
        if k in splats:
            out[k] = torch.stack(out[k], 0)
    return out


# ------------------------------------------------------------------------------------------------ render (rasterization.py:166-246)
def translation_scale(context_c2w: torch.Tensor, all_c2w: torch.Tensor, S: int) -> torch.Tensor:
    """rasterization.py:194-202 as written: mean over views and xyz of the context pass's translations over (the same of the all-view
    pass's first S views + 1e-6); [B, 1, 1]"""
    return context_c2w[:, :S, :3, 3].mean(dim=(1, 2), keepdim=True) / (all_c2w[:, :S, :3, 3].mean(dim=(1, 2), keepdim=True) + 1e-6)


@torch.no_grad()
def render(renderer, images: torch.Tensor, predictions: Dict, views: Optional[Dict] = None, context_predictions: Optional[Dict] = None,
           chunk_size: int = 4) -> Dict:
    """GaussianSplatRenderer.render (rasterization.py:166-246) without its first argument gs_feats, which never leaves wm_forward here:
    the splats come from ``predictions`` (a WorldMirror forward over all S + V views of ``images`` [B,S+V,3,H,W] with
    views["context_nums"] = S).  Fills and returns ``predictions`` with rendered_colors [B,S+V,H,W,3], rendered_depths, rendered_alphas
    [B,S+V,H,W,1], gt_colors, rendered_extrinsics (camera to world), rendered_intrinsics, splats and, when V > 0 and views carries
    depthmap, camera_pose and camera_intrinsics, valid_masks [B,V,H,W] (the reference computes the images and drops them; its docstring
    :174-179 names these fields).

    With ``context_predictions`` (the forward over the S context views alone) the translations of all cameras are scaled by
    translation_scale and the splats are rebuilt from predictions["splats_raw"] with means from predictions["gs_depth"][:, :S] and the
    context pass's cameras (:469-484), then filtered and pruned as in the forward."""
    from .geometry import depth_to_world_coords_points
    if images.dim() != 5 or images.shape[2] != 3:
        raise ValueError(f"images: expected [B, S+V, 3, H, W], got {tuple(images.shape)}")
    if not isinstance(chunk_size, int) or chunk_size < 1:
        raise ValueError(f"chunk_size must be a positive int, got {chunk_size!r}")
    B, n_all, _, H, W = (int(x) for x in images.shape)
    S = check_context_nums(views["context_nums"], n_all, allow_all=True) if views is not None and "context_nums" in views else n_all   # :181
    V = n_all - S
    for k in ("camera_poses", "camera_intrs"):
        if k not in predictions or predictions[k].shape[:2] != (B, n_all):
            raise ValueError(f"predictions[{k!r}] must cover the {n_all} views of images")
    c2w = predictions["camera_poses"].detach().to(torch.float32).clone()                                      # :190-192
    Ks = predictions["camera_intrs"].detach().to(torch.float32)
    if context_predictions is not None:
        ctx_c2w = context_predictions["camera_poses"].detach().to(torch.float32)
        if ctx_c2w.shape[:2] != (B, S):
            raise ValueError(f"context_predictions['camera_poses'] {tuple(ctx_c2w.shape)} does not hold the {S} context views")
        c2w[..., :3, 3] = c2w[..., :3, 3] * translation_scale(ctx_c2w, c2w, S)                                # :194-202
        raw = dict(predictions["splats_raw"])
        if raw["means"].shape[:2] != (B, S * H * W):
            raise ValueError("predictions['splats_raw'] does not hold the context views' splats: run the forward with views['context_nums']")
        depth = predictions["gs_depth"][:, :S].reshape(B * S, H, W)                                           # :470-484
        pts, _, _ = depth_to_world_coords_points(depth, ctx_c2w.reshape(B * S, 4, 4), context_predictions["camera_intrs"].reshape(B * S, 3, 3))
        raw["means"] = pts.reshape(B, S * H * W, 3)
        splats = renderer.finish_splats(raw, predictions.get("depth_conf"), S)                                # :211-216
    else:
        splats = predictions["splats"]
    sh = splats["sh"] if "sh" in splats else splats["colors"]
    rc, rd, ra = [], [], []
    for i in range(0, n_all, chunk_size):                                                                     # :221-241
        c, d, a = renderer.rasterizer.rasterize_batches(splats["means"], splats["quats"], splats["scales"], splats["opacities"], sh,
                                                        c2w[:, i:i + chunk_size], Ks[:, i:i + chunk_size], width=W, height=H,
                                                        sh_degree=min(renderer.sh_degree, 0) if "sh" in splats else None)
        rc.append(c); rd.append(d); ra.append(a)
    predictions["rendered_colors"], predictions["rendered_depths"], predictions["rendered_alphas"] = (torch.cat(x, 1) for x in (rc, rd, ra))
    predictions["gt_colors"] = images.permute(0, 1, 3, 4, 2)                                                  # :206
    predictions["rendered_extrinsics"], predictions["rendered_intrinsics"] = c2w, Ks
    predictions["splats"] = splats                                                                            # :244
    if V > 0 and views is not None and all(k in views for k in ("depthmap", "camera_pose", "camera_intrinsics")):
        predictions["valid_masks"] = calculate_unprojected_mask(views, S)
    return predictions
