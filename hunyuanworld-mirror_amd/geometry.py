"""Post-path geometry on the GPU: drop-in for the reference helper the callers run right after
the forward pass (reference: src/models/utils/geometry.py:57-89; infer.py:303, app.py:151)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ptr, stream


def depth_to_world_coords_points(depth_map: Optional[torch.Tensor], extrinsic: torch.Tensor, intrinsic: torch.Tensor,
                                 eps: float = 1e-8) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Same signature and return triple as the reference: (world [B,H,W,3], camera [B,H,W,3], mask [B,H,W] bool);
    ``extrinsic`` is camera-to-world.  Tensors must live on a HIP device (there is no CPU path)."""
    if depth_map is None:
        return None, None, None
    if depth_map.device.type != "cuda":
        raise RuntimeError("depth_to_world_coords_points runs in libwm_hip.so: tensors must be on the GPU")
    B, H, W = depth_map.shape
    d = depth_map.contiguous().float()
    e = extrinsic.to(d.device).contiguous().float()
    k = intrinsic.to(d.device).contiguous().float()
    if e.shape != (B, 4, 4) or k.shape != (B, 3, 3):
        raise ValueError(f"extrinsic {tuple(e.shape)} / intrinsic {tuple(k.shape)} do not match depth {tuple(d.shape)}")
    world = torch.empty(B, H, W, 3, device=d.device)
    cam = torch.empty(B, H, W, 3, device=d.device)
    mask = torch.empty(B, H, W, device=d.device, dtype=torch.uint8)
    if _lib.lib().wm_depth_to_world(ptr(d), ptr(e), ptr(k), ptr(world), ptr(cam), ptr(mask), B, H, W, C.c_float(eps), stream(d.device)) != 0:
        raise RuntimeError("wm_depth_to_world failed")
    return world, cam, mask.bool()


def create_confidence_mask(confidence: torch.Tensor, conf_threshold_percent: float = 30.0) -> torch.Tensor:
    """Drop-in for infer.py:25-59: flat bool mask keeping the top (100 - p) % confidences (conf <= 1e-5 counts as
    -inf).  Exact radix select on the GPU; ties at the threshold value go to the lowest indices."""
    if confidence.device.type != "cuda":
        raise RuntimeError("create_confidence_mask runs in libwm_hip.so: the tensor must be on the GPU")
    c = confidence.contiguous().float().flatten()
    n = c.numel()
    mask = torch.empty(n, device=c.device, dtype=torch.uint8)
    if n == 0:
        return mask.bool()
    L = _lib.lib()
    wsb = L.wm_confidence_mask_workspace_bytes(n)
    ws = torch.empty(wsb, device=c.device, dtype=torch.uint8)
    if L.wm_confidence_mask(ptr(c), n, C.c_double(conf_threshold_percent), ptr(mask), ptr(ws), wsb, stream(c.device)) != 0:
        raise RuntimeError("wm_confidence_mask failed")
    return mask.bool()



# ---- point-cloud filter masks (app.py:172-206; depth_edge / normals_edge: src/utils/geometry.py:374-416 / 472-531) ----

def _views(t: torch.Tensor, name: str, trailing: int = 0):
    """(..., H, W[, C]) -> contiguous fp32 [S, H, W(, C)] view of a GPU tensor and (S, H, W)."""
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} runs in libwm_hip.so: the tensor must be on the GPU")
    if t.dim() < 2 + trailing:
        raise ValueError(f"{name}: expected (..., H, W{', 3' if trailing else ''}), got {tuple(t.shape)}")
    H, W = t.shape[t.dim() - 2 - trailing], t.shape[t.dim() - 1 - trailing]
    S = t.numel() // max(H * W * (t.shape[-1] if trailing else 1), 1) if t.numel() else 0
    return t.contiguous().float(), S, H, W


def _view_mask(mask: Optional[torch.Tensor], shape, device) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    return torch.broadcast_to(mask.to(device=device, dtype=torch.bool), shape).contiguous().view(torch.uint8)


def _check_k(kernel_size: int) -> int:
    if kernel_size not in (3, 5, 7):
        raise ValueError(f"kernel_size must be 3, 5 or 7 (got {kernel_size})")
    return int(kernel_size)


def depth_edge(depth: torch.Tensor, atol: Optional[float] = None, rtol: Optional[float] = None, kernel_size: int = 3,
               mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Drop-in for the reference's depth_edge on GPU tensors: depth (..., H, W), mask broadcastable to it (bool); returns a
    bool tensor of depth's shape.  Windows are clipped at the border; masked-out depths count as -inf."""
    k = _check_k(kernel_size)
    d, S, H, W = _views(depth, "depth_edge")
    out = torch.empty(depth.shape, device=d.device, dtype=torch.uint8)
    if out.numel() == 0:
        return out.bool()
    m = _view_mask(mask, depth.shape, d.device)
    st = _lib.lib().wm_depth_edge(ptr(d), ptr(m), S, H, W, k, int(atol is not None), C.c_float(atol or 0.0), int(rtol is not None),
                                  C.c_float(rtol or 0.0), ptr(out), stream(d.device))
    if st != 0:
        raise RuntimeError(f"wm_depth_edge failed ({st})")
    return out.bool()


def normals_edge(normals: torch.Tensor, tol: float, kernel_size: int = 3, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Drop-in for the reference's normals_edge on GPU tensors: normals (..., H, W, 3), tol in degrees; returns bool (..., H, W).
    With a mask, the reference only accepts a single 2-D view (its np.pad call fails on a batch); here a batched masked call is
    defined as that 2-D call per view, mask broadcastable to (..., H, W).  The mask window keeps the reference's transposed
    orientation (csrc/pointmask.hip, item 1)."""
    k = _check_k(kernel_size)
    if normals.dim() < 3 or normals.shape[-1] != 3:
        raise ValueError(f"normals_edge: expected (..., H, W, 3), got {tuple(normals.shape)}")
    n, S, H, W = _views(normals, "normals_edge", trailing=1)
    out = torch.empty(normals.shape[:-1], device=n.device, dtype=torch.uint8)
    if out.numel() == 0:
        return out.bool()
    m = _view_mask(mask, normals.shape[:-1], n.device)
    st = _lib.lib().wm_normals_edge(ptr(n), ptr(m), S, H, W, k, C.c_double(tol), ptr(out), stream(n.device))
    if st != 0:
        raise RuntimeError(f"wm_normals_edge failed ({st})")
    return out.bool()


def filter_points_mask(depth_conf: torch.Tensor, depth: torch.Tensor, normals: torch.Tensor, confidence_percentile: float = 10,
                       edge_normal_threshold: float = 5.0, edge_depth_threshold: float = 0.03, apply_confidence_mask: bool = True,
                       apply_edge_mask: bool = True, return_thresholds: bool = False):
    """The point-cloud filter mask of app.py:172-206 (run_model) in one fused call: per view,
    conf >= np.quantile(conf, p / 100) (exact order statistics, numpy's linear interpolation in fp32), then
    & ~(depth_edge(rtol) & normals_edge(tol)) with that mask.  Returns [S, H, W] bool (all ones when neither mask applies);
    with ``return_thresholds`` also the per-view quantile thresholds [S] f32 (None without the confidence mask).

    Shapes: depth_conf [S, H, W] or the forward's [1, S, H, W]; depth [S, H, W], [S, H, W, 1] or [1, S, H, W, 1];
    normals [S, H, W, 3] or [1, S, H, W, 3].  GPU tensors only."""
    for t, name in ((depth_conf, "depth_conf"), (depth, "depth"), (normals, "normals")):
        if t.device.type != "cuda":
            raise RuntimeError(f"filter_points_mask runs in libwm_hip.so: {name} must be on the GPU")
    if normals.dim() == 5 and normals.shape[0] == 1:
        normals = normals[0]
    if normals.dim() != 4 or normals.shape[-1] != 3:
        raise ValueError(f"normals: expected [S, H, W, 3] or [1, S, H, W, 3], got {tuple(normals.shape)}")
    S, H, W = normals.shape[:3]
    if depth.dim() == 5 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() == 4 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth_conf.dim() == 4 and depth_conf.shape[0] == 1:
        depth_conf = depth_conf[0]
    if tuple(depth.shape) != (S, H, W) or tuple(depth_conf.shape) != (S, H, W):
        raise ValueError(f"depth {tuple(depth.shape)} / depth_conf {tuple(depth_conf.shape)} do not match normals {tuple(normals.shape)}")
    dev = normals.device
    c, d, n = depth_conf.contiguous().float(), depth.contiguous().float(), normals.contiguous().float()
    out = torch.empty(S, H, W, device=dev, dtype=torch.uint8)
    thr = torch.empty(S, device=dev, dtype=torch.float32) if apply_confidence_mask else None
    if out.numel():
        L = _lib.lib()
        wsb = L.wm_point_filter_mask_workspace_bytes(S, H, W)
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        st = L.wm_point_filter_mask(ptr(c), ptr(d), ptr(n), S, H, W, int(bool(apply_confidence_mask)), C.c_double(confidence_percentile),
                                    int(bool(apply_edge_mask)), C.c_double(edge_normal_threshold), C.c_float(edge_depth_threshold),
                                    ptr(thr), ptr(out), ptr(ws), wsb, stream(dev))
        if st != 0:
            raise RuntimeError(f"wm_point_filter_mask failed ({st})")
    return (out.bool(), thr) if return_thresholds else out.bool()
