"""The photometric loss of the reference's "Post 3DGS Optimization" (gsplat's simple_trainer_worldmirror.py:785-792) over the C ABI
entries ``wm_photometric_loss`` / ``wm_photometric_loss_backward`` (hand-written HIP, csrc/photoloss.hip):

    l1loss   = F.l1_loss(colors, pixels)
    ssimloss = 1.0 - fused_ssim(colors.permute(0, 3, 1, 2), pixels.permute(0, 3, 1, 2), padding="valid")
    loss     = l1loss * (1.0 - ssim_lambda) + ssimloss * ssim_lambda

``fused_ssim`` keeps the CUDA extension's signature; ``photometric_loss`` is the three lines in one forward and one backward launch
sequence on the channels-last tensors ``Rasterizer.rasterize_splats`` returns.  Differentiable with respect to the first image only
(the extension's rule: the target gets no gradient).  No CPU fallback: tensors must live on a HIP device.

``depth_loss`` is the trainer's ``--depth_loss`` branch (:793-811) over ``wm_depth_loss`` / ``wm_depth_loss_backward`` and
``project_depth_points`` the dataset-side projection that feeds it (examples/datasets/colmap.py:412-433) over
``wm_project_depth_points`` (csrc/depthloss.hip):

    points, depths_gt, valid = project_depth_points(points_world, camtoworlds, Ks, width, height)
    depthloss = depth_loss(renders[..., 3:4], points, depths_gt, valid) * scene_scale
    loss += depthloss * depth_lambda"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream

_PADDING = {"same": 0, "valid": 1}


def _strides(t: torch.Tensor):
    return (C.c_int64 * 4)(*t.stride())


def _check(img1, img2, padding):
    if padding not in _PADDING:
        raise ValueError(f"padding must be 'same' or 'valid', got {padding!r}")
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"img1 and img2 must be [B, C, H, W] of one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if min(img1.shape) < 1:
        raise ValueError(f"empty image: {tuple(img1.shape)}")
    if padding == "valid" and (img1.shape[2] < 11 or img1.shape[3] < 11):
        raise ValueError(f"padding='valid' needs at least 11 x 11 pixels (the cropped map would be empty), got {img1.shape[2]} x {img1.shape[3]}")
    if img1.device.type != "cuda" or img2.device.type != "cuda":
        raise RuntimeError("the photometric loss runs in libwm_hip.so on the GPU: move the images to a HIP device")
    if img1.device != img2.device:
        raise RuntimeError(f"img1 and img2 are on different devices: {img1.device} and {img2.device}")


def _forward(a: torch.Tensor, b: torch.Tensor, valid: int, want_backward: bool):
    """One wm_photometric_loss call on fp32 [B,C,H,W] tensors of any strides -> ssim, l1 (0-d), workspace."""
    L = _lib.lib()
    B, Ch, H, W = (int(x) for x in a.shape)
    dev = a.device
    ssim = torch.empty((), device=dev, dtype=torch.float32)
    l1 = torch.empty((), device=dev, dtype=torch.float32)
    # forward-only: the per-tile partial sums alone, not the three derivative maps
    size = L.wm_photometric_loss_workspace_bytes if want_backward else L.wm_photometric_loss_forward_workspace_bytes
    need = size(B, Ch, H, W)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        st = L.wm_photometric_loss(ptr(a), _strides(a), ptr(b), _strides(b), B, Ch, H, W, valid, 1 if want_backward else 0, ptr(ssim), ptr(l1),
                                   ptr(ws), ws.numel(), stream(dev))
    check(st, "wm_photometric_loss")
    return ssim, l1, ws


class _PhotometricLoss(torch.autograd.Function):
    """(ssim, l1) of one image pair with a backward for img1.  The node owns the forward's workspace (the three derivative maps)
    until its backward has run, as _RasterizeSplats does."""

    @staticmethod
    def forward(ctx, img1, img2, valid):
        a = img1.detach().to(torch.float32)
        if torch.empty_like(a).stride() != a.stride():     # overlapping or gapped view: the gradient is written with a's strides
            a = a.contiguous()
        b = img2.detach().to(torch.float32)
        ssim, l1, ws = _forward(a, b, valid, True)
        ctx.save_for_backward(a, b)
        ctx.ws, ctx.valid, ctx.dtype = ws, valid, img1.dtype
        return ssim, l1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ssim, g_l1):
        L = _lib.lib()
        a, b = ctx.saved_tensors
        dev = a.device
        B, Ch, H, W = (int(x) for x in a.shape)
        zero = torch.zeros((), device=dev)
        g = torch.stack([zero if g_ssim is None else g_ssim, zero if g_l1 is None else g_l1]).to(torch.float32)   # device scalars: no host sync
        grad = torch.empty_like(a)                          # a's strides (forward made sure of it)
        ws = ctx.ws
        with torch.cuda.device(dev):
            st = L.wm_photometric_loss_backward(ptr(a), _strides(a), ptr(b), _strides(b), B, Ch, H, W, ctx.valid, ptr(g[0]), ptr(g[1]), ptr(grad),
                                                ptr(ws), ws.numel(), stream(dev))
        check(st, "wm_photometric_loss_backward")
        return grad.to(ctx.dtype), None, None               # the target: no gradient


def _ssim_l1(img1, img2, padding, train=True) -> Tuple[torch.Tensor, torch.Tensor]:
    _check(img1, img2, padding)
    if train and torch.is_grad_enabled() and img1.requires_grad:
        return _PhotometricLoss.apply(img1, img2, _PADDING[padding])
    ssim, l1, _ = _forward(img1.detach().to(torch.float32), img2.detach().to(torch.float32), _PADDING[padding], False)
    return ssim, l1


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """SSIM of two [B,C,H,W] image batches (any strides) as a 0-d tensor; gradient for img1 only.  train=False, torch.no_grad() or an
    img1 that does not require grad takes the forward-only call (same bits)."""
    return _ssim_l1(img1, img2, padding, train)[0]


def photometric_loss(render: torch.Tensor, target: torch.Tensor, ssim_lambda: float = 0.2,
                     padding: str = "valid") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """render, target: channels-last [..., H, W, C] (what Rasterizer.rasterize_splats returns).  -> (loss, l1, ssim), 0-d tensors, with
    loss = (1 - ssim_lambda) * l1 + ssim_lambda * (1 - ssim).  Gradient for render only."""
    if render.shape != target.shape or render.dim() < 3:
        raise ValueError(f"render and target must be [..., H, W, C] of one shape, got {tuple(render.shape)} and {tuple(target.shape)}")
    H, W, Ch = render.shape[-3:]
    a = render.reshape(-1, H, W, Ch).permute(0, 3, 1, 2)
    b = target.reshape(-1, H, W, Ch).permute(0, 3, 1, 2)
    ssim, l1 = _ssim_l1(a, b, padding)
    loss = l1 * (1.0 - ssim_lambda) + (1.0 - ssim) * ssim_lambda
    return loss, l1, ssim


def _strides3(t: torch.Tensor):
    return (C.c_int64 * 3)(*t.stride())


def _depth_args(depths, points, depths_gt, valid):
    """checks, then -> the fp32 [C,H,W] view of depths (copied only when it is not fp32), points, depths_gt, valid as the entries take them"""
    if depths.dim() == 4 and depths.shape[-1] == 1:
        d = depths[..., 0]
    elif depths.dim() == 3:
        d = depths
    else:
        raise ValueError(f"depths must be [C, H, W, 1] or [C, H, W], got {tuple(depths.shape)}")
    Cn, H, W = (int(x) for x in d.shape)
    if Cn < 1 or H < 2 or W < 2:
        raise ValueError(f"depths needs at least one camera and 2 x 2 pixels (the coordinates are normalised with W - 1 and H - 1), got {tuple(d.shape)}")
    if points.dim() != 3 or points.shape[0] != Cn or points.shape[2] != 2:
        raise ValueError(f"points must be [C, M, 2] with C = {Cn}, got {tuple(points.shape)}")
    M = int(points.shape[1])
    if tuple(depths_gt.shape) != (Cn, M):
        raise ValueError(f"depths_gt must be [C, M] = [{Cn}, {M}], got {tuple(depths_gt.shape)}")
    if valid is not None and tuple(valid.shape) != (Cn, M):
        raise ValueError(f"valid must be [C, M] = [{Cn}, {M}], got {tuple(valid.shape)}")
    tensors = [depths, points, depths_gt] + ([] if valid is None else [valid])
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("the depth loss runs in libwm_hip.so on the GPU: move the tensors to a HIP device")
    if any(t.device != depths.device for t in tensors):
        raise RuntimeError("depths, points, depths_gt and valid are on different devices")
    d = d.detach().to(torch.float32)
    p = points.detach().to(torch.float32).contiguous()
    gt = depths_gt.detach().to(torch.float32).contiguous()
    v = None if valid is None else (valid.detach() != 0).contiguous()          # bool: one byte per row, 0 / 1
    return d, p, gt, v, M


def _depth_forward(d, p, gt, v, M, want_backward: bool):
    L = _lib.lib()
    Cn, H, W = (int(x) for x in d.shape)
    dev = d.device
    out = torch.empty((), device=dev, dtype=torch.float32)
    ws = torch.empty(L.wm_depth_loss_workspace_bytes(Cn, H, W, M, 1 if want_backward else 0), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        st = L.wm_depth_loss(ptr(d), _strides3(d), Cn, H, W, ptr(p), ptr(gt), ptr(v), M, 1 if want_backward else 0, ptr(out), ptr(ws), ws.numel(),
                             stream(dev))
    check(st, "wm_depth_loss")
    return out, ws


class _DepthLoss(torch.autograd.Function):
    """The sparse disparity loss with a backward for the depth image.  The node owns the forward's workspace (the valid count and one
    coefficient per row) until its backward has run."""

    @staticmethod
    def forward(ctx, depths, d, p, gt, v, M):
        out, ws = _depth_forward(d, p, gt, v, M, True)
        ctx.save_for_backward(p)                            # the backward reads the points and the workspace, not the image again
        ctx.ws, ctx.M, ctx.dtype, ctx.shape, ctx.geom = ws, M, depths.dtype, depths.shape, tuple(int(x) for x in d.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        L = _lib.lib()
        p, = ctx.saved_tensors
        dev = p.device
        Cn, H, W = ctx.geom
        g = g_out.detach().to(torch.float32).reshape(())                       # a device scalar: no host sync
        grad = torch.empty((Cn, H, W), device=dev, dtype=torch.float32)        # dense, whatever the strides of the image were
        ws = ctx.ws
        with torch.cuda.device(dev):
            st = L.wm_depth_loss_backward(Cn, H, W, ptr(p), ctx.M, ptr(g), ptr(grad), _strides3(grad), ptr(ws), ws.numel(), stream(dev))
        check(st, "wm_depth_loss_backward")
        return grad.reshape(ctx.shape).to(ctx.dtype), None, None, None, None, None


def depth_loss(depths: torch.Tensor, points: torch.Tensor, depths_gt: torch.Tensor, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The trainer's depth loss in disparity space, as a 0-d tensor: depths [C,H,W,1] or [C,H,W] (any strides: ``renders[..., 3:4]`` of an
    RGB+ED render is read in place; fp16 / bf16 are cast) is sampled bilinearly at the pixel coordinates points [C,M,2] (pixel centres at
    integers, zero outside the image), disp = 1 / d where d > 0 else 0, and the result is the mean of |disp - 1 / depths_gt| over the
    rows valid [C,M] flags (None: all of them; a flagged-out row may hold anything, NaN included).  No valid row: NaN, and a zero
    gradient.  Gradient for depths only, in its dtype; under torch.no_grad() or for depths that do not require grad the forward-only
    call runs (same bits).  Multiply by scene_scale and depth_lambda yourself, as the trainer does."""
    d, p, gt, v, M = _depth_args(depths, points, depths_gt, valid)
    if torch.is_grad_enabled() and depths.requires_grad:
        return _DepthLoss.apply(depths, d, p, gt, v, M)
    return _depth_forward(d, p, gt, v, M, False)[0]


def project_depth_points(points_world: torch.Tensor, camtoworlds: torch.Tensor, Ks: torch.Tensor, width: int, height: int,
                         visible: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """World points [P,3] into every camera (camtoworlds [C,4,4], rigid; Ks [C,3,3]) -> points [C,P,2] in pixels, depths [C,P] (camera-space
    z), valid [C,P] bool = visible & (0 <= x < width) & (0 <= y < height) & (z > 0).  visible [C,P] stands for the dataset's per-image
    point lists (None: every point in every camera).  Nothing is compacted: hand valid to depth_loss.  No gradients."""
    if points_world.dim() != 2 or points_world.shape[1] != 3:
        raise ValueError(f"points_world must be [P, 3], got {tuple(points_world.shape)}")
    if camtoworlds.dim() != 3 or tuple(camtoworlds.shape[1:]) != (4, 4) or camtoworlds.shape[0] < 1:
        raise ValueError(f"camtoworlds must be [C, 4, 4], got {tuple(camtoworlds.shape)}")
    Cn, P = int(camtoworlds.shape[0]), int(points_world.shape[0])
    if tuple(Ks.shape) != (Cn, 3, 3):
        raise ValueError(f"Ks must be [C, 3, 3] = [{Cn}, 3, 3], got {tuple(Ks.shape)}")
    if visible is not None and tuple(visible.shape) != (Cn, P):
        raise ValueError(f"visible must be [C, P] = [{Cn}, {P}], got {tuple(visible.shape)}")
    if int(width) < 1 or int(height) < 1:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    tensors = [points_world, camtoworlds, Ks] + ([] if visible is None else [visible])
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("the projection runs in libwm_hip.so on the GPU: move the tensors to a HIP device")
    if any(t.device != points_world.device for t in tensors):
        raise RuntimeError("points_world, camtoworlds, Ks and visible are on different devices")
    L = _lib.lib()
    dev = points_world.device
    pw = points_world.detach().to(torch.float32).contiguous()
    c2w = camtoworlds.detach().to(torch.float32).contiguous()
    K = Ks.detach().to(torch.float32).contiguous()
    vis = None if visible is None else (visible.detach() != 0).contiguous()
    points = torch.empty((Cn, P, 2), device=dev, dtype=torch.float32)
    depths = torch.empty((Cn, P), device=dev, dtype=torch.float32)
    valid = torch.empty((Cn, P), device=dev, dtype=torch.bool)
    with torch.cuda.device(dev):
        st = L.wm_project_depth_points(ptr(pw), ptr(c2w), ptr(K), ptr(vis), Cn, P, int(width), int(height), ptr(points), ptr(depths), ptr(valid),
                                       stream(dev))
    check(st, "wm_project_depth_points")
    return points, depths, valid
