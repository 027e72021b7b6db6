"""The photometric loss of the reference's "Post 3DGS Optimization" (gsplat's simple_trainer_worldmirror.py:785-792) over the C ABI
entries ``wm_photometric_loss`` / ``wm_photometric_loss_backward`` (hand-written HIP, csrc/photoloss.hip):

    l1loss   = F.l1_loss(colors, pixels)
    ssimloss = 1.0 - fused_ssim(colors.permute(0, 3, 1, 2), pixels.permute(0, 3, 1, 2), padding="valid")
    loss     = l1loss * (1.0 - ssim_lambda) + ssimloss * ssim_lambda

``fused_ssim`` keeps the CUDA extension's signature; ``photometric_loss`` is the three lines in one forward and one backward launch
sequence on the channels-last tensors ``Rasterizer.rasterize_splats`` returns.  Differentiable with respect to the first image only
(the extension's rule: the target gets no gradient).  No CPU fallback: tensors must live on a HIP device."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch

from . import _lib

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
        st = L.wm_photometric_loss(C.c_void_p(a.data_ptr()), _strides(a), C.c_void_p(b.data_ptr()), _strides(b), B, Ch, H, W, valid,
                                   1 if want_backward else 0, C.c_void_p(ssim.data_ptr()), C.c_void_p(l1.data_ptr()),
                                   C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if st != 0:
        raise RuntimeError(f"wm_photometric_loss failed with status {st}")
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
            st = L.wm_photometric_loss_backward(C.c_void_p(a.data_ptr()), _strides(a), C.c_void_p(b.data_ptr()), _strides(b), B, Ch, H, W,
                                                ctx.valid, C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 4), C.c_void_p(grad.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if st != 0:
            raise RuntimeError(f"wm_photometric_loss_backward failed with status {st}")
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
