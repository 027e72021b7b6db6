"""Bilateral-grid appearance correction of the reference's "Post 3DGS Optimization" (gsplat's simple_trainer_worldmirror.py with
--use_bilateral_grid: :758-770 builds the grids, :812-814 slices every render, :555-570 adds the total-variation term), over the C ABI
entries ``wm_bilagrid_slice`` / ``wm_bilagrid_slice_backward`` / ``wm_bilagrid_tv`` / ``wm_bilagrid_tv_backward`` (hand-written HIP,
csrc/bilagrid.hip).  The three names the trainer imports from examples/lib_bilagrid.py (or from the CUDA-only fused_bilagrid package):

    self.bil_grids = BilateralGrid(len(self.trainset), grid_X=16, grid_Y=16, grid_W=8)
    colors = slice(self.bil_grids, grid_xy, colors, image_ids)["rgb"]
    tvloss = 10 * total_variation_loss(self.bil_grids.grids)

What differs from lib_bilagrid.py, on purpose: the sliced [..., 3, 4] matrices are never materialised, so the dict ``slice`` returns has
no "rgb_affine_mats"; ``BilateralGrid.forward`` (which returns those matrices) and 2-D inputs (one grid index per sample) raise
NotImplementedError; the CP-decomposed 4-D grid (``BilateralGridCP4D``, ``slice4d``: they need tensorly) is not part of this library.
``color_correct``, the evaluation-time colour fit, lives in metrics.py (``wm_color_correct``) and is re-exported here under the name
lib_bilagrid gives it.  No CPU fallback: tensors must live on a HIP device."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream
from .metrics import color_correct  # noqa: F401

MAX_CELLS = 4096      # include/wm_hip.h: L * Hg * Wg the grid gradient keeps in registers
MAX_AXIS = 1024


def _slice_forward(grids, idx, xy, rgb):
    """grids [G,12,L,Hg,Wg], idx int32 [B], xy [B,n,2], rgb [B,n,3]: contiguous fp32 / int32 on one HIP device -> out [B,n,3]"""
    G, _, L, Hg, Wg = (int(x) for x in grids.shape)
    B, n = int(rgb.shape[0]), int(rgb.shape[1])
    out = torch.empty_like(rgb)
    with torch.cuda.device(rgb.device):
        st = _lib.lib().wm_bilagrid_slice(ptr(grids), G, L, Hg, Wg, ptr(idx), ptr(xy), ptr(rgb), B, n, ptr(out), stream(rgb.device))
    check(st, "wm_bilagrid_slice")
    return out


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, rgb, xy, idx):
        ctx.save_for_backward(grids, rgb, xy, idx)
        return _slice_forward(grids, idx, xy, rgb)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_out):
        L_ = _lib.lib()
        grids, rgb, xy, idx = ctx.saved_tensors
        G, _, L, Hg, Wg = (int(x) for x in grids.shape)
        B, n = int(rgb.shape[0]), int(rgb.shape[1])
        dev = rgb.device
        v_out = v_out.to(torch.float32).contiguous()
        want_g, want_rgb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        v_grids = torch.empty_like(grids) if want_g else None
        v_rgb = torch.empty_like(rgb) if want_rgb else None
        need = L_.wm_bilagrid_slice_backward_workspace_bytes(G, L, Hg, Wg, B, n) if want_g else 0
        ws = torch.empty(max(need, 1), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            st = L_.wm_bilagrid_slice_backward(ptr(grids), G, L, Hg, Wg, ptr(idx), ptr(xy), ptr(rgb), B, n, ptr(v_out),
                                               ptr(v_grids) if want_g else None, ptr(v_rgb) if want_rgb else None, ptr(ws), ws.numel(), stream(dev))
        check(st, "wm_bilagrid_slice_backward")
        return v_grids, v_rgb, None, None        # xy: the trainer's constant meshgrid, no gradient


def _row_indices(grid_idx, B, G, dev):
    """grid_idx as the reference takes it ((..., 1): row b uses grid_idx[b, 0, ...]), a plain [B] tensor, or ints -> int32 [B] on dev.
    Values the host can see without a synchronisation are checked here; the kernels refuse the rest (NaN rows)."""
    if not torch.is_tensor(grid_idx):
        grid_idx = torch.as_tensor(grid_idx)
    if grid_idx.dtype.is_floating_point or grid_idx.dtype == torch.bool:
        raise TypeError(f"grid_idx must hold integers, got {grid_idx.dtype}")
    if grid_idx.dim() == 0 or grid_idx.shape[0] != B:
        raise ValueError(f"grid_idx must have one leading entry per row ({B}), got shape {tuple(grid_idx.shape)}")
    rows = grid_idx.reshape(B, -1)[:, 0]
    if rows.device.type == "cpu":
        bad = [int(v) for v in rows.tolist() if not 0 <= int(v) < G]
        if bad:
            raise IndexError(f"grid index {bad[0]} is out of range for {G} grids")
    return rows.to(device=dev, dtype=torch.int32).contiguous()


def slice(bil_grids, xy, rgb, grid_idx):
    """lib_bilagrid.slice for 3-D [B,n,.] and 4-D [B,h,w,.] inputs: every sample of row b is corrected by grid ``grid_idx[b, 0, ...]``
    looked up at (x, y, grey(rgb)).  -> {"rgb": tensor of rgb's shape and dtype}; there is no "rgb_affine_mats" (the matrices are not
    materialised).  Differentiable with respect to rgb and bil_grids.grids; xy gets no gradient.  grid_idx is read on the device: no
    torch.unique, no host synchronisation; a device index outside [0, num) gives a NaN row and no gradient from it, a CPU tensor or
    ints with such a value raise IndexError."""
    grids = bil_grids.grids if isinstance(bil_grids, nn.Module) else bil_grids
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"grids must be [G, 12, L, Hg, Wg], got {tuple(grids.shape)}")
    if rgb.dim() == 2:
        raise NotImplementedError("slice with 2-D inputs (one grid index per sample) is not built: pass [B, n, .] or [B, h, w, .] rows, "
                                  "each row naming one grid")
    if rgb.dim() not in (3, 4) or xy.dim() != rgb.dim():
        raise ValueError(f"xy and rgb must both be [B, n, .] or [B, h, w, .], got {tuple(xy.shape)} and {tuple(rgb.shape)}")
    if rgb.shape[-1] != 3 or xy.shape[-1] != 2 or xy.shape[:-1] != rgb.shape[:-1]:
        raise ValueError(f"xy must be [..., 2] and rgb [..., 3] over the same samples, got {tuple(xy.shape)} and {tuple(rgb.shape)}")
    if rgb.numel() == 0:
        raise ValueError(f"no samples: rgb is {tuple(rgb.shape)}")
    if grids.device.type != "cuda" or rgb.device.type != "cuda" or xy.device.type != "cuda":
        raise RuntimeError("bilateral-grid slicing runs in libwm_hip.so on the GPU: move the grids, xy and rgb to a HIP device")
    if not (grids.device == rgb.device == xy.device):
        raise RuntimeError(f"grids, xy and rgb are on different devices: {grids.device}, {xy.device}, {rgb.device}")
    G, _, L, Hg, Wg = (int(x) for x in grids.shape)
    if L * Hg * Wg > MAX_CELLS or max(L, Hg, Wg) > MAX_AXIS:
        raise NotImplementedError(f"a bilateral grid of {Wg} x {Hg} x {L} cells is beyond what the grid gradient kernel holds "
                                  f"({MAX_CELLS} cells, {MAX_AXIS} per axis); there is no slower path")
    B = int(rgb.shape[0])
    idx = _row_indices(grid_idx, B, G, rgb.device)
    shape, dtype = rgb.shape, rgb.dtype
    g32 = grids.to(torch.float32).contiguous()
    c32 = rgb.to(torch.float32).reshape(B, -1, 3).contiguous()
    xy32 = xy.detach().to(torch.float32).reshape(B, -1, 2).contiguous()
    if torch.is_grad_enabled() and (g32.requires_grad or c32.requires_grad):
        out = _Slice.apply(g32, c32, xy32, idx)
    else:
        out = _slice_forward(g32.detach(), idx, xy32, c32.detach())
    return {"rgb": out.reshape(shape).to(dtype)}


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _tv_forward(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, Ch, L, H, W = (int(v) for v in x.shape)
        g = g.to(torch.float32).contiguous()          # a device scalar: no host sync
        v_x = torch.empty_like(x)
        with torch.cuda.device(x.device):
            st = _lib.lib().wm_bilagrid_tv_backward(ptr(x), B, Ch, L, H, W, ptr(g), ptr(v_x), stream(x.device))
        check(st, "wm_bilagrid_tv_backward")
        return v_x


def _tv_forward(x):
    L_ = _lib.lib()
    B, Ch, L, H, W = (int(v) for v in x.shape)
    out = torch.empty((), device=x.device, dtype=torch.float32)
    ws = torch.empty(max(L_.wm_bilagrid_tv_workspace_bytes(B, Ch, L, H, W), 1), device=x.device, dtype=torch.uint8)
    with torch.cuda.device(x.device):
        st = L_.wm_bilagrid_tv(ptr(x), B, Ch, L, H, W, ptr(out), ptr(ws), ws.numel(), stream(x.device))
    check(st, "wm_bilagrid_tv")
    return out


def total_variation_loss(x):
    """lib_bilagrid.total_variation_loss for 5-D x [B,C,L,H,W] (the grids): a 0-d tensor, fused, with backward."""
    if x.dim() != 5:
        raise NotImplementedError(f"total_variation_loss is built for 5-D [B, C, L, H, W] tensors (the bilateral grids), got {x.dim()}-D")
    if x.numel() == 0:
        raise ValueError(f"empty tensor: {tuple(x.shape)}")
    if x.device.type != "cuda":
        raise RuntimeError("total_variation_loss runs in libwm_hip.so on the GPU: move the tensor to a HIP device")
    x32 = x.to(torch.float32).contiguous()
    out = _TotalVariation.apply(x32) if torch.is_grad_enabled() and x32.requires_grad else _tv_forward(x32.detach())
    return out.to(x.dtype)


class BilateralGrid(nn.Module):
    """lib_bilagrid.BilateralGrid: ``num`` grids [num, 12, grid_W, grid_Y, grid_X], each cell the 3 x 4 matrix [I | 0]."""

    def __init__(self, num, grid_X=16, grid_Y=16, grid_W=8):
        super().__init__()
        self.grid_width = grid_X
        self.grid_height = grid_Y
        self.grid_guidance = grid_W
        cell = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32)
        self.grids = nn.Parameter(cell.reshape(1, 12, 1, 1, 1).repeat(num, 1, grid_W, grid_Y, grid_X))

    def tv_loss(self):
        return total_variation_loss(self.grids)

    def forward(self, grid_xy, rgb, idx=None):
        raise NotImplementedError("BilateralGrid.forward returns the sliced [..., 3, 4] matrices, which this library never materialises: "
                                  "call slice(bil_grids, xy, rgb, grid_idx)['rgb']")
