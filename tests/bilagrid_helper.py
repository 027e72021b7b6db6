"""A torch restatement of the bilateral-grid slice and of the grids' total variation (what hunyuanworld_mirror_amd.bilagrid fuses),
generic in the dtype: in fp64 it is the reference for the GPU tests, in fp32 their yardstick, and on the GPU in fp32 the torch
composition tools/bench_bilagrid.py times.  Pinned to the reference's own numbers by tests/test_bilagrid_cpu.py.

slice: row b of xy [B,...,2] / rgb [B,...,3] reads grids[idx[b]] ([G,12,L,Hg,Wg]) at (2 (x - .5), 2 (y - .5), 2 grey - 1) with
F.grid_sample (trilinear, align_corners=True, padding_mode="border"); the 12 numbers are a 3 x 4 matrix A, out = A[:, :3] rgb + A[:, 3].
The grey weights are the fp32 values of (.299, .587, .114) in every dtype (the reference keeps them in an fp32 buffer)."""
import numpy as np
import torch
import torch.nn.functional as F


def grey_weights(dtype, device=None):
    return torch.tensor([0.299, 0.587, 0.114], dtype=torch.float32, device=device).to(dtype)


def coords(xy, rgb):
    """-> grid_sample coordinates [B, n, 3] (x, y, z) in [-1, 1] before any clamp"""
    B = rgb.shape[0]
    c = rgb.reshape(B, -1, 3)
    z = (c * grey_weights(c.dtype, c.device)).sum(-1, keepdim=True) * 2.0 - 1.0
    return torch.cat([(xy.reshape(B, -1, 2) - 0.5) * 2.0, z], -1)


def affine(grids, xy, rgb, idx):
    """-> the sliced matrices [B, n, 3, 4]"""
    B = rgb.shape[0]
    p = coords(xy, rgb).reshape(B, 1, 1, -1, 3)
    a = F.grid_sample(grids[idx], p, mode="bilinear", align_corners=True, padding_mode="border")     # [B, 12, 1, 1, n]
    return a.reshape(B, 12, -1).permute(0, 2, 1).reshape(B, -1, 3, 4)


def slice_rgb(grids, xy, rgb, idx):
    A = affine(grids, xy, rgb, idx)
    c = rgb.reshape(rgb.shape[0], -1, 3)
    out = (A[..., :3] * c[:, :, None, :]).sum(-1) + A[..., 3]
    return out.reshape(rgb.shape)


def total_variation(x):
    tv = 0.0
    for ax in range(2, x.dim()):
        n = x.shape[ax]
        d = x.narrow(ax, 1, n - 1) - x.narrow(ax, 0, n - 1)
        tv = tv + (d * d).sum() / max(d[0].numel(), 1)
    return tv / x.shape[0]


def gradients(grids, xy, rgb, idx, v_out, dtype):
    """slice in dtype from (fp32) inputs -> dict(out, v_grids, v_rgb) as CPU tensors of dtype"""
    g = grids.detach().to(dtype).requires_grad_(True)
    c = rgb.detach().to(dtype).requires_grad_(True)
    out = slice_rgb(g, xy.detach().to(dtype), c, idx)
    (out * v_out.to(dtype)).sum().backward()
    return dict(out=out.detach(), v_grids=g.grad, v_rgb=c.grad)


def tv_gradients(x, dtype):
    t = x.detach().to(dtype).requires_grad_(True)
    tv = total_variation(t)
    tv.backward()
    return dict(tv=tv.detach(), v_x=t.grad)


def boundary_margin(grids_shape, xy, rgb):
    """smallest distance, in grid units, of any sample's UNCLAMPED coordinate to a cell boundary (the integers 0 .. size - 1), per axis
    (x, y, z), computed in fp64.  The interpolant has kinks there (and the clamp rule switches at the two ends): closer than fp32
    rounding, and fp32 and fp64 could pick different cells."""
    _, _, L, Hg, Wg = grids_shape
    p = coords(xy.double(), rgb.double()).reshape(-1, 3)
    top = torch.tensor([Wg - 1, Hg - 1, L - 1], dtype=torch.float64)
    u = (p + 1.0) / 2.0 * top
    near = torch.minimum(torch.maximum(u.round(), torch.zeros(3, dtype=torch.float64)), top)
    return [float((u[:, i] - near[:, i]).abs().min()) for i in range(3)]


def z_clamped(grids_shape, rgb):
    """bool [...]: samples whose guidance coordinate lies on or outside the clamp range (fp64)"""
    L = grids_shape[2]
    z = (rgb.double() * grey_weights(torch.float64)).sum(-1) * 2.0 - 1.0
    u = (z + 1.0) / 2.0 * (L - 1)
    return (u <= 0) | (u >= L - 1)


def max_rel(a, b):
    """largest |a - b| relative to the largest |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def load_golden(name):
    """tests/golden/bilagrid_<name>*.npz merged (scene b is split over three files) -> dict of arrays"""
    import glob
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    files = sorted(glob.glob(os.path.join(gold, f"bilagrid_{name}*.npz")))
    assert files, name
    z = {}
    for f in files:
        z.update(np.load(f, allow_pickle=False))
    return z
