"""Torch restatement of the novel-view path's arithmetic (no GPU needed), the yardstick of tests/test_nvs_cpu.py, tests/test_nvs_gpu.py,
tools/gen_golden_nvs.py and tools/bench_nvs.py.

in_frustum_mask restates the reference's algorithm (src/models/utils/frustum.py:26-89) step by step, intermediates of shape
[b, v1, v2, h, w, 3] included, in the dtype of its depth input; marginal_pixels marks the pixels whose threshold decisions sit too
close to their thresholds to be compared across arithmetic orders; filter_indices and translation_scale restate
rasterization.py:248-299 and :194-202."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK_SCENES = ("a", "b", "c", "d")                     # (B, V1, V2, H, W) = (2,3,2,37,45), (1,2,3,19,70), (1,1,1,5,7), (1,1,2,16,16)
HAND_SCENES = ("hand_split", "hand_nan")
MARGIN = 2.0 ** -10                                     # px for the frustum bounds (64 fp32 ulps at 128 px), depth units for the match
MAX_MARGINAL = 1e-3                                     # a recipe scene may hold at most this share of marginal pixels


def load(name):
    return dict(np.load(os.path.join(GOLD, f"nvs_{name}.npz"), allow_pickle=False))


def project(depth_1, K1, c2w_1, K2, c2w_2):
    """frustum.py:48-55: (points_2d [b,v1,v2,h,w,2], z [b,v1,v2,h,w]) of every target pixel in every context view"""
    b, v1, h, w = depth_1.shape
    dt, dev = depth_1.dtype, depth_1.device
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt, device=dev), torch.arange(w, dtype=dt, device=dev), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)                                       # [h,w,3]
    cam = torch.einsum("bvij,hwj->bvhwi", torch.linalg.inv(K1), pix) * depth_1[..., None]     # :102-117
    cam1 = torch.cat([cam, torch.ones_like(cam[..., :1])], -1)
    world = torch.einsum("bvij,bvhwj->bvhwi", c2w_1, cam1)[..., :3]                            # :120-133
    world1 = torch.cat([world, torch.ones_like(world[..., :1])], -1)
    cam2 = torch.einsum("buij,bvhwj->bvuhwi", torch.linalg.inv(c2w_2), world1)[..., :3]       # :152-165
    n = cam2 / cam2[..., -1:]                                                                  # :97-99, no z > 0 test
    p2d = torch.einsum("buij,bvuhwj->bvuhwi", K2, n)[..., :2]                                  # :136-149
    return p2d, cam2[..., 2]


def sample(depth_2, p2d):
    """frustum.py:74-83: grid_sample(align_corners=False) of depth_2[b, j] at the projected points, [b,v1,v2,h,w]"""
    b, v1, v2, h, w, _ = p2d.shape
    g = torch.stack([p2d[..., 0] / w, p2d[..., 1] / h], -1) * 2 - 1
    out = torch.empty(p2d.shape[:-1], dtype=p2d.dtype, device=p2d.device)
    for bb in range(b):
        for j in range(v2):
            img = depth_2[bb, j][None, None].expand(v1, 1, h, w)
            out[bb, :, j] = F.grid_sample(img, g[bb, :, j], align_corners=False)[:, 0]
    return out


def in_frustum_mask(depth_1, K1, c2w_1, depth_2, K2, c2w_2):
    """frustum.py:26-89 -> bool [b,v1,h,w]"""
    _, _, h, w = depth_1.shape
    p2d, z = project(depth_1, K1, c2w_1, K2, c2w_2)
    inside = ((p2d[..., 0] > 0) & (p2d[..., 0] < w) & (p2d[..., 1] > 0) & (p2d[..., 1] < h)).any(dim=2)
    match = torch.isclose(z, sample(depth_2, p2d), atol=1e-1).any(dim=2)
    return inside & (depth_1 > 1e-6) & match


def marginal_pixels(depth_1, K1, c2w_1, depth_2, K2, c2w_2):
    """bool [b,v1,h,w] in fp64: a pixel any of whose decisions lies within MARGIN of its threshold (a projected coordinate of 0, w or h;
    |z - s| of 0.1 + 1e-5 |s|) or whose depth lies within 1e-7 of 1e-6.  A NaN is on neither side and marks nothing."""
    d1, K1, c2w_1, d2, K2, c2w_2 = (t.double() for t in (depth_1, K1, c2w_1, depth_2, K2, c2w_2))
    _, _, h, w = d1.shape
    p2d, z = project(d1, K1, c2w_1, K2, c2w_2)
    px, py = p2d[..., 0], p2d[..., 1]
    near = (px.abs() < MARGIN) | ((px - w).abs() < MARGIN) | (py.abs() < MARGIN) | ((py - h).abs() < MARGIN)
    s = sample(d2, p2d)
    near |= ((z - s).abs() - (0.1 + 1e-5 * s.abs())).abs() < MARGIN
    return near.any(dim=2) | ((d1 - 1e-6).abs() < 1e-7)


def scene_tensors(z, dtype=torch.float32, device="cpu"):
    return tuple(torch.from_numpy(z[k]).to(device=device, dtype=dtype) for k in ("depth_1", "K1", "c2w_1", "depth_2", "K2", "c2w_2"))


def assert_mask(got, z, what=""):
    """got (bool array [b,v1,h,w]) equals the reference's fp64 mask on every non-marginal pixel"""
    got = np.asarray(got).astype(bool)
    free = z["marginal"].astype(bool)
    bad = (got != z["mask64"].astype(bool)) & ~free
    assert got.shape == z["mask64"].shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist())


# ---- confidence filter (rasterization.py:248-299) with this project's two fixed rules
def keep_count(n, p, max_gaussians):
    keep = int(math.ceil(n * (100.0 - p) / 100.0)) if p > 0 else n
    return max(1, min(max_gaussians, keep))


def filter_indices(conf, p, max_gaussians):
    """conf [B,N] (numpy) -> [B,K] kept indices in ascending order: the K highest of conf' (conf <= 1e-5 -> -inf), NaN above +inf,
    ties at the K-th value to the lowest indices"""
    conf = np.asarray(conf, np.float32)
    B, N = conf.shape
    K = keep_count(N, p, max_gaussians)
    out = np.empty((B, K), np.int64)
    for b in range(B):
        c = conf[b].astype(np.float64)
        with np.errstate(invalid="ignore"):
            key = np.where(conf[b] <= np.float32(1e-5), -np.inf, c)
        rank = np.where(np.isnan(c), 2.0, np.where(np.isposinf(key), 1.0, 0.0))               # NaN > +inf > the rest
        order = np.lexsort((np.arange(N), -np.where(rank > 0, 0.0, key), -rank))             # last key first: rank, then value, then index
        out[b] = np.sort(order[:K])
    return out


# ---- rasterization.py:194-202
def translation_scale(ctx_c2w, all_c2w, S):
    return ctx_c2w[:, :S, :3, 3].mean(dim=(1, 2), keepdim=True) / (all_c2w[:, :S, :3, 3].mean(dim=(1, 2), keepdim=True) + 1e-6)
