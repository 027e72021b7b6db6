"""The trainer's splat initialisation: ``create_splats_with_optimizers`` of submodules/gsplat/examples/simple_trainer_worldmirror.py:280-402
with its helpers ``knn`` and ``rgb_to_sh`` (submodules/gsplat/examples/utils.py:141-150).

The reference's ``knn`` copies the cloud to the host and runs scikit-learn's kd-tree; here the search runs on the device in libwm_hip.so
(csrc/knn.hip) and the cloud never leaves it.  There is no CPU path: a tensor that is not on a HIP device raises RuntimeError.

The search is exact (the Morton-sorted cell structure only prunes) and deterministic.  Its worst case: a query costs the points of its
3 x 3 x 3 cells, so a cloud whose dense part is smaller than 2^-21 of its bounding box (one cell) degrades towards every query scanning that
part, and a far outlier scans up to the whole cloud; many far outliers cost N each.  Both stay correct.

The optimisers are ``torch.optim.Adam``; ``sparse_grad`` and ``visible_adam`` (SparseAdam, SelectiveAdam) are not built."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .exporter import splats_from_ply

SH_C0 = 0.28209479177387814
KNN_MAX_K = 16


def knn(x: torch.Tensor, K: int = 4, return_indices: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """utils.py:141-145 on the device: x [N,3] on a HIP device -> the distances [N,K] from every point to its K nearest points of x, itself
    included (column 0 is 0), ascending, in x's dtype; with return_indices also their rows [N,K] int64.  Computed in fp32 (another dtype
    is converted first): sqrt(dx^2 + dy^2 + dz^2) on the coordinate differences, duplicates give exact zeros.  Indices are ordered by
    row where distances tie.  1 <= K <= 16, K <= N; a NaN or infinite coordinate raises ValueError (scikit-learn refuses it too).  The call
    synchronises once, to learn whether the input was finite."""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError("knn runs in libwm_hip.so on the GPU: pass a tensor on a HIP device")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"knn: x must be [N, 3], got {tuple(x.shape)}")
    if int(K) != K or not 1 <= int(K) <= KNN_MAX_K:
        raise ValueError(f"knn: K must be an integer in 1..{KNN_MAX_K}, got {K!r}")
    K, N = int(K), int(x.shape[0])
    if K > N:
        raise ValueError(f"knn: K = {K} neighbours of a cloud of {N} points")
    if x.device.type != "cuda":
        raise RuntimeError("knn runs in libwm_hip.so on the GPU: move the tensor to a HIP device")
    dev = x.device
    pts = x.detach().to(torch.float32).contiguous()
    L = _lib.lib()
    ws_bytes = L.wm_knn_workspace_bytes(N, K)
    if ws_bytes == 0:
        raise ValueError(f"knn: {N} points with K = {K} are outside what the library searches (N < 2^31)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    dist = torch.empty((N, K), device=dev, dtype=torch.float32)
    idx = torch.empty((N, K), device=dev, dtype=torch.int32) if return_indices else None
    flag = torch.empty(1, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(L.wm_knn(ptr(pts), N, K, ptr(ws), ws_bytes, ptr(dist), ptr(idx), ptr(flag), stream(dev)), "wm_knn")
    if int(flag.item()):          # the one synchronisation
        raise ValueError("knn: x holds a NaN or infinite coordinate")
    dist = dist.to(x.dtype) if x.dtype.is_floating_point else dist
    return (dist, idx.to(torch.int64)) if return_indices else dist


def rgb_to_sh(rgb: torch.Tensor) -> torch.Tensor:
    """utils.py:148-150: (rgb - 0.5) / C0"""
    return (rgb - 0.5) / SH_C0


def knn_scales(points: torch.Tensor, init_scale: float = 1.0) -> torch.Tensor:
    """simple_trainer_worldmirror.py:334-337: the log-scale [N,3] of every Gaussian from the root mean square distance to its 3 nearest
    neighbours, log(sqrt(mean(knn(points, 4)[:, 1:]^2)) * init_scale), the same value on the three axes.  A point with three duplicates
    gets -inf, as in the reference: nothing is clamped."""
    dist2_avg = (knn(points, 4)[:, 1:] ** 2).mean(dim=-1)
    dist_avg = torch.sqrt(dist2_avg)
    return torch.log(dist_avg * init_scale).unsqueeze(-1).repeat(1, 3)


def _device_tensor(a, device) -> torch.Tensor:
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device)


def create_splats_with_optimizers(
    parser,
    init_type: str = "sfm",
    init_num_pts: int = 100_000,
    init_extent: float = 3.0,
    init_opacity: float = 0.1,
    init_scale: float = 1.0,
    means_lr: float = 1.6e-4,
    scales_lr: float = 5e-3,
    opacities_lr: float = 5e-2,
    quats_lr: float = 1e-3,
    sh0_lr: float = 2.5e-3,
    shN_lr: float = 2.5e-3 / 20,
    scene_scale: float = 1.0,
    sh_degree: int = 3,
    sparse_grad: bool = False,
    visible_adam: bool = False,
    batch_size: int = 1,
    feature_dim: Optional[int] = None,
    device: str = "cuda",
    world_rank: int = 0,
    world_size: int = 1,
    ply_path: Optional[str] = None,
    generator: Optional[torch.Generator] = None,
) -> Tuple[torch.nn.ParameterDict, Dict[str, torch.optim.Optimizer]]:
    """simple_trainer_worldmirror.py:280-402 with the reference's arguments and defaults, everything on ``device``.

    parser: what load_colmap returns (host numpy, or after .to(device)); only ``points`` [P,3] and ``points_rgb`` [P,3] u8 are read, and
    it may be None for init_type "random" and "ffgs".  generator: a generator of ``device`` for the random draws (quats, the random
    cloud, features); None is the device's default generator.
      sfm     means = parser.points, colours = parser.points_rgb / 255
      random  means = init_extent * scene_scale * (rand * 2 - 1), colours = rand, init_num_pts of them
      ffgs    splats_from_ply(ply_path): scales, quats and opacities as stored, the colours are already SH coefficients
    For sfm and random the scales are knn_scales(means, init_scale) of the FULL cloud (duplicate points give -inf, as in the reference),
    quats are rand and opacities logit(init_opacity); then every tensor keeps its rows world_rank::world_size.  feature_dim None gives
    sh0 [N,1,3] and shN [N,(sh_degree+1)^2-1,3]; otherwise features [N,feature_dim] (rand) and colors = logit(colours).

    Returns the ParameterDict and {name: torch.optim.Adam} with, for BS = batch_size * world_size, lr * sqrt(BS) (means: means_lr *
    scene_scale), eps = 1e-15 / sqrt(BS), betas = (1 - BS * 0.1, 1 - BS * 0.001) and the parameter's name in the param group.
    sparse_grad=True and visible_adam=True raise NotImplementedError.  Every argument is checked before the first GPU call."""
    if init_type not in ("sfm", "random", "ffgs"):
        raise ValueError("Please specify a correct init_type: sfm, random, or ffgs")
    if init_type == "ffgs" and ply_path is None:
        raise ValueError("ply_path must be provided when using ffgs initialization")
    if sparse_grad:
        raise NotImplementedError("create_splats_with_optimizers: sparse_grad=True (torch.optim.SparseAdam) is not built")
    if visible_adam:
        raise NotImplementedError("create_splats_with_optimizers: visible_adam=True (SelectiveAdam) is not built")
    if init_type == "sfm" and (parser is None or not hasattr(parser, "points") or not hasattr(parser, "points_rgb")):
        raise ValueError("create_splats_with_optimizers: init_type='sfm' needs a parser with points and points_rgb")
    world_rank, world_size, batch_size, sh_degree = int(world_rank), int(world_size), int(batch_size), int(sh_degree)
    if world_size < 1 or not 0 <= world_rank < world_size:
        raise ValueError(f"world_rank {world_rank} is outside world_size {world_size}")
    if batch_size < 1 or sh_degree < 0:
        raise ValueError(f"batch_size must be >= 1 and sh_degree >= 0, got {batch_size} and {sh_degree}")
    if init_type == "random" and int(init_num_pts) < 4:
        raise ValueError(f"init_num_pts must be at least 4 (three neighbours size a Gaussian), got {init_num_pts}")
    if feature_dim is not None and int(feature_dim) < 1:
        raise ValueError(f"feature_dim must be positive, got {feature_dim}")

    def rand(*shape):
        return torch.rand(shape, device=device, generator=generator)

    if init_type == "sfm":
        points = _device_tensor(parser.points, device).float()
        rgbs = (_device_tensor(parser.points_rgb, device).to(torch.float64) / 255.0).float()
        if points.dim() != 2 or points.shape[1] != 3 or tuple(rgbs.shape) != tuple(points.shape):
            raise ValueError(f"parser.points {tuple(points.shape)} and parser.points_rgb {tuple(rgbs.shape)} must both be [P, 3]")
    elif init_type == "random":
        points = init_extent * scene_scale * (rand(int(init_num_pts), 3) * 2 - 1)
        rgbs = rand(int(init_num_pts), 3)
    else:
        ply = splats_from_ply(ply_path, sh_degree=0, opacity="probability", device=device)
        points, rgbs = ply["means"], ply["sh0"][:, 0, :]

    if init_type == "ffgs":
        scales, quats, opacities = ply["scales"], ply["quats"], ply["opacities"]
    else:
        scales = knn_scales(points, init_scale)          # on the full cloud, in front of the split

    points = points[world_rank::world_size]
    rgbs = rgbs[world_rank::world_size]
    scales = scales[world_rank::world_size]
    N = points.shape[0]
    if init_type == "ffgs":
        quats = quats[world_rank::world_size]
        opacities = opacities[world_rank::world_size]
    else:
        quats = rand(N, 4)
        opacities = torch.logit(torch.full((N,), float(init_opacity), device=device))

    params = [
        ("means", points, means_lr * scene_scale),
        ("scales", scales, scales_lr),
        ("quats", quats, quats_lr),
        ("opacities", opacities, opacities_lr),
    ]
    if feature_dim is None:
        colors = torch.zeros((N, (sh_degree + 1) ** 2, 3), device=device)
        colors[:, 0, :] = rgbs if init_type == "ffgs" else rgb_to_sh(rgbs)
        params.append(("sh0", colors[:, :1, :], sh0_lr))
        params.append(("shN", colors[:, 1:, :], shN_lr))
    else:
        params.append(("features", rand(N, int(feature_dim)), sh0_lr))
        params.append(("colors", torch.logit(rgbs), sh0_lr))

    splats = torch.nn.ParameterDict({n: torch.nn.Parameter(v.detach().clone().contiguous()) for n, v, _ in params}).to(device)
    BS = batch_size * world_size
    optimizers = {
        name: torch.optim.Adam(
            [{"params": splats[name], "lr": lr * math.sqrt(BS), "name": name}],
            eps=1e-15 / math.sqrt(BS),
            betas=(1 - BS * (1 - 0.9), 1 - BS * (1 - 0.999)),
        )
        for name, _, lr in params
    }
    return splats, optimizers
