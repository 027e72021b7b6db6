"""Appearance optimisation of the reference's "Post 3DGS Optimization": gsplat's ``AppearanceOptModule`` (examples/utils.py:51-114), which
simple_trainer_worldmirror.py builds under ``--app_opt`` (:532-552) and evaluates every step (:603-611), over the C ABI entries
``wm_appearance_forward`` / ``wm_appearance_backward`` (hand-written HIP, csrc/appearance.hip).  The trainer's lines read as they do there:

    self.app_module = AppearanceOptModule(len(self.trainset), feature_dim, app_embed_dim, sh_degree)
    colors = self.app_module(features=self.splats["features"], embed_ids=image_ids, dirs=means[None] - camtoworlds[:, None, :3, 3],
                             sh_degree=sh_degree_to_use)
    colors = torch.sigmoid(colors + self.splats["colors"])          # [C, N, 3] -> rasterization(..., sh_degree=None)

Same parameters under the same names (``embeds.weight``, ``color_head.{0,2,4}.{weight,bias}``): the ``app_module`` entry of a trainer
checkpoint loads as it is.  The forward is one fused kernel (nothing of size [C,N,64] is written), the backward recomputes the
activations and sums the weight gradients in a fixed order, so gradients are identical bits run to run.  ``dirs`` receives its gradient,
which autograd carries on to whatever built it (``means``, ``camtoworlds``).

Built for the trainer's configuration: ``feature_dim=32``, ``embed_dim=16``, ``mlp_width=64``, ``mlp_depth=2``, module ``sh_degree`` 0-3,
call ``sh_degree`` at most the module's.  Anything else raises ``NotImplementedError`` naming the argument.  No CPU fallback: tensors
must live on a HIP device."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream

FEATURE_DIM, EMBED_DIM, MLP_WIDTH, MLP_DEPTH = 32, 16, 64, 2
TILE = 128          # csrc/wm_kernels.h WM_APPEARANCE_TILE: Gaussians per block tile
MAX_BLOCKS = 512    # WM_APPEARANCE_MAX_BLOCKS: the backward's grid is min(ceil(N / TILE), MAX_BLOCKS) blocks


class _Appearance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, dirs, embeds, W1, b1, W2, b2, W3, b3, ids, module_degree, degree):
        """features [N,32], dirs [C,N,3], embeds [n,16] and the six weights: contiguous fp32 on one HIP device; ids int32 [C] or None"""
        ctx.save_for_backward(features, dirs, embeds, W1, b1, W2, b2, W3, b3)
        ctx.ids, ctx.degrees = ids, (module_degree, degree)
        return _forward(features, dirs, embeds, W1, b1, W2, b2, W3, b3, ids, module_degree, degree)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_out):
        L_ = _lib.lib()
        features, dirs, embeds, W1, b1, W2, b2, W3, b3 = ctx.saved_tensors
        ids, (module_degree, degree) = ctx.ids, ctx.degrees
        dev = features.device
        Cn, N = int(dirs.shape[0]), int(dirs.shape[1])
        v_out = v_out.to(torch.float32).contiguous()
        v_features, v_dirs = torch.empty_like(features), torch.empty_like(dirs)
        v_embeds = torch.empty_like(embeds) if ids is not None and ctx.needs_input_grad[2] else None
        grads = [torch.empty_like(t) for t in (W1, b1, W2, b2, W3, b3)]
        ws = torch.empty(max(L_.wm_appearance_backward_workspace_bytes(N, Cn), 1), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            st = L_.wm_appearance_backward(ptr(features), ptr(embeds), int(embeds.shape[0]), ptr(ids), ptr(dirs), ptr(W1), ptr(b1), ptr(W2), ptr(b2),
                                           ptr(W3), ptr(b3), N, Cn, module_degree, degree, ptr(v_out), ptr(v_features), ptr(v_dirs), ptr(v_embeds),
                                           *(ptr(g) for g in grads), ptr(ws), ws.numel(), stream(dev))
        check(st, "wm_appearance_backward")
        return (v_features, v_dirs, v_embeds, *grads, None, None, None)


def _forward(features, dirs, embeds, W1, b1, W2, b2, W3, b3, ids, module_degree, degree):
    Cn, N = int(dirs.shape[0]), int(dirs.shape[1])
    out = torch.empty((Cn, N, 3), device=features.device, dtype=torch.float32)
    with torch.cuda.device(features.device):
        st = _lib.lib().wm_appearance_forward(ptr(features), ptr(embeds), int(embeds.shape[0]), ptr(ids), ptr(dirs), ptr(W1), ptr(b1), ptr(W2), ptr(b2),
                                              ptr(W3), ptr(b3), N, Cn, module_degree, degree, ptr(out), stream(features.device))
    check(st, "wm_appearance_forward")
    return out


class AppearanceOptModule(nn.Module):
    """examples/utils.py AppearanceOptModule: ``embeds`` (n x embed_dim) and ``color_head`` = Linear(embed_dim + feature_dim +
    (sh_degree + 1)^2, width), ReLU, Linear(width, width), ReLU, Linear(width, 3), evaluated per (camera, Gaussian) pair."""

    def __init__(self, n, feature_dim, embed_dim=16, sh_degree=3, mlp_width=64, mlp_depth=2):
        super().__init__()
        for name, got, built in (("feature_dim", feature_dim, FEATURE_DIM), ("embed_dim", embed_dim, EMBED_DIM),
                                 ("mlp_width", mlp_width, MLP_WIDTH), ("mlp_depth", mlp_depth, MLP_DEPTH)):
            if int(got) != built:
                raise NotImplementedError(f"AppearanceOptModule: {name} = {got} is not built (the kernels are written for {name} = {built})")
        if not 0 <= int(sh_degree) <= 3:
            raise NotImplementedError(f"AppearanceOptModule: sh_degree = {sh_degree} is not built (0 to 3 are)")
        self.embed_dim, self.sh_degree = int(embed_dim), int(sh_degree)
        self.embeds = nn.Embedding(n, embed_dim)
        layers = [nn.Linear(embed_dim + feature_dim + (self.sh_degree + 1) ** 2, mlp_width), nn.ReLU(inplace=True)]
        for _ in range(mlp_depth - 1):
            layers += [nn.Linear(mlp_width, mlp_width), nn.ReLU(inplace=True)]
        layers.append(nn.Linear(mlp_width, 3))
        self.color_head = nn.Sequential(*layers)

    def forward(self, features, embed_ids, dirs, sh_degree):
        """features [N,32], embed_ids [C] integers or None (zero embeddings), dirs [C,N,3] (normalised inside), sh_degree <= the module's
        (bands at or above (sh_degree + 1)^2 are zero inputs) -> colours [C,N,3] before the sigmoid, fp32.  An id outside [0, n) raises
        IndexError where the host can see it (a CPU tensor, a list); on the device it reads a zero embedding and receives no gradient."""
        if not 0 <= int(sh_degree) <= self.sh_degree:
            raise NotImplementedError(f"AppearanceOptModule: sh_degree = {sh_degree} at the call, the module was built with {self.sh_degree}")
        if dirs.dim() != 3 or dirs.shape[-1] != 3:
            raise ValueError(f"dirs must be [C, N, 3], got {tuple(dirs.shape)}")
        Cn, N = int(dirs.shape[0]), int(dirs.shape[1])
        if features.dim() != 2 or int(features.shape[0]) != N:
            raise ValueError(f"features must be [N, feature_dim] = [{N}, {FEATURE_DIM}], got {tuple(features.shape)}")
        if int(features.shape[1]) != FEATURE_DIM:
            raise NotImplementedError(f"AppearanceOptModule: feature_dim = {int(features.shape[1])} is not built ({FEATURE_DIM} is)")
        if Cn == 0 or N == 0:
            raise ValueError(f"no pairs: dirs is {tuple(dirs.shape)}")
        dev = self.embeds.weight.device
        if features.device.type != "cuda" or dirs.device.type != "cuda" or dev.type != "cuda":
            raise RuntimeError("the appearance module runs in libwm_hip.so on the GPU: move the module, features and dirs to a HIP device")
        if not (features.device == dirs.device == dev):
            raise RuntimeError(f"module, features and dirs are on different devices: {dev}, {features.device}, {dirs.device}")
        ids = None
        if embed_ids is not None:
            ids = embed_ids if torch.is_tensor(embed_ids) else torch.as_tensor(embed_ids)
            if ids.dtype.is_floating_point or ids.dtype == torch.bool:
                raise TypeError(f"embed_ids must hold integers, got {ids.dtype}")
            if tuple(ids.shape) != (Cn,):
                raise ValueError(f"embed_ids must be [C] = [{Cn}], got {tuple(ids.shape)}")
            if ids.device.type == "cpu":
                bad = [int(v) for v in ids.tolist() if not 0 <= int(v) < self.embeds.num_embeddings]
                if bad:
                    raise IndexError(f"embed id {bad[0]} is out of range for {self.embeds.num_embeddings} embeddings")
            # (clamped first, on the device: a 64-bit id must not wrap into range when it is narrowed; -1 and n are both out of range)
            ids = ids.to(dev).clamp(-1, self.embeds.num_embeddings).to(torch.int32).contiguous()
        head = self.color_head
        tensors = [features, dirs, self.embeds.weight, head[0].weight, head[0].bias, head[2].weight, head[2].bias, head[4].weight, head[4].bias]
        t32 = [t.to(torch.float32).contiguous() for t in tensors]
        if torch.is_grad_enabled() and any(t.requires_grad for t in t32):
            return _Appearance.apply(*t32, ids, self.sh_degree, int(sh_degree))
        return _forward(*(t.detach() for t in t32), ids, self.sh_degree, int(sh_degree))
