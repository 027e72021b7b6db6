"""TEST INFRASTRUCTURE ONLY (not a test file): view-dependent colour for the torch restatement of the rasteriser
(tests/raster_grad_helper.py), in any float dtype: the real spherical-harmonics basis of degree <= 3, the colours
gsplat.rasterization makes of SH coefficients (gsplat/rendering.py:509-525) and the gradients the GPU tests compare with.

The basis is written from the published Cartesian polynomials of the real spherical harmonics (Sloan, "Efficient Spherical Harmonic
Evaluation", JCGT 2013, with the sign convention of 3DGS: odd-m terms negated); tests/test_raster_sh_cpu.py pins its colours and
gradients to the reference's own evaluation (tests/golden/raster_sh_*.npz, tools/gen_raster_sh_golden.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

import raster_grad_helper as RG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = {"raster_600g_2c_80x56": "raster_sh_600g_2c", "raster_1500g_3c_100x70": "raster_sh_1500g_3c"}


def higher_bands(n):
    """bands 1..15 of the recorded scenes, [n,15,3] float32: uniform(-0.6, 0.6) from Philox(key=[19, 5]), drawn anew per scene"""
    return np.random.Generator(np.random.Philox(key=[19, 5])).uniform(-0.6, 0.6, size=(n, 15, 3)).astype(np.float32)


def load_scene(name):
    """-> inputs (numpy: means, quats, scales, opacities, sh [N,16,3], viewmats, Ks), width, height, the recorded reference arrays"""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    rec = dict(np.load(os.path.join(GOLD, SCENES[name] + ".npz")))
    shN = higher_bands(z["in_means"].shape[0])
    assert shN.astype(np.float64).sum() == float(rec["shN_sum"]) and np.array_equal(shN[[0, -1]], rec["shN_probe"]), "the higher bands drawn differ from the recorded ones"
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    inp["sh"] = np.concatenate([z["in_sh"], shN], 1)
    rec["radii"] = z["ref_radii"]
    return inp, int(z["width"]), int(z["height"]), rec


def sh_basis(d, L):
    """d [...,3] unit directions -> [..., (L + 1)^2]"""
    x, y, z = d.unbind(-1)
    B = [torch.full_like(x, 0.28209479177387814)]
    if L >= 1:
        c = 0.4886025119029199                      # sqrt(3 / (4 pi))
        B += [-c * y, c * z, -c * x]
    if L >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [1.0925484305920792 * xy,              # sqrt(15 / (4 pi))
              -1.0925484305920792 * yz,
              0.9461746957575601 * zz - 0.31539156525252005,      # sqrt(5 / (16 pi)) (3 z^2 - 1)
              -1.0925484305920792 * xz,
              0.5462742152960396 * (xx - yy)]       # sqrt(15 / (16 pi))
    if L >= 3:
        B += [-0.5900435899266435 * y * (3 * xx - yy),            # sqrt(35 / (32 pi))
              2.890611442640554 * xy * z,                         # sqrt(105 / (4 pi))
              -0.4570457994644658 * y * (5 * zz - 1),             # sqrt(21 / (32 pi))
              0.3731763325901154 * z * (5 * zz - 3),              # sqrt(7 / (16 pi))
              -0.4570457994644658 * x * (5 * zz - 1),
              1.445305721320277 * z * (xx - yy),                  # sqrt(105 / (16 pi))
              -0.5900435899266435 * x * (xx - 3 * yy)]
    if L >= 4:
        raise NotImplementedError("degrees 0 to 3")
    return torch.stack(B, -1)


def sh_colors(means, sh, campos, L, visible):
    """[C,N,3]: clamp_min(sum_k B_k(normalize(means - campos)) sh[:, k] + 0.5, 0); the sum is 0 where not visible [C,N].  Bands at or above
    (L + 1)^2 are not read."""
    d = means[None, :, :] - campos[:, None, :]
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    raw = (sh_basis(d, L)[..., None] * sh[None, :, :(L + 1) ** 2, :]).sum(-2)
    return torch.clamp_min(torch.where(visible[..., None], raw, torch.zeros_like(raw)) + 0.5, 0.0)


def rasterize_sh(means, quats, scales, opacities, sh, L, viewmats, Ks, width, height, campos=None):
    """sh [N,K,3].  campos: the cameras' world positions, by default inverse(viewmats)[:, :3, 3].  -> rgb, expected depth, alpha"""
    if campos is None:
        campos = torch.linalg.inv(viewmats)[:, :3, 3]
    radii, m2, depths, conics, _ = RG.project(means, quats, scales, viewmats, Ks, width, height)
    colors = sh_colors(means, sh, campos, L, (radii > 0).all(-1))
    outs = [RG.composite(m2[c:c + 1], conics[c:c + 1], depths[c:c + 1], opacities, colors[c], radii[c:c + 1], width, height) for c in range(viewmats.shape[0])]
    return tuple(torch.cat([o[i] for o in outs], 0) for i in range(3))


NAMES = ("means", "quats", "scales", "opacities", "sh", "camtoworlds")


def gradients_sh(inputs, cotangents, L, width, height, dtype):
    """inputs: numpy means / quats / scales / opacities / sh [N,K,3] / camtoworlds / Ks; cotangents: (v_rgb, v_depth, v_alpha) numpy.
    viewmats = inv(camtoworlds) and campos = camtoworlds[:, :3, 3] are taken in the graph, in `dtype`.
    -> (outputs, dict of the gradients of NAMES), as numpy float64."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in inputs.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    outs = rasterize_sh(t["means"], t["quats"], t["scales"], t["opacities"], t["sh"], L, torch.linalg.inv(t["camtoworlds"]), t["Ks"], width, height,
                        campos=t["camtoworlds"][:, :3, 3])
    loss = sum((o * torch.from_numpy(v).to(dtype)).sum() for o, v in zip(outs, cotangents))
    g = torch.autograd.grad(loss, [t[k] for k in NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(t[k]) if gi is None else gi).double().numpy() for k, gi in zip(NAMES, g)}
    return [o.detach().double().numpy() for o in outs], grads
