"""TEST INFRASTRUCTURE ONLY (not a test file): gsplat.rasterization's options on top of tests/raster_grad_helper.py, in any float
dtype and differentiable — the antialiased compensation (gsplat/cuda/_torch_impl.py:329-344), eps2d and the planes (already arguments
of RG.project), radius_clip (gsplat's ProjectionEWA3DGSFused.cu; the torch projection has no such rule), backgrounds and the depth
mode (gsplat/rendering.py:926-939, :984-992).  The compensation and radii are pinned to the reference's own by
tests/golden/raster_modes_*.npz (tools/gen_raster_modes_golden.py).
"""
from __future__ import annotations

import numpy as np
import torch

import raster_grad_helper as RG


def project(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0):
    """RG.project + compensations [C,N] = sqrt(max(det(cov2d) / det(cov2d + eps2d I), 0)) (det the clamped one) and radius_clip.
    -> radii, means2d, depths, conics, cov2d diagonal (blurred), compensations"""
    radii, m2, depths, conics, cdiag = RG.project(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane)
    # the blurred covariance back out of its conic (det >= 1e-10 clamped as in the projection: conic = adj / det)
    a, b, c = conics.unbind(-1)
    c00, c11 = cdiag.unbind(-1)
    det = c00 / c                                   # conic[2] = c00 / det
    c01 = -b * det
    det_orig = (c00 - eps2d) * (c11 - eps2d) - c01 * c01
    vis = (radii > 0).all(-1)                       # culled pairs: 1 (never read; keeps autograd away from sqrt(0) and non-finite values)
    comp = torch.sqrt(torch.clamp(torch.where(vis, det_orig / det, torch.ones_like(det)), min=0.0))
    if radius_clip > 0:
        small = (radii <= radius_clip).all(-1)      # both radii at most radius_clip: culled
        radii = torch.where(small[..., None], torch.zeros_like(radii), radii)
    return radii, m2, depths, conics, cdiag, comp


def rasterize(means, quats, scales, opacities, colors, is_sh, viewmats, Ks, width, height, antialiased=False, eps2d=0.3, near_plane=0.01,
              far_plane=1e10, radius_clip=0.0, backgrounds=None, depth_mode="ED", margins=None):
    """-> rgb [C,H,W,3], depth [C,H,W,1] (depth_mode "ED": expected, "D": accumulated), alpha [C,H,W,1].  The compensated opacity
    [C,N] is what the compositing (and its alpha_threshold / alpha_cap margins) sees."""
    radii, m2, depths, conics, cdiag, comp = project(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip)
    if margins is not None:
        vis = (radii > 0).all(-1)
        if vis.any():
            margins["radius"] = float(RG._dist_to_integer(3.33 * torch.sqrt(cdiag.detach()[vis])).min())
    col = torch.clamp_min(RG.SH_C0 * colors + 0.5, 0.0) if is_sh else colors
    outs = []
    for c in range(viewmats.shape[0]):         # per camera: the opacity of a pair depends on the camera
        op = opacities * comp[c] if antialiased else opacities
        outs.append(RG.composite(m2[c:c + 1], conics[c:c + 1], depths[c:c + 1], op, col, radii[c:c + 1], width, height, margins))
    rgb, ed, al = (torch.cat([o[i] for o in outs], 0) for i in range(3))
    depth = ed if depth_mode == "ED" else ed * al.clamp(min=1e-10)     # D = ED * max(alpha, 1e-10), undoing the helper's division
    if backgrounds is not None:
        rgb = rgb + backgrounds[:, None, None, :] * (1.0 - al)
    return rgb, depth, al


NAMES = ("means", "quats", "scales", "opacities", "colors")


def gradients(inputs, cotangents, is_sh, width, height, dtype, **options):
    """as RG.gradients with the options of rasterize; options["backgrounds"] (numpy [C,3]) also gets a gradient.
    -> (outputs, dict of gradients), numpy float64"""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in inputs.items()}
    leaves = list(NAMES)
    for k in NAMES:
        t[k].requires_grad_(True)
    if options.get("backgrounds") is not None:
        t["backgrounds"] = torch.from_numpy(np.ascontiguousarray(options["backgrounds"])).to(dtype).requires_grad_(True)
        options = {**options, "backgrounds": t["backgrounds"]}
        leaves.append("backgrounds")
    outs = rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], is_sh, t["viewmats"], t["Ks"], width, height, **options)
    loss = sum((o * torch.from_numpy(v).to(dtype)).sum() for o, v in zip(outs, cotangents))
    g = torch.autograd.grad(loss, [t[k] for k in leaves], allow_unused=True)
    grads = {k: (torch.zeros_like(t[k]) if gi is None else gi).double().numpy() for k, gi in zip(leaves, g)}
    return [o.detach().double().numpy() for o in outs], grads
