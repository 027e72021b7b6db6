"""TEST INFRASTRUCTURE ONLY (not a test file): a differentiable torch restatement of the rasteriser, in any float dtype, that
the gradient tests differentiate with autograd.

Projection: the formulas of gsplat/cuda/_torch_impl.py (_quat_to_rotmat :11-29, _quat_scale_to_covar_preci :45-61, _world_to_cam
:250-283, _persp_proj :78-133, _fully_fused_projection :329-374) — its gradients are pinned to the reference's own by
tests/golden/raster_grad_*.npz (tools/gen_raster_grad_golden.py).
Compositing: the rules of oracle/raster_ref.composite (RasterizeToPixels3DGSFwd.cu:118-184) written without the sequential
loop: per pixel, all Gaussians of the camera in the forward's sorted order (depth bits, stable), restricted to those whose
tile rectangle covers the pixel's tile; the skip (sigma < 0, alpha < 1/255), cap (0.999) and stop (T (1 - alpha) <= 1e-4,
before blending) rules are masks, the transmittance an exclusive cumprod.  The masks are decided without gradient (they are
piecewise constant), everything else is differentiable.
"""
from __future__ import annotations

import math

import torch

SH_C0 = 0.28209479177387814
ALPHA_THRESHOLD = 1.0 / 255.0
TILE = 16


def quat_scale_to_covar(quats, scales):
    q = quats / quats.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = R * scales[:, None, :]
    return torch.einsum("nij,nkj->nik", M, M)


def project(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10):
    """-> radii [C,N,2] (int, no gradient), means2d [C,N,2], depths [C,N], conics [C,N,3], cov2d diagonal [C,N,2]"""
    covars = quat_scale_to_covar(quats, scales)
    R, t = viewmats[:, :3, :3], viewmats[:, :3, 3]
    mc = torch.einsum("cij,nj->cni", R, means) + t[:, None, :]
    cc = torch.einsum("cij,njk,clk->cnil", R, covars, R)
    tx, ty, tz = mc.unbind(-1)
    tz2 = tz * tz
    fx, fy, cx, cy = Ks[:, 0, 0, None], Ks[:, 1, 1, None], Ks[:, 0, 2, None], Ks[:, 1, 2, None]
    tfx, tfy = 0.5 * width / fx, 0.5 * height / fy
    lxp, lxn = (width - cx) / fx + 0.3 * tfx, cx / fx + 0.3 * tfx
    lyp, lyn = (height - cy) / fy + 0.3 * tfy, cy / fy + 0.3 * tfy
    txc = tz * torch.minimum(torch.maximum(tx / tz, -lxn), lxp)
    tyc = tz * torch.minimum(torch.maximum(ty / tz, -lyn), lyp)
    O = torch.zeros_like(tz)
    J = torch.stack([fx / tz, O, -fx * txc / tz2, O, fy / tz, -fy * tyc / tz2], -1).reshape(tz.shape + (2, 3))
    cov2d = torch.einsum("cnij,cnjk,cnlk->cnil", J, cc, J)
    m2 = torch.einsum("cij,cnj->cni", Ks[:, :2, :3], mc) / tz[..., None]
    cov2d = cov2d + torch.eye(2, dtype=means.dtype) * eps2d
    det = cov2d[..., 0, 0] * cov2d[..., 1, 1] - cov2d[..., 0, 1] * cov2d[..., 1, 0]
    det = det.clamp(min=1e-10)
    conics = torch.stack([cov2d[..., 1, 1] / det, -(cov2d[..., 0, 1] + cov2d[..., 1, 0]) / 2.0 / det, cov2d[..., 0, 0] / det], -1)
    with torch.no_grad():
        radius = torch.stack([torch.ceil(3.33 * torch.sqrt(cov2d[..., 0, 0])), torch.ceil(3.33 * torch.sqrt(cov2d[..., 1, 1]))], -1)
        valid = (det > 0) & (tz > near_plane) & (tz < far_plane)
        radius[~valid] = 0.0
        inside = (m2[..., 0] + radius[..., 0] > 0) & (m2[..., 0] - radius[..., 0] < width) & \
                 (m2[..., 1] + radius[..., 1] > 0) & (m2[..., 1] - radius[..., 1] < height)
        radius[~inside] = 0.0
        radius = torch.nan_to_num(radius, nan=0.0, posinf=0.0, neginf=0.0)
    return radius.to(torch.int32), m2, tz, conics, torch.stack([cov2d[..., 0, 0], cov2d[..., 1, 1]], -1)


def _dist_to_integer(x):
    return (x - torch.round(x)).abs()


def composite(m2, conics, depths, opacities, colors, radii, width, height, margins=None):
    """-> rgb [C,H,W,3], expected depth [C,H,W,1], alpha [C,H,W,1].  margins: a dict that receives, per kind of threshold, the
    smallest distance of any decided quantity from it."""
    C, N = depths.shape
    dt = m2.dtype
    tw, th = math.ceil(width / TILE), math.ceil(height / TILE)
    rgb_rows, ed_rows, al_rows = [], [], []
    note = (lambda k, v: margins.__setitem__(k, min(margins.get(k, float("inf")), float(v)))) if margins is not None else (lambda k, v: None)
    for c in range(C):
        with torch.no_grad():
            vis = torch.nonzero((radii[c] > 0).all(-1))[:, 0]
            order = vis[torch.argsort(depths[c, vis].detach().to(torch.float32), stable=True)]
            tm, tr = m2[c, order].detach() / TILE, radii[c, order].to(dt) / TILE
            lo_f, hi_f = tm - tr, tm + tr
            lo, hi = torch.floor(lo_f).long(), torch.ceil(hi_f).long()
            x0, x1 = lo[:, 0].clamp(0, tw), hi[:, 0].clamp(0, tw)
            y0, y1 = lo[:, 1].clamp(0, th), hi[:, 1].clamp(0, th)
            if len(order):
                lim = torch.tensor([tw, th], dtype=dt)      # an edge beyond the grid is clamped: a flip there changes nothing
                edges = torch.cat([lo_f[(lo_f > 0) & (lo_f < lim)], hi_f[(hi_f > 0) & (hi_f < lim)]])
                if edges.numel():
                    note("tile", _dist_to_integer(edges).min())
        cam_rgb, cam_ed, cam_al = [], [], []
        for ty in range(th):
            r0, r1 = ty * TILE, min(ty * TILE + TILE, height)
            sel = torch.nonzero((y0 <= ty) & (ty < y1))[:, 0]
            ids = order[sel]
            ys, xs = torch.meshgrid(torch.arange(r0, r1), torch.arange(width), indexing="ij")
            py, px = (ys.reshape(-1).to(dt) + 0.5), (xs.reshape(-1).to(dt) + 0.5)
            P = px.numel()
            if len(ids) == 0:
                cam_rgb.append(torch.zeros(r1 - r0, width, 3, dtype=dt)); cam_ed.append(torch.zeros(r1 - r0, width, 1, dtype=dt))
                cam_al.append(torch.zeros(r1 - r0, width, 1, dtype=dt))
                continue
            tx = (xs.reshape(-1) // TILE)[:, None]
            cover = (x0[sel][None, :] <= tx) & (tx < x1[sel][None, :])
            dx, dy = m2[c, ids, 0][None, :] - px[:, None], m2[c, ids, 1][None, :] - py[:, None]
            ca, cb, cc = conics[c, ids, 0][None, :], conics[c, ids, 1][None, :], conics[c, ids, 2][None, :]
            sigma = 0.5 * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
            raw = opacities[ids][None, :] * torch.exp(-sigma)
            alpha = raw.clamp(max=0.999)
            one = torch.ones_like(alpha)
            with torch.no_grad():
                hit = cover & ~(sigma < 0) & ~(alpha < ALPHA_THRESHOLD)
                f0 = torch.where(hit, 1 - alpha, one)
                Tall = torch.cat([one[:, :1], torch.cumprod(f0, 1)[:, :-1]], 1)
                nT = Tall * (1 - alpha)
                stopflag = hit & (nT <= 1e-4)
                stopped_before = (torch.cumsum(stopflag.to(torch.int64), 1) - stopflag.to(torch.int64)) > 0
                blend = hit & ~stopflag & ~stopped_before
                if margins is not None:
                    live = cover & ~stopped_before
                    if live.any():
                        note("alpha_threshold", (alpha - ALPHA_THRESHOLD).abs()[live].min())
                        note("alpha_cap", (raw - 0.999).abs()[live].min())
                    if (hit & ~stopped_before).any():
                        note("stop", (nT - 1e-4).abs()[hit & ~stopped_before].min())
            fac = torch.where(blend, 1 - alpha, one)
            cp = torch.cumprod(fac, 1)
            T = torch.cat([one[:, :1], cp[:, :-1]], 1)
            w = torch.where(blend, alpha * T, torch.zeros_like(alpha))
            rgb = w @ colors[ids]
            D = (w * depths[c, ids][None, :]).sum(1, keepdim=True)
            al = 1 - cp[:, -1:]
            ed = D / al.clamp(min=1e-10)
            cam_rgb.append(rgb.reshape(r1 - r0, width, 3)); cam_ed.append(ed.reshape(r1 - r0, width, 1)); cam_al.append(al.reshape(r1 - r0, width, 1))
        rgb_rows.append(torch.cat(cam_rgb, 0)); ed_rows.append(torch.cat(cam_ed, 0)); al_rows.append(torch.cat(cam_al, 0))
    return torch.stack(rgb_rows, 0), torch.stack(ed_rows, 0), torch.stack(al_rows, 0)


def rasterize(means, quats, scales, opacities, colors, is_sh, viewmats, Ks, width, height, margins=None):
    """colors [N,3]: degree-0 SH coefficients (is_sh) or final colours.  All float inputs in one dtype."""
    radii, m2, depths, conics, cdiag = project(means, quats, scales, viewmats, Ks, width, height)
    if margins is not None:
        vis = (radii > 0).all(-1)
        if vis.any():
            margins["radius"] = float(_dist_to_integer(3.33 * torch.sqrt(cdiag.detach()[vis])).min())
    col = torch.clamp_min(SH_C0 * colors + 0.5, 0.0) if is_sh else colors
    return composite(m2, conics, depths, opacities, col, radii, width, height, margins)


def gradients(inputs, cotangents, is_sh, width, height, dtype):
    """inputs: dict of numpy arrays means / quats / scales / opacities / colors / viewmats / Ks; cotangents: (v_rgb, v_depth,
    v_alpha) numpy.  -> (outputs, dict of the five gradients), all in `dtype`, as numpy float64."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inputs.items()}
    names = ("means", "quats", "scales", "opacities", "colors")
    for k in names:
        t[k].requires_grad_(True)
    outs = rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], is_sh, t["viewmats"], t["Ks"], width, height)
    loss = sum((o * torch.from_numpy(v).to(dtype)).sum() for o, v in zip(outs, cotangents))
    g = torch.autograd.grad(loss, [t[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(t[k]) if gi is None else gi).double().numpy() for k, gi in zip(names, g)}
    return [o.detach().double().numpy() for o in outs], grads
