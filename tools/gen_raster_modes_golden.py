"""Generate tests/golden/raster_modes_*.npz: the REFERENCE's own projection with compensations (gsplat's pure-torch
_quat_scale_to_covar_preci + _fully_fused_projection(calc_compensations=True), gsplat/cuda/_torch_impl.py:45-61,286-375) in fp64 on the
inputs of the committed raster scenes, for two settings of (eps2d, near_plane, far_plane): gsplat's defaults and one whose planes cut
through the scene.  Per setting: radii, compensations, conics, and the gradients to means / quats / scales of seeded cotangents over
means2d / depths / conics / compensations (zero on culled pairs).  Recorded results only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_raster_modes_golden.py <path to the reference checkout>
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SETTINGS = {"default": (0.3, 0.01, 1e10), "cut": (0.1, 2.0, 4.5)}     # eps2d, near_plane, far_plane


def project(z, dtype, eps2d, near, far, grad=False):
    from gsplat.cuda._torch_impl import _fully_fused_projection, _quat_scale_to_covar_preci
    W, H = int(z["width"]), int(z["height"])
    t = {k: torch.from_numpy(z["in_" + k]).to(dtype) for k in ("means", "quats", "scales", "viewmats", "Ks")}
    if grad:
        for k in ("means", "quats", "scales"):
            t[k].requires_grad_(True)
    covars, _ = _quat_scale_to_covar_preci(t["quats"], t["scales"], True, False, triu=False)
    out = _fully_fused_projection(t["means"], covars, t["viewmats"], t["Ks"], W, H, eps2d=eps2d, near_plane=near, far_plane=far,
                                  calc_compensations=True)
    return t, out


def det_orig(z, eps2d, conics):
    """det of the 2-D covariance before the blur, from the blurred conic: cov_blur = inv(conic), cov = cov_blur - eps2d I"""
    a, b, c = conics[..., 0], conics[..., 1], conics[..., 2]
    d = a * c - b * b
    c00, c11, c01 = c / d - eps2d, a / d - eps2d, -b / d
    return c00 * c11 - c01 * c01


def run(name, seed):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    out, counts = {}, {}
    for tag, (eps2d, near, far) in SETTINGS.items():
        t, (radii, means2d, depths, conics, comps) = project(z, torch.float64, eps2d, near, far, grad=True)
        _, (radii32, *_rest) = project(z, torch.float32, eps2d, near, far)
        assert torch.equal(radii, radii32), "fp64 and fp32 reference projections disagree on a culling decision"
        vis = (radii > 0).all(-1)
        counts[tag] = int(vis.sum())
        assert float(det_orig(z, eps2d, conics.detach())[vis].min()) > 0, "a visible pair with det_orig <= 0 (the NaN corner of autograd)"
        assert float(comps.detach()[vis].min()) > 0
        g = torch.Generator().manual_seed(seed)
        cot = {"means2d": torch.randn(means2d.shape, generator=g, dtype=torch.float64) * vis[..., None],
               "depths": torch.randn(depths.shape, generator=g, dtype=torch.float64) * vis,
               "conics": torch.randn(conics.shape, generator=g, dtype=torch.float64) * vis[..., None],
               "compensations": torch.randn(comps.shape, generator=g, dtype=torch.float64) * vis}
        zero = lambda x: torch.where(vis if x.dim() == 2 else vis[..., None], x, torch.zeros_like(x))   # culled pairs may hold NaN
        loss = (zero(means2d) * cot["means2d"]).sum() + (zero(depths) * cot["depths"]).sum() + (zero(conics) * cot["conics"]).sum() + \
               (zero(comps) * cot["compensations"]).sum()
        gm, gq, gs = torch.autograd.grad(loss, [t["means"], t["quats"], t["scales"]])
        assert all(torch.isfinite(x).all() for x in (gm, gq, gs))
        out.update({f"{tag}_cot_{k}": v.numpy() for k, v in cot.items()})
        out.update({f"{tag}_radii": radii.numpy().astype(np.int32), f"{tag}_compensations": zero(comps.detach()).numpy(),
                    f"{tag}_conics": zero(conics.detach()).numpy(), f"{tag}_grad_means": gm.numpy(), f"{tag}_grad_quats": gq.numpy(),
                    f"{tag}_grad_scales": gs.numpy(), f"{tag}_setting": np.array([eps2d, near, far]), f"{tag}_visible": np.array(counts[tag])})
    assert np.array_equal(out["default_radii"], z["ref_radii"])
    # the planes must cut through the scene: fewer visible pairs than by default, but more than a third of them
    assert counts["default"] / 3 < counts["cut"] < counts["default"], counts
    path = os.path.join(GOLD, name.replace("raster_", "raster_modes_") + ".npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", "visible pairs", counts)


if __name__ == "__main__":
    ref = sys.argv[1]
    sys.path[:0] = [ref, os.path.join(ref, "submodules", "gsplat")]
    run("raster_600g_2c_80x56", 21)
    run("raster_1500g_3c_100x70", 22)
