"""Generate tests/golden/raster_grad_*.npz: gradients of the REFERENCE's own projection (gsplat's pure-torch
_quat_scale_to_covar_preci + _fully_fused_projection, gsplat/cuda/_torch_impl.py:45-61,286-375) in fp64 on the inputs of the
committed raster scenes, for seeded cotangents of means2d / depths / conics (zero on culled pairs).  Recorded results only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_raster_grad_golden.py <path to the reference checkout>
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def run(name, seed):
    from gsplat.cuda._torch_impl import _fully_fused_projection, _quat_scale_to_covar_preci
    z = np.load(os.path.join(GOLD, name + ".npz"))
    W, H = int(z["width"]), int(z["height"])
    t = {k: torch.from_numpy(z["in_" + k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    for k in ("means", "quats", "scales"):
        t[k].requires_grad_(True)
    covars, _ = _quat_scale_to_covar_preci(t["quats"], t["scales"], True, False, triu=False)
    radii, means2d, depths, conics, _ = _fully_fused_projection(t["means"], covars, t["viewmats"], t["Ks"], W, H)
    vis = (radii > 0).all(-1)
    assert np.array_equal(radii.numpy(), z["ref_radii"]), "fp64 and fp32 reference projections disagree on a culling decision"
    g = torch.Generator().manual_seed(seed)
    cot = {"means2d": torch.randn(means2d.shape, generator=g, dtype=torch.float64) * vis[..., None],
           "depths": torch.randn(depths.shape, generator=g, dtype=torch.float64) * vis,
           "conics": torch.randn(conics.shape, generator=g, dtype=torch.float64) * vis[..., None]}
    loss = (means2d * cot["means2d"]).sum() + (depths * cot["depths"]).sum() + (conics * cot["conics"]).sum()
    gm, gq, gs = torch.autograd.grad(loss, [t["means"], t["quats"], t["scales"]])
    out = {"cot_" + k: v.numpy() for k, v in cot.items()}
    out.update(grad_means=gm.numpy(), grad_quats=gq.numpy(), grad_scales=gs.numpy())
    path = os.path.join(GOLD, name.replace("raster_", "raster_grad_") + ".npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", "visible pairs", int(vis.sum()))


if __name__ == "__main__":
    ref = sys.argv[1]
    sys.path[:0] = [ref, os.path.join(ref, "submodules", "gsplat")]
    run("raster_600g_2c_80x56", 11)
    run("raster_1500g_3c_100x70", 12)
