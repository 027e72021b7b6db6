"""Generate the recorded results the camera-gradient tests compare with, from the REFERENCE's own code in fp64 (recorded arrays only):

  tests/golden/camera_grad_*.npz   grad_viewmats: the gradient of gsplat's pure-torch _fully_fused_projection
                                   (gsplat/cuda/_torch_impl.py:286-375, through _world_to_cam :250-283) with respect to viewmats, on the
                                   inputs of the committed raster scenes and for the cotangents stored in the matching raster_grad_*.npz
  tests/golden/pose_adjust.npz     the reference trainer's CameraOptModule (gsplat examples/utils.py): seeded embeds.weight (n = 5,
                                   std 0.1), seeded camtoworlds and embed_ids with a repeat -> its output, and its gradient with respect
                                   to embeds.weight for a seeded cotangent

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_camera_grad_golden.py <path to the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def camera_grad(name):
    from gsplat.cuda._torch_impl import _fully_fused_projection, _quat_scale_to_covar_preci
    z = np.load(os.path.join(GOLD, name + ".npz"))
    gz = np.load(os.path.join(GOLD, name.replace("raster_", "raster_grad_") + ".npz"))
    W, H = int(z["width"]), int(z["height"])
    t = {k: torch.from_numpy(z["in_" + k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    t["viewmats"].requires_grad_(True)
    covars, _ = _quat_scale_to_covar_preci(t["quats"], t["scales"], True, False, triu=False)
    radii, means2d, depths, conics, _ = _fully_fused_projection(t["means"], covars, t["viewmats"], t["Ks"], W, H)
    assert np.array_equal(radii.numpy(), z["ref_radii"]), "fp64 and fp32 reference projections disagree on a culling decision"
    loss = (means2d * torch.from_numpy(gz["cot_means2d"])).sum() + (depths * torch.from_numpy(gz["cot_depths"])).sum() + \
           (conics * torch.from_numpy(gz["cot_conics"])).sum()
    (gv,) = torch.autograd.grad(loss, [t["viewmats"]])
    path = os.path.join(GOLD, name.replace("raster_", "camera_grad_") + ".npz")
    np.savez_compressed(path, grad_viewmats=gv.numpy())
    print(path, os.path.getsize(path), "bytes")


def pose_adjust(ref):
    spec = importlib.util.spec_from_file_location("gsplat_examples_utils", os.path.join(ref, "submodules", "gsplat", "examples", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_default_dtype(torch.float64)      # the module builds its transform with the default dtype
    g = torch.Generator().manual_seed(17)
    n = 5
    weight = 0.1 * torch.randn(n, 9, generator=g, dtype=torch.float64)
    ids = torch.tensor([3, 0, 3, 4, 1, 2])
    # non-trivial poses: a rotation from a random quaternion and a translation of a few units
    q = torch.nn.functional.normalize(torch.randn(len(ids), 4, generator=g, dtype=torch.float64), dim=-1)
    w, x, y, zq = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y),
                     2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x),
                     2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    c2w = torch.eye(4, dtype=torch.float64).repeat(len(ids), 1, 1)
    c2w[:, :3, :3] = R
    c2w[:, :3, 3] = 3.0 * torch.randn(len(ids), 3, generator=g, dtype=torch.float64)
    cot = torch.randn(len(ids), 4, 4, generator=g, dtype=torch.float64)
    m = mod.CameraOptModule(n).double()
    with torch.no_grad():
        m.embeds.weight.copy_(weight)
    out = m(c2w, ids)
    (gw,) = torch.autograd.grad((out * cot).sum(), [m.embeds.weight])
    assert out.dtype == torch.float64 and sorted(m.state_dict()) == ["embeds.weight", "identity"]
    path = os.path.join(GOLD, "pose_adjust.npz")
    np.savez_compressed(path, weight=weight.numpy(), embed_ids=ids.numpy(), camtoworlds=c2w.numpy(), cotangent=cot.numpy(),
                        out=out.detach().numpy(), grad_weight=gw.numpy())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1]
    sys.path[:0] = [ref, os.path.join(ref, "submodules", "gsplat")]
    camera_grad("raster_600g_2c_80x56")
    camera_grad("raster_1500g_3c_100x70")
    pose_adjust(ref)
