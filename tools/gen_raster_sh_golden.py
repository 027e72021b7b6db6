"""Generate the recorded results the view-dependent-colour tests compare with, from the REFERENCE's own code in fp64 (recorded arrays only):

  tests/golden/raster_sh_600g_2c.npz, raster_sh_1500g_3c.npz
      shN_sum, shN_probe        the higher bands are not stored: in_shN [N,15,3] float32 is drawn again by tests/raster_sh_helper.higher_bands
                                (uniform(-0.6, 0.6) from np.random.Philox(key=[19, 5]), per scene) and checked against its fp64 sum and its
                                first and last rows; the committed scene's in_sh is band 0
      cot                       [C,N,3] seeded cotangent of the colours (float32 values), zero on culled pairs
      colors_L{1,2,3}           [C,N,3] what gsplat.rasterization makes of the coefficients (rendering.py:509-525): gsplat's pure-torch
                                _spherical_harmonics (gsplat/cuda/_torch_impl.py:804-822) along means - inverse(viewmats)[:, :3, 3], zero
                                where ref_radii is 0, then clamp_min(. + 0.5, 0)
      grad_sh_L*, grad_means_L*, grad_campos_L*
                                gradients of sum(colors * cot) with respect to the coefficients [N,16,3], means [N,3] and the camera
                                positions [C,3]

The script refuses inputs on which a colour channel comes closer than 1e-5 to the clamp (100 x the fp32 evaluation error of these colours,
1e-7 relative): the clamp decision is then the same in fp32 and fp64.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_raster_sh_golden.py <path to the reference checkout>
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raster_sh_helper import higher_bands  # noqa: E402


def scene(name):
    from gsplat.cuda._torch_impl import _spherical_harmonics
    z = np.load(os.path.join(GOLD, name + ".npz"))
    N, C = z["in_means"].shape[0], z["in_viewmats"].shape[0]
    shN = higher_bands(N)
    vis = torch.from_numpy((z["ref_radii"] > 0).all(-1))
    rng = np.random.Generator(np.random.Philox(key=[19, 6]))
    cot = torch.from_numpy(rng.standard_normal((C, N, 3)).astype(np.float32)) * vis[..., None]
    out = {"shN_sum": shN.astype(np.float64).sum(), "shN_probe": shN[[0, -1]], "cot": cot.numpy()}
    cot = cot.double()
    margin = np.inf
    for L in (1, 2, 3):
        coeffs = torch.from_numpy(np.concatenate([z["in_sh"], shN], 1)).double().requires_grad_(True)
        means = torch.from_numpy(z["in_means"]).double().requires_grad_(True)
        campos = torch.linalg.inv(torch.from_numpy(z["in_viewmats"]).double())[:, :3, 3].clone().requires_grad_(True)
        dirs = means[None, :, :] - campos[:, None, :]
        raw = _spherical_harmonics(L, dirs, coeffs[None].expand(C, -1, -1, -1)) * vis[..., None]
        colors = torch.clamp_min(raw + 0.5, 0.0)
        margin = min(margin, float((raw.detach() + 0.5).abs()[vis].min()))
        g = torch.autograd.grad((colors * cot).sum(), [coeffs, means, campos])
        assert float(g[0][:, (L + 1) ** 2:].abs().sum()) == 0.0
        out[f"colors_L{L}"] = colors.detach().numpy()
        out[f"grad_sh_L{L}"], out[f"grad_means_L{L}"], out[f"grad_campos_L{L}"] = (x.numpy() for x in g)
        clamped = float((colors.detach()[vis] == 0).double().mean())
        print(f"{name} L={L}: {100 * clamped:.1f} % of the visible colour channels clamp")
    return margin, os.path.join(GOLD, name.replace("raster_", "raster_sh_").rsplit("_", 1)[0] + ".npz"), out


if __name__ == "__main__":
    ref = sys.argv[1]
    sys.path[:0] = [ref, os.path.join(ref, "submodules", "gsplat")]
    scenes = [scene("raster_600g_2c_80x56"), scene("raster_1500g_3c_100x70")]
    margin = min(m for m, _, _ in scenes)
    print("min |colour + 0.5| over the visible pairs, all degrees, both scenes:", margin)
    assert margin >= 1e-5, "a colour channel sits on the clamp: change the key"
    for _, path, out in scenes:
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20
