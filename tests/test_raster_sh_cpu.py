"""View-dependent colour, CPU side: the yardstick of the GPU tests (tests/raster_sh_helper.py) is pinned to the reference's own
evaluation in fp64 (gsplat's pure-torch _spherical_harmonics along means - inverse(viewmats)[:, :3, 3]; recorded results
tests/golden/raster_sh_*.npz, tools/gen_raster_sh_golden.py), and the new entry points are checked at build level.
Measured values: profiles/r10_spherical_harmonics.md."""
import functools

import numpy as np
import pytest
import torch

import raster_sh_helper as SH
from conftest import rel_l2

CASES = list(SH.SCENES)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SH.load_scene(name)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("name", CASES)
def test_helper_colours_and_gradients_match_gsplat_torch(name, L):
    """colours [C,N,3] and the gradients of sum(colours * cot) for the coefficients, the means and the camera positions, all in fp64 on
    both sides: rel-L2 <= 1e-12 (the same polynomials of a few hundred operations)."""
    inp, _, _, rec = _scene(name)
    sh = torch.from_numpy(inp["sh"]).double().requires_grad_(True)
    means = torch.from_numpy(inp["means"]).double().requires_grad_(True)
    campos = torch.linalg.inv(torch.from_numpy(inp["viewmats"]).double())[:, :3, 3].clone().requires_grad_(True)
    vis = torch.from_numpy((rec["radii"] > 0).all(-1))
    colors = SH.sh_colors(means, sh, campos, L, vis)
    g = torch.autograd.grad((colors * torch.from_numpy(rec["cot"]).double()).sum(), [sh, means, campos])
    errs = {"colours": rel_l2(colors.detach().numpy(), rec[f"colors_L{L}"]), "sh": rel_l2(g[0].numpy(), rec[f"grad_sh_L{L}"]),
            "means": rel_l2(g[1].numpy(), rec[f"grad_means_L{L}"]), "campos": rel_l2(g[2].numpy(), rec[f"grad_campos_L{L}"])}
    print(name, "L", L, "helper against gsplat torch:", errs)
    clamped = float((colors.detach()[vis] == 0).double().mean())
    assert 0.05 < clamped < 0.25, clamped                       # the clamp is exercised without dominating
    assert float(np.abs(rec[f"grad_campos_L{L}"]).min()) > 0 and float(np.abs(rec[f"grad_means_L{L}"]).max()) > 0
    for k, e in errs.items():
        assert e <= 1e-12, (k, e)
    # bands at or above (L + 1)^2 are not read: exact-zero gradient, in the helper and in the record
    nb = (L + 1) ** 2
    assert not g[0][:, nb:].any() and not rec[f"grad_sh_L{L}"][:, nb:].any() and g[0][:, :nb].abs().sum() > 0


def test_helper_renders_through_the_restatement():
    """rasterize_sh goes through raster_grad_helper.project / composite one camera at a time: shapes, and degree 1 with zero higher bands
    is the degree-0 restatement up to rounding (fp64: 1e-14)."""
    import raster_grad_helper as RG
    inp, W, H, _ = _scene(CASES[0])
    t = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    sh = t["sh"].clone()
    sh[:, 1:] = 0
    outs = SH.rasterize_sh(t["means"], t["quats"], t["scales"], t["opacities"], sh, 1, t["viewmats"], t["Ks"], W, H)
    want = RG.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], sh[:, 0], True, t["viewmats"], t["Ks"], W, H)
    C = inp["viewmats"].shape[0]
    assert [tuple(o.shape) for o in outs] == [(C, H, W, 3), (C, H, W, 1), (C, H, W, 1)]
    for a, b in zip(outs, want):
        assert rel_l2(a.numpy(), b.numpy()) < 1e-14


def test_exports_name_the_sh_entries():
    from hunyuanworld_mirror_amd import _lib
    for name in ("wm_rasterize_splats_sh", "wm_rasterize_backward_workspace_bytes_sh", "wm_rasterize_splats_backward_sh"):
        assert name in _lib.EXPORTS, name
