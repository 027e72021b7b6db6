"""Rasterizer.rasterize_splats(return_info=True) on the GPU: info["means2d"] / its .grad (wm_rasterize_splats_backward_ex) and
.absgrad, info["radii"], against the fp64 torch restatement tests/raster_grad_helper.py; the absgrad reference (sum over pixels of
|d (cotangent . outputs at that pixel) / d means2d|) is in tests/golden/absgrad_24g_2c_33x18.npz (tools/gen_golden_densify.py).
The project's rule: e64 = rel-L2(GPU, fp64) <= 4 e32 = 4 rel-L2(restatement fp32, fp64), and e64 < 1e-3."""
import os

import numpy as np
import pytest
import torch

import raster_grad_helper as RG
from conftest import GOLD, rel_l2

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]
NAMES = ("means", "quats", "scales", "opacities", "colors")
pytestmark = pytest.mark.gpu


def _load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    inp["colors"] = z["in_sh"][:, 0]
    return inp, int(z["width"]), int(z["height"])


def _helper(inp, cot, is_sh, W, H, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    radii, m2, depths, conics, _ = RG.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H)
    m2.retain_grad()
    col = torch.clamp_min(RG.SH_C0 * t["colors"] + 0.5, 0.0) if is_sh else t["colors"]
    outs = RG.composite(m2, conics, depths, t["opacities"], col, radii, W, H)
    sum((o * torch.from_numpy(c).to(dtype)).sum() for o, c in zip(outs, cot)).backward()
    return radii.numpy(), m2.detach().double().numpy(), m2.grad.double().numpy()


def _gpu(inp, cot, is_sh, W, H, return_info, absgrad=None):
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(dev) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    col = t["colors"][:, None, :] if is_sh else t["colors"]
    kw = dict(return_info=True, absgrad=absgrad) if return_info else {}
    res = Rasterizer().rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], col, torch.linalg.inv(t["viewmats"]), t["Ks"], W, H,
                                        sh_degree=0 if is_sh else None, **kw)
    info = res[3] if return_info else None
    if info is not None:
        info["means2d"].retain_grad()
    sum((o * torch.from_numpy(c).float().to(dev)).sum() for o, c in zip(res[:3], cot)).backward()
    torch.cuda.synchronize()
    return res[:3], {k: t[k].grad for k in NAMES}, info


@pytest.mark.parametrize("name", CASES)
def test_gpu_means2d_gradient(name):
    inp, W, H = _load(name)
    C_ = inp["viewmats"].shape[0]
    g = torch.Generator().manual_seed(3)
    cot = [torch.randn(C_, H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]
    radii, m64, g64 = _helper(inp, cot, True, W, H, torch.float64)
    _, m32, g32 = _helper(inp, cot, True, W, H, torch.float32)
    outs0, grads0, _ = _gpu(inp, cot, True, W, H, False)
    outs1, grads1, info = _gpu(inp, cot, True, W, H, True, absgrad=False)
    outs2, grads2, info2 = _gpu(inp, cot, True, W, H, True, absgrad=False)
    m2 = info["means2d"]
    assert m2.shape == (C_, inp["means"].shape[0], 2) and m2.dtype == torch.float32 and m2.grad is not None and not hasattr(m2, "absgrad")
    assert info["width"] == W and info["height"] == H and info["n_cameras"] == C_ and info["gaussian_ids"] is None
    assert info["radii"].dtype == torch.int32 and np.array_equal(info["radii"].cpu().numpy(), radii)
    for a, b in zip(outs0, outs1):
        assert torch.equal(a, b)
    for k in NAMES:                                       # the five parameter gradients: bitwise those of the plain route
        assert torch.equal(grads0[k], grads1[k]), k
        assert torch.equal(grads1[k], grads2[k]), k
    assert torch.equal(m2.grad, info2["means2d"].grad) and torch.equal(m2, info2["means2d"])      # run to run
    vis = (radii > 0).all(-1)
    gg, mm = m2.grad.double().cpu().numpy(), m2.detach().double().cpu().numpy()
    assert vis.any() and (~vis).any()
    assert float(np.abs(gg[~vis]).max()) == 0.0 and float(np.abs(mm[~vis]).max()) == 0.0
    e32, e64 = rel_l2(g32, g64), rel_l2(gg, g64)
    print(f"{name} v_means2d: e32 {e32:.3e} e64 {e64:.3e}")
    assert np.isfinite(gg).all() and e64 <= 4 * e32 and e64 < 1e-3, (e32, e64)
    e32m, e64m = rel_l2(m32[vis], m64[vis]), rel_l2(mm[vis], m64[vis])
    print(f"{name} means2d: e32 {e32m:.3e} e64 {e64m:.3e}")
    assert e64m <= 4 * e32m and e64m < 1e-3, (e32m, e64m)


def test_gpu_absgrad():
    z = dict(np.load(os.path.join(GOLD, "absgrad_24g_2c_33x18.npz")))
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "colors", "viewmats", "Ks")}
    W, H = int(z["width"]), int(z["height"])
    cot = [z["cot_rgb"], z["cot_depth"], z["cot_alpha"]]
    _, grads_a, info_a = _gpu(inp, cot, False, W, H, True, absgrad=True)
    _, grads_b, info_b = _gpu(inp, cot, False, W, H, True, absgrad=False)
    _, grads_c, info_c = _gpu(inp, cot, False, W, H, True)             # None: the constructor's abs_grad (True by default)
    ma, mb = info_a["means2d"], info_b["means2d"]
    assert np.array_equal(info_a["radii"].cpu().numpy(), z["radii"])
    assert torch.equal(ma.grad, mb.grad)                                # .grad does not depend on absgrad
    assert not hasattr(mb, "absgrad") and torch.equal(info_c["means2d"].absgrad, ma.absgrad)
    for k in NAMES:
        assert torch.equal(grads_a[k], grads_b[k]), k
    ab, gr = ma.absgrad.double().cpu().numpy(), ma.grad.double().cpu().numpy()
    assert ab.shape == gr.shape == z["absgrad64"].shape
    assert (ab >= np.abs(gr) * (1 - 1e-6)).all()
    vis = (z["radii"] > 0).all(-1)
    assert float(np.abs(ab[~vis]).max(initial=0.0)) == 0.0
    for name, got, r64, r32 in (("absgrad", ab, z["absgrad64"], z["absgrad32"]), ("grad", gr, z["grad64"], z["grad32"])):
        e32, e64 = rel_l2(r32.astype(np.float64), r64), rel_l2(got, r64)
        print(f"{name}: e32 {e32:.3e} e64 {e64:.3e}")
        assert e64 <= 4 * e32 and e64 < 1e-3, (name, e32, e64)
    with pytest.raises(TypeError):
        from hunyuanworld_mirror_amd import Rasterizer
        t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
        Rasterizer().rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], W, H, packed=True)


def test_gpu_means2d_is_not_a_route_to_the_splats():
    """means2d takes gradient from the images only: a loss that uses it directly is refused in backward(), not silently dropped;
    rasterize_batches does not take return_info."""
    from hunyuanworld_mirror_amd import Rasterizer
    inp, W, H = _load(CASES[0])
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(dev) for k, v in inp.items()}
    t["means"].requires_grad_(True)
    c2w = torch.linalg.inv(t["viewmats"])
    rz = Rasterizer()
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :], c2w, t["Ks"], W, H)
    for loss_of in (lambda rgb, m2: rgb.sum() + m2.sum(), lambda rgb, m2: m2.sum()):
        rgb, _, _, info = rz.rasterize_splats(*args, sh_degree=0, return_info=True)
        with pytest.raises(NotImplementedError):
            loss_of(rgb, info["means2d"]).backward()
    rgb, _, _, info = rz.rasterize_splats(*args, sh_degree=0, return_info=True)      # without retain_grad the plain use still works
    rgb.sum().backward()
    assert t["means"].grad is not None and float(t["means"].grad.abs().sum()) > 0
    with pytest.raises(TypeError):
        rz.rasterize_batches(*[x[None] for x in args[:7]], W, H, sh_degree=0, return_info=True)
