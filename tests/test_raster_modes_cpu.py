"""gsplat.rasterization's options, CPU side: the torch restatement the GPU tests compare with (tests/raster_modes_helper.py) is itself
pinned — compensations, radii and projection gradients (compensation cotangent included) to the reference's own gsplat torch
implementation under two settings of (eps2d, near_plane, far_plane) (tests/golden/raster_modes_*.npz, tools/gen_raster_modes_golden.py),
backgrounds and depth modes to rendering.py's formulas written out here — and the option checks of the C ABI entries, which sit in front
of the first HIP call, are exercised without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raster_grad_helper as RG
import raster_modes_helper as RM
from conftest import GOLD, rel_l2

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]
SETTINGS = ["default", "cut"]


def _load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    inp["colors"] = z["in_sh"][:, 0]
    return z, inp, int(z["width"]), int(z["height"]), np.load(os.path.join(GOLD, name.replace("raster_", "raster_modes_") + ".npz"))


@pytest.mark.parametrize("tag", SETTINGS)
@pytest.mark.parametrize("name", CASES)
def test_helper_compensations_radii_and_gradients_match_gsplat_torch(name, tag):
    """the tolerances of test_raster_backward_cpu.test_helper_projection_gradients_match_gsplat_torch: radii equal, rel-L2 < 1e-9"""
    z, s, W, H, gz = _load(name)
    eps2d, near, far = (float(x) for x in gz[tag + "_setting"])
    t = {k: torch.from_numpy(s[k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    for k in ("means", "quats", "scales"):
        t[k].requires_grad_(True)
    radii, m2, depths, conics, _, comp = RM.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H, eps2d, near, far)
    assert np.array_equal(radii.numpy(), gz[tag + "_radii"])
    vis = (radii > 0).all(-1)
    assert int(vis.sum()) == int(gz[tag + "_visible"])
    if tag == "cut":       # the planes cut through the scene: fewer pairs than by default, more than a third of them
        assert int(gz["default_visible"]) / 3 < int(vis.sum()) < int(gz["default_visible"])
    e_comp = rel_l2(comp.detach().numpy()[vis.numpy()], gz[tag + "_compensations"][vis.numpy()])
    e_con = rel_l2(conics.detach().numpy()[vis.numpy()], gz[tag + "_conics"][vis.numpy()])
    print(name, tag, "visible", int(vis.sum()), "compensations", e_comp, "conics", e_con)
    assert e_comp < 1e-9 and e_con < 1e-9
    assert float(comp.detach()[vis].min()) > 0 and float(comp.detach()[vis].max()) < 1
    zero = lambda x: torch.where(vis if x.dim() == 2 else vis[..., None], x, torch.zeros_like(x))
    loss = sum((zero(v) * torch.from_numpy(gz[f"{tag}_cot_{k}"])).sum()
               for k, v in (("means2d", m2), ("depths", depths), ("conics", conics), ("compensations", comp)))
    g = torch.autograd.grad(loss, [t["means"], t["quats"], t["scales"]])
    for k, gi in zip(("means", "quats", "scales"), g):
        e = rel_l2(gi.numpy(), gz[f"{tag}_grad_{k}"])
        print(name, tag, k, e)
        assert e < 1e-9, (k, e)


def test_helper_defaults_are_the_gradient_helper():
    z, s, W, H, _ = _load(CASES[0])
    t = {k: torch.from_numpy(v).double() for k, v in s.items()}
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], True, t["viewmats"], t["Ks"], W, H)
    with torch.no_grad():
        a, b = RG.rasterize(*args), RM.rasterize(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_helper_backgrounds_depth_modes_and_radius_clip():
    """rendering.py:926-939 (render_colors + backgrounds * (1 - render_alphas), colour channels only) and :984-992 (the expected depth is
    the accumulated depth / render_alphas.clamp(min=1e-10)), written out; radius_clip: ProjectionEWA3DGSFused.cu's rule restated."""
    z, s, W, H, _ = _load(CASES[0])
    t = {k: torch.from_numpy(v).double() for k, v in s.items()}
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], True, t["viewmats"], t["Ks"], W, H)
    bg = torch.tensor([[0.1, 0.5, 0.9], [1.0, 0.0, 0.25]], dtype=torch.float64)
    with torch.no_grad():
        rgb, ed, al = RM.rasterize(*args, antialiased=True)
        rgb_b, ed_b, al_b = RM.rasterize(*args, antialiased=True, backgrounds=bg)
        _, d, al_d = RM.rasterize(*args, antialiased=True, depth_mode="D")
        _, d_b, _ = RM.rasterize(*args, antialiased=True, depth_mode="D", backgrounds=bg)
    assert torch.equal(rgb_b, rgb + bg[:, None, None, :] * (1.0 - al))
    assert torch.equal(ed_b, ed) and torch.equal(al_b, al) and torch.equal(d_b, d) and torch.equal(al_d, al)
    assert rgb.shape == (2, H, W, 3) and ed.shape == (2, H, W, 1) and d.shape == (2, H, W, 1) and al.shape == (2, H, W, 1)
    assert rel_l2((d / al.clamp(min=1e-10)).numpy(), ed.numpy()) < 1e-14
    m = al[..., 0] > 1e-3
    assert float((d[..., 0][m] / al[..., 0][m]).min()) > 0 and float(d[al == 0].abs().max() if (al == 0).any() else 0.0) == 0.0
    assert float((d - ed).abs().max()) > 1e-3           # the two depth channels do differ
    # antialiasing dims every splat (comp < 1): less is covered overall (per pixel the stop rule may go either way)
    with torch.no_grad():
        _, _, al_c = RM.rasterize(*args)
    assert float(al.mean()) < float(al_c.mean()) and float((al_c - al).max()) > 1e-3
    # radius_clip between the smallest and the median radius: exactly the pairs with both radii <= clip leave
    r0 = RM.project(*args[:3], t["viewmats"], t["Ks"], W, H)[0]
    vis = (r0 > 0).all(-1)
    big = r0.max(-1).values[vis]
    clip = float((big.min() + big.median()) // 2)
    assert big.min() <= clip < big.median()
    r1 = RM.project(*args[:3], t["viewmats"], t["Ks"], W, H, radius_clip=clip)[0]
    gone = vis & ~(r1 > 0).all(-1)
    assert torch.equal(gone, vis & (r0 <= clip).all(-1)) and 0 < int(gone.sum()) < int(vis.sum())
    assert torch.equal(r1[~gone], r0[~gone]) and int(r1[gone].abs().sum()) == 0


def test_single_gaussian_closed_form_in_the_helper():
    """A pin on the helper alone (no library code runs here; the kernels meet the same closed form in test_raster_modes_gpu.py).
    One isotropic Gaussian on the optical axis: comp = s2 / (s2 + eps2d), alpha = min(0.999, o comp exp(-d^2 / (2 (s2 + eps2d)))),
    accumulated depth = alpha z, expected depth = z."""
    W = H = 32
    f, z0, s3, o = 40.0, 2.0, 0.05, 0.8
    for eps2d in (0.3, 0.1):
        T = lambda x: torch.tensor(x, dtype=torch.float64)
        t = dict(means=T([[0.0, 0.0, z0]]), quats=T([[1.0, 0, 0, 0]]), scales=T([[s3] * 3]), opacities=T([o]), colors=T([[0.7, 0.2, 0.5]]),
                 viewmats=torch.eye(4, dtype=torch.float64)[None], Ks=T([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]]))
        with torch.no_grad():
            rgb, d, al = RM.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], False, t["viewmats"], t["Ks"], W, H,
                                      antialiased=True, eps2d=eps2d, depth_mode="D")
        s2 = (f * s3 / z0) ** 2
        comp = s2 / (s2 + eps2d)
        want = min(0.999, o * comp * np.exp(-0.5 / (2 * (s2 + eps2d))))       # the centre pixels sit half a pixel off in x and y
        assert abs(float(al[0, H // 2, W // 2, 0]) - want) < 1e-12
        assert abs(float(d[0, H // 2, W // 2, 0]) - want * z0) < 1e-12


# ------------------------------------------------------------------------------------------------ the C ABI's option checks (no GPU)
def _opt_call(L, lib, opt, sh_degree=0, n_coeffs=0, campos=None):
    x = C.c_void_p(256)        # never dereferenced: the entry returns before anything is launched
    return L.wm_rasterize_splats_opt(x, x, x, x, x, 0, n_coeffs, sh_degree, campos, 4, x, x, 1, 32, 32, None if opt is None else C.byref(opt),
                                     x, x, x, None, x, 1 << 20, 16, None, None)


def test_invalid_options_are_refused_before_any_launch():
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    WM_ERR_INVALID = 1
    ok = dict(antialiased=0, depth_mode=0, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0, backgrounds=None)
    bad = [dict(eps2d=-0.1), dict(near_plane=2.0, far_plane=2.0), dict(near_plane=3.0, far_plane=1.0), dict(radius_clip=-1.0), dict(depth_mode=2),
           dict(depth_mode=-1), dict(antialiased=2), dict(eps2d=float("nan"))]
    for change in bad:
        assert _opt_call(L, _lib, _lib.wm_raster_options(**{**ok, **change})) == WM_ERR_INVALID, change
    good = _lib.wm_raster_options(**ok)
    x = C.c_void_p(256)
    for deg, k, cp in ((4, 25, x), (-1, 1, x), (2, 8, x), (2, 9, None)):      # a bad SH degree, too few bands, no campos
        assert _opt_call(L, _lib, good, deg, k, cp) == WM_ERR_INVALID, (deg, k)
    # the backward entry checks the same options, and that v_backgrounds comes with backgrounds and the forward's alpha
    b = L.wm_rasterize_splats_backward_opt
    args = lambda opt, v_bg, alpha: (x, x, x, x, x, 0, 0, 0, None, 4, x, x, 1, 32, 32, opt, x, 1 << 20, 16, 0, None, x, alpha, x, x, x, x, x, x, x, x,
                                     None, None, 0, None, None, v_bg, x, 1 << 20, None)
    assert b(*args(C.byref(_lib.wm_raster_options(**{**ok, "eps2d": -1.0})), None, None)) == WM_ERR_INVALID
    assert b(*args(C.byref(good), x, x)) == WM_ERR_INVALID          # v_backgrounds without options->backgrounds
    assert b(*args(None, x, x)) == WM_ERR_INVALID


def test_python_surface_refuses_what_is_not_built():
    import hunyuanworld_mirror_amd as P
    from hunyuanworld_mirror_amd import Rasterizer, rasterization
    assert P.rasterization is rasterization
    t = torch.zeros(4, 3)
    base = dict(means=t, quats=torch.zeros(4, 4), scales=t, opacities=torch.zeros(4), colors=t, viewmats=torch.eye(4)[None], Ks=torch.eye(3)[None],
                width=32, height=32)
    for kw in (dict(packed=True), dict(sparse_grad=True), dict(distributed=True), dict(tile_size=8), dict(camera_model="fisheye"), dict(with_ut=True),
               dict(with_eval3d=True), dict(colors=torch.zeros(4, 5)), dict(rolling_shutter=1), dict(render_mode="RGB+N"),
               dict(rasterize_mode="soft"), dict(sh_degree=4, colors=torch.zeros(4, 25, 3))):
        with pytest.raises(NotImplementedError) as e:
            rasterization(**{**base, **kw})
        key = next(iter(kw))
        assert key in str(e.value) or key == "colors" and "colors" in str(e.value), (kw, str(e.value))
    assert Rasterizer(rasterization_mode="antialiased").rasterization_mode == "antialiased"
    with pytest.raises(TypeError):
        Rasterizer().rasterize_splats(t, torch.zeros(4, 4), t, torch.zeros(4), t, torch.eye(4)[None], torch.eye(3)[None], 32, 32, render_mode="RGB")
