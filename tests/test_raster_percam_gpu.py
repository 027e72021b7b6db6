"""Per-camera colours in the rasteriser: colors [C,N,3] with sh_degree = None (colors_are_sh0 = WM_COLORS_PER_CAMERA of the entries with
options), on the committed raster scenes (raster_600g_2c_80x56, raster_1500g_3c_100x70: the inputs of the raster_grad_* / raster_modes_*
fixtures).  Everything here is an exact statement: the same colours with a camera axis give the same bits as the shared-colour call, and
camera c of a per-camera call gives the bits of a one-camera call with that camera's colours."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("raster_600g_2c_80x56", "raster_1500g_3c_100x70")
SPLATS = ("means", "quats", "scales", "opacities", "colors")
ROUTES = ("splats", "info", "camera", "rasterization", "antialiased+backgrounds", "batches")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> CPU fp32 tensors (colors [N,3] in (0.1, 0.9), per-camera colours [C,N,3], backgrounds, cotangents), width, height"""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    t = {k: torch.from_numpy(z["in_" + k].astype(np.float32)) for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    W, H, V, N = int(z["width"]), int(z["height"]), t["viewmats"].shape[0], t["means"].shape[0]
    g = torch.Generator().manual_seed(17 + N)
    t["colors"] = 0.1 + 0.8 * torch.rand(N, 3, generator=g)
    t["colors_pc"] = 0.1 + 0.8 * torch.rand(V, N, 3, generator=g)
    t["backgrounds"] = torch.rand(V, 3, generator=g)
    t["cot"] = [torch.randn(V, H, W, ch, generator=g) for ch in (3, 1, 1)]
    t["camtoworlds"] = torch.linalg.inv(t["viewmats"].double()).float()
    return t, W, H


def _run(name, colors, route, cams=None):
    """One forward + backward.  colors: CPU [N,3] or [C,N,3]; cams: None or the list of cameras to render.
    -> dict of CPU tensors: rgb, depth, alpha, the splat gradients and, where the route has them, radii, means2d, v_means2d, v_cameras"""
    import hunyuanworld_mirror_amd as wm
    t, W, H = _scene(name)
    sel = slice(None) if cams is None else cams
    d = {k: t[k].to(DEV).requires_grad_(True) for k in SPLATS[:4]}
    d["colors"] = colors.to(DEV).requires_grad_(True)
    args = [d[k] for k in SPLATS]
    c2w, vm, Ks = t["camtoworlds"][sel].to(DEV), t["viewmats"][sel].to(DEV), t["Ks"][sel].to(DEV)
    cot = [c[sel].to(DEV) for c in t["cot"]]
    info, cam = None, None
    if route == "splats":
        rgb, depth, alpha = wm.Rasterizer().rasterize_splats(*args, c2w, Ks, W, H, sh_degree=None)
    elif route == "info":
        rgb, depth, alpha, info = wm.Rasterizer().rasterize_splats(*args, c2w, Ks, W, H, sh_degree=None, return_info=True, absgrad=True)
    elif route == "camera":
        cam = c2w.requires_grad_(True)
        rgb, depth, alpha = wm.Rasterizer(camera_grad=True).rasterize_splats(*args, cam, Ks, W, H, sh_degree=None)
    elif route == "batches":
        b = lambda x: x.unsqueeze(0)
        rgb, depth, alpha = (o[0] for o in wm.Rasterizer().rasterize_batches(*(b(a) for a in args), b(c2w), b(Ks), W, H, sh_degree=None))
    else:
        kw = {}
        if route == "antialiased+backgrounds":
            kw = dict(rasterize_mode="antialiased", backgrounds=t["backgrounds"][sel].to(DEV).requires_grad_(True), eps2d=0.35, near_plane=0.05)
        cam = vm.requires_grad_(True)
        out, alpha, info = wm.rasterization(*args, cam, Ks, W, H, sh_degree=None, render_mode="RGB+ED", absgrad=True, **kw)
        rgb, depth = out[..., :3], out[..., 3:]
        if kw:
            d["backgrounds"] = kw["backgrounds"]
    if info is not None:
        info["means2d"].retain_grad()
    (rgb * cot[0]).sum().add((depth * cot[1]).sum()).add((alpha * cot[2]).sum()).backward()
    torch.cuda.synchronize()
    res = dict(rgb=rgb, depth=depth, alpha=alpha, **{"v_" + k: v.grad for k, v in d.items()})
    if info is not None:
        res.update(radii=info["radii"], means2d=info["means2d"], v_means2d=info["means2d"].grad, v_means2d_abs=info["means2d"].absgrad)
    if cam is not None:
        res["v_cameras"] = cam.grad
    return {k: v.detach().cpu() for k, v in res.items()}


def _same(a, b, skip=("v_colors",)):
    assert set(a) == set(b)
    bad = [k for k in a if k not in skip and not torch.equal(a[k], b[k])]
    assert not bad, bad


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SCENES)
def test_gpu_the_same_colours_with_a_camera_axis_give_the_same_bits(name, route):
    t, W, H = _scene(name)
    V = t["viewmats"].shape[0]
    shared = _run(name, t["colors"], route)
    pc = _run(name, t["colors"][None].expand(V, -1, -1).contiguous(), route)
    _same(shared, pc)
    assert pc["v_colors"].shape == (V, t["means"].shape[0], 3)
    total = pc["v_colors"][0].clone()
    for c in range(1, V):
        total = total + pc["v_colors"][c]          # camera order, fp32: the order of the shared call's accumulation
    assert torch.equal(total, shared["v_colors"])
    assert shared["v_colors"].abs().sum() > 0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SCENES)
def test_gpu_each_camera_renders_its_own_colours(name, route):
    t, W, H = _scene(name)
    V = t["viewmats"].shape[0]
    pc = _run(name, t["colors_pc"], route)
    for c in range(V):
        one = _run(name, t["colors_pc"][c], route, cams=[c])
        for k in ("rgb", "depth", "alpha"):
            assert torch.equal(pc[k][c], one[k][0]), (c, k)
        assert torch.equal(pc["v_colors"][c], one["v_colors"]), c
    if "radii" in pc:
        culled = (pc["radii"] <= 0).any(-1)
        assert int(culled.sum()) > 0 and not pc["v_colors"][culled].any()      # exact zeros, and there are culled pairs to show it
        assert pc["v_colors"][~culled].abs().sum() > 0


def test_gpu_c_abi_writes_every_slot_and_refuses_bad_colour_forms():
    """wm_rasterize_splats_opt / _backward_opt directly: v_colors [C,N,3] pre-filled with NaN comes back without one (zeros where culled)
    and equals the autograd result; colors_are_sh0 = 2 with sh_degree = 1, and = 3, return WM_ERR_INVALID before any launch."""
    import importlib
    from hunyuanworld_mirror_amd import _lib
    R = importlib.import_module("hunyuanworld_mirror_amd.rasterization")      # (the package exports a function of the same name)
    name = SCENES[0]
    t, W, H = _scene(name)
    L = _lib.lib()
    rz = R.Rasterizer()
    d = {k: t[k].to(DEV) for k in ("means", "quats", "scales", "opacities", "camtoworlds", "Ks")}
    cin = t["colors_pc"].to(DEV)
    V, N = cin.shape[:2]
    radii = torch.empty((V, N, 2), device=DEV, dtype=torch.int32)
    opts = R._Opts(0, 0, **R._OPTION_DEFAULTS)
    rgb, depth, alpha, state = rz._forward(d["means"], d["quats"], d["scales"], d["opacities"], cin, R.PER_CAMERA, d["camtoworlds"], d["Ks"], W, H,
                                           own_workspace=True, radii=radii, opts=opts)
    means, quats, scales, opac, cin, viewmats, Ks, ws, cap, n = state[:10]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    cot = [c.to(DEV).contiguous() for c in t["cot"]]
    g = [torch.empty_like(x) for x in (means, quats, scales, opac)]
    v_col = torch.full_like(cin, float("nan"))
    gws = torch.empty(L.wm_rasterize_backward_workspace_bytes_opt(N, V, W, H, n, 0, 0, 0, 0, 0), device=DEV, dtype=torch.uint8)
    assert gws.numel() == L.wm_rasterize_backward_workspace_bytes(N, V, W, H, n)            # workspace sizes are unchanged
    head = (p(means), p(quats), p(scales), p(opac), p(cin))
    mid = (N, p(viewmats), p(Ks), V, W, H, C.byref(opts.struct(None)), p(ws), ws.numel(), cap, n, None, p(depth), None, p(cot[0]), p(cot[1]), p(cot[2]),
           p(g[0]), p(g[1]), p(g[2]), p(g[3]), p(v_col), None, None, 0, None, None, None, p(gws), gws.numel(), None)
    torch.cuda.synchronize()
    assert L.wm_rasterize_splats_backward_opt(*head, 2, 0, 0, None, *mid) == 0
    torch.cuda.synchronize()
    auto = _run(name, t["colors_pc"], "splats")
    assert torch.equal(v_col.cpu(), auto["v_colors"]) and torch.equal(g[0].cpu(), auto["v_means"])
    culled = (radii.cpu() <= 0).any(-1)
    assert int(culled.sum()) > 0 and not v_col.cpu()[culled].any()
    # refused before any launch: the outputs keep their fill
    v_col.fill_(7.0)
    campos = d["camtoworlds"][:, :3, 3].contiguous()
    assert L.wm_rasterize_splats_backward_opt(*head, 2, 4, 1, p(campos), *mid) == 1
    assert L.wm_rasterize_splats_backward_opt(*head, 3, 0, 0, None, *mid) == 1
    out = [torch.full_like(x, 7.0) for x in (rgb, depth, alpha)]
    nn = C.c_ulonglong(0)
    tail = (N, p(viewmats), p(Ks), V, W, H, C.byref(opts.struct(None)), p(out[0]), p(out[1]), p(out[2]), None, p(ws), ws.numel(), cap, C.byref(nn), None)
    assert L.wm_rasterize_splats_opt(*head, 2, 4, 1, p(campos), *tail) == 1
    assert L.wm_rasterize_splats_opt(*head, 3, 0, 0, None, *tail) == 1
    assert L.wm_rasterize_splats_opt(*head, -1, 0, 0, None, *tail) == 1
    torch.cuda.synchronize()
    assert bool((v_col == 7.0).all()) and all(bool((o == 7.0).all()) for o in out)


def test_gpu_a_wrong_camera_count_is_a_value_error_and_refusals_stay():
    import hunyuanworld_mirror_amd as wm
    t, W, H = _scene(SCENES[0])
    d = {k: t[k].to(DEV) for k in ("means", "quats", "scales", "opacities", "camtoworlds", "viewmats", "Ks")}
    args = (d["means"], d["quats"], d["scales"], d["opacities"])
    three = t["colors_pc"][:1].expand(3, -1, -1).contiguous().to(DEV)          # C' = 3 for two cameras
    with pytest.raises(ValueError):
        wm.Rasterizer().rasterize_splats(*args, three, d["camtoworlds"], d["Ks"], W, H, sh_degree=None)
    with pytest.raises(ValueError):
        wm.rasterization(*args, three, d["viewmats"], d["Ks"], W, H, sh_degree=None)
    with pytest.raises(ValueError):
        wm.rasterization(*args, t["colors_pc"][:, :5].contiguous().to(DEV), d["viewmats"], d["Ks"], W, H, sh_degree=None)
    with pytest.raises(NotImplementedError):
        wm.rasterization(*args, torch.zeros(4, 5, device=DEV), d["viewmats"], d["Ks"], W, H)
    with pytest.raises(NotImplementedError):
        wm.rasterization(*args, t["colors_pc"].to(DEV), d["viewmats"], d["Ks"], W, H, sh_degree=None, packed=True)
    with pytest.raises(NotImplementedError):
        wm.rasterization(*args, torch.zeros(600, 25, 3, device=DEV), d["viewmats"], d["Ks"], W, H, sh_degree=4)
    with pytest.raises(ValueError):
        wm.Rasterizer().rasterize_splats(*args, t["colors"].to(DEV), d["camtoworlds"], d["Ks"], W, H, sh_degree=0)
