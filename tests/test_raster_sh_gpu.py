"""View-dependent colour on the GPU: SH degrees 1-3 through Rasterizer.rasterize_splats (wm_rasterize_splats_sh / _backward_sh,
csrc/raster_sh.hip) against the fp64 torch restatement tests/raster_sh_helper.py (pinned to the reference by
tests/test_raster_sh_cpu.py), the agreement of the routes, the degree schedule of the reference trainer, the edges and the
optimisation loop.  Values measured on MI355X are recorded in profiles/r10_spherical_harmonics.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raster_sh_helper as SH
from conftest import rel_l2

pytestmark = pytest.mark.gpu
SPLATS = ("means", "quats", "scales", "opacities", "sh")
DEV = "cuda:0"


def _with_c2w(inp):
    """the scene with camtoworlds = the fp64 inverse of its viewmats rounded to fp32: the value the GPU and the helper both start from"""
    out = {k: v for k, v in inp.items() if k != "viewmats"}
    out["camtoworlds"] = torch.linalg.inv(torch.from_numpy(inp["viewmats"]).double()).float().numpy()
    return out


def _cotangents(V, H, W, seed=3, rgb=True):
    g = torch.Generator().manual_seed(seed)
    cot = [torch.randn(V, H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]
    if not rgb:
        cot[0][:] = 0
    return cot


@functools.lru_cache(maxsize=None)
def _scene(name):
    inp, W, H, _ = SH.load_scene(name)
    return _with_c2w(inp), W, H


@functools.lru_cache(maxsize=None)
def _yardstick(name, L):
    """(outputs, gradients) of the restatement in fp64 and in fp32 on a committed scene: computed once, shared, never written to"""
    inp, W, H = _scene(name)
    cot = _cotangents(inp["camtoworlds"].shape[0], H, W)
    return SH.gradients_sh(inp, cot, L, W, H, torch.float64), SH.gradients_sh(inp, cot, L, W, H, torch.float32)


def _run(inp, cot, L, W, H, camera_grad=False, splat_grad=True, return_info=False, absgrad=True, backward_twice=False):
    """One forward + backward through the Rasterizer.  L: sh_degree (0: degree 0 of the same [N,K,3] tensor).
    -> outputs, dict of gradients (camtoworlds: None where there is none), info"""
    from hunyuanworld_mirror_amd import Rasterizer
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    if splat_grad:
        for k in SPLATS:
            t[k].requires_grad_(True)
    t["camtoworlds"].requires_grad_(True)
    kw = dict(return_info=True, absgrad=absgrad) if return_info else {}
    res = Rasterizer(camera_grad=camera_grad).rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], t["sh"], t["camtoworlds"], t["Ks"],
                                                               W, H, sh_degree=L, **kw)
    outs, info = res[:3], (res[3] if return_info else None)
    if return_info:
        info["means2d"].retain_grad()
    loss = sum((o * torch.from_numpy(c).float().to(DEV)).sum() for o, c in zip(outs, cot))
    leaves = [t[k] for k in SPLATS + ("camtoworlds",) if t[k].requires_grad]
    if backward_twice:
        first = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        second = torch.autograd.grad(loss, leaves, allow_unused=True)
        torch.cuda.synchronize()
        return first, second
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: t[k].grad for k in SPLATS + ("camtoworlds",)}
    return outs, grads, info


def _np(x):
    return x.detach().double().cpu().numpy()


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name,L", [("raster_600g_2c_80x56", 1), ("raster_600g_2c_80x56", 2), ("raster_600g_2c_80x56", 3), ("raster_1500g_3c_100x70", 3)])
def test_gpu_sh_parity(name, L):
    """e64 = rel-L2(GPU, helper fp64) against e32 = rel-L2(helper fp32, helper fp64): e64 <= 4 e32 and e64 < 1e-3, for rgb / depth / alpha
    and the gradients of means, quats, scales, opacities, the coefficients [N,16,3] and camtoworlds (camera_grad=True)."""
    inp, W, H = _scene(name)
    cot = _cotangents(inp["camtoworlds"].shape[0], H, W)
    (o64, g64), (o32, g32) = _yardstick(name, L)
    outs, grads, _ = _run(inp, cot, L, W, H, camera_grad=True)
    pairs = [(k, _np(o), a, b) for k, o, a, b in zip(("rgb", "depth", "alpha"), outs, o32, o64)]
    pairs += [("grad " + k, _np(grads[k]), g32[k], g64[k]) for k in SH.NAMES]
    bad = []
    for k, got, h32, h64 in pairs:
        e32, e64 = rel_l2(h32, h64), rel_l2(got, h64)
        print(f"{name} L={L} {k}: e32 {e32:.3e} e64 {e64:.3e}")
        if not (np.isfinite(got).all() and e64 <= 4 * e32 and e64 < 1e-3):
            bad.append((k, e32, e64))
    assert grads["sh"].shape == (inp["sh"].shape[0], 16, 3) and not grads["sh"][:, (L + 1) ** 2:].any()
    assert float(np.abs(g64["camtoworlds"]).max()) > 0 and float(np.abs(g64["sh"][:, 1:(L + 1) ** 2]).max()) > 0
    assert not bad, bad


# ------------------------------------------------------------------ 2. routes agree
def test_gpu_sh_routes_give_the_same_bits():
    name, L = "raster_600g_2c_80x56", 3
    inp, W, H = _scene(name)
    cot = _cotangents(inp["camtoworlds"].shape[0], H, W)
    o_plain, plain, _ = _run(inp, cot, L, W, H)
    o_abs, info_abs, i_abs = _run(inp, cot, L, W, H, return_info=True, absgrad=True)
    _, info_no, i_no = _run(inp, cot, L, W, H, return_info=True, absgrad=False)
    o_cam, cam, _ = _run(inp, cot, L, W, H, camera_grad=True)
    _, cam_info, i_cam = _run(inp, cot, L, W, H, camera_grad=True, return_info=True, absgrad=True)
    assert plain["camtoworlds"] is None and info_abs["camtoworlds"] is None and cam["camtoworlds"] is not None
    for a, b, c in zip(o_plain, o_abs, o_cam):
        assert torch.equal(a, b) and torch.equal(a, c)
    for k in SPLATS:
        for other in (info_abs, info_no, cam, cam_info):
            assert torch.equal(plain[k], other[k]), k
        assert float(plain[k].abs().sum()) > 0, k
    assert torch.equal(cam["camtoworlds"], cam_info["camtoworlds"])
    assert torch.equal(i_abs["means2d"].grad, i_no["means2d"].grad) and torch.equal(i_abs["means2d"].grad, i_cam["means2d"].grad)
    assert torch.equal(i_abs["means2d"].absgrad, i_cam["means2d"].absgrad) and not hasattr(i_no["means2d"], "absgrad")
    # two backward calls on the same forward: identical bits, camtoworlds.grad included
    first, second = _run(inp, cot, L, W, H, camera_grad=True, backward_twice=True)
    assert len(first) == 6 and all(torch.equal(a, b) for a, b in zip(first, second))


def test_gpu_means2d_gradient_does_not_depend_on_the_degree():
    """means2d.grad with sh_degree=3 and sh_degree=0, same geometry, same image cotangent: the same bits.  The cotangent is that of
    depth and alpha (v_rgb = 0): through v_rgb the colours do enter the 2-D mean term (the compositing backward's alpha gradient holds
    colour x v_rgb), so with a colour cotangent the two differ as the colours do."""
    inp, W, H = _scene("raster_600g_2c_80x56")
    cot = _cotangents(inp["camtoworlds"].shape[0], H, W, rgb=False)
    _, g3, i3 = _run(inp, cot, 3, W, H, return_info=True)
    _, g0, i0 = _run(inp, cot, 0, W, H, return_info=True)
    assert float(i3["means2d"].grad.abs().sum()) > 0
    assert torch.equal(i3["means2d"].grad, i0["means2d"].grad) and torch.equal(i3["means2d"].absgrad, i0["means2d"].absgrad)
    assert torch.equal(i3["means2d"], i0["means2d"]) and torch.equal(i3["radii"], i0["radii"])
    assert not g3["sh"].any() and not g0["sh"].any()          # no colour cotangent: no colour gradient


# ------------------------------------------------------------------ 3. degree schedule
def test_gpu_degree_schedule():
    """the reference trainer's schedule: one [N,16,3] tensor rendered with sh_degree 0, 1, 2, 3"""
    from hunyuanworld_mirror_amd import Rasterizer
    inp, W, H = _scene("raster_600g_2c_80x56")
    cot = _cotangents(inp["camtoworlds"].shape[0], H, W)
    t = {k: torch.from_numpy(v).float().to(DEV) for k, v in inp.items()}
    rz = Rasterizer()
    render = lambda sh, L: rz.rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], sh, t["camtoworlds"], t["Ks"], W, H, sh_degree=L)
    # degree 0 of the 16-band tensor is the degree-0 render of its first band, bit for bit
    d0 = render(t["sh"], 0)
    assert all(torch.equal(a, b) for a, b in zip(d0, render(t["sh"][:, :1].contiguous(), 0)))
    imgs = [d0[0]] + [render(t["sh"], L)[0] for L in (1, 2, 3)]
    assert all(rel_l2(_np(imgs[i]), _np(imgs[i + 1])) > 1e-3 for i in range(3))      # every degree changes the picture
    # bands 1..15 zero: degree 3 is degree 0 up to a few fp32 roundings (the order of operations differs)
    flat = t["sh"].clone()
    flat[:, 1:] = 0
    for a, b in zip(render(flat, 3), render(flat, 0)):
        assert rel_l2(_np(a), _np(b)) < 1e-6
    # bands 4..15 are not read at degree 1: 1e30 there gives the bits zeros give, and exactly zero gradient
    huge, zero = dict(inp), dict(inp)
    huge["sh"], zero["sh"] = inp["sh"].copy(), inp["sh"].copy()
    huge["sh"][:, 4:], zero["sh"][:, 4:] = 1e30, 0.0
    o_h, g_h, _ = _run(huge, cot, 1, W, H, camera_grad=True)
    o_z, g_z, _ = _run(zero, cot, 1, W, H, camera_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(o_h, o_z))
    for k in SH.NAMES:
        assert torch.equal(g_h[k], g_z[k]) and torch.isfinite(g_h[k]).all(), k
    assert not g_h["sh"][:, 4:].any() and g_h["sh"][:, 1:4].abs().sum() > 0


# ------------------------------------------------------------------ 4. edges
def _tiny(N, V=3, K=16, seed=5, blind=None, W=33, H=18):
    """N Gaussians in front of V cameras that look down +z from shifted positions; blind: index of a camera turned the other way"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([1.6, 0.9]), 2.0 + u(N, 1)], 1)
    c2w = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    for c in range(V):
        a = 0.12 * c
        c2w[c, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c2w[c, :3, 3] = torch.tensor([0.45 * c, -0.05 * c, 0.1 * c])
    if blind is not None:
        c2w[blind, :3, :3] = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    Ks = torch.tensor([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], dtype=torch.float64).repeat(V, 1, 1)
    sh = torch.cat([2.0 * (u(N, 1, 3) - 0.3), 1.2 * (u(N, K - 1, 3) - 0.5)], 1)
    inp = dict(means=means, quats=torch.randn(N, 4, generator=g, dtype=torch.float64), scales=torch.exp(-2.6 + 1.0 * u(N, 3)), opacities=0.3 + 0.6 * u(N),
               sh=sh, camtoworlds=c2w, Ks=Ks)
    return {k: v.float().numpy() for k, v in inp.items()}, W, H


def _check_against_helper(inp, cot, L, W, H, names, splat_grad=True):
    _, g64 = SH.gradients_sh(inp, cot, L, W, H, torch.float64)
    _, g32 = SH.gradients_sh(inp, cot, L, W, H, torch.float32)
    _, grads, _ = _run(inp, cot, L, W, H, camera_grad=True, splat_grad=splat_grad)
    for k in names:
        e32, e64 = rel_l2(g32[k], g64[k]), rel_l2(_np(grads[k]), g64[k])
        print(f"N={inp['means'].shape[0]} L={L} grad {k}: e32 {e32:.3e} e64 {e64:.3e}")
        assert np.abs(g64[k]).max() > 0 and e64 <= 4 * e32 and e64 < 1e-3, (k, e32, e64)
    return grads


@pytest.mark.parametrize("N", [1, 65, 130])
def test_gpu_sh_small_counts(N):
    """one Gaussian; 65 and 130: one lane and two lanes in the last wave of the camera-position sum"""
    inp, W, H = _tiny(N)
    if N == 1:
        inp["means"][0] = (0.1, -0.05, 2.5)
    _check_against_helper(inp, _cotangents(3, H, W, seed=7), 3, W, H, SH.NAMES)


def test_gpu_sh_pose_only():
    """no splat tensor requires grad, camera_grad=True, degree 2"""
    inp, W, H = _tiny(130, seed=9)
    grads = _check_against_helper(inp, _cotangents(3, H, W, seed=8), 2, W, H, ("camtoworlds",), splat_grad=False)
    assert all(grads[k] is None for k in SPLATS)


def _c_sh(inp, cot, L, W, H, fill=0, want_campos=True, want_viewmats=True):
    """wm_rasterize_splats_sh + wm_rasterize_splats_backward_sh on device tensors.  fill: the byte the gradient workspace holds before.
    -> forward status, backward status, v_sh, v_means, v_viewmats, v_campos"""
    from hunyuanworld_mirror_amd import _lib
    lib = _lib.lib()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV).contiguous() for k, v in inp.items()}
    vm, campos = torch.linalg.inv(t["camtoworlds"]).contiguous(), t["camtoworlds"][:, :3, 3].contiguous()
    N, V, K = t["means"].shape[0], vm.shape[0], t["sh"].shape[1]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [torch.empty(V, H, W, 3, device=DEV), torch.empty(V, H, W, device=DEV), torch.empty(V, H, W, device=DEV)]
    cap = 1 << 16
    ws = torch.empty(lib.wm_rasterize_workspace_bytes(N, V, W, H, cap), device=DEV, dtype=torch.uint8)
    n = C.c_ulonglong(0)
    head = (p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(t["sh"]), K, L, p(campos), N, p(vm), p(t["Ks"]), V, W, H)
    st_f = lib.wm_rasterize_splats_sh(*head, p(o[0]), p(o[1]), p(o[2]), None, p(ws), ws.numel(), cap, C.byref(n), stream)
    if st_f != 0:
        return st_f, None, None, None, None, None
    need = lib.wm_rasterize_backward_workspace_bytes_sh(N, V, W, H, n.value, 0, int(want_viewmats), int(want_campos))
    gws = torch.full((need,), fill, device=DEV, dtype=torch.uint8)
    g = [torch.empty_like(t[k]) for k in SPLATS]
    v_vm = torch.full((V, 4, 4), float("nan"), device=DEV) if want_viewmats else None
    v_cp = torch.full((V, 3), float("nan"), device=DEV) if want_campos else None
    c = [torch.from_numpy(x).float().to(DEV).contiguous() for x in cot]
    st_b = lib.wm_rasterize_splats_backward_sh(*head, p(ws), ws.numel(), cap, n.value, None, p(o[1]), None, p(c[0]), p(c[1]), p(c[2]),
                                               *[p(x) for x in g], None, None, 0, p(v_vm), p(v_cp), p(gws), gws.numel(), stream)
    torch.cuda.synchronize()
    return st_f, st_b, g[4], g[0], v_vm, v_cp


def test_gpu_sh_camera_that_sees_nothing():
    """camera 1 of 3 looks away: its v_campos (and v_viewmats) row is exact zeros, and the rows of the other cameras are the bits of the
    two-camera call without it.  Nothing depends on what the gradient workspace held; without v_campos the other outputs keep their bits."""
    inp, W, H = _tiny(130, V=3, blind=1)
    cot = _cotangents(3, H, W, seed=11)
    st_f, st_b, v_sh, v_means, v_vm, v_cp = _c_sh(inp, cot, 3, W, H)
    assert (st_f, st_b) == (0, 0)
    assert not v_cp[1].any() and not v_vm[1].any() and v_cp[0].abs().min() > 0 and v_cp[2].abs().min() > 0 and not v_vm[:, 3].any()
    keep = [0, 2]
    two = {k: (v[keep] if k in ("camtoworlds", "Ks") else v) for k, v in inp.items()}
    _, st2, v_sh2, v_means2, v_vm2, v_cp2 = _c_sh(two, [x[keep] for x in cot], 3, W, H)
    assert st2 == 0 and torch.equal(v_cp[keep], v_cp2) and torch.equal(v_vm[keep], v_vm2) and torch.equal(v_sh, v_sh2) and torch.equal(v_means, v_means2)
    ff = _c_sh(inp, cot, 3, W, H, fill=0xFF)
    assert all(torch.equal(a, b) for a, b in zip((v_sh, v_means, v_vm, v_cp), ff[2:]))
    bare = _c_sh(inp, cot, 3, W, H, want_campos=False, want_viewmats=False)
    assert bare[1] == 0 and torch.equal(bare[2], v_sh) and torch.equal(bare[3], v_means)
    # the C entries refuse what the Python surface refuses
    small = dict(inp, sh=inp["sh"][:, :8])
    assert _c_sh(inp, cot, 4, W, H)[0] == 1 and _c_sh(inp, cot, 0, W, H)[0] == 1 and _c_sh(small, cot, 2, W, H)[0] == 1     # WM_ERR_INVALID


def test_gpu_sh_gaussian_seen_by_one_camera():
    """a Gaussian visible in camera 0 only: its coefficient gradient is the bits of the one-camera call"""
    inp, W, H = _tiny(130, V=2, seed=13)
    inp["camtoworlds"][1, :3, 3] = (1.1, 0.0, 0.0)             # camera 1 far to the side: part of the scene leaves its image
    cot = _cotangents(2, H, W, seed=12)
    _, both, info = _run(inp, cot, 3, W, H, return_info=True)
    seen = (info["radii"] > 0).all(-1)
    only0 = seen[0] & ~seen[1]
    assert int(only0.sum()) >= 5 and int((seen[0] & seen[1]).sum()) >= 5
    one = {k: (v[:1] if k in ("camtoworlds", "Ks") else v) for k, v in inp.items()}
    _, single, _ = _run(one, [x[:1] for x in cot], 3, W, H)
    assert torch.equal(both["sh"][only0], single["sh"][only0]) and float(single["sh"][only0].abs().sum()) > 0
    both_seen = seen[0] & seen[1]
    assert not torch.equal(both["sh"][both_seen], single["sh"][both_seen])


@pytest.mark.parametrize("K,L", [(4, 1), (9, 2)])
def test_gpu_sh_exact_band_count(K, L):
    """K = (L + 1)^2: the bits of the 16-band call on its first K bands"""
    inp, W, H = _tiny(65, seed=15)
    cot = _cotangents(3, H, W, seed=14)
    o16, g16, _ = _run(inp, cot, L, W, H, camera_grad=True)
    oK, gK, _ = _run(dict(inp, sh=np.ascontiguousarray(inp["sh"][:, :K])), cot, L, W, H, camera_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(o16, oK)) and gK["sh"].shape == (65, K, 3)
    assert torch.equal(g16["sh"][:, :K], gK["sh"]) and not g16["sh"][:, K:].any() and float(gK["sh"][:, 1:].abs().sum()) > 0
    for k in ("means", "quats", "scales", "opacities", "camtoworlds"):
        assert torch.equal(g16[k], gK[k]), k


def test_gpu_sh_refuses_what_is_not_built():
    inp, W, H = _tiny(4)
    cot = _cotangents(3, H, W)
    with pytest.raises(NotImplementedError):
        _run(inp, cot, 4, W, H)
    with pytest.raises(ValueError):
        _run(dict(inp, sh=np.ascontiguousarray(inp["sh"][:, :8])), cot, 2, W, H)
    with pytest.raises(ValueError):
        _run(dict(inp, sh=np.ascontiguousarray(inp["sh"][:, :15])), cot, 3, W, H)


# ------------------------------------------------------------------ 5. in the loop
def test_gpu_sh_in_the_optimisation_loop():
    """10 steps: rasterize_splats(cat(sh0, shN), sh_degree=3, return_info=True) -> photometric_loss -> DefaultStrategy -> Adam per parameter,
    with one refinement.  No numeric bound: the pieces compose, shN follows N, every gradient is finite, shN.grad is not zero."""
    import hunyuanworld_mirror_amd as wm
    g = torch.Generator().manual_seed(21)
    N, W, H = 150, 64, 48
    u = lambda *s: torch.rand(*s, generator=g)
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([2.4, 1.8]), 2.0 + 1.5 * u(N, 1)], 1)
    vm = torch.eye(4).repeat(2, 1, 1)
    vm[1, :3, :3] = torch.tensor([[np.cos(0.15), 0, np.sin(0.15)], [0, 1, 0], [-np.sin(0.15), 0, np.cos(0.15)]], dtype=torch.float32)
    vm[1, :3, 3] = torch.tensor([0.2, -0.05, 0.1])
    c2w, Ks = torch.linalg.inv(vm).to(DEV), torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]]).repeat(2, 1, 1).to(DEV)
    true = dict(means=means, quats=torch.randn(N, 4, generator=g), scales=torch.exp(-2.6 + 1.2 * u(N, 3)), opacities=0.2 + 0.6 * u(N),
                sh=torch.cat([2.0 * (u(N, 1, 3) - 0.3), 0.8 * (u(N, 15, 3) - 0.5)], 1))
    rz = wm.Rasterizer()
    with torch.no_grad():
        f = lambda k: true[k].to(DEV)
        target = rz.rasterize_splats(f("means"), f("quats"), f("scales"), f("opacities"), f("sh"), c2w, Ks, W, H, sh_degree=3)[0]
    params = torch.nn.ParameterDict({"means": means + 0.03 * torch.randn(N, 3, generator=g), "scales": torch.log(true["scales"]), "quats": true["quats"].clone(),
                                     "opacities": torch.logit(true["opacities"]), "sh0": true["sh"][:, :1] + 0.2 * (u(N, 1, 3) - 0.5),
                                     "shN": torch.zeros(N, 15, 3)}).to(DEV)
    opts = {k: torch.optim.Adam([params[k]], lr=2e-2 / (20.0 if k == "shN" else 1.0)) for k in params}
    strat = wm.DefaultStrategy(refine_start_iter=0, refine_every=5, refine_stop_iter=9, grow_grad2d=0.012, absgrad=False, verbose=False)
    strat.check_sanity(params, opts)
    state = strat.initialize_state(scene_scale=10.0)
    gen = torch.Generator(device=DEV).manual_seed(1)
    sizes, shn_grad = [], []
    for step in range(10):
        rgb, _, _, info = rz.rasterize_splats(params["means"], params["quats"], torch.exp(params["scales"]), torch.sigmoid(params["opacities"]),
                                              torch.cat([params["sh0"], params["shN"]], 1), c2w, Ks, W, H, sh_degree=3, return_info=True, absgrad=False)
        loss = wm.photometric_loss(rgb, target, 0.2, "valid")[0]
        strat.step_pre_backward(params, opts, state, step, info)
        for o in opts.values():
            o.zero_grad()
        loss.backward()
        for k in params:
            assert params[k].grad is not None and params[k].grad.shape == params[k].shape and bool(torch.isfinite(params[k].grad).all()), (step, k)
        shn_grad.append(float(params["shN"].grad.abs().sum()))
        for o in opts.values():
            o.step()
        strat.step_post_backward(params, opts, state, step, info, generator=gen)
        sizes.append(len(params["means"]))
        assert params["shN"].shape == (sizes[-1], 15, 3) and params["sh0"].shape == (sizes[-1], 1, 3)
    print("N per step", sizes, "loss", float(loss.detach()), "sum |shN.grad|", shn_grad)
    assert len(set(sizes)) > 1 and all(x > 0 for x in shn_grad) and np.isfinite(float(loss.detach()))
