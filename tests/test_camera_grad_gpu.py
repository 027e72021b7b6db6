"""Camera-pose gradients on the GPU: wm_rasterize_splats_backward_cam through Rasterizer(camera_grad=True) and through the C entry,
against the fp64 torch restatement tests/raster_grad_helper.py differentiated with respect to viewmats (pinned to the reference by
tests/test_camera_grad_cpu.py), and pose refinement with pose.CameraOptModule.

Values measured on MI355X are recorded in profiles/r09_camera_gradients.md."""
import ctypes as C
import functools
import os
import time

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


def _cotangents(name):
    """the seeded randn cotangents of test_raster_backward_gpu.test_gpu_gradient_parity"""
    inp, W, H = _load(name)
    g = torch.Generator().manual_seed(3)
    return [torch.randn(inp["viewmats"].shape[0], H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]


def _helper_grads(inp, cot, is_sh, W, H, dtype):
    """-> dict of float64 numpy gradients of the restatement for the five splat inputs and viewmats"""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in inp.items()}
    names = NAMES + ("viewmats",)
    for k in names:
        t[k].requires_grad_(True)
    outs = RG.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], is_sh, t["viewmats"], t["Ks"], W, H)
    loss = sum((o * torch.from_numpy(c).to(dtype)).sum() for o, c in zip(outs, cot))
    g = torch.autograd.grad(loss, [t[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(t[k]) if gi is None else gi).double().numpy() for k, gi in zip(names, g)}


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(fp64 gradients, fp32 gradients) of the restatement on a committed scene: computed once, shared, never written to"""
    inp, W, H = _load(name)
    cot = _cotangents(name)
    return _helper_grads(inp, cot, True, W, H, torch.float64), _helper_grads(inp, cot, True, W, H, torch.float32)


def _autograd_run(inp, cot, is_sh, W, H, camera_grad, splat_grad=True, return_info=False, rz=None):
    """One forward + backward through the Rasterizer.  camtoworlds is the fp64 inverse of the scene's viewmats, rounded to fp32.
    -> outputs, dict of gradients (camtoworlds included, None where there is none), the camtoworlds given, info"""
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(dev) for k, v in inp.items()}
    if splat_grad:
        for k in NAMES:
            t[k].requires_grad_(True)
    c2w = torch.linalg.inv(torch.from_numpy(inp["viewmats"]).double()).float().to(dev).requires_grad_(True)
    col = t["colors"][:, None, :] if is_sh else t["colors"]
    rz = rz or Rasterizer(camera_grad=camera_grad)
    kw = dict(return_info=True, absgrad=True) if return_info else {}
    res = rz.rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], col, c2w, t["Ks"], W, H, sh_degree=0 if is_sh else None, **kw)
    outs, info = res[:3], (res[3] if return_info else None)
    if return_info:
        info["means2d"].retain_grad()
    loss = sum((o * torch.from_numpy(c).float().to(dev)).sum() for o, c in zip(outs, cot))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: t[k].grad for k in NAMES}
    grads["camtoworlds"] = c2w.grad
    return outs, grads, c2w.detach(), info


def _viewmats_grad_from(c2w, c2w_grad):
    """viewmats = inv(camtoworlds), so d loss / d viewmats = -camtoworlds^T (d loss / d camtoworlds) camtoworlds^T; in fp64"""
    A = c2w.double().cpu()
    return (-A.transpose(-1, -2) @ c2w_grad.double().cpu() @ A.transpose(-1, -2)).numpy()


@pytest.mark.parametrize("name", CASES)
def test_gpu_camera_gradient_parity(name):
    """e64 = rel-L2(GPU, helper fp64) against e32 = rel-L2(helper fp32, helper fp64), for the 3 x 4 block of the viewmats gradient:
    e64 <= 4 e32 and e64 < 1e-3.  The GPU value is camtoworlds.grad pulled back through the inverse in fp64.  The bottom rows of
    v_viewmats (seen through the C entry) are exactly 0; the five splat gradients are the bits of a camera_grad=False rasteriser."""
    inp, W, H = _load(name)
    cot = _cotangents(name)
    g64, g32 = _yardstick(name)
    outs_on, on, c2w, _ = _autograd_run(inp, cot, True, W, H, camera_grad=True)
    outs_off, off, _, _ = _autograd_run(inp, cot, True, W, H, camera_grad=False)
    assert off["camtoworlds"] is None and on["camtoworlds"] is not None
    assert all(torch.equal(a, b) for a, b in zip(outs_on, outs_off))          # forward: same bits
    for k in NAMES:
        assert torch.equal(on[k], off[k]), k
    gv = _viewmats_grad_from(c2w, on["camtoworlds"])
    e32, e64 = rel_l2(g32["viewmats"][:, :3], g64["viewmats"][:, :3]), rel_l2(gv[:, :3], g64["viewmats"][:, :3])
    # the same scene through the C entry, on the scene's own fp32 viewmats: v_viewmats itself, whose bottom rows are exact zeros
    t = _dev(inp)
    t["colors"] = torch.clamp_min(RG.SH_C0 * t["colors"] + 0.5, 0.0)
    st, v_vm, _ = _c_backward(t, torch.from_numpy(inp["viewmats"]).cuda(), torch.from_numpy(inp["Ks"]).cuda(), W, H, [torch.from_numpy(c).cuda() for c in cot])
    assert st == 0 and float(v_vm[:, 3].abs().max()) == 0.0 and np.all(g64["viewmats"][:, 3] == 0)
    e64_c = rel_l2(v_vm[:, :3].double().cpu().numpy(), g64["viewmats"][:, :3])
    print(f"{name} grad viewmats: e32 {e32:.3e} e64 {e64:.3e} (through camtoworlds.grad), {e64_c:.3e} (v_viewmats of the C entry)")
    assert np.isfinite(gv).all()
    assert e64 <= 4 * e32 and e64 < 1e-3, (e32, e64)


@pytest.mark.parametrize("name", CASES)
def test_gpu_camera_gradient_both_routes(name):
    inp, W, H = _load(name)
    cot = _cotangents(name)
    _, plain, _, _ = _autograd_run(inp, cot, True, W, H, camera_grad=True)
    _, info_on, _, i_on = _autograd_run(inp, cot, True, W, H, camera_grad=True, return_info=True)
    _, info_off, _, i_off = _autograd_run(inp, cot, True, W, H, camera_grad=False, return_info=True)
    assert info_off["camtoworlds"] is None
    assert torch.equal(info_on["camtoworlds"], plain["camtoworlds"])
    assert torch.equal(i_on["means2d"], i_off["means2d"])
    assert torch.equal(i_on["means2d"].grad, i_off["means2d"].grad) and torch.equal(i_on["means2d"].absgrad, i_off["means2d"].absgrad)
    assert float(i_on["means2d"].grad.abs().sum()) > 0
    for k in NAMES:
        assert torch.equal(info_on[k], plain[k]) and torch.equal(info_on[k], info_off[k]), k


# ------------------------------------------------------------------ the C entry
def _c_backward(t, viewmats, Ks, W, H, cot, fill=None, short=0, sentinel=None):
    """wm_rasterize_splats + wm_rasterize_splats_backward_cam on device tensors (colours given, no SH).  fill: byte value the gradient
    workspace holds before the call; short: bytes the workspace is too small by.  -> status, v_viewmats [C,4,4], v_means [N,3]"""
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    dev = viewmats.device
    N, V = int(t["means"].shape[0]), int(viewmats.shape[0])
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [torch.empty(V, H, W, 3, device=dev), torch.empty(V, H, W, device=dev), torch.empty(V, H, W, device=dev)]
    cap = 1 << 16
    ws = torch.empty(L.wm_rasterize_workspace_bytes(N, V, W, H, cap), device=dev, dtype=torch.uint8)
    n = C.c_ulonglong(0)
    st = L.wm_rasterize_splats(p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(t["colors"]), 0, N, p(viewmats), p(Ks), V, W, H,
                               p(o[0]), p(o[1]), p(o[2]), None, p(ws), ws.numel(), cap, C.byref(n), stream)
    assert st == 0, st
    need = L.wm_rasterize_backward_workspace_bytes_cam(N, V, W, H, n.value, 0)
    assert need >= L.wm_rasterize_backward_workspace_bytes_ex(N, V, W, H, n.value, 0) + 96 * V * ((N + 63) // 64)
    gws = torch.full((need - short,), 0 if fill is None else fill, device=dev, dtype=torch.uint8)
    g = [torch.empty_like(t[k]) for k in NAMES]
    v_vm = torch.full((V, 4, 4), float("nan") if sentinel is None else sentinel, device=dev)
    st = L.wm_rasterize_splats_backward_cam(p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(t["colors"]), 0, N, p(viewmats), p(Ks),
                                            V, W, H, p(ws), ws.numel(), cap, n.value, None, p(o[1]), None, p(cot[0]), p(cot[1]), p(cot[2]),
                                            *[p(x) for x in g], None, None, 0, p(v_vm), p(gws), gws.numel(), stream)
    torch.cuda.synchronize()
    return st, v_vm, g[0]


def _dev(inp, keys=NAMES):
    return {k: torch.from_numpy(np.ascontiguousarray(inp[k])).float().cuda().contiguous() for k in keys}


@pytest.mark.parametrize("name", CASES)
def test_gpu_translation_identity(name):
    """One camera c alone: v_means[g] = Rv^T v_mc[g] and v_t = sum_g v_mc[g], so Rv^T v_viewmats[c,:3,3] = sum_g v_means[g] in real
    arithmetic.  Both sides in fp64 from the GPU's fp32 outputs; |difference| <= 64 * 2^-23 * sum_g |v_means[g]| (each v_means[g] is Rv^T
    applied to the fp32 terms the camera sum takes: ~3 multiply-adds of rounding per component + one store rounding, 10-15 units of
    2^-23; the bar leaves ~4 x; the restatement in fp32 sits at 0.08-0.31 units, |v_t| is 0.14-0.36 of the right-hand sum)."""
    inp, W, H = _load(name)
    cot_all = _cotangents(name)
    t = _dev(inp)
    t["colors"] = torch.clamp_min(RG.SH_C0 * t["colors"] + 0.5, 0.0)          # the C entry with final colours
    for c in range(inp["viewmats"].shape[0]):
        vm = torch.from_numpy(inp["viewmats"][c:c + 1]).cuda().contiguous()
        K = torch.from_numpy(inp["Ks"][c:c + 1]).cuda().contiguous()
        cot = [torch.from_numpy(np.ascontiguousarray(x[c:c + 1])).cuda() for x in cot_all]
        st, v_vm, v_means = _c_backward(t, vm, K, W, H, cot)
        assert st == 0 and float(v_vm[0, 3].abs().max()) == 0.0
        Rv = vm[0, :3, :3].double().cpu()
        lhs = Rv.T @ v_vm[0, :3, 3].double().cpu()
        rhs = v_means.double().cpu().sum(0)
        scale = float(v_means.double().cpu().norm(dim=1).sum())
        units = float((lhs - rhs).norm()) / (2.0 ** -23 * scale)
        print(f"{name} camera {c}: |Rv^T v_t - sum v_means| = {units:.3f} units of 2^-23 sum|v_means|, |v_t| / sum = {float(v_vm[0, :3, 3].double().norm()) / scale:.3f}")
        assert scale > 0 and units <= 64.0, units


def test_gpu_camera_gradient_surface():
    from hunyuanworld_mirror_amd import Rasterizer
    inp, W, H = _load(CASES[0])
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    c2w = torch.linalg.inv(t["viewmats"])
    rz, rz_off = Rasterizer(camera_grad=True), Rasterizer()
    args = lambda d, cam, K=None: (d["means"], d["quats"], d["scales"], d["opacities"], d["colors"][:, None, :], cam, t["Ks"] if K is None else K, W, H)
    loss_of = lambda o: o[0].square().sum() + o[1].sum() + 2 * o[2].sum()
    # camera_grad=True, nothing requires grad: the plain path
    plain = rz.rasterize_splats(*args(t, c2w), sh_degree=0)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    a = {k: v.clone().requires_grad_(k in NAMES) for k, v in t.items()}
    splat_only = rz.rasterize_splats(*args(a, c2w), sh_degree=0)                # a camtoworlds that does not require grad
    assert all(o.grad_fn is not None for o in splat_only) and all(torch.equal(x, y) for x, y in zip(plain, splat_only))
    cam = c2w.clone().requires_grad_(True)
    with torch.no_grad():
        ng = rz.rasterize_splats(*args(a, cam), sh_degree=0)
    assert all(o.grad_fn is None for o in ng) and all(torch.equal(x, y) for x, y in zip(plain, ng))
    # splats and camera
    Kg = t["Ks"].clone().requires_grad_(True)
    both = rz.rasterize_splats(*args(a, cam, Kg), sh_degree=0)
    assert all(torch.equal(x, y) for x, y in zip(plain, both))                  # forward: same bits
    loss_of(both).backward()
    assert Kg.grad is None
    g_both = cam.grad.clone()
    assert torch.isfinite(g_both).all() and float(g_both.abs().sum()) > 0
    # pose only: splats detached
    cam2 = c2w.clone().requires_grad_(True)
    pose_only = rz.rasterize_splats(*args(t, cam2), sh_degree=0)
    assert all(o.grad_fn is not None for o in pose_only) and all(torch.equal(x, y) for x, y in zip(plain, pose_only))
    loss_of(pose_only).backward()
    assert torch.isfinite(cam2.grad).all() and float(cam2.grad.abs().sum()) > 0 and torch.equal(cam2.grad, g_both)
    # ... and on the return_info route
    cam3 = c2w.clone().requires_grad_(True)
    r = rz.rasterize_splats(*args(t, cam3), sh_degree=0, return_info=True, absgrad=True)
    loss_of(r[:3]).backward()
    assert torch.equal(cam3.grad, g_both)
    # the default rasteriser leaves the camera alone
    cam4 = c2w.clone().requires_grad_(True)
    b = {k: v.clone().requires_grad_(k in NAMES) for k, v in t.items()}
    loss_of(rz_off.rasterize_splats(*args(b, cam4), sh_degree=0)).backward()
    assert cam4.grad is None and all(torch.equal(b[k].grad, a[k].grad) for k in NAMES)
    # the gradient reaches what produced camtoworlds
    from hunyuanworld_mirror_amd import CameraOptModule
    pose = CameraOptModule(2).to(dev)
    pose.zero_init()
    loss_of(rz.rasterize_splats(*args(t, pose(c2w, torch.arange(2, device=dev))), sh_degree=0)).backward()
    assert torch.isfinite(pose.embeds.weight.grad).all() and float(pose.embeds.weight.grad.abs().sum()) > 0
    # two forwards, then two backwards: each node owns its workspace -> bitwise the camera gradient of each pair run alone
    def leaf(shift):
        x = c2w.clone()
        x[:, 0, 3] += shift
        return x.requires_grad_(True)
    alone = []
    for sh in (0.0, 0.05):
        x = leaf(sh)
        loss_of(rz.rasterize_splats(*args(t, x), sh_degree=0)).backward()
        alone.append(x.grad.clone())
    assert not torch.equal(alone[0], alone[1])
    x1, x2 = leaf(0.0), leaf(0.05)
    o1 = rz.rasterize_splats(*args(t, x1), sh_degree=0)
    o2 = rz.rasterize_splats(*args(t, x2), sh_degree=0)
    rz.rasterize_splats(*args(t, c2w), sh_degree=0)                             # and a plain call on the shared workspace in between
    l1, l2 = loss_of(o1), loss_of(o2)
    l1.backward(retain_graph=True)
    l2.backward()
    assert torch.equal(x1.grad, alone[0]) and torch.equal(x2.grad, alone[1])
    # the same backward again: reproducible
    x1.grad = None
    l1.backward()
    assert torch.equal(x1.grad, alone[0])


def _edge_scene():
    g = torch.Generator().manual_seed(9)
    N, W, H = 65, 41, 29                                    # two waves of a four-wave block, the second with one live lane; ragged tiles
    u = lambda *s: torch.rand(*s, generator=g)
    t = dict(means=torch.cat([(u(N, 2) - 0.5) * torch.tensor([0.5, 0.35]), 1.2 + 0.6 * u(N, 1)], 1), quats=torch.randn(N, 4, generator=g),
             scales=torch.exp(-3.4 + 0.8 * u(N, 3)), opacities=0.2 + 0.7 * u(N), colors=u(N, 3))
    vm = torch.eye(4).repeat(2, 1, 1)
    a = 0.1
    vm[1, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    vm[1, :3, 3] = torch.tensor([0.05, -0.02, 0.1])
    K = torch.tensor([[60.0, 0, 20.5], [0, 60.0, 14.5], [0, 0, 1]]).repeat(2, 1, 1)
    cot = [torch.randn(2, H, W, ch, generator=g) for ch in (3, 1, 1)]
    return t, vm, K, cot, W, H


def test_gpu_camera_gradient_edges_through_the_c_entry():
    t_cpu, vm_cpu, K_cpu, cot_cpu, W, H = _edge_scene()
    t = {k: v.cuda().contiguous() for k, v in t_cpu.items()}
    vm, K, cot = vm_cpu.cuda(), K_cpu.cuda(), [c.cuda() for c in cot_cpu]
    # workspace independence: NaN patterns or zeros in the gradient workspace before the call
    st1, v_ff, _ = _c_backward(t, vm, K, W, H, cot, fill=0xFF)
    st0, v_00, _ = _c_backward(t, vm, K, W, H, cot, fill=0x00)
    assert st1 == 0 and st0 == 0
    assert torch.isfinite(v_ff).all() and torch.equal(v_ff, v_00) and float(v_ff.abs().sum()) > 0
    assert float(v_ff[:, 3].abs().max()) == 0.0
    inp = {k: v.numpy() for k, v in t_cpu.items()}
    inp.update(viewmats=vm_cpu.numpy(), Ks=K_cpu.numpy())
    g64 = _helper_grads(inp, [c.numpy() for c in cot_cpu], False, W, H, torch.float64)
    e = rel_l2(v_ff.double().cpu().numpy(), g64["viewmats"])
    print("edge scene (65 Gaussians, 41 x 29, 2 cameras): rel-L2 of v_viewmats to the fp64 restatement", e)
    assert e < 1e-3
    # everything behind the cameras
    behind = dict(t)
    behind["means"] = (t["means"] * torch.tensor([1.0, 1.0, -1.0], device="cuda")).contiguous()
    st, v, _ = _c_backward(behind, vm[:1].contiguous(), K[:1].contiguous(), W, H, [c[:1].contiguous() for c in cot])
    assert st == 0 and float(v.abs().max()) == 0.0
    # zero cotangents
    st, v, _ = _c_backward(t, vm, K, W, H, [torch.zeros_like(c) for c in cot])
    assert st == 0 and float(v.abs().max()) == 0.0
    # one camera sees the scene, the other looks away
    blind = vm.clone()
    blind[1] = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])).cuda()
    st, v2, _ = _c_backward(t, blind, K, W, H, cot)
    st_single, v1, _ = _c_backward(t, vm[:1].contiguous(), K[:1].contiguous(), W, H, [c[:1].contiguous() for c in cot])
    assert st == 0 and st_single == 0
    assert float(v2[1].abs().max()) == 0.0 and torch.equal(v2[0], v1[0]) and torch.equal(v2[0], v_ff[0])
    # a workspace one byte short: WM_ERR_INVALID, nothing launched (the output keeps what it held)
    st, v, _ = _c_backward(t, vm, K, W, H, cot, short=1, sentinel=7.0)
    assert st == 1 and bool((v == 7.0).all())


def _opt_scene():
    """the scene of test_raster_backward_gpu._opt_scene: 150 Gaussians, 64 x 48, 2 cameras (true splats only)"""
    g = torch.Generator().manual_seed(21)
    N, W, H = 150, 64, 48
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([2.4, 1.8]), 2.0 + 1.5 * u(N, 1)], 1)
    quats = torch.randn(N, 4, generator=g, dtype=torch.float64)
    scales = torch.exp(-2.6 + 1.2 * u(N, 3))
    opac = 0.2 + 0.6 * u(N)
    colors = u(N, 3)
    vm = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    vm[1, :3, :3] = torch.tensor([[np.cos(0.15), 0, np.sin(0.15)], [0, 1, 0], [-np.sin(0.15), 0, np.cos(0.15)]])
    vm[1, :3, 3] = torch.tensor([0.2, -0.05, 0.1])
    K = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], dtype=torch.float64).repeat(2, 1, 1)
    return dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors), vm, K, W, H


def test_gpu_pose_refinement_like_the_fp64_restatement():
    """True splats fixed, poses off by CameraOptModule noise (seed 5, std 0.02 on all 9 numbers); 30 Adam steps (lr 2e-3) on a
    zero-initialised CameraOptModule, L1 loss to the render from the true poses, on the GPU (fp32) and on the CPU restatement (fp64):
    the loss curves stay within 2 % of each other at every step, both final losses are below a quarter of their first, and the mean
    absolute pose error (over the 4 x 4 entries) ends below half its start.  The restatement alone: fp64 loss 0.0322 -> 0.0021, pose
    error 0.0081 -> 0.0017; its fp32 curve differs from the fp64 one by 6.0e-4."""
    from hunyuanworld_mirror_amd import CameraOptModule, Rasterizer
    true, vm, K, W, H = _opt_scene()
    dev = torch.device("cuda:0")
    c2w_true = torch.linalg.inv(vm)
    ids = torch.arange(2)
    noise = CameraOptModule(2).double()
    torch.manual_seed(5)
    noise.random_init(0.02)
    with torch.no_grad():
        c2w_start = noise(c2w_true, ids)

    def run(render, cast):
        with torch.no_grad():
            target = render(cast(c2w_true))
        pose = cast(CameraOptModule(2))
        pose.zero_init()
        opt = torch.optim.Adam(pose.parameters(), lr=2e-3)
        err = lambda: float((pose(cast(c2w_start), cast(ids)).detach().double().cpu() - c2w_true).abs().mean())
        curve, e0 = [], err()
        for _ in range(30):
            opt.zero_grad()
            loss = (render(pose(cast(c2w_start), cast(ids))) - target).abs().mean()
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
        return curve, e0, err()

    rz = Rasterizer(camera_grad=True)
    sg = {k: v.float().to(dev) for k, v in true.items()}
    Kg = K.float().to(dev)
    to_gpu = lambda x: x.to(dev) if isinstance(x, torch.nn.Module) or not x.is_floating_point() else x.float().to(dev)
    to_cpu = lambda x: x.double() if isinstance(x, torch.nn.Module) else x
    gpu, g0, g1 = run(lambda c: rz.rasterize_splats(sg["means"], sg["quats"], sg["scales"], sg["opacities"], sg["colors"], c, Kg, W, H)[0], to_gpu)
    cpu, c0, c1 = run(lambda c: RG.rasterize(true["means"], true["quats"], true["scales"], true["opacities"], true["colors"], False,
                                             torch.linalg.inv(c), K, W, H)[0], to_cpu)
    gap = max(abs(a - b) / b for a, b in zip(gpu, cpu))
    print(f"pose refinement: loss gpu {gpu[0]:.5f} -> {gpu[-1]:.5f}, cpu fp64 {cpu[0]:.5f} -> {cpu[-1]:.5f}, largest gap {gap:.3e}; "
          f"pose error gpu {g0:.5f} -> {g1:.5f}, cpu {c0:.5f} -> {c1:.5f}")
    assert gap < 0.02
    assert gpu[-1] < 0.25 * gpu[0] and cpu[-1] < 0.25 * cpu[0]
    assert g1 < 0.5 * g0 and c1 < 0.5 * c0


def test_gpu_camera_gradient_full_size():
    """4 views of 518 x 518, one splat per pixel (the inputs of test_gpu_backward_full_size): one forward + backward with camera_grad
    off and one with it on, the second round timed warm.  No time is asserted; the times go into profiles/r09_camera_gradients.md."""
    from hunyuanworld_mirror_amd import Rasterizer
    g = torch.Generator().manual_seed(5)
    N, V, W, H = 4 * 518 * 518, 4, 518, 518
    dev = torch.device("cuda:0")
    means = torch.cat([torch.rand(N, 2, generator=g) * 3 - 1.5, torch.rand(N, 1, generator=g) * 2 + 1.5], 1).to(dev)
    quats = torch.randn(N, 4, generator=g).to(dev)
    scales = torch.exp(torch.rand(N, 3, generator=g) * 1.5 - 6.5).to(dev)
    opac = torch.rand(N, generator=g).to(dev)
    sh = (torch.rand(N, 1, 3, generator=g) * 2 - 1).to(dev)
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, 0, 3] = torch.linspace(-0.3, 0.3, V)
    K = torch.tensor([[500.0, 0, 259], [0, 500.0, 259], [0, 0, 1]]).repeat(V, 1, 1)
    c2w, K = c2w.to(dev).requires_grad_(True), K.to(dev)
    leaves = [x.requires_grad_(True) for x in (means, quats, scales, opac, sh)]
    tgt = torch.rand(V, H, W, 3, generator=g).to(dev)
    got, ms = {}, {}
    for on in (False, True):
        rz = Rasterizer(camera_grad=on)
        for _ in range(2):                                                   # the second round is timed warm
            for x in leaves + [c2w]:
                x.grad = None
            rgb, dep, al = rz.rasterize_splats(*leaves, c2w, K, W, H, sh_degree=0)
            loss = (rgb - tgt).abs().mean() + 0.1 * dep.mean() + 0.1 * al.mean()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize(); t2 = time.perf_counter()
        ms[on] = (t2 - t1) * 1e3
        got[on] = [x.grad.clone() for x in leaves] + [None if c2w.grad is None else c2w.grad.clone()]
    print(f"full-size backward: pairs {rz.last_n_isects}, camera_grad off {ms[False]:.2f} ms, on {ms[True]:.2f} ms")
    assert got[False][5] is None
    assert torch.isfinite(got[True][5]).all() and float(got[True][5].abs().sum()) > 0
    for a, b in zip(got[False][:5], got[True][:5]):
        assert torch.equal(a, b)
