"""Rasteriser backward on the GPU (wm_rasterize_splats_backward through hunyuanworld_mirror_amd.Rasterizer's autograd path)
against the fp64 torch restatement tests/raster_grad_helper.py (pinned by tests/test_raster_backward_cpu.py).

Values measured on MI355X are recorded in profiles/r05_raster_backward.md."""
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


def _gpu_grads(inp, cot, is_sh, W, H, rz=None):
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(dev) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    col = t["colors"][:, None, :] if is_sh else t["colors"]
    rz = rz or Rasterizer()
    outs = rz.rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], col, torch.linalg.inv(t["viewmats"]), t["Ks"], W, H,
                               sh_degree=0 if is_sh else None)
    loss = sum((o * torch.from_numpy(c).float().to(dev)).sum() for o, c in zip(outs, cot))
    loss.backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], {k: t[k].grad.double().cpu().numpy() for k in NAMES}


@pytest.mark.parametrize("name", CASES)
def test_gpu_gradient_parity(name):
    """e64 = rel-L2(GPU, helper fp64) against the yardstick e32 = rel-L2(helper fp32, helper fp64): e64 <= 4 e32 and e64 < 1e-3."""
    inp, W, H = _load(name)
    C_ = inp["viewmats"].shape[0]
    g = torch.Generator().manual_seed(3)
    cot = [torch.randn(C_, H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]
    _, g64 = RG.gradients(inp, cot, True, W, H, torch.float64)
    _, g32 = RG.gradients(inp, cot, True, W, H, torch.float32)
    _, gg = _gpu_grads(inp, cot, True, W, H)
    res = {}
    for k in NAMES:
        res[k] = (rel_l2(g32[k], g64[k]), rel_l2(gg[k], g64[k]))
        print(f"{name} grad {k}: e32 {res[k][0]:.3e} e64 {res[k][1]:.3e}")
    for k, (e32, e64) in res.items():
        assert np.isfinite(gg[k]).all()
        assert e64 <= 4 * e32 and e64 < 1e-3, (k, e32, e64)


def test_gpu_autograd_surface():
    from hunyuanworld_mirror_amd import Rasterizer
    inp, W, H = _load(CASES[0])
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    c2w = torch.linalg.inv(t["viewmats"])
    rz = Rasterizer()
    args = lambda d: (d["means"], d["quats"], d["scales"], d["opacities"], d["colors"][:, None, :], c2w, d["Ks"], W, H)
    plain = rz.rasterize_splats(*args(t), sh_degree=0)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    a = dict(t)
    a["means"] = t["means"].clone().requires_grad_(True)
    a["opacities"] = t["opacities"].clone().requires_grad_(True)
    cam = c2w.clone().requires_grad_(True)
    att = rz.rasterize_splats(a["means"], a["quats"], a["scales"], a["opacities"], a["colors"][:, None, :], cam, a["Ks"], W, H, sh_degree=0)
    assert all(o.grad_fn is not None for o in att)
    assert all(torch.equal(x, y) for x, y in zip(plain, att))          # same bits on both routes
    with torch.no_grad():
        ng = rz.rasterize_splats(*args(a), sh_degree=0)
    assert all(o.grad_fn is None for o in ng) and all(torch.equal(x, y) for x, y in zip(ng, att))
    det = rz.rasterize_splats(*args({k: v.detach() for k, v in a.items()}), sh_degree=0)
    assert all(o.grad_fn is None for o in det) and all(torch.equal(x, y) for x, y in zip(det, att))
    (att[0].sum() + att[1].sum() + att[2].sum()).backward()
    assert a["means"].grad is not None and a["opacities"].grad is not None and cam.grad is None
    assert a["means"].grad.shape == a["means"].shape and float(a["means"].grad.abs().sum()) > 0
    assert all(t[k].grad is None for k in ("quats", "scales", "colors"))
    # two forwards, then two backwards: each node owns its workspace -> bitwise the gradients of each pair run alone
    def leaf(scale):
        d = {k: v.clone() for k, v in t.items()}
        d["scales"] = (d["scales"] * scale).requires_grad_(True)
        d["means"].requires_grad_(True)
        return d
    alone = []
    for sc in (1.0, 1.7):
        d = leaf(sc)
        o = rz.rasterize_splats(*args(d), sh_degree=0)
        (o[0].square().sum() + o[2].sum()).backward()
        alone.append((d["means"].grad.clone(), d["scales"].grad.clone()))
    d1, d2 = leaf(1.0), leaf(1.7)
    o1 = rz.rasterize_splats(*args(d1), sh_degree=0)
    o2 = rz.rasterize_splats(*args(d2), sh_degree=0)
    rz.rasterize_splats(*args(t), sh_degree=0)                           # and a plain call on the shared workspace in between
    (o1[0].square().sum() + o1[2].sum()).backward()
    (o2[0].square().sum() + o2[2].sum()).backward()
    for d, (gm, gs) in zip((d1, d2), alone):
        assert torch.equal(d["means"].grad, gm) and torch.equal(d["scales"].grad, gs)


def test_gpu_closed_form_opacity_gradient():
    """One isotropic Gaussian straight ahead (the scene of test_oracle_compositing_closed_form), loss = sum(alpha):
    d loss / d opacity = sum over unclamped, unskipped pixels of exp(-r^2 / (2 s2))."""
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    W = H = 48
    f, z0, s3, o = 40.0, 2.0, 0.1, 0.8
    means = torch.tensor([[0.0, 0.0, z0]], device=dev); quats = torch.tensor([[1.0, 0, 0, 0]], device=dev)
    scales = torch.full((1, 3), s3, device=dev); opac = torch.tensor([o], device=dev, requires_grad=True)
    col = torch.tensor([[0.7, 0.2, 0.5]], device=dev)
    K = torch.tensor([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]], device=dev)
    rgb, dep, al = Rasterizer().rasterize_splats(means, quats, scales, opac, col, torch.eye(4, device=dev)[None], K, W, H)
    al.sum().backward()
    s2 = (f * s3 / z0) ** 2 + 0.3
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    e = np.exp(-((px - W / 2) ** 2 + (py - H / 2) ** 2) / (2 * s2))
    use = (o * e >= 1 / 255.0) & (o * e <= 0.999)
    want = float(e[use].sum())
    got = float(opac.grad[0])
    print("closed form d sum(alpha) / d opacity:", got, "expected", want)
    assert abs(got - want) <= 1e-5 * want


def _opt_scene():
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
    true = dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors)
    start = dict(means=means + 0.03 * torch.randn(N, 3, generator=g, dtype=torch.float64), quats=quats + 0.05 * torch.randn(N, 4, generator=g, dtype=torch.float64),
                 scales=scales * torch.exp(0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64)), opacities=(opac + 0.1 * (u(N) - 0.5)).clamp(0.05, 0.95),
                 colors=(colors + 0.1 * (u(N, 3) - 0.5)).clamp(0, 1))
    return true, start, vm, K, W, H


def test_gpu_optimises_like_the_fp64_restatement():
    """20 Adam steps on an L1 loss from a perturbed start, on the GPU (fp32) and on the CPU restatement (fp64): the loss curves
    stay within 2 % of each other at every step and both end below their start."""
    from hunyuanworld_mirror_amd import Rasterizer
    true, start, vm, K, W, H = _opt_scene()
    dev = torch.device("cuda:0")

    def run(render, cast):
        p = {k: cast(v).clone().requires_grad_(True) for k, v in start.items()}
        with torch.no_grad():
            target = render({k: cast(v) for k, v in true.items()})[0]
        opt = torch.optim.Adam(list(p.values()), lr=2e-3)
        curve = []
        for _ in range(20):
            opt.zero_grad()
            loss = (render(p)[0] - target).abs().mean()
            loss.backward()
            opt.step()
            curve.append(float(loss))
        return curve

    rz = Rasterizer()
    c2w, Kg = torch.linalg.inv(vm).float().to(dev), K.float().to(dev)
    gpu = run(lambda p: rz.rasterize_splats(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], c2w, Kg, W, H), lambda v: v.float().to(dev))
    cpu = run(lambda p: RG.rasterize(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], False, vm, K, W, H), lambda v: v)
    gap = max(abs(a - b) / b for a, b in zip(gpu, cpu))
    print("loss curves: gpu", [f"{x:.5f}" for x in gpu], "cpu fp64", [f"{x:.5f}" for x in cpu], "largest gap", gap)
    assert gap < 0.02
    assert gpu[-1] < gpu[0] and cpu[-1] < cpu[0]


def test_gpu_backward_edge_cases():
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    rz = Rasterizer()
    c2w = torch.eye(4, device=dev)[None]
    K = torch.tensor([[[60.0, 0, 20.5], [0, 60.0, 14.5], [0, 0, 1]]], device=dev)
    W, H = 41, 29                                                        # ragged last tiles
    mk = lambda x: x.to(dev).requires_grad_(True)

    def grads(means, q, sc, op, col, weight=1.0):
        leaves = [mk(means), mk(q), mk(sc), mk(op), mk(col)]
        o = rz.rasterize_splats(*leaves, c2w, K, W, H)
        (weight * (o[0].sum() + 2 * o[1].sum() + 3 * o[2].sum())).backward()
        torch.cuda.synchronize()
        return [x.grad for x in leaves]

    q = torch.tensor([[1.0, 0, 0, 0]] * 2); sc = torch.full((2, 3), 0.05); op = torch.tensor([0.9, 0.5]); col = torch.rand(2, 3)
    behind = torch.tensor([[0.0, 0.0, -2.0], [0.3, 0.1, -1.0]])
    for gr in grads(behind, q, sc, op, col):                             # everything culled
        assert gr is not None and float(gr.abs().max()) == 0.0
    front = torch.tensor([[0.02, -0.01, 1.5], [0.1, 0.05, 1.2]])
    for gr in grads(front, q, sc, op, col, weight=0.0):                  # zero cotangents
        assert float(gr.abs().max()) == 0.0
    gr = grads(front, q, sc, op, col)
    assert all(torch.isfinite(x).all() for x in gr) and float(gr[0].abs().max()) > 0
    # ragged image against the restatement
    inp = dict(means=front.numpy(), quats=q.numpy(), scales=sc.numpy(), opacities=op.numpy(), colors=col.numpy(),
               viewmats=np.eye(4, dtype=np.float32)[None], Ks=K.cpu().numpy())
    cot = [np.ones((1, H, W, 3), np.float32), 2 * np.ones((1, H, W, 1), np.float32), 3 * np.ones((1, H, W, 1), np.float32)]
    _, g64 = RG.gradients(inp, cot, False, W, H, torch.float64)
    for k, x in zip(NAMES, gr):
        assert rel_l2(x.double().cpu().numpy(), g64[k]) < 1e-3, k
    # saturation: a stack of opaque splats on the same pixels reaches the T <= 1e-4 stop
    n = 12
    stack = torch.tensor([[0.0, 0.0, 1.0 + 0.1 * i] for i in range(n)])
    gr = grads(stack, torch.tensor([[1.0, 0, 0, 0]] * n), torch.full((n, 3), 0.2), torch.full((n,), 0.995), torch.rand(n, 3))
    assert all(torch.isfinite(x).all() for x in gr)


def test_gpu_backward_full_size():
    """4 views of 518 x 518, one splat per pixel (the inputs of test_gpu_rasterizer_full_size_properties)."""
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
    c2w, K = c2w.to(dev), K.to(dev)
    leaves = [x.requires_grad_(True) for x in (means, quats, scales, opac, sh)]
    rz = Rasterizer()
    tgt = torch.rand(V, H, W, 3, generator=g).to(dev)
    times = []
    for _ in range(2):                                                   # the second round is timed warm
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        rgb, dep, al = rz.rasterize_splats(*leaves, c2w, K, W, H, sh_degree=0)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        ((rgb - tgt).abs().mean() + 0.1 * dep.mean() + 0.1 * al.mean()).backward()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        times.append((t1 - t0, t2 - t1))
    print(f"full-size backward: pairs {rz.last_n_isects}, forward {times[-1][0] * 1e3:.2f} ms, backward {times[-1][1] * 1e3:.2f} ms")
    assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in leaves)
    from hunyuanworld_mirror_amd import _lib
    Lb = _lib.lib()
    # Gaussians no camera sees (no tile pair anywhere) get exactly zero: find them from the projection's radii
    import ctypes as C
    radii = torch.zeros((V, N, 2), device=dev, dtype=torch.int32)
    o = [torch.empty(V, H, W, 3, device=dev), torch.empty(V, H, W, device=dev), torch.empty(V, H, W, device=dev)]
    cap = rz.last_n_isects + 1024
    ws = torch.empty(Lb.wm_rasterize_workspace_bytes(N, V, W, H, cap), device=dev, dtype=torch.uint8)
    n = C.c_ulonglong(0)
    p = lambda x: C.c_void_p(x.data_ptr())
    st = Lb.wm_rasterize_splats(p(means.detach()), p(quats.detach()), p(scales.detach()), p(opac.detach()), p(sh.detach().reshape(N, 3).contiguous()), 1, N,
                                p(torch.linalg.inv(c2w).contiguous()), p(K), V, W, H, p(o[0]), p(o[1]), p(o[2]), p(radii), p(ws), ws.numel(), cap,
                                C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    culled = ~((radii > 0).all(-1).any(0))
    assert int(culled.sum()) > 0
    for x in leaves:
        assert float(x.grad[culled].abs().max()) == 0.0
    assert float(means.grad[~culled].abs().max()) > 0
