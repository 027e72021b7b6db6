"""3D-Gaussian-splat rasteriser forward (reference call: src/models/models/rasterization.py:29-66 ->
gsplat.rasterization, render_mode RGB+ED, sh_degree 0).

CPU: oracle/raster_ref.py against outputs of the reference's own gsplat torch implementation (tests/golden/raster_*.npz,
written by oracle/gen_golden_raster.py): covariances, projection, radii, conics, SH colours, tile-intersection lists.
The compositing stage has no runnable reference here (PARITY UNPINNED for that stage, see the oracle's header): it is a
restatement of gsplat's CUDA kernel, checked by a second tiling-free formulation and by closed-form cases.
GPU: libwm_hip.so (wm_rasterize_splats) against the oracle.
The scenes here run the 2-pixel-per-lane compositing kernel only; all three kernels, and the list-walk edges (list lengths, saturation
exits, image edges), are compared per pixel with the fp64 restatement in tests/test_raster_composite_gpu.py."""
import os

import numpy as np
import pytest

from conftest import GOLD, rel_l2
from oracle import raster_ref as R

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]


def _load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    s = {k[3:]: v for k, v in z.items() if k.startswith("in_")}
    return z, s, int(z["width"]), int(z["height"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_projection_matches_gsplat_torch(name):
    z, s, W, H = _load(name)
    assert rel_l2(R.quat_scale_to_covar(s["quats"], s["scales"]), z["ref_covars"]) < 1e-6
    radii, m2, depths, conics = R.project(s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H)
    vis = (z["ref_radii"] > 0).all(-1)
    assert np.array_equal(radii, z["ref_radii"])          # integer radii incl. every culling decision
    assert vis.sum() > 100
    assert rel_l2(m2[vis], z["ref_means2d"][vis]) < 1e-6
    assert rel_l2(depths[vis], z["ref_depths"][vis]) < 1e-6
    assert rel_l2(conics[vis], z["ref_conics"][vis]) < 1e-5
    assert rel_l2(R.sh0_colors(s["sh"][:, 0]), z["ref_colors"][0]) < 1e-6
    assert (z["ref_colors"] == z["ref_colors"][:1]).all()   # degree 0: no view dependence


@pytest.mark.parametrize("name", CASES)
def test_oracle_tile_intersection_matches_gsplat_torch(name):
    z, s, W, H = _load(name)
    # from the REFERENCE's projection outputs, so the lists must agree exactly (integer work)
    keys, vals, offs, tw, th = R.isect_tiles(z["ref_means2d"], z["ref_radii"], z["ref_depths"], W, H)
    _, _, cnt, _, _ = R.tile_rects(z["ref_means2d"], z["ref_radii"], W, H)
    assert np.array_equal(cnt, z["ref_tiles_per_gauss"])
    assert np.array_equal(keys.astype(np.int64), z["ref_isect_ids"])
    assert np.array_equal(offs[:-1].reshape(z["ref_offsets"].shape), z["ref_offsets"])
    # equal keys (same tile, same depth bits) may be ordered differently by the two sorts: compare as sets per key
    a = sorted(zip(keys.tolist(), vals.tolist())); b = sorted(zip(z["ref_isect_ids"].astype(np.uint64).tolist(), z["ref_flatten_ids"].tolist()))
    assert a == b


def test_oracle_compositing_tiled_equals_bruteforce():
    z, s, W, H = _load(CASES[0])
    rgb, ed, al, meta = R.rasterize(s["means"], s["quats"], s["scales"], s["opacities"], s["sh"][:, 0], s["viewmats"], s["Ks"], W, H)
    rgb2, ed2, al2 = R.composite_bruteforce(meta["means2d"], meta["conics"], s["opacities"], meta["colors"], meta["depths"], meta["radii"], W, H)
    # a Gaussian contributes outside its 3.33-sigma tile rectangle only with alpha < 1/255 * ... -> tiny, not zero
    assert np.abs(rgb - rgb2).max() < 2e-2 and rel_l2(rgb, rgb2) < 5e-3
    assert rel_l2(al, al2) < 5e-3
    assert al.min() >= 0 and al.max() <= 1.0 and (al > 0.5).mean() > 0.2


def test_oracle_compositing_closed_form():
    """One isotropic Gaussian straight ahead: alpha(p) = min(0.999, o exp(-|p - mu|^2 / (2 s2))), colour = alpha * c, ED = z."""
    W = H = 48
    f, z0, s3 = 40.0, 2.0, 0.1
    means = np.array([[0.0, 0.0, z0]], np.float32); quats = np.array([[1.0, 0, 0, 0]], np.float32)
    scales = np.full((1, 3), s3, np.float32); opac = np.array([0.8], np.float32); sh = np.array([[1.0, -0.5, 0.2]], np.float32)
    vm = np.eye(4, dtype=np.float32)[None]; K = np.array([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]], np.float32)
    rgb, ed, al, meta = R.rasterize(means, quats, scales, opac, sh, vm, K, W, H)
    s2 = (f * s3 / z0) ** 2 + 0.3
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    a = np.minimum(0.999, 0.8 * np.exp(-((px - W / 2) ** 2 + (py - H / 2) ** 2) / (2 * s2)))
    a = np.where(a < 1 / 255.0, 0.0, a)
    r = int(meta["radii"][0, 0, 0])
    inside = (np.abs(px - W / 2) < 16 * np.ceil((r) / 16 + 1)) & (np.abs(py - H / 2) < 16 * np.ceil(r / 16 + 1))
    col = np.maximum(R.SH_C0 * sh[0] + 0.5, 0)
    assert np.abs(al[0, ..., 0] - a)[inside].max() < 1e-5
    assert np.abs(rgb[0] - a[..., None] * col)[inside].max() < 1e-5
    assert np.abs(ed[0, ..., 0] - z0)[a > 0].max() < 1e-5


# ------------------------------------------------------------------------------------------------ GPU (through the C ABI)
def _gpu_raster(s, W, H, want_radii=True):
    import ctypes as C
    import torch
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in s.items()}
    N, Cc = s["means"].shape[0], s["viewmats"].shape[0]
    sh = t["sh"][:, 0].contiguous()
    rgb = torch.full((Cc, H, W, 3), float("nan"), device=dev); dep = torch.full((Cc, H, W), float("nan"), device=dev)
    al = torch.full((Cc, H, W), float("nan"), device=dev); radii = torch.zeros((Cc, N, 2), device=dev, dtype=torch.int32)
    cap = 1 << 20
    ws = torch.empty(L.wm_rasterize_workspace_bytes(N, Cc, W, H, cap), device=dev, dtype=torch.uint8)
    n = C.c_ulonglong(0)
    p = lambda x: C.c_void_p(x.data_ptr())
    st = L.wm_rasterize_splats(p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(sh), 1, N, p(t["viewmats"]), p(t["Ks"]), Cc, W, H,
                               p(rgb), p(dep), p(al), p(radii) if want_radii else None, p(ws), ws.numel(), cap, C.byref(n),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    return rgb.cpu().numpy(), dep.cpu().numpy()[..., None], al.cpu().numpy()[..., None], radii.cpu().numpy(), int(n.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_rasterizer_matches_oracle_and_reference_projection(name):
    z, s, W, H = _load(name)
    rgb, ed, al, radii, n = _gpu_raster(s, W, H)
    # projection stage against the REFERENCE's outputs: integer radii (every culling decision) and the pair count
    assert (radii != z["ref_radii"]).any(-1).mean() < 2e-3          # a ceil() may flip on a last-bit difference
    assert abs(n - len(z["ref_isect_ids"])) <= 0.002 * len(z["ref_isect_ids"]) + 4
    # image against the oracle (its compositing stage is a restatement: parity unpinned, see the module docstring)
    r0, e0, a0, _ = R.rasterize(s["means"], s["quats"], s["scales"], s["opacities"], s["sh"][:, 0], s["viewmats"], s["Ks"], W, H)
    print(name, "rgb", rel_l2(rgb, r0), np.abs(rgb - r0).max(), "alpha", rel_l2(al, a0), "ed", rel_l2(ed * (a0 > 1e-3), e0 * (a0 > 1e-3)))
    assert np.isfinite(rgb).all() and np.isfinite(ed).all() and np.isfinite(al).all()
    assert rel_l2(rgb, r0) < 2e-4 and np.abs(rgb - r0).max() < 2e-2   # a threshold (alpha < 1/255, T <= 1e-4) may flip on one pixel
    assert rel_l2(al, a0) < 2e-4
    m = a0 > 1e-3
    assert rel_l2(ed[m], e0[m]) < 2e-4


@pytest.mark.gpu
def test_gpu_rasterizer_python_mirror_and_workspace_growth():
    """hunyuanworld_mirror_amd.Rasterizer keeps the reference's call shapes (rasterization.py:29-93): camera-to-world
    matrices in, (colors [B,V,H,W,3], depths [B,V,H,W,1], alphas [B,V,H,W,1]) out; the workspace grows when the pair
    count exceeds the first guess; results are bit-identical run to run (stable radix sort, no atomics)."""
    import torch
    from hunyuanworld_mirror_amd import Rasterizer
    z, s, W, H = _load(CASES[1])
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    c2w = torch.linalg.inv(t["viewmats"])
    rz = Rasterizer()
    rz._cap = 0
    out = rz.rasterize_batches([t["means"]], [t["quats"]], [t["scales"]], [t["opacities"]], [t["sh"]], c2w[None], t["Ks"][None], W, H, sh_degree=0)
    C_ = s["viewmats"].shape[0]
    assert out[0].shape == (1, C_, H, W, 3) and out[1].shape == (1, C_, H, W, 1) and out[2].shape == (1, C_, H, W, 1)
    r0, e0, a0, _ = R.rasterize(s["means"], s["quats"], s["scales"], s["opacities"], s["sh"][:, 0], s["viewmats"], s["Ks"], W, H)
    assert rel_l2(out[0][0].cpu().numpy(), r0) < 5e-4 and rel_l2(out[2][0].cpu().numpy(), a0) < 5e-4
    again = rz.rasterize_batches([t["means"]], [t["quats"]], [t["scales"]], [t["opacities"]], [t["sh"]], c2w[None], t["Ks"][None], W, H, sh_degree=0)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    # final colours instead of SH (sh_degree None): colour = clamp_min(C0 sh + 0.5, 0) given directly
    col = torch.clamp_min(R.SH_C0 * t["sh"][:, 0] + 0.5, 0.0)
    direct = rz.rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], col, c2w, t["Ks"], W, H)
    assert torch.allclose(direct[0], out[0][0], atol=1e-6)
    # a tiny first workspace must be re-sized transparently
    small = Rasterizer()
    import hunyuanworld_mirror_amd.rasterization as RM
    big = torch.cat([t["scales"] * 8.0], 0)
    o2 = small.rasterize_splats(t["means"], t["quats"], big, t["opacities"], t["sh"], c2w, t["Ks"], W, H, sh_degree=0)
    assert small.last_n_isects > 0 and torch.isfinite(o2[0]).all()


@pytest.mark.gpu
def test_gpu_rasterizer_full_size_properties():
    """One splat per pixel of 4 views at 518 x 518 (the reference's gsdepth+predcamera splats are exactly that many):
    alpha in [0, 1], colours bounded by the brightest splat, expected depth inside the depth range, determinism."""
    import torch
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
    rz = Rasterizer()
    rgb, dep, al = rz.rasterize_splats(means, quats, scales, opac, sh, c2w.to(dev), K.to(dev), W, H, sh_degree=0)
    torch.cuda.synchronize()
    assert rgb.shape == (V, H, W, 3) and torch.isfinite(rgb).all() and torch.isfinite(dep).all()
    assert float(al.min()) >= 0 and float(al.max()) <= 1.0 and float((al > 0.5).float().mean()) > 0.5
    cmax = float(torch.clamp_min(R.SH_C0 * sh + 0.5, 0).max())
    assert float(rgb.max()) <= cmax * (1 + 1e-5)
    m = al[..., 0] > 1e-3
    assert float(dep[..., 0][m].min()) >= 1.5 - 1e-3 and float(dep[..., 0][m].max()) <= 3.5 + 1e-3
    again = rz.rasterize_splats(means, quats, scales, opac, sh, c2w.to(dev), K.to(dev), W, H, sh_degree=0)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], dep)
    print("full-size raster: pairs", rz.last_n_isects)


@pytest.mark.gpu
def test_gpu_forward_splats_render_through_model_rasterizer():
    """The caller's flow (infer.py:259-264, GaussianSplatRenderer.render rasterization.py:221-241): forward with the
    3D-Gaussian head -> predictions["splats"] -> model.gs_renderer.rasterizer.rasterize_batches at the predicted
    cameras.  Checked against the oracle rasteriser on the same splats and cameras."""
    import torch
    from conftest import load_golden
    from hunyuanworld_mirror_amd import WorldMirror
    cfg, views, flags, outs, z = load_golden("tiny_gs_2v_70x70")
    m = WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0")
    pred = m({k: torch.from_numpy(v).cuda() for k, v in views.items()}, flags)
    sp = pred["splats"]
    c2w, K = pred["camera_poses"], pred["camera_intrs"]          # [1, S, 4, 4], [1, S, 3, 3]
    H, W = views["img"].shape[-2:]
    col, dep, al = m.gs_renderer.rasterizer.rasterize_batches(sp["means"], sp["quats"], sp["scales"], sp["opacities"], sp["sh"],
                                                              c2w, K, width=W, height=H, sh_degree=0)
    torch.cuda.synchronize()
    S = views["img"].shape[1]
    assert col.shape == (1, S, H, W, 3) and dep.shape == (1, S, H, W, 1) and al.shape == (1, S, H, W, 1)
    assert torch.isfinite(col).all() and torch.isfinite(dep).all() and float(al.min()) >= 0 and float(al.max()) <= 1
    vm = np.linalg.inv(c2w[0].cpu().numpy().astype(np.float64)).astype(np.float32)
    r0, e0, a0, _ = R.rasterize(sp["means"][0].cpu().numpy(), sp["quats"][0].cpu().numpy(), sp["scales"][0].cpu().numpy(),
                                sp["opacities"][0].cpu().numpy(), sp["sh"][0][:, 0].cpu().numpy(), vm, K[0].cpu().numpy(), W, H)
    print("model splats rendered: coverage", float((a0 > 0.5).mean()), "rgb", rel_l2(col[0].cpu().numpy(), r0))
    assert rel_l2(col[0].cpu().numpy(), r0) < 2e-3 and rel_l2(al[0].cpu().numpy(), a0) < 2e-3


@pytest.mark.gpu
def test_gpu_rasterizer_edge_cases():
    """Everything culled (behind the camera): empty pair list, black transparent image.  A single opaque splat: exactly the
    oracle's footprint.  Image size that is not a multiple of the tile (ragged last tiles)."""
    import torch
    from hunyuanworld_mirror_amd import Rasterizer
    dev = torch.device("cuda:0")
    rz = Rasterizer()
    c2w = torch.eye(4, device=dev)[None]
    K = torch.tensor([[[60.0, 0, 20.5], [0, 60.0, 14.5], [0, 0, 1]]], device=dev)
    W, H = 41, 29
    behind = torch.tensor([[0.0, 0.0, -2.0], [0.3, 0.1, -1.0]], device=dev)
    q = torch.tensor([[1.0, 0, 0, 0]] * 2, device=dev); sc = torch.full((2, 3), 0.05, device=dev)
    op = torch.tensor([0.9, 0.5], device=dev); col = torch.rand(2, 3, device=dev)
    rgb, dep, al = rz.rasterize_splats(behind, q, sc, op, col, c2w, K, W, H)
    assert rz.last_n_isects == 0 and float(rgb.abs().max()) == 0 and float(al.max()) == 0 and float(dep.abs().max()) == 0
    one = torch.tensor([[0.02, -0.01, 1.5]], device=dev)
    rgb, dep, al = rz.rasterize_splats(one, q[:1], sc[:1], op[:1], col[:1], c2w, K, W, H)
    r0, e0, a0, _ = R.rasterize(one.cpu().numpy(), q[:1].cpu().numpy(), sc[:1].cpu().numpy(), op[:1].cpu().numpy(), col[:1].cpu().numpy(),
                                np.eye(4, dtype=np.float32)[None], K.cpu().numpy(), W, H)
    # colours given directly (sh_degree None) on the GPU side: feed the oracle the inverse SH mapping
    r0 = a0 * col[:1].cpu().numpy().reshape(1, 1, 1, 3)
    assert np.abs(al.cpu().numpy() - a0).max() < 1e-5 and np.abs(rgb.cpu().numpy() - r0).max() < 1e-5
    assert float(al.max()) > 0.5 and abs(float(dep[al > 0.1].mean()) - 1.5) < 1e-4
