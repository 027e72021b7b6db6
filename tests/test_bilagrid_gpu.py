"""The bilateral-grid slice and the grids' total variation on the GPU (wm_bilagrid_* through hunyuanworld_mirror_amd.slice,
BilateralGrid and total_variation_loss) against the reference's own fp64 numbers (tests/golden/bilagrid_*.npz) and against the torch
restatement tests/bilagrid_helper.py (pinned to those numbers by tests/test_bilagrid_cpu.py).

Tolerance (the convention of test_photometric_gpu.py): the yardstick of a quantity is the helper's own fp32-against-fp64 error on
the same inputs, as the largest element error relative to the largest element, and never less than one fp32 ulp of that largest
element (a single correctly rounded value is already half an ulp off).  The kernels order their sums differently and contract to
FMA, so they may exceed the yardstick by FACTOR = 4; more than that is a defect.  Ratios measured on MI355X:
profiles/r13_bilateral_grid.md."""
import functools

import numpy as np
import pytest
import torch

import bilagrid_helper as BH
import photometric_helper as PH

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
KEYS = ("out", "v_grids", "v_rgb")


def _dev():
    return torch.device("cuda:0")


def _identity(G, L, Hg, Wg):
    return torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(1, 12, 1, 1, 1).repeat(G, 1, L, Hg, Wg)


def _gpu(grids, xy, rgb, ids, v_out):
    """-> dict(out, v_grids, v_rgb) as CPU fp32 tensors, through the public slice and autograd"""
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    g = grids.to(dev).requires_grad_(True)
    c = rgb.to(dev).requires_grad_(True)
    out = wm.slice(g, xy.to(dev), c, ids.to(dev))["rgb"]
    out.backward(v_out.to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), v_grids=g.grad.cpu(), v_rgb=c.grad.cpu())


def _check(tag, got, ref, f32):
    """got (GPU), ref (fp64), f32 (helper fp32): dicts over KEYS.  Prints every ratio, then asserts."""
    fails = []
    for k in KEYS:
        assert torch.isfinite(got[k]).all(), (tag, k)
        yard = max(BH.max_rel(f32[k].numpy(), ref[k]), ULP)
        err = BH.max_rel(got[k].numpy(), ref[k])
        print(f"{tag} {k}: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.2f}")
        if not err <= FACTOR * yard:
            fails.append((tag, k, yard, err))
    assert not fails, fails


@functools.lru_cache(maxsize=None)
def _golden(name):
    z = BH.load_golden(name)
    t = {k: torch.from_numpy(z[k]) for k in ("grids", "xy", "rgb", "v_out")}
    t["ids"] = torch.from_numpy(z["ids"])
    f32 = BH.gradients(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"], torch.float32)
    return z, t, f32


@functools.lru_cache(maxsize=None)
def _scene(G, L, Hg, Wg, shape, ids):
    """random scene with every sample at least 1e-4 grid units from a cell boundary -> inputs, fp64 reference, fp32 yardstick"""
    for seed in range(200):
        g = torch.Generator().manual_seed(1000 * seed + L * Hg * Wg + sum(shape))
        xy = torch.rand(*shape, 2, generator=g) * 1.2 - 0.1
        rgb = torch.rand(*shape, 3, generator=g) * 1.3 - 0.15
        if min(BH.boundary_margin((G, 12, L, Hg, Wg), xy, rgb)) >= 1e-4:
            break
    else:
        raise AssertionError("no seed keeps the samples off the cell boundaries")
    grids = _identity(G, L, Hg, Wg) + 0.2 * torch.randn(G, 12, L, Hg, Wg, generator=g)
    v_out = torch.randn(*shape, 3, generator=g)
    t = dict(grids=grids, xy=xy, rgb=rgb, v_out=v_out, ids=torch.tensor(ids))
    ref = BH.gradients(grids, xy, rgb, t["ids"], v_out, torch.float64)
    f32 = BH.gradients(grids, xy, rgb, t["ids"], v_out, torch.float32)
    return t, {k: v.numpy() for k, v in ref.items()}, f32


@pytest.mark.parametrize("name", ["a", "b"])
def test_gpu_matches_the_reference_goldens(name):
    z, t, f32 = _golden(name)
    got = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    _check(f"golden {name}", got, z, f32)
    if name == "a":
        assert not got["v_grids"][1].any()                      # the grid no row names: exactly zero, every element written


# (G, L, Hg, Wg, shape, ids): one sample; the forward's 256-sample block seam; the grid backward's 512-sample run seam and several
# segments per row; B = 1; the default grid on a 37 x 29 image (4-D input); 3072 and 4096 cells (three and four cells per thread)
EXTRA = [
    (1, 8, 16, 16, (1, 1), (0,)),
    (3, 3, 4, 5, (2, 255), (2, 0)),
    (3, 3, 4, 5, (2, 256), (0, 0)),
    (3, 3, 4, 5, (2, 257), (1, 2)),
    (2, 3, 4, 5, (2, 511), (1, 0)),
    (2, 3, 4, 5, (2, 512), (1, 0)),
    (2, 3, 4, 5, (3, 1537), (0, 1, 0)),
    (2, 8, 16, 16, (1, 700), (1,)),
    (2, 8, 16, 16, (2, 29, 37), (1, 0)),
    (2, 12, 16, 16, (2, 600), (1, 0)),
    (1, 16, 16, 16, (1, 600), (0,)),
]


@pytest.mark.parametrize("case", EXTRA, ids=[f"G{c[0]}-{c[3]}x{c[2]}x{c[1]}-{'x'.join(map(str, c[4]))}" for c in EXTRA])
def test_gpu_matches_the_helper_on_extra_shapes(case):
    t, ref, f32 = _scene(*case)
    got = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    _check(str(case), got, ref, f32)


def test_gpu_clamped_samples_have_no_guidance_gradient():
    """A sample whose z lies on or beyond the clamp range: rgb.grad is A[:, :3]^T v_out alone."""
    z, t, f32 = _golden("a")
    got = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    clamped = BH.z_clamped(z["grids"].shape, t["rgb"]).reshape(-1)
    assert int(clamped.sum()) >= 5
    A = BH.affine(t["grids"].double(), t["xy"].double(), t["rgb"].double(), t["ids"]).reshape(-1, 3, 4)
    want = (A[:, :, :3] * t["v_out"].double().reshape(-1, 3, 1)).sum(1)
    yard = max(BH.max_rel(f32["v_rgb"].numpy(), z["v_rgb"]), ULP) * float(np.abs(z["v_rgb"]).max())
    err = float((got["v_rgb"].double().reshape(-1, 3) - want)[clamped].abs().max())
    print(f"clamped samples: {int(clamped.sum())}, |v_rgb - A^T v_out| {err:.3e}, yardstick {yard:.3e}")
    assert err <= FACTOR * yard


def test_gpu_identity_grids_return_the_input():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    bil = wm.BilateralGrid(3).to(dev)
    assert bil.grids.shape == (3, 12, 8, 16, 16) and (bil.grid_width, bil.grid_height, bil.grid_guidance) == (16, 16, 8)
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand(3, 29, 37, 3, generator=g).to(dev)
    xy = torch.rand(3, 29, 37, 2, generator=g).to(dev)
    with torch.no_grad():
        res = wm.slice(bil, xy, rgb, torch.tensor([[2], [0], [1]], device=dev))
    assert set(res) == {"rgb"}
    ulp = torch.from_numpy(np.spacing(rgb.abs().cpu().numpy())).to(dev)
    assert bool(((res["rgb"] - rgb).abs() <= ulp).all())
    with pytest.raises(NotImplementedError, match="slice"):
        bil(xy, rgb, torch.tensor([2, 0, 1], device=dev))


def test_gpu_rows_naming_one_grid_sum():
    """scene b names grid 1 in rows 0 and 1: its gradient is the sum of the two single-row calls"""
    z, t, f32 = _golden("b")
    both = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])["v_grids"][1].double()
    parts = [_gpu(t["grids"], t["xy"][r:r + 1], t["rgb"][r:r + 1], t["ids"][r:r + 1], t["v_out"][r:r + 1])["v_grids"][1].double() for r in (0, 1)]
    yard = max(BH.max_rel(f32["v_grids"].numpy(), z["v_grids"]), ULP)
    err = BH.max_rel(both.numpy(), (parts[0] + parts[1]).numpy())
    print(f"grid 1 of scene b, both rows against the sum of single rows: {err:.3e}, yardstick {yard:.3e}")
    assert parts[0].abs().sum() > 0 and parts[1].abs().sum() > 0 and err <= FACTOR * yard


@pytest.mark.parametrize("name", ["a", "b"])
def test_gpu_bitwise_reproducible_and_one_forward(name):
    import hunyuanworld_mirror_amd as wm
    z, t, _ = _golden(name)
    first = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    again = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    assert all(torch.equal(first[k], again[k]) for k in KEYS)
    dev = _dev()
    with torch.no_grad():
        plain = wm.slice(t["grids"].to(dev).requires_grad_(True), t["xy"].to(dev), t["rgb"].to(dev), t["ids"].to(dev))["rgb"]
    detached = wm.slice(t["grids"].to(dev), t["xy"].to(dev), t["rgb"].to(dev), t["ids"].to(dev))["rgb"]
    assert plain.grad_fn is None and detached.grad_fn is None
    assert torch.equal(plain.cpu(), first["out"]) and torch.equal(detached.cpu(), first["out"])


def test_gpu_surface_strides_dtypes_and_index_forms():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    z, t, _ = _golden("a")
    base = _gpu(t["grids"], t["xy"], t["rgb"], t["ids"], t["v_out"])
    grids, ids = t["grids"].to(dev), t["ids"].to(dev)
    # an expanded xy (stride 0), a permuted rgb view, the reference's (..., 1) index forms and host ints
    rgb_view = t["rgb"].permute(3, 0, 1, 2).contiguous().to(dev).permute(1, 2, 3, 0)
    assert not rgb_view.is_contiguous()
    for idx in (ids.unsqueeze(-1), ids.reshape(2, 1, 1, 1), [2, 0], t["ids"]):
        out = wm.slice(grids, t["xy"].to(dev), rgb_view, idx)["rgb"]
        assert torch.equal(out.cpu(), base["out"])
    one = t["xy"][:1].to(dev)
    a = wm.slice(grids, one.expand(2, -1, -1, -1), t["rgb"].to(dev), ids)["rgb"]
    b = wm.slice(grids, one.repeat(2, 1, 1, 1), t["rgb"].to(dev), ids)["rgb"]
    assert torch.equal(a, b)
    # only rgb requires grad / only the grids do: the same bits as both together
    c = t["rgb"].to(dev).requires_grad_(True)
    wm.slice(grids, t["xy"].to(dev), c, ids)["rgb"].backward(t["v_out"].to(dev))
    assert torch.equal(c.grad.cpu(), base["v_rgb"])
    g = grids.clone().requires_grad_(True)
    wm.slice(g, t["xy"].to(dev), t["rgb"].to(dev), ids)["rgb"].backward(t["v_out"].to(dev))
    assert torch.equal(g.grad.cpu(), base["v_grids"])
    # half inputs are computed in fp32 and cast back
    h = t["rgb"].to(dev).half().requires_grad_(True)
    out = wm.slice(grids, t["xy"].to(dev).half(), h, ids)["rgb"]
    out.float().sum().backward()
    assert out.dtype == torch.float16 and h.grad.dtype == torch.float16 and torch.isfinite(h.grad).all()


def test_gpu_guards():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    grids = _identity(2, 3, 4, 5).to(dev)
    xy, rgb = torch.rand(2, 7, 2, device=dev), torch.rand(2, 7, 3, device=dev)
    with pytest.raises(NotImplementedError):
        wm.slice(grids, xy[0], rgb[0], torch.zeros(7, 1, dtype=torch.long, device=dev))          # 2-D: one index per sample
    with pytest.raises(RuntimeError):
        wm.slice(grids, xy, rgb.cpu(), torch.tensor([0, 1]))
    with pytest.raises(RuntimeError):
        wm.slice(grids.cpu(), xy, rgb, torch.tensor([0, 1]))
    with pytest.raises(NotImplementedError):
        wm.slice(_identity(1, 17, 16, 16).to(dev), xy[:1], rgb[:1], torch.tensor([0]))           # 4352 cells
    with pytest.raises(IndexError):
        wm.slice(grids, xy, rgb, torch.tensor([0, 2]))
    with pytest.raises(IndexError):
        wm.slice(grids, xy, rgb, [-1, 0])
    with pytest.raises(NotImplementedError):
        wm.total_variation_loss(torch.rand(2, 12, 4, 4, device=dev))
    with pytest.raises(RuntimeError):
        wm.total_variation_loss(torch.rand(2, 12, 3, 4, 4))
    # the C entry refuses before launching
    import ctypes as C
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    p = lambda x: C.c_void_p(x.data_ptr())
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.full_like(rgb, 7.0)
    assert L.wm_bilagrid_slice(p(grids), 2, 17, 16, 16, p(idx), p(xy), p(rgb), 2, 7, p(out), None) != 0
    assert L.wm_bilagrid_slice(p(grids), 2, 3, 4, 5, p(idx), p(xy), p(rgb), 2, 0, p(out), None) != 0
    assert L.wm_bilagrid_slice_backward(p(grids), 2, 3, 4, 5, p(idx), p(xy), p(rgb), 2, 7, p(out), p(torch.empty_like(grids)), None, None, 0, None) != 0
    assert L.wm_bilagrid_slice_backward_workspace_bytes(2, 17, 16, 16, 2, 7) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_gpu_device_index_out_of_range_gives_nan_rows_only():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    z, t, _ = _golden("b")
    ids = torch.tensor([1, 5, 0], device=dev)
    g = t["grids"].to(dev).requires_grad_(True)
    c = t["rgb"].to(dev).requires_grad_(True)
    out = wm.slice(g, t["xy"].to(dev), c, ids)["rgb"]
    v = t["v_out"].to(dev).clone()
    out.backward(v)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()
    assert torch.isfinite(g.grad).all() and torch.isfinite(c.grad[0]).all() and torch.isfinite(c.grad[2]).all() and torch.isnan(c.grad[1]).all()
    alone = _gpu(t["grids"], t["xy"][[0, 2]], t["rgb"][[0, 2]], torch.tensor([1, 0]), t["v_out"][[0, 2]])
    assert torch.equal(out[[0, 2]].detach().cpu(), alone["out"]) and torch.equal(g.grad.cpu(), alone["v_grids"])


TV_SHAPES = [(1, 12, 2, 2, 2), (3, 12, 8, 16, 16)]


def _tv_gpu(x):
    import hunyuanworld_mirror_amd as wm
    t = x.to(_dev()).requires_grad_(True)
    tv = wm.total_variation_loss(t)
    assert tv.dim() == 0
    tv.backward()
    with torch.no_grad():
        assert torch.equal(wm.total_variation_loss(t), tv.detach())
    return float(tv.detach()), t.grad.cpu()


def _tv_check(tag, x, ref_tv, ref_grad):
    f32 = BH.tv_gradients(x, torch.float32)
    tv, grad = _tv_gpu(x)
    y_v = max(abs(float(f32["tv"]) - ref_tv), ULP * abs(ref_tv))
    print(f"{tag} tv: gpu {tv:.9g} fp64 {ref_tv:.12g} |gpu - fp64| {abs(tv - ref_tv):.3e} yardstick {y_v:.3e}")
    assert abs(tv - ref_tv) <= FACTOR * y_v
    if ref_grad is not None:
        y_g = max(BH.max_rel(f32["v_x"].numpy(), ref_grad), ULP)
        e_g = BH.max_rel(grad.numpy(), ref_grad)
        print(f"{tag} tv gradient: yardstick {y_g:.3e} gpu {e_g:.3e} ratio {e_g / y_g:.2f}")
        assert e_g <= FACTOR * y_g


def test_gpu_total_variation():
    for name in ("a", "b"):
        z, t, _ = _golden(name)
        _tv_check(f"golden {name}", t["grids"], float(z["tv"]), z["tv_grad"] if "tv_grad" in z else None)
    for shape in TV_SHAPES:
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
        ref = BH.tv_gradients(x, torch.float64)
        _tv_check(str(shape), x, float(ref["tv"]), ref["v_x"].numpy())
    tv, grad = _tv_gpu(torch.full((2, 12, 3, 4, 5), 0.37))
    assert tv == 0.0 and not grad.any()
    import hunyuanworld_mirror_amd as wm
    bil = wm.BilateralGrid(2, 5, 4, 3).to(_dev())
    assert float(bil.tv_loss().detach()) == 0.0


def _loop_scene():
    """a fixed smooth 2 x 40 x 56 image with a little noise, its target under a per-image affine colour change, the trainer's meshgrid"""
    C_, H, W = 2, 40, 56
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ph = torch.arange(C_ * 3, dtype=torch.float64).reshape(C_, 1, 1, 3)
    img = 0.5 + 0.3 * torch.sin(0.23 * xx[None, :, :, None] + 0.7 * ph) * torch.cos(0.17 * yy)[None, :, :, None]
    img = (img + 0.03 * torch.randn(C_, H, W, 3, generator=g, dtype=torch.float64)).clamp(0, 1).float().double()
    M = torch.eye(3, dtype=torch.float64) * torch.tensor([[[0.8]], [[1.15]]], dtype=torch.float64) + 0.05 * torch.randn(C_, 3, 3, generator=g, dtype=torch.float64)
    off = torch.tensor([[0.06, -0.02, 0.03], [-0.05, 0.04, 0.0]], dtype=torch.float64)
    target = (torch.einsum("cij,chwj->chwi", M, img) + off[:, None, None, :]).float().double()
    gy, gx = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H, (torch.arange(W, dtype=torch.float64) + 0.5) / W, indexing="ij")
    xy = torch.stack([gx, gy], -1).unsqueeze(0).expand(C_, -1, -1, -1).float().double()
    return img, target, xy, torch.tensor([1, 0])


def _loop_run(cast, slice_fn, loss_fn, tv_fn, steps=30):
    img, target, xy, _ = _loop_scene()
    grids = cast(_identity(2, 8, 16, 16).double()).clone().requires_grad_(True)
    opt = torch.optim.Adam([grids], lr=5e-3)
    im, tg, p = cast(img), cast(target), cast(xy)
    curve = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(slice_fn(grids, p, im), tg) + 10 * tv_fn(grids)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return curve


def _loop_cpu():
    ids = _loop_scene()[3]
    return _loop_run(lambda v: v, lambda gr, p, im: BH.slice_rgb(gr, p, im, ids),
                     lambda a, b: PH.loss(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), "valid", 0.2)[0], BH.total_variation)


def test_gpu_grids_optimise_like_the_fp64_restatement():
    """30 Adam steps on the grids alone through slice -> photometric_loss + 10 * total_variation_loss, towards a target that is a fixed
    image under a known per-image affine colour change: on the GPU (fp32, the fused kernels) and on the CPU restatements (fp64) from
    the same start.  The curves stay within 2 % of each other at every step (the bound of test_photometric_gpu.py's loop) and fall."""
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    ids = _loop_scene()[3].to(dev)
    gpu = _loop_run(lambda v: v.float().to(dev), lambda gr, p, im: wm.slice(gr, p, im, ids.unsqueeze(-1))["rgb"],
                    lambda a, b: wm.photometric_loss(a, b, 0.2, "valid")[0], wm.total_variation_loss)
    cpu = _loop_cpu()
    gap = max(abs(a - b) / b for a, b in zip(gpu, cpu))
    print("loss curves: gpu", [f"{x:.5f}" for x in gpu], "cpu fp64", [f"{x:.5f}" for x in cpu], "largest gap", gap)
    assert gap < 0.02
    assert gpu[-1] < gpu[0] and cpu[-1] < cpu[0]
