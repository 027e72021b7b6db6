"""The sparse disparity loss and the point projection on the GPU (wm_depth_loss / wm_depth_loss_backward / wm_project_depth_points
through hunyuanworld_mirror_amd.depth_loss and project_depth_points) against the reference's own fp64 numbers
(tests/golden/depth_loss_*.npz) and against the torch restatement tests/depth_loss_helper.py (pinned to those numbers by
tests/test_depth_loss_cpu.py).

Tolerances.  Gradient tensors and projection outputs (the convention of test_bilagrid_gpu.py): the yardstick of a quantity is the
helper's own fp32-against-fp64 error on the same inputs, as the largest element error relative to the largest element, never less than
one fp32 ulp; the GPU may exceed it by FACTOR = 4.  The scalar loss has a derived bound instead (one number's fp32 error can be luckily
small): |gpu - fp64| <= 16 * 2^-24 * mean(disp_i + disp_gt_i) — per term at most ~6 roundings in the non-negative bilinear sum, one each
in the two reciprocals and the subtraction, doubled for slack; the reduction itself is fp64.

Seams of the kernels (csrc/depthloss.hip): the forward and the key pass take 256 rows per block over the flat row index c * M + m
(M = 255 / 256 / 257; a camera boundary inside a block with M = 63 / 65); the backward takes 256 pixels per block over the flat pixel
index (c * H + y) * W + x, so a block seam falls in the middle of an image row and on a camera boundary (_seam_scene puts footprints
across both); there are no image tiles: a footprint is the 2 x 2 pixels of one cell of the (H + 1) x (W + 1) cell grid, and the cells of
column / row 0 and W / H are the ones with corners outside.  Ratios measured on MI355X: profiles/r15_depth_loss.md."""
import functools

import numpy as np
import pytest
import torch

import depth_loss_helper as DH
import raster_modes_helper as RM

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23


def _dev():
    return torch.device("cuda:0")


def _gpu(depths, points, depths_gt, valid=None, g=None, layout="plain"):
    """-> dict(loss 0-d, v_depth [C,H,W]) as CPU fp32 tensors through the public depth_loss and autograd.  layout "plain": contiguous
    [C,H,W]; "channel": channel 3 of a [C,H,W,4] tensor, passed as the [C,H,W,1] view the trainer passes"""
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    if layout == "channel":
        full = torch.full((*depths.shape, 4), 7.0, device=dev)
        full[..., 3] = depths.to(dev)
        full.requires_grad_(True)
        leaf, d = full, full[..., 3:4]
    else:
        leaf = depths.to(dev).requires_grad_(True)
        d = leaf
    out = wm.depth_loss(d, points.to(dev), depths_gt.to(dev), None if valid is None else valid.to(dev))
    if g is None:
        out.backward()
    else:
        out.backward(g.to(dev))
    torch.cuda.synchronize()
    grad = leaf.grad
    if layout == "channel":
        assert not grad[..., :3].any()
        grad = grad[..., 3]
    return dict(loss=out.detach().cpu(), v_depth=grad.cpu().contiguous())


def _check(tag, got, ref, f32, bound):
    """got (GPU), ref (fp64), f32 (helper fp32): dict(loss, v_depth).  Prints every figure, then asserts."""
    assert torch.isfinite(got["v_depth"]).all() and got["loss"].dim() == 0, tag
    r64 = np.asarray(ref["v_depth"], np.float64)
    yard = max(DH.max_rel(f32["v_depth"].numpy(), r64), ULP)
    err = DH.max_rel(got["v_depth"].numpy(), r64)
    d = abs(float(got["loss"]) - float(ref["loss"]))
    print(f"{tag} v_depth: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.3f}")
    print(f"{tag} loss: gpu {float(got['loss']):.9g} fp64 {float(ref['loss']):.12g} |gpu - fp64| {d:.3e} bound {bound:.3e} ratio {d / bound:.3f}")
    assert err <= FACTOR * yard, (tag, yard, err)
    assert d <= bound, (tag, d, bound)


@functools.lru_cache(maxsize=None)
def _golden(name):
    z = DH.load_golden(name)
    t = {k: torch.from_numpy(z[k]) for k in ("depths", "points", "depths_gt")}
    f32 = DH.gradients(t["depths"], t["points"], t["depths_gt"], None, torch.float32)
    return z, t, f32, DH.scalar_bound(t["depths"], t["points"], t["depths_gt"])


@pytest.mark.parametrize("name", ["a", "b"])
def test_gpu_matches_the_reference_goldens(name):
    z, t, f32, bound = _golden(name)
    got = _gpu(t["depths"], t["points"], t["depths_gt"])
    _check(f"golden {name}", got, z, f32, bound)
    # The yardstick is loose on these scenes (partly zero footprints give small samples and large 1 / d^2: 4.5e-6 and 5.9e-5), so the
    # goldens are also held to the bound that follows from the kernels' own arithmetic (depth_loss_helper.gradient_bound), element by
    # element.  (Scene b keeps points that sit ON a grid line off samples of exactly 0: tools/gen_golden_depth_loss.py says why.)
    gb = DH.gradient_bound(t["depths"], t["points"], t["depths_gt"])
    worst = float(np.abs(got["v_depth"].numpy().astype(np.float64) - z["v_depth"]).max())
    print(f"golden {name} v_depth: largest element error {worst:.3e} derived bound {gb:.3e} ratio {worst / gb:.3f}")
    assert worst <= gb


def _draw_points(g, depths, M, lo, hi):
    """M points per camera, uniform in [lo, W + hi) x [lo, H + hi), each at least 1e-4 px from an integer, with a sample that is exactly 0
    or at least 0.02, and a term at least 1e-3 disp_gt from the L1 kink -> points [C,M,2], depths_gt [C,M]"""
    C, H, W = depths.shape
    n = 4 * M + 64
    p = torch.rand(C, n, 2, generator=g) * torch.tensor([W + hi - lo, H + hi - lo]) + lo
    gt = 0.4 + 3.6 * torch.rand(C, n, generator=g)
    d = DH.sample(depths.double(), p.double())
    disp, disp_gt = DH.disparity(d), 1.0 / gt.double()
    ok = ((p.double() - p.double().round()).abs().min(-1).values >= 1e-4) & ((d == 0) | (d >= 0.02)) & ((disp - disp_gt).abs() >= 1e-3 * disp_gt)
    pts, gts = [], []
    for c in range(C):
        idx = torch.nonzero(ok[c])[:M, 0]
        assert idx.numel() == M
        pts.append(p[c, idx])
        gts.append(gt[c, idx])
    return torch.stack(pts), torch.stack(gts)


def _depths(g, C, H, W):
    d = 0.3 + 2.7 * torch.rand(C, H, W, generator=g)
    d[torch.rand(C, H, W, generator=g) < 0.15] = 0.0       # scattered zero pixels: rows with a zero, a partly zero and a live sample
    return d


@functools.lru_cache(maxsize=None)
def _scene(C, H, W, M, kind):
    """-> inputs, fp64 reference, fp32 yardstick, scalar bound.  kind "inside": points over the image and its last half-pixel strips;
    "around": up to 1.5 px outside on every side; "masked": a valid mask over ~70 % of the rows, the others NaN; "one_dead": as masked
    with every row of camera 0 flagged out"""
    g = torch.Generator().manual_seed(97 * C + 31 * H + 7 * W + M + len(kind))
    depths = _depths(g, C, H, W)
    lo, hi = (-1.5, 2.0) if kind == "around" else (0.0, 0.0)
    points, gt = _draw_points(g, depths, M, lo, hi)
    valid = None
    if kind in ("masked", "one_dead"):
        valid = torch.rand(C, M, generator=g) < 0.7
        valid[-1, 0] = True
        if kind == "one_dead":
            valid[0] = False
        points[~valid] = float("nan")
        gt[~valid] = float("nan")
    ref = DH.gradients(depths, points, gt, valid, torch.float64)
    f32 = DH.gradients(depths, points, gt, valid, torch.float32)
    t = dict(depths=depths, points=points, depths_gt=gt, valid=valid)
    return t, ref, f32, DH.scalar_bound(depths, torch.nan_to_num(points), torch.nan_to_num(gt, nan=1.0), valid)


# (C, H, W, M, kind): one row; the camera boundary inside a 256-row block; the 256-row block seam; the smallest images; masks
EXTRA = [(1, 9, 13, 1, "inside"), (2, 9, 13, 63, "inside"), (2, 9, 13, 64, "around"), (2, 9, 13, 65, "masked"), (1, 21, 17, 255, "around"),
         (1, 21, 17, 256, "inside"), (2, 21, 17, 257, "masked"), (3, 21, 17, 257, "around"), (2, 2, 7, 65, "around"), (2, 7, 2, 65, "around"),
         (1, 2, 2, 64, "around"), (2, 21, 17, 257, "one_dead"), (2, 37, 29, 1537, "around")]


@pytest.mark.parametrize("case", EXTRA, ids=[f"C{c[0]}-{c[1]}x{c[2]}-M{c[3]}-{c[4]}" for c in EXTRA])
def test_gpu_matches_the_helper_on_extra_shapes(case):
    t, ref, f32, bound = _scene(*case)
    got = _gpu(t["depths"], t["points"], t["depths_gt"], t["valid"])
    _check(str(case), got, ref, f32, bound)
    if case[4] == "one_dead":
        assert not got["v_depth"][0].any() and got["v_depth"][1].any()        # the camera without a valid row: exact zeros beside a live one


def test_gpu_points_outside_the_image_count_with_zero_disparity_and_no_gradient():
    """A point further than one pixel outside, on every side: its term is |0 - disp_gt| and it reaches no pixel."""
    g = torch.Generator().manual_seed(5)
    C, H, W = 2, 9, 13
    depths = 0.5 + torch.rand(C, H, W, generator=g)
    out = torch.tensor([[-1.0, 4.0], [-7.5, 3.0], [13.0, 4.0], [20.25, 2.0], [5.0, -1.0], [5.0, -3.5], [5.0, 9.0], [6.0, 30.0], [-2.0, -2.0], [14.0, 11.0],
                        [1e30, 2.0], [3.0, -1e30]])
    points = out.repeat(C, 1, 1)
    gt = 0.5 + torch.rand(C, out.shape[0], generator=g)
    got = _gpu(depths, points, gt)
    want = float((1.0 / gt.double()).mean())
    assert abs(float(got["loss"]) - want) <= 16 * 2.0 ** -24 * want
    assert not got["v_depth"].any()


def _seam_scene():
    """2 cameras of 20 x 24 = 480 pixels: the backward's 256-pixel blocks end after flat pixel 255 = (y 10, x 15) of camera 0, after
    pixel 511 = camera 1 (y 1, x 7), and camera 0's last pixel 479 is followed by camera 1's first in one block.  Footprints across each,
    several rows per cell, plus the four image corners."""
    g = torch.Generator().manual_seed(8)
    C, H, W = 2, 20, 24
    depths = 0.5 + 2.0 * torch.rand(C, H, W, generator=g)
    base = torch.tensor([[15.4, 10.3], [15.7, 9.6], [15.2, 10.8], [22.6, 18.7], [23.3, 19.4], [22.9, 19.2], [0.3, 0.2], [-0.4, -0.7], [7.5, 1.5], [7.2, 0.6],
                         [23.5, -0.5], [-0.5, 19.5], [23.6, 19.7], [6.7, 1.1]])
    points = torch.stack([base, base.flip(0)])
    gt = 0.4 + 3.0 * torch.rand(C, base.shape[0], generator=g)
    assert DH.kink_margin(depths, points, gt) >= 1e-3
    return depths, points, gt


def test_gpu_footprints_across_the_block_seams():
    depths, points, gt = _seam_scene()
    ref = DH.gradients(depths, points, gt, None, torch.float64)
    f32 = DH.gradients(depths, points, gt, None, torch.float32)
    got = _gpu(depths, points, gt)
    _check("seams", got, ref, f32, DH.scalar_bound(depths, points, gt))
    touched = ref["v_depth"] != 0
    assert touched[0, 10, 15] and touched[0, 10, 16] and touched[0, 19, 23] and touched[1, 0, 0] and touched[1, 1, 7] and touched[1, 1, 8]


def _raw(depth_view, points, gt, valid, g, v_fill=float("nan")):
    """the two C ABI calls on device tensors -> loss (0-d), v_depth [C,H,W] contiguous, pre-filled with v_fill"""
    import ctypes as C
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    dev = depth_view.device
    Cn, H, W = depth_view.shape
    M = points.shape[1]
    out = torch.empty((), device=dev)
    v = torch.full((Cn, H, W), v_fill, device=dev)
    ws = torch.empty(L.wm_depth_loss_workspace_bytes(Cn, H, W, M, 1), device=dev, dtype=torch.uint8)
    st = (C.c_int64 * 3)(*depth_view.stride())
    vst = (C.c_int64 * 3)(*v.stride())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
    assert L.wm_depth_loss(ptr(depth_view), st, Cn, H, W, ptr(points), ptr(gt), ptr(valid), M, 1, ptr(out), ptr(ws), ws.numel(), stream) == 0
    assert L.wm_depth_loss_backward(Cn, H, W, ptr(points), M, ptr(g), ptr(v), vst, ptr(ws), ws.numel(), stream) == 0
    torch.cuda.synchronize()
    return out, v


def test_gpu_every_pixel_is_written_and_untouched_pixels_are_exact_zeros():
    """v_depth pre-filled with NaN: afterwards no NaN is left, and every pixel that no valid row with d > 0 reaches holds 0.0"""
    dev = _dev()
    z, t, _, _ = _golden("b")
    g = torch.ones((), device=dev)
    out, v = _raw(t["depths"].to(dev), t["points"].to(dev), t["depths_gt"].to(dev), None, g)
    assert torch.isfinite(v).all()
    # by geometry, not by the reference's values (its own normalisation gives a point on an integer coordinate a weight of ~1e-16 in a
    # neighbour column): a pixel one pixel or more away from every point on either axis is untouched; a pixel strictly inside the
    # footprint of a point whose sample is above 0 is touched
    Cn, H, W = t["depths"].shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    live = DH.sample(t["depths"].double(), t["points"].double()) > 0
    untouched, touched = torch.ones(Cn, H, W, dtype=torch.bool), torch.zeros(Cn, H, W, dtype=torch.bool)
    for c in range(Cn):
        px, py = t["points"][c, :, 0].double(), t["points"][c, :, 1].double()
        dist = torch.maximum((xx[None] - px[:, None, None]).abs(), (yy[None] - py[:, None, None]).abs())      # [M,H,W]
        untouched[c] = (dist >= 1.0).all(0)
        touched[c] = (dist[live[c]] < 1.0 - 1e-6).any(0)
    assert int(untouched.sum()) > 100 and int(touched.sum()) > 100
    assert not v.cpu()[untouched].any() and v.cpu()[touched].all()
    # M = 0: NaN (the mean of nothing) and an all-zero gradient; so with rows that are all flagged out
    empty = torch.empty(3, 0, 2, device=dev)
    out0, v0 = _raw(t["depths"].to(dev), empty, empty[..., 0], None, g)
    assert torch.isnan(out0) and not v0.any() and torch.isfinite(v0).all()
    none = torch.zeros(t["depths_gt"].shape, dtype=torch.bool, device=dev)
    out1, v1 = _raw(t["depths"].to(dev), t["points"].to(dev), t["depths_gt"].to(dev), none, g)
    assert torch.isnan(out1) and not v1.any() and torch.isfinite(v1).all()
    import hunyuanworld_mirror_amd as wm
    d = t["depths"].to(dev).requires_grad_(True)
    loss = wm.depth_loss(d, empty, empty[..., 0])
    loss.backward()
    assert torch.isnan(loss) and d.grad is not None and not d.grad.any()


def test_gpu_bitwise_reproducible_and_layout_independent():
    z, t, _, _ = _golden("b")
    first = _gpu(t["depths"], t["points"], t["depths_gt"])
    again = _gpu(t["depths"], t["points"], t["depths_gt"])
    channel = _gpu(t["depths"], t["points"], t["depths_gt"], layout="channel")
    for other in (again, channel):
        assert torch.equal(first["loss"], other["loss"]) and torch.equal(first["v_depth"], other["v_depth"])
    # and the C ABI writing v_depth with the depth image's own strides into channel 3 of a [C,H,W,4] buffer
    import ctypes as C
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    dev = _dev()
    full = torch.zeros(*t["depths"].shape, 4, device=dev)
    full[..., 3] = t["depths"].to(dev)
    view = full[..., 3]
    p, gt = t["points"].to(dev), t["depths_gt"].to(dev)
    Cn, H, W = view.shape
    M = p.shape[1]
    out, g = torch.empty((), device=dev), torch.ones((), device=dev)
    vfull = torch.full_like(full, -3.0)
    ws = torch.empty(L.wm_depth_loss_workspace_bytes(Cn, H, W, M, 1), device=dev, dtype=torch.uint8)
    st = (C.c_int64 * 3)(*view.stride())
    vp = lambda x: C.c_void_p(x.data_ptr())
    assert L.wm_depth_loss(vp(view), st, Cn, H, W, vp(p), vp(gt), None, M, 1, vp(out), vp(ws), ws.numel(), None) == 0
    assert L.wm_depth_loss_backward(Cn, H, W, vp(p), M, vp(g), vp(vfull[..., 3]), st, vp(ws), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), first["loss"]) and torch.equal(vfull[..., 3].cpu(), first["v_depth"]) and bool((vfull[..., :3] == -3.0).all())


def test_gpu_sort_scratch_rule_covers_the_library_at_the_largest_timed_size():
    """The workspace counts the radix sort's scratch by a rule of its own (8 bytes per row + 1 MiB, csrc/depthloss.hip) and the backward asks
    the library on the device what it needs, refusing with an error status if that were more.  8 views of 518 x 518 with 262 144 rows each
    (2.1 M pairs, 22-bit keys; the largest size of profiles/r15_depth_loss.md) is where a library configuration that needs more would show:
    the backward must succeed there.  The loss of that many row blocks is held to the scalar bound against the restatement in fp64 on the
    same device, and the gradient is finite and not empty."""
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(11)
    C, H, W, M = 8, 518, 518, 262144
    full = torch.rand(C, H, W, 4, device=dev, generator=g)
    view = full[..., 3].mul_(3.0).add_(0.5)                        # channel 3 of a render, in [0.5, 3.5)
    points = torch.rand(C, M, 2, device=dev, generator=g) * torch.tensor([float(W), float(H)], device=dev)
    gt = 0.4 + 3.6 * torch.rand(C, M, device=dev, generator=g)
    out, v = _raw(view, points, gt, None, torch.ones((), device=dev))      # asserts that both calls return WM_OK
    ref = float(DH.loss(view.double(), points.double(), gt.double()))
    bound = DH.scalar_bound(view, points, gt)
    d = abs(float(out) - ref)
    print(f"8 x 518 x 518 x 262144 loss: gpu {float(out):.9g} fp64 {ref:.12g} |gpu - fp64| {d:.3e} bound {bound:.3e} ratio {d / bound:.3f}")
    assert d <= bound
    assert torch.isfinite(v).all() and v.any()


def test_gpu_autograd_surface():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    z, t, _, _ = _golden("a")
    dep, p, gt = t["depths"].to(dev), t["points"].to(dev), t["depths_gt"].to(dev)
    # a gradient for depths only
    d = dep.clone().requires_grad_(True)
    p_, gt_ = p.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    loss = wm.depth_loss(d, p_, gt_)
    assert loss.dim() == 0 and loss.grad_fn is not None
    loss.backward()
    assert p_.grad is None and gt_.grad is None and d.grad is not None and d.grad.shape == d.shape and d.grad.dtype == torch.float32
    base = d.grad.clone()
    # [C,H,W,1] gives the same bits and a gradient of that shape
    d4 = dep.clone()[..., None].requires_grad_(True)
    l4 = wm.depth_loss(d4, p, gt)
    l4.backward()
    assert torch.equal(l4.detach(), loss.detach()) and d4.grad.shape == d4.shape and torch.equal(d4.grad[..., 0], base)
    # forward-only paths: no_grad, and depths that do not require grad
    with torch.no_grad():
        ng = wm.depth_loss(dep.clone().requires_grad_(True), p, gt)
    plain = wm.depth_loss(dep, p, gt)
    assert ng.grad_fn is None and plain.grad_fn is None and torch.equal(ng, loss.detach()) and torch.equal(plain, loss.detach())
    # a non-unit upstream gradient, as a device scalar: fp64 reference at that g, the yardstick of the golden
    gup = torch.tensor(-2.75, device=dev)
    d2 = dep.clone().requires_grad_(True)
    wm.depth_loss(d2, p, gt).backward(gup)
    torch.cuda.synchronize()
    f32 = DH.gradients(t["depths"], t["points"], t["depths_gt"], None, torch.float32, -2.75)
    yard = max(DH.max_rel(f32["v_depth"].numpy(), -2.75 * z["v_depth"]), ULP)
    err = DH.max_rel(d2.grad.cpu().numpy(), -2.75 * z["v_depth"])
    print(f"upstream gradient -2.75: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.3f}")
    assert err <= FACTOR * yard
    d0 = dep.clone().requires_grad_(True)
    (0.0 * wm.depth_loss(d0, p, gt)).backward()                     # a zero upstream gradient gives an all-zero gradient
    assert not d0.grad.any() and torch.isfinite(d0.grad).all()
    # half precision in: the same loss as the cast-up image, the gradient back in the input's dtype
    for dt in (torch.float16, torch.bfloat16):
        h = dep.to(dt).requires_grad_(True)
        lh = wm.depth_loss(h, p, gt)
        lh.backward()
        up = h.detach().float().requires_grad_(True)
        lu = wm.depth_loss(up, p, gt)
        lu.backward()
        assert lh.dtype == torch.float32 and torch.equal(lh.detach(), lu.detach())
        assert h.grad.dtype == dt and torch.equal(h.grad, up.grad.to(dt))
    # two forwards, then two backwards: each node owns its workspace
    a, b = dep.clone().requires_grad_(True), (dep * 1.5).requires_grad_(True)
    la, lb = wm.depth_loss(a, p, gt), wm.depth_loss(b, p, gt)
    la.backward()
    lb.backward()
    assert torch.equal(a.grad, base) and not torch.equal(b.grad, base)


def test_gpu_errors_raise_before_any_launch():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    d = torch.rand(2, 9, 13, device=dev, requires_grad=True)
    p, gt = torch.rand(2, 5, 2, device=dev), torch.rand(2, 5, device=dev) + 0.5
    with pytest.raises(RuntimeError):
        wm.depth_loss(d.detach().cpu(), p.cpu(), gt.cpu())
    with pytest.raises(RuntimeError):
        wm.depth_loss(d, p.cpu(), gt)
    for bad in (dict(depths=torch.rand(2, 9, 13, 2, device=dev)), dict(depths=torch.rand(9, 13, device=dev)), dict(depths=torch.rand(2, 1, 13, device=dev)),
                dict(depths=torch.rand(2, 9, 1, device=dev)), dict(points=torch.rand(3, 5, 2, device=dev)), dict(points=torch.rand(2, 5, 3, device=dev)),
                dict(depths_gt=torch.rand(2, 6, device=dev)), dict(valid=torch.ones(2, 4, dtype=torch.bool, device=dev))):
        kw = dict(depths=d, points=p, depths_gt=gt, valid=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            wm.depth_loss(**kw)
    pw, c2w, K = torch.rand(7, 3, device=dev), torch.eye(4, device=dev).repeat(2, 1, 1), torch.eye(3, device=dev).repeat(2, 1, 1)
    with pytest.raises(RuntimeError):
        wm.project_depth_points(pw.cpu(), c2w.cpu(), K.cpu(), 13, 9)
    for bad in (dict(points_world=torch.rand(7, 2, device=dev)), dict(camtoworlds=torch.eye(4, device=dev)), dict(Ks=K[:1]),
                dict(visible=torch.ones(2, 6, dtype=torch.bool, device=dev)), dict(width=0)):
        kw = dict(points_world=pw, camtoworlds=c2w, Ks=K, width=13, height=9, visible=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            wm.project_depth_points(**kw)


def _check_projection(tag, got, ref, f32, live):
    """points / depths under the yardstick rule on the rows `live` [C,P] (where the inputs are defined); the selector exactly"""
    for k in ("points", "depths"):
        r64 = np.asarray(ref[k], np.float64)[live]
        yard = max(DH.max_rel(f32[k].numpy()[live], r64), ULP)
        err = DH.max_rel(got[k].numpy()[live], r64)
        print(f"{tag} {k}: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.3f}")
        assert err <= FACTOR * yard, (tag, k, yard, err)
    assert np.array_equal(got["valid"].numpy(), np.asarray(ref["valid"])), tag


def _gpu_project(pw, c2w, Ks, W, H, vis):
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    p, d, v = wm.project_depth_points(pw.to(dev), c2w.to(dev), Ks.to(dev), W, H, None if vis is None else vis.to(dev))
    torch.cuda.synchronize()
    assert p.dtype == torch.float32 and d.dtype == torch.float32 and v.dtype == torch.bool
    return dict(points=p.cpu(), depths=d.cpu(), valid=v.cpu())


def test_gpu_projection_matches_the_reference_golden():
    z = DH.load_golden("proj")
    pw, c2w, Ks, vis = (torch.from_numpy(z[k]) for k in ("points_world", "camtoworlds", "Ks", "visible"))
    W, H = int(z["width"]), int(z["height"])
    f32 = dict(zip(("points", "depths", "valid"), DH.project(pw, c2w, Ks, W, H, vis)))
    got = _gpu_project(pw, c2w, Ks, W, H, vis)
    _check_projection("golden proj", got, z, f32, vis.numpy())
    # without the mask: the helper in fp64 is the reference (pinned to the golden by the CPU test)
    ref = dict(zip(("points", "depths", "valid"), (x.numpy() for x in DH.project(pw.double(), c2w.double(), Ks.double(), W, H))))
    f32 = dict(zip(("points", "depths", "valid"), DH.project(pw, c2w, Ks, W, H)))
    _check_projection("golden proj, no mask", _gpu_project(pw, c2w, Ks, W, H, None), ref, f32, np.ones(vis.shape, bool))


def test_gpu_projection_selector_edges_exactly():
    """Identity camera, power-of-two numbers: x = 0 and y = 0 are inside, x = W and y = H are not, z = 0 is not (nor z < 0)."""
    W, H = 16, 8
    K = torch.tensor([[4.0, 0, 8.0], [0, 4.0, 4.0], [0, 0, 1.0]])[None]
    c2w = torch.eye(4)[None]
    #                  x = 0            x = W           inside            y = 0            y = H           z = 0           behind           x = W - 1/4
    pw = torch.tensor([[-4.0, 0, 2.0], [4.0, 0, 2.0], [0.0, 0.0, 1.0], [0.0, -2.0, 2.0], [0.0, 2.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [7.875, 0, 4.0],
                       [-4.0, -2.0, 2.0], [-4.25, 0, 2.0]])          # the corner (0, 0); just left of x = 0
    got = _gpu_project(pw, c2w, K, W, H, None)
    assert got["valid"][0].tolist() == [True, False, True, True, False, False, False, True, True, False]
    assert got["points"][0, 0].tolist() == [0.0, 4.0] and got["points"][0, 1].tolist() == [16.0, 4.0] and got["points"][0, 4].tolist() == [8.0, 8.0]
    assert got["points"][0, 7].tolist() == [15.875, 4.0] and got["depths"][0].tolist() == [2.0, 2.0, 1.0, 2.0, 2.0, 0.0, -1.0, 4.0, 2.0, 2.0]
    vis = torch.tensor([[True, True, False, True, True, True, True, True, False, True]])
    assert _gpu_project(pw, c2w, K, W, H, vis)["valid"][0].tolist() == [True, False, False, True, False, False, False, True, False, False]


def _opt_scene():
    """the 150-Gaussian, 2-view, 64 x 48 scene of tests/test_photometric_gpu.py"""
    import test_photometric_gpu as TP
    return TP._opt_scene()


def test_gpu_optimises_with_the_depth_loss_like_the_fp64_restatement():
    """20 Adam steps at lr 2e-3 on photometric_loss + 1e-2 * depth_loss from a perturbed start, on the GPU (fp32: Rasterizer's RGB+ED
    triple, photometric_loss, project_depth_points, depth_loss) and on the CPU restatements in fp64.  Supervision: the true scene's expected
    depth unprojected at ~200 pixels per view whose true alpha exceeds 0.5, all ~400 world points projected into both views.  (This is
    not 400 points unprojected and kept per camera, as the feature's description words it: the points are pooled, so that each view gets
    its ~400 rows (398 and 381 valid) and also meets rows that fall outside it, which the selector has to flag out.)  The depth-loss curves stay within 2 % of each other at every step (the bound the parent's loop tests hold on this scene: the depth loss
    adds no new fp32 path inside the rasteriser and its own gradient is pinned above) and both end below their start."""
    import hunyuanworld_mirror_amd as wm
    import photometric_helper as PH
    true, start, vm, K, W, H = _opt_scene()
    dev = _dev()
    c2w64 = torch.linalg.inv(vm)
    with torch.no_grad():
        _, depth_true, alpha_true = RM.rasterize(true["means"], true["quats"], true["scales"], true["opacities"], true["colors"], False, vm, K, W, H)
    world = []
    for c in range(2):
        ys, xs = torch.nonzero(alpha_true[c, ..., 0] > 0.5, as_tuple=True)
        pick = torch.arange(0, ys.numel(), max(ys.numel() // 200, 1))[:200]
        ys, xs = ys[pick], xs[pick]
        z = depth_true[c, ys, xs, 0]
        ray = torch.linalg.inv(K[c]) @ torch.stack([xs.double(), ys.double(), torch.ones_like(z)])
        cam = ray * z
        world.append((c2w64[c, :3, :3] @ cam + c2w64[c, :3, 3:4]).T)
    world = torch.cat(world).float()                     # the supervision both runs see: fp32 world points
    assert 300 <= world.shape[0] <= 400

    def run(render, cast, photo, sup, sup_loss):
        points, gts, valid = sup
        assert int(valid.sum(1).min()) >= 200
        p = {k: cast(v).clone().requires_grad_(True) for k, v in start.items()}
        with torch.no_grad():
            target = render({k: cast(v) for k, v in true.items()})[0]
        opt = torch.optim.Adam(list(p.values()), lr=2e-3)
        curve = []
        for _ in range(20):
            opt.zero_grad()
            rgb, depth, _ = render(p)
            dl = sup_loss(depth, points, gts, valid)
            (photo(rgb, target) + 1e-2 * dl).backward()
            opt.step()
            curve.append(float(dl.detach()))
        return curve

    rz = wm.Rasterizer()
    c2w, Kg = c2w64.float().to(dev), K.float().to(dev)
    gpu = run(lambda p: rz.rasterize_splats(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], c2w, Kg, W, H), lambda v: v.float().to(dev),
              lambda rgb, tgt: wm.photometric_loss(rgb, tgt, 0.2, "valid")[0], wm.project_depth_points(world.to(dev), c2w, Kg, W, H), wm.depth_loss)
    cpu = run(lambda p: RM.rasterize(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], False, vm, K, W, H), lambda v: v,
              lambda rgb, tgt: PH.loss(rgb.permute(0, 3, 1, 2), tgt.permute(0, 3, 1, 2), "valid", 0.2)[0], DH.project(world.double(), c2w64, K, W, H),
              lambda depth, points, gts, valid: DH.loss(depth[..., 0], points, gts, valid))
    gap = max(abs(a - b) / b for a, b in zip(gpu, cpu))
    print("depth-loss curves: gpu", [f"{x:.6f}" for x in gpu], "cpu fp64", [f"{x:.6f}" for x in cpu], "largest gap", gap)
    assert gap < 0.02
    assert gpu[-1] < gpu[0] and cpu[-1] < cpu[0]
