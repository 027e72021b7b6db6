"""CPU: the torch restatement tests/depth_loss_helper.py against the reference's own numbers (tests/golden/depth_loss_*.npz, written by
tools/gen_golden_depth_loss.py from the trainer's `if cfg.depth_loss:` block and the dataset's `if self.load_depths:` block), against
finite differences, and the argument checks of the C ABI entries, which come before any launch and so answer without a GPU.

About the gradient goldens.  The reference differentiates torch.where(d > 0, 1 / d, 0) as written, so a row whose sampled depth is
EXACTLY 0 sends 0 * (-1 / 0^2) = NaN into the four pixels under it (`v_depth_raw`; both scenes hold such rows: the rectangle of zero
depths).  The kernels, the header and the helper define such a row to add nothing.  `v_depth` is the reference's own number for that
definition: the same block run per camera on the rows with d > 0, weighted by their share of the mean.  The helper is held to
`v_depth` everywhere and to `v_depth_raw` wherever that is finite, and the NaN pixels must be the pixels under the d = 0 rows."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import depth_loss_helper as DH
from conftest import ROOT

LIB = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
WM_OK, WM_ERR_INVALID = 0, 1


def _scene(name):
    z = DH.load_golden(name)
    return z, {k: torch.from_numpy(z[k]) for k in ("depths", "points", "depths_gt")}


@pytest.mark.parametrize("name", ["a", "b"])
def test_helper_matches_the_reference_loss_and_gradient(name):
    z, t = _scene(name)
    assert t["depths"].dtype == torch.float32 and t["points"].dtype == torch.float32
    got = DH.gradients(t["depths"], t["points"], t["depths_gt"], None, torch.float64)
    e_loss = abs(float(got["loss"]) - float(z["loss"])) / abs(float(z["loss"]))
    e_grad = DH.max_rel(got["v_depth"].numpy(), z["v_depth"])
    raw = z["v_depth_raw"]
    fin = np.isfinite(raw)
    e_raw = float(np.abs(got["v_depth"].numpy() - raw)[fin].max() / np.abs(z["v_depth"]).max())
    print(f"{name}: loss {e_loss:.3e} gradient {e_grad:.3e} raw gradient on its finite pixels {e_raw:.3e}")
    assert e_loss <= 1e-12 and e_grad <= 1e-12 and e_raw <= 1e-12
    # the NaN pixels of the reference's raw gradient: the pixels under the rows whose sample is exactly 0.  Every pixel nearer than one
    # pixel on both axes must be NaN, none further away may be; a pixel at a distance of exactly one (a corner of weight 0, which
    # grid_sample reaches or not depending on how its own normalisation rounds) may be either.
    d = DH.sample(t["depths"].double(), t["points"].double())
    Cn, H, W = t["depths"].shape
    must, may = np.zeros((Cn, H, W), bool), np.zeros((Cn, H, W), bool)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for c, m in zip(*np.nonzero((d == 0).numpy())):
        dist = np.maximum(np.abs(xx - float(t["points"][c, m, 0])), np.abs(yy - float(t["points"][c, m, 1])))
        must[c] |= dist < 1 - 1e-9
        may[c] |= dist < 1 + 1e-9
    assert int((d == 0).sum()) >= 5 and (~fin)[must].all() and not (~fin)[~may].any()


@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_scenes_are_what_they_are_meant_to_be(name):
    z, t = _scene(name)
    Cn, H, W = t["depths"].shape
    M = t["points"].shape[1]
    assert (Cn, H, W, M) == {"a": (2, 9, 13, 50), "b": (3, 48, 64, 1537)}[name]
    dep, p = t["depths"], t["points"]
    assert ((dep == 0) | (dep >= 0.2)).all() and int((dep == 0).sum()) > 0
    assert (p[..., 0] >= 0).all() and (p[..., 0] < W).all() and (p[..., 1] >= 0).all() and (p[..., 1] < H).all()       # what the dataset keeps
    assert int((p[..., 0] > W - 1).sum()) >= 5
    assert DH.kink_margin(dep, p, t["depths_gt"]) >= 1e-3
    if name == "b":
        assert int((p[..., 1] > H - 1).sum()) >= 5 and int((p[..., 0] == W - 1).sum()) >= 5
        assert int(((p == p.round()).all(-1)).sum()) >= 20
        cell = torch.floor(p[..., 0]) + W * torch.floor(p[..., 1])
        for c in range(Cn):
            assert int(torch.bincount(cell[c].long()).max()) >= 300      # one cell's four pixels take 300 rows or more


def test_helper_mask_is_the_loss_of_the_selected_rows():
    """valid = the reference run on the selected subset (one camera) and F.l1_loss over the concatenation (several); rows that are
    flagged out may hold NaN."""
    z, t = _scene("a")
    g = torch.Generator().manual_seed(3)
    valid = torch.rand(t["depths_gt"].shape, generator=g) < 0.6
    valid[1] = False
    valid[1, :7] = True
    dep = t["depths"].double().requires_grad_(True)
    disp = [DH.disparity(DH.sample(dep[c:c + 1], t["points"].double()[c:c + 1, valid[c]])) for c in range(2)]
    gt = [1.0 / t["depths_gt"].double()[c:c + 1, valid[c]] for c in range(2)]
    want = torch.nn.functional.l1_loss(torch.cat(disp, 1), torch.cat(gt, 1))
    want.backward()
    poisoned = {k: t[k].clone() for k in ("points", "depths_gt")}
    poisoned["points"][~valid] = float("nan")
    poisoned["depths_gt"][~valid] = float("nan")
    got = DH.gradients(t["depths"], poisoned["points"], poisoned["depths_gt"], valid, torch.float64)
    assert abs(float(got["loss"]) - float(want.detach())) <= 1e-14 and DH.max_rel(got["v_depth"].numpy(), dep.grad.numpy()) <= 1e-13
    none = DH.gradients(t["depths"], t["points"], t["depths_gt"], torch.zeros_like(valid), torch.float64)
    assert torch.isnan(none["loss"]) and not none["v_depth"].any()


def test_helper_gradient_matches_finite_differences():
    """central differences on scene a, over every pixel with a depth above 0 (a zero pixel sits on the d > 0 switch of the rows that
    sample exactly 0 there: the loss jumps, no derivative to compare)"""
    z, t = _scene("a")
    dep = t["depths"].double()
    p, gt = t["points"].double(), t["depths_gt"].double()
    grad = DH.gradients(t["depths"], t["points"], t["depths_gt"], None, torch.float64)["v_depth"]
    h = 1e-6
    worst = 0.0
    for c, y, x in zip(*np.nonzero((dep > 0).numpy())):
        a, b = dep.clone(), dep.clone()
        a[c, y, x] += h
        b[c, y, x] -= h
        fd = (float(DH.loss(a, p, gt)) - float(DH.loss(b, p, gt))) / (2 * h)
        worst = max(worst, abs(fd - float(grad[c, y, x])))
    scale = float(grad.abs().max())
    print(f"finite differences: largest gap {worst:.3e} against max |gradient| {scale:.3e}")
    assert worst <= 1e-7 * scale


def test_helper_projection_matches_the_reference():
    z = DH.load_golden("proj")
    vis = torch.from_numpy(z["visible"])
    pts, dep, valid = DH.project(torch.from_numpy(z["points_world"]).double(), torch.from_numpy(z["camtoworlds"]).double(),
                                 torch.from_numpy(z["Ks"]).double(), int(z["width"]), int(z["height"]), vis)
    W, H = int(z["width"]), int(z["height"])
    v = vis.numpy()
    e_p, e_d = DH.max_rel(pts.numpy()[v], z["points"][v]), DH.max_rel(dep.numpy()[v], z["depths"][v])
    print(f"projection: points {e_p:.3e} depths {e_d:.3e}; valid {int(z['valid'].sum())} of {int(v.sum())} visible")
    assert e_p <= 1e-12 and e_d <= 1e-12
    assert np.array_equal(valid.numpy(), z["valid"])
    # the fixture keeps clear of the selector's edges, and holds every way of being left out
    x, y, d = z["points"][v][:, 0], z["points"][v][:, 1], z["depths"][v]
    assert min(np.abs(x).min(), np.abs(x - W).min(), np.abs(y).min(), np.abs(y - H).min()) >= 1e-4 and np.abs(d).min() >= 1e-5
    front = d > 0
    assert (d < 0).sum() >= 5 and (x[front] < 0).sum() >= 5 and (x[front] >= W).sum() >= 5 and (y[front] < 0).sum() >= 5 and (y[front] >= H).sum() >= 5
    assert not z["valid"][~v].any() and 0 < z["valid"].sum() < v.sum()


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(LIB)
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    lib.wm_depth_loss_workspace_bytes.argtypes = [i32] * 5
    lib.wm_depth_loss_workspace_bytes.restype = C.c_size_t
    lib.wm_depth_loss.argtypes = [vp, i64p, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, C.c_size_t, vp]
    lib.wm_depth_loss_backward.argtypes = [i32, i32, i32, vp, i32, vp, vp, i64p, vp, C.c_size_t, vp]
    lib.wm_project_depth_points.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    return lib


def test_cabi_guards_answer_before_any_launch(L):
    """Every refusal below is decided on the host: the pointers are host buffers no kernel could read, and there is no GPU here."""
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    st = (C.c_int64 * 3)(13 * 9, 13, 1)
    Cn, H, W, M = 2, 9, 13, 50
    big = L.wm_depth_loss_workspace_bytes(Cn, H, W, M, 1)
    small = L.wm_depth_loss_workspace_bytes(Cn, H, W, M, 0)
    assert 0 < small < big

    def fwd(depth=p, strides=st, c=Cn, h=H, w=W, points=p, gt=p, m=M, want=1, out=p, ws=p, nbytes=None):
        return L.wm_depth_loss(depth, strides, c, h, w, points, gt, None, m, want, out, ws, big if nbytes is None else nbytes, None)

    def bwd(strides=st, c=Cn, h=H, w=W, points=p, m=M, g=p, v=p, ws=p, nbytes=None):       # (the backward takes neither the image nor depth_gt)
        return L.wm_depth_loss_backward(c, h, w, points, m, g, v, strides, ws, big if nbytes is None else nbytes, None)

    common = (dict(strides=None), dict(points=None), dict(ws=None), dict(c=0), dict(c=-1), dict(h=0), dict(w=0), dict(h=1), dict(w=1), dict(m=-1),
              dict(nbytes=big - 1), dict(nbytes=0))
    for call, cases in ((fwd, common + (dict(depth=None), dict(gt=None))), (bwd, common)):
        for kw in cases:
            assert call(**kw) == WM_ERR_INVALID, (call.__name__, kw)
    assert fwd(out=None) == WM_ERR_INVALID
    assert fwd(want=0, nbytes=small - 1) == WM_ERR_INVALID
    assert bwd(g=None) == WM_ERR_INVALID and bwd(v=None) == WM_ERR_INVALID
    assert bwd(nbytes=small) == WM_ERR_INVALID                      # the forward-only size is not enough for a backward
    assert fwd(m=0, points=None, gt=None, ws=None) == WM_ERR_INVALID           # M = 0 is legal, a null workspace is not

    def proj(pw=p, c2w=p, Ks=p, c=3, n=10, w=64, h=48, pts=p, dep=p, val=p):
        return L.wm_project_depth_points(pw, c2w, Ks, None, c, n, w, h, pts, dep, val, None)

    for kw in (dict(pw=None), dict(c2w=None), dict(Ks=None), dict(pts=None), dict(dep=None), dict(val=None), dict(c=0), dict(n=-1), dict(w=0), dict(h=0)):
        assert proj(**kw) == WM_ERR_INVALID, kw
    assert proj(n=0, pw=None, pts=None, dep=None, val=None) == WM_OK          # nothing to do, nothing launched


def test_cabi_workspace_size(L):
    size = L.wm_depth_loss_workspace_bytes
    assert size(0, 9, 13, 5, 1) == 0 and size(1, 1, 13, 5, 1) == 0 and size(1, 9, 1, 5, 1) == 0 and size(1, 9, 13, -1, 1) == 0
    assert size(1, 2, 2, 0, 1) > 0 and size(1, 2, 2, 0, 0) > 0                # M = 0 is a legal call
    assert size(1, 40000, 60000, 5, 1) == 0 and size(1 << 12, 9, 13, 1 << 20, 1) == 0     # beyond 31-bit cell keys / row indices
    for want in (0, 1):
        rows = [size(c, 48, 64, m, want) for c, m in ((1, 0), (1, 1), (1, 255), (1, 256), (1, 257), (2, 1537), (3, 1537), (8, 4096), (8, 262144))]
        assert rows == sorted(rows), rows
    assert len(set(size(c, 48, 64, m, 1) for c, m in ((1, 1), (1, 257), (2, 1537), (8, 4096), (8, 262144)))) == 5
    pix = [size(2, h, w, 300, 1) for h, w in ((2, 2), (9, 13), (48, 64), (518, 518), (1036, 1036))]
    assert pix == sorted(pix) and len(set(pix)) == len(pix), pix
    fwd_only = [size(2, h, w, 300, 0) for h, w in ((2, 2), (48, 64), (518, 518))]
    assert len(set(fwd_only)) == 1                                            # the forward alone keeps nothing per pixel
