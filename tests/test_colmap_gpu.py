"""GPU: hunyuanworld_mirror_amd.colmap (csrc/colmap.hip) against the reference's own recorded values (tests/golden/colmap_a.npz, written by
tools/gen_golden_colmap.py from the reference's --save_colmap statements in fp64 with a recording stand-in for pycolmap), against numpy
structured-dtype rebuilds of every file, and through load_colmap and project_depth_points back onto the source pixels.

Bounds.  Integers (ids, pixel coordinates, colours, track elements, counts, K) are exact.  Floating point: the golden file records how far
the reference's OWN fp32 CPU run of the same statements is from its fp64 run; a bound is 4 x that figure, the factor for another fp32
operation order (fused multiply-adds, the pose inverse rounded once instead of an fp32 elimination):
  point positions      recorded 5.45e-07 (largest of the three runs)  -> bound 2.18e-06     measured on MI355X: 3.25e-07
  reprojected pixel    recorded 6.61e-06                              -> bound 2.64e-05     measured on MI355X: 3.82e-06
  reprojected depth    recorded 7.15e-07                              -> bound 2.86e-06     measured on MI355X: 2.38e-07
The constants are read from the file; the numbers above are what it holds (profiles/r17_colmap_handoff.md has the table per run).

Seams of the kernels: 512 pixels of one view per selection block (two rounds of 256) and 256 records per packing block.  5 views of 37 x 53
are 4 blocks per view with a partial last one, so both scans cross blocks and views; P = 4097 is 16 full packing blocks and one record,
whose 59 bytes and 15 bytes both end off a dword boundary; P = 1 and P = 0 are the tails alone and nothing."""
import os

import numpy as np
import pytest
import torch

import colmap_helper as CH
from hunyuanworld_mirror_amd import (colmap, colmap_points_from_depth, load_colmap, project_depth_points, save_colmap, save_points_ply,
                                     save_scene_ply)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0


@pytest.fixture(scope="module")
def gold():
    return CH.load_golden("a")


def _gpu(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _select(z, percent, out_size=None, depth=None, conf=None):
    d, c, im, w2c, K = _gpu(z["depth"] if depth is None else depth, z["conf"] if conf is None else conf, z["images"], z["w2c"], z["K_in"])
    return colmap_points_from_depth(d, c, im, w2c, K, percent, out_size=out_size)


def _restate_selection(depth, conf, percent):
    """infer.py:296-324 with the library's tie rule on the CPU -> flat indices (view-major, row-major) of the kept pixels, ascending"""
    d, c = torch.from_numpy(depth).reshape(-1), torch.from_numpy(conf).reshape(-1)
    cand = torch.nonzero(d > 1e-8)[:, 0]
    if not len(cand):
        return cand.numpy()
    cc = c[cand]
    cc = torch.where(cc <= 1e-5, torch.full_like(cc, float("-inf")), cc)
    n = len(cand)
    K = max(1, int(np.ceil(n * (100.0 - percent) / 100.0))) if percent > 0 else n
    v = cc.numpy()
    nan = np.isnan(v)                                                         # torch.topk's order: a NaN of either sign is the largest value
    order = np.lexsort((np.where(nan, np.float32(0), -v), ~nan))[:K]          # NaNs, then descending; stable: equal values in candidate order
    return torch.sort(cand[torch.from_numpy(order)]).values.numpy()


def _scene(S, H, W, seed, n_valid=None):
    g = torch.Generator().manual_seed(seed)
    depth = 1.5 + 2.0 * torch.rand(S, H, W, generator=g)
    depth[torch.rand(S, H, W, generator=g) < 0.2] = 0.0
    if n_valid is not None:          # exactly n_valid candidates
        flat = depth.reshape(-1)
        flat[:] = 2.0
        flat[torch.randperm(S * H * W, generator=g)[n_valid:]] = -1.0
    conf = 1.0 + 9.0 * torch.rand(S, H, W, generator=g)
    conf[torch.rand(S, H, W, generator=g) < 0.1] = 0.0
    images = torch.rand(S, 3, H, W, generator=g) * 1.2 - 0.1          # some values outside [0, 1]: clamped
    w2c = torch.eye(4).repeat(S, 1, 1)
    for i in range(S):
        a = 0.2 * i - 0.3
        w2c[i, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float64).float()
        w2c[i, :3, 3] = torch.tensor([0.1 * i, -0.05 * i, 0.02])
    K = torch.tensor([[40.0, 0, W / 2], [0, 41.0, H / 2], [0, 0, 1]]).repeat(S, 1, 1)
    return dict(depth=depth.numpy(), conf=conf.numpy(), images=images.numpy(), w2c=w2c.numpy(), K_in=K.numpy())


def _write(tmp, z, sel, names, size, model="SIMPLE_PINHOLE", K=None, sub="m"):
    d = os.path.join(str(tmp), sub)
    (w2c, Kt) = _gpu(z["w2c"], z["K_out"] if K is None else K)
    save_colmap(d, *sel, w2c, Kt, names, size, camera_model=model)
    return d


@pytest.mark.parametrize("percent", [0.0, 30.0, 100.0])
def test_golden_parity(gold, tmp_path, percent):
    z, tag = gold, f"p{int(percent)}"
    out_size = tuple(int(v) for v in z["out_size"])
    sel = _select(z, percent, out_size)
    names = [str(n) for n in z["names"]]
    d = _write(tmp_path, z, sel, names, out_size)
    cams, imgs, pts = (CH.read_cameras(os.path.join(d, "cameras.bin")), CH.read_images(os.path.join(d, "images.bin")),
                       CH.read_points3d(os.path.join(d, "points3D.bin")))
    P = int(z[f"{tag}_K"])
    assert len(pts) == P == sel[0].shape[0]
    assert np.array_equal(sel[3].cpu().numpy(), z[f"{tag}_counts"])
    assert np.array_equal(sel[2].cpu().numpy(), z[f"{tag}_xyf"])
    assert np.array_equal(sel[1].cpu().numpy(), z[f"{tag}_colors"])
    # points3D.bin
    assert [p[0] for p in pts] == z[f"{tag}_point3D_ids"].tolist()
    assert np.array_equal(np.array([p[2] for p in pts], dtype=np.uint8).reshape(-1, 3), z[f"{tag}_colors"])
    assert all(p[3] == -1.0 and len(p[4]) == 1 for p in pts)
    assert np.array_equal(np.array([p[4][0] for p in pts], dtype=np.int64).reshape(-1, 2), z[f"{tag}_tracks"])
    xyz = np.array([p[1] for p in pts], dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(xyz, sel[0].cpu().numpy().astype(np.float64))          # widened from the returned fp32, nothing else
    err, bound = float(np.abs(xyz - z[f"{tag}_points"]).max()), MARGIN * float(z["err_points"])
    print(f"colmap golden {tag}: {P} points, max |xyz - fp64 reference| {err:.3e} (reference's own fp32 run {float(z[f'{tag}_err_points']):.3e}, bound {bound:.3e})")
    assert err <= bound
    # images.bin: every view is there, the one without points too
    assert [im[0] for im in imgs] == z["image_ids"].tolist() and [im[3] for im in imgs] == z["image_camera_ids"].tolist()
    assert [im[4] for im in imgs] == names
    p2d = np.array([[x, y, pid] for im in imgs for x, y, pid in im[5]], dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(p2d, z[f"{tag}_points2D"].astype(np.float64))
    assert [len(im[5]) for im in imgs] == z[f"{tag}_counts"].tolist()
    for i, im in enumerate(imgs):
        assert abs(np.linalg.norm(im[1]) - 1) < 1e-15
        assert np.abs(CH.quat_to_rot(im[1]) - z["image_rotations"][i]).max() < 1e-7          # the recorded rotation is fp32-valued, orthonormal to 1e-7
        assert np.array_equal(np.array(im[2]), z["image_translations"][i])
    # cameras.bin
    assert [c[0] for c in cams] == z["camera_ids"].tolist() and all(c[1] == 0 for c in cams) and set(z["camera_models"].tolist()) == {"SIMPLE_PINHOLE"}
    assert [[c[2], c[3]] for c in cams] == z["camera_sizes"].tolist()
    for c, want in zip(cams, z["camera_params"]):
        assert np.abs(np.array(c[4]) - want).max() <= 2.0 ** -23 * np.abs(want).max()          # the focal mean is taken in fp32
    got_pts, got_cols = CH.read_point_ply(os.path.join(d, "points3D.ply"))
    assert np.array_equal(got_pts, sel[0].cpu().numpy()) and np.array_equal(got_cols, z[f"{tag}_colors"])


def _check_bytes(tmp, z, sel, S, size, model):
    names = [f"frame_{i:03d}.png" for i in range(S)]
    pts, cols, xyf, counts = (t.cpu().numpy() for t in sel)
    assert int(counts.sum()) == len(pts) and counts.dtype == np.int64 and xyf.dtype == np.int32 and cols.dtype == np.uint8 and pts.dtype == np.float32
    out = []
    for sub in ("first", "second"):
        d = _write(tmp, z, sel, names, size, model, K=z["K_in"], sub=sub)
        out.append({f: open(os.path.join(d, f), "rb").read() for f in ("cameras.bin", "images.bin", "points3D.bin", "points3D.ply")})
    assert out[0] == out[1]
    quats = [colmap.rotation_to_quaternion(z["w2c"][i, :3, :3].astype(np.float64)) for i in range(S)]
    assert out[0]["points3D.bin"] == CH.points3d_bytes(pts, cols, counts)
    assert out[0]["images.bin"] == CH.images_bytes(xyf, counts, quats, z["w2c"], names)
    assert out[0]["cameras.bin"] == CH.cameras_bytes(z["K_in"], size, model)
    assert out[0]["points3D.ply"] == CH.ply_bytes(pts, cols)
    ply = os.path.join(str(tmp), "scene.ply")
    save_scene_ply(ply, sel[0], sel[1])
    assert open(ply, "rb").read() == (CH.ply_bytes(pts, cols) if len(pts) else CH.ply_bytes(np.zeros((1, 3), np.float32), np.full((1, 3), 255, np.uint8)))
    return out[0]


@pytest.mark.parametrize("case", ["P0", "P1", "P4097", "views5"])
def test_file_bytes(tmp_path, case):
    S, H, W = (5, 37, 53) if case == "views5" else (3, 37, 53)
    z = _scene(S, H, W, seed=len(case) * 7 + S, n_valid={"P0": 0, "P1": None, "P4097": 4097, "views5": None}[case])
    percent = {"P0": 30.0, "P1": 100.0, "P4097": 0.0, "views5": 30.0}[case]
    size = (71, 50)
    sel = _select(z, percent, size)
    sel2 = _select(z, percent, size)
    assert all(torch.equal(a, b) for a, b in zip(sel, sel2))
    keep = _restate_selection(z["depth"], z["conf"], percent)
    assert sel[0].shape[0] == len(keep) == {"P0": 0, "P1": 1, "P4097": 4097}.get(case, len(keep))
    view, rem = keep // (H * W), keep % (H * W)
    y, x = rem // W, rem % W
    want_xyf = np.stack([(x * (size[0] / W)).astype(np.int32), (y * (size[1] / H)).astype(np.int32), view.astype(np.int32)], 1).reshape(-1, 3)
    assert np.array_equal(sel[2].cpu().numpy(), want_xyf)
    assert np.array_equal(sel[3].cpu().numpy(), np.bincount(view, minlength=S))
    want_col = (torch.from_numpy(z["images"]).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).reshape(-1, 3).numpy()[keep]
    assert np.array_equal(sel[1].cpu().numpy(), want_col.reshape(-1, 3))
    _check_bytes(tmp_path, z, sel, S, size, "PINHOLE" if case == "views5" else "SIMPLE_PINHOLE")


def test_ties_go_to_the_lowest_index():
    """a plateau of equal confidences across the threshold, spread over blocks and views: exactly K kept, the plateau's first ones"""
    S, H, W = 3, 37, 53
    z = _scene(S, H, W, seed=3)
    conf = z["conf"].copy().reshape(-1)
    g = torch.Generator().manual_seed(9)
    plateau = torch.randperm(S * H * W, generator=g)[:2500].numpy()
    conf[plateau] = 4.0          # 42 % of the pixels; with the live values uniform in (1, 10) and 10 % dead, 4.0 spans the 23 % to 65 % quantiles: across the 30 % line
    conf = conf.reshape(S, H, W)
    keep = _restate_selection(z["depth"], conf, 30.0)
    flat_valid = z["depth"].reshape(-1) > 1e-8
    kept_plateau = np.intersect1d(keep, plateau)
    all_plateau = np.sort(plateau[flat_valid[plateau]])
    assert 0 < len(kept_plateau) < len(all_plateau) and np.array_equal(kept_plateau, all_plateau[:len(kept_plateau)])          # the scene does what it is for
    pts, cols, xyf, counts = _select(z, 30.0, (W, H), conf=conf)
    n_valid = int(flat_valid.sum())
    assert pts.shape[0] == int(np.ceil(n_valid * 70.0 / 100.0)) == len(keep)
    got = xyf.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[:, 2] * H * W + got[:, 1] * W + got[:, 0], keep)


def test_sign_bit_nan_confidence_is_kept_first():
    """torch.topk ranks a NaN of either sign above +inf.  0xFFC00000, the NaN a host's 0/0 gives, on a valid-depth pixel in the middle of
    the second view: the only point kept at K = 1, and among the kept at 30 %; a +inf elsewhere does not displace it."""
    S, H, W = 3, 37, 53
    z = _scene(S, H, W, seed=5)
    flat_valid = z["depth"].reshape(-1) > 1e-8
    at = int(np.nonzero(flat_valid)[0][np.searchsorted(np.nonzero(flat_valid)[0], H * W + 700)])
    inf_at = int(np.nonzero(flat_valid)[0][10])
    conf = z["conf"].copy().reshape(-1)
    conf[at] = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    conf[inf_at] = np.inf
    assert np.isnan(conf[at]) and np.signbit(conf[at]) and flat_valid[at] and inf_at < at
    conf = conf.reshape(S, H, W)
    n_valid = int(flat_valid.sum())
    for percent in (99.99, 30.0):
        keep = _restate_selection(z["depth"], conf, percent)
        K = max(1, int(np.ceil(n_valid * (100.0 - percent) / 100.0)))
        assert len(keep) == K and at in keep
        pts, cols, xyf, counts = _select(z, percent, (W, H), conf=conf)
        got = xyf.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:, 2] * H * W + got[:, 1] * W + got[:, 0], keep), percent
    assert K > 1 and len(_restate_selection(z["depth"], conf, 99.99)) == 1          # the first percent kept the NaN alone, past the +inf


def test_save_scene_ply_filters(tmp_path):
    g = torch.Generator().manual_seed(4)
    N = 1000
    pts = torch.randn(N, 3, generator=g)
    pts[5, 1], pts[300, 0], pts[999, 2], pts[256, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
    cols = torch.randint(0, 256, (N, 3), generator=g, dtype=torch.uint8)
    path = os.path.join(str(tmp_path), "s.ply")
    save_scene_ply(path, pts.to(DEV), cols.to(DEV))
    fin = torch.isfinite(pts).all(1).numpy()
    assert int(fin.sum()) == N - 4
    assert open(path, "rb").read() == CH.ply_bytes(pts.numpy()[fin], cols.numpy()[fin])
    mask = torch.rand(N, generator=g) < 0.4
    save_scene_ply(path, pts.reshape(10, 100, 3).to(DEV), cols.reshape(10, 100, 3).to(DEV), mask.reshape(10, 100).to(DEV))
    assert open(path, "rb").read() == CH.ply_bytes(pts.numpy()[mask.numpy()], cols.numpy()[mask.numpy()])          # the mask alone decides: NaN rows stay
    white = CH.ply_bytes(np.zeros((1, 3), np.float32), np.full((1, 3), 255, np.uint8))
    save_scene_ply(path, pts.to(DEV), cols.to(DEV), torch.zeros(N, dtype=torch.bool, device=DEV))
    assert open(path, "rb").read() == white
    save_scene_ply(path, torch.full((3, 3), float("nan"), device=DEV), torch.zeros(3, 3, dtype=torch.uint8, device=DEV))
    assert open(path, "rb").read() == white
    save_points_ply(path, pts.to(DEV), cols.to(DEV))
    assert open(path, "rb").read() == CH.ply_bytes(pts.numpy(), cols.numpy())
    with pytest.raises(ValueError):
        save_scene_ply(path, pts.to(DEV), cols.to(DEV), mask[:10].to(DEV))


def test_round_trip_to_the_source_pixels(gold, tmp_path):
    """save_colmap -> load_colmap -> project_depth_points: every kept point is valid in its own view alone, lands on its source pixel and has
    the input depth there.  Pixel row 0 and column 0 hold no candidate here: such a point reprojects to 0 +- rounding, and which side of
    the image bound it falls on is not decided in fp32 (tools/gen_golden_colmap.py makes the same exception for the reference's chain)."""
    z = gold
    S, H, W = z["depth"].shape
    depth = z["depth"].copy()
    depth[:, 0, :] = 0.0
    depth[:, :, 0] = 0.0
    pts, cols, xyf, counts = _select(z, 30.0, (W, H), depth=depth)
    names = [str(n) for n in z["names"]]
    (w2c, K) = _gpu(z["w2c"], z["K_in"])
    d = os.path.join(str(tmp_path), "data", "sparse", "0")
    save_colmap(d, pts, cols, xyf, counts, w2c, K, names, (W, H), camera_model="PINHOLE")
    m = load_colmap(os.path.join(str(tmp_path), "data"))
    assert m.image_names == sorted(names) and int(m.points.shape[0]) == pts.shape[0] > 1000
    assert np.array_equal(m.points, pts.cpu().numpy()) and np.array_equal(m.points_rgb, cols.cpu().numpy())
    view_of_row = [names.index(n) for n in m.image_names]          # row of the sorted model -> view of the scene
    t = m.to(DEV)
    Ks = torch.stack([t.Ks_dict[c] for c in t.camera_ids])
    assert torch.equal(Ks.cpu(), torch.from_numpy(z["K_in"])[view_of_row])
    pix, dep, valid = project_depth_points(t.points, t.camtoworlds, Ks, W, H, visible=m.visible(DEV))
    src = xyf.cpu().numpy().astype(np.int64)
    want_valid = np.stack([src[:, 2] == v for v in view_of_row])
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    rows = np.array([view_of_row.index(v) for v in src[:, 2]])
    cols_ = np.arange(len(src))
    got_px = pix.cpu().numpy().astype(np.float64)[rows, cols_]
    got_z = dep.cpu().numpy().astype(np.float64)[rows, cols_]
    want_z = depth[src[:, 2], src[:, 1], src[:, 0]].astype(np.float64)
    e_px, e_z = float(np.abs(got_px - src[:, :2]).max()), float(np.abs(got_z - want_z).max())
    b_px, b_z = MARGIN * float(z["err_reproj_px"]), MARGIN * float(z["err_reproj_depth"])
    print(f"colmap round trip: {len(src)} points, pixel error {e_px:.3e} (bound {b_px:.3e}), depth error {e_z:.3e} (bound {b_z:.3e})")
    assert e_px <= b_px and e_z <= b_z
