"""CPU: hunyuanworld_mirror_amd.load_colmap (host numpy) on COLMAP models written by tests/colmap_helper.py from the published format,
every Parser field against the helper's restatement of the Parser's lines (datasets/colmap.py:83-160, 201-215, 262-273, 344-348).

The model: 4 images out of sorted name order with ids that are neither dense nor ordered, two of them sharing a PINHOLE camera, one on a
SIMPLE_PINHOLE camera; a camera no image uses; 7 points with tracks of lengths 0 to 3 mixed (one names the same image twice), ids out of
order; 2-D points whose point3D id is the invalid id (all ones)."""
import os

import numpy as np
import pytest
import torch

import colmap_helper as CH
from hunyuanworld_mirror_amd import colmap, load_colmap


def _rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return np.array({0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax])


def _model():
    rng = np.random.default_rng(5)
    cameras = [(7, 1, 640, 480, [500.5, 498.25, 321.0, 239.5]), (2, 0, 800, 600, [610.0, 400.5, 299.0]), (9, 1, 100, 100, [90.0, 91.0, 50.0, 50.0])]
    images = []
    for iid, cid, name in ((12, 7, "c/img_10.png"), (3, 2, "a_first.jpg"), (40, 7, "c/img_02.png"), (5, 2, "b.png")):
        R = _rot(0, rng.uniform(-1, 1)) @ _rot(1, rng.uniform(-1, 1)) @ _rot(2, rng.uniform(-3, 3))
        q = colmap.rotation_to_quaternion(R) * (1 if iid % 2 else -1)
        pts2d = [(float(rng.uniform(0, 600)), float(rng.uniform(0, 400)), CH.INVALID_ID if j % 3 == 0 else j + 1) for j in range(iid % 5)]
        images.append((iid, q.tolist(), rng.uniform(-2, 2, 3).tolist(), cid, name, pts2d))
    tracks = [[(12, 0)], [], [(3, 1), (40, 0), (12, 1)], [(5, 0), (5, 2)], [(40, 3), (3, 0)], [], [(12, 2), (5, 1), (3, 3)]]
    points = [(pid, rng.normal(size=3).tolist(), rng.integers(0, 256, 3).tolist(), float(rng.uniform(0, 2)) if t else -1.0, t)
              for pid, t in zip((11, 2, 30, 4, 5, 60, 7), tracks)]
    return cameras, images, points


def _write(d, cameras, images, points, sub="sparse/0"):
    m = os.path.join(d, sub)
    os.makedirs(m, exist_ok=True)
    CH.write_cameras(os.path.join(m, "cameras.bin"), cameras)
    CH.write_images(os.path.join(m, "images.bin"), images)
    CH.write_points3d(os.path.join(m, "points3D.bin"), points)
    return m


def _check(got, want):
    assert got.image_names == want["image_names"] and got.image_names == sorted(got.image_names)
    assert got.camera_ids == want["camera_ids"]
    assert got.camtoworlds.dtype == np.float64 and np.array_equal(got.camtoworlds, want["camtoworlds"])
    assert set(got.Ks_dict) == set(want["Ks_dict"]) == set(got.imsize_dict) == set(got.params_dict)
    for c in want["Ks_dict"]:
        assert np.array_equal(got.Ks_dict[c], want["Ks_dict"][c]), c
        assert tuple(got.imsize_dict[c]) == tuple(want["imsize_dict"][c]), c
        assert len(got.params_dict[c]) == 0
    for k, dt in (("points", np.float32), ("points_err", np.float32), ("points_rgb", np.uint8)):
        assert getattr(got, k).dtype == dt and np.array_equal(getattr(got, k), want[k]), k
    assert set(got.point_indices) == set(want["point_indices"])
    for n in want["point_indices"]:
        assert got.point_indices[n].dtype == np.int32 and np.array_equal(got.point_indices[n], want["point_indices"][n]), n
    assert got.scene_scale == float(want["scene_scale"])
    assert np.array_equal(got.transform, np.eye(4))
    assert np.array_equal(got.Ks, np.stack([want["Ks_dict"][c] for c in want["camera_ids"]]))


@pytest.mark.parametrize("factor,size", [(1, None), (2, None), (1, (320, 250)), (4, (161, 119))])
def test_parser_fields_general_model(tmp_path, factor, size):
    cameras, images, points = _model()
    _write(str(tmp_path), cameras, images, points)
    got = load_colmap(str(tmp_path), factor=factor, image_size=size)
    _check(got, CH.parser_fields(cameras, images, points, factor, size))
    assert 9 not in got.Ks_dict                                # the camera without an image, as in the Parser
    assert got.point_indices["b.png"].tolist() == [3, 3, 6]    # the track that names an image twice; file order of the points
    vis = got.visible()
    assert vis.dtype == torch.bool and tuple(vis.shape) == (4, 7)
    for i, n in enumerate(got.image_names):
        want = np.zeros(7, bool)
        want[got.point_indices[n]] = True
        assert np.array_equal(vis[i].numpy(), want)


def test_model_directory_forms(tmp_path):
    cameras, images, points = _model()
    want = CH.parser_fields(cameras, images, points)
    for sub in ("sparse/0", "sparse", "."):
        d = tmp_path / sub.replace("/", "_").replace(".", "flat")
        m = _write(str(d), cameras, images, points, sub)
        _check(load_colmap(str(d)), want)
        _check(load_colmap(m), want)


def test_fixed_stride_and_walk_agree(tmp_path):
    """every track of length 2: the strided read applies; the sequential walk gives the same"""
    cameras, images, points = _model()
    ids = [im[0] for im in images]
    points = [(p[0], p[1], p[2], 0.5 + j, [(ids[j % 4], j), (ids[(j + 1) % 4], j)]) for j, p in enumerate(points)]
    m = _write(str(tmp_path), cameras, images, points)
    data = open(os.path.join(m, "points3D.bin"), "rb").read()
    assert colmap._points3d_fixed(data) is not None
    a, b = load_colmap(str(tmp_path)), load_colmap(str(tmp_path), _force_walk=True)
    want = CH.parser_fields(cameras, images, points)
    _check(a, want)
    _check(b, want)
    # a mixed file of a size that a constant record length also explains: the track-length column decides
    mixed = [(p[0], p[1], p[2], p[3], [(ids[0], 0)] * (3 if j == 0 else 1 if j == 1 else 2)) for j, p in enumerate(points)]
    m2 = _write(str(tmp_path / "mixed"), cameras, images, mixed)
    data = open(os.path.join(m2, "points3D.bin"), "rb").read()
    assert (len(data) - 8) % len(mixed) == 0 and colmap._points3d_fixed(data) is None
    _check(load_colmap(str(tmp_path / "mixed")), CH.parser_fields(cameras, images, mixed))


def test_empty_points_and_to(tmp_path):
    cameras, images, _ = _model()
    _write(str(tmp_path), cameras, images, [])
    got = load_colmap(str(tmp_path))
    assert got.points.shape == (0, 3) and got.points_rgb.shape == (0, 3) and got.point_indices == {}
    assert tuple(got.visible().shape) == (4, 0)
    t = got.to("cpu")
    assert isinstance(t.camtoworlds, torch.Tensor) and t.camtoworlds.dtype == torch.float32 and t.points.dtype == torch.float32
    assert tuple(t.Ks.shape) == (4, 3, 3) and t.Ks.dtype == torch.float32
    assert t.image_names == got.image_names
    t2 = load_colmap(str(tmp_path), device="cpu")
    assert torch.equal(t2.camtoworlds, t.camtoworlds)


def test_not_built_raises(tmp_path):
    cameras, images, points = _model()
    m = _write(str(tmp_path / "ok"), cameras, images, points)
    with pytest.raises(NotImplementedError, match="normalize"):
        load_colmap(str(tmp_path / "ok"), normalize=True)
    for extra in ("rigs.bin", "frames.bin"):
        open(os.path.join(m, extra), "wb").close()
        with pytest.raises(NotImplementedError, match=extra):
            load_colmap(str(tmp_path / "ok"))
        os.remove(os.path.join(m, extra))
    distorted = [(7, 2, 640, 480, [500.0, 320.0, 240.0, 0.01])] + cameras[1:]
    _write(str(tmp_path / "radial"), distorted, images, points)
    with pytest.raises(NotImplementedError, match="SIMPLE_RADIAL"):
        load_colmap(str(tmp_path / "radial"))
    fisheye = [(7, 5, 640, 480, [500.0, 500.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0])] + cameras[1:]
    _write(str(tmp_path / "fisheye"), fisheye, images, points)
    with pytest.raises(NotImplementedError, match="OPENCV_FISHEYE"):
        load_colmap(str(tmp_path / "fisheye"))


def test_argument_errors(tmp_path):
    cameras, images, points = _model()
    _write(str(tmp_path), cameras, images, points)
    for bad in ((320,), (320, 0), "ab", 5):
        with pytest.raises(ValueError):
            load_colmap(str(tmp_path), image_size=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            load_colmap(str(tmp_path), factor=bad)
    with pytest.raises(FileNotFoundError):
        load_colmap(str(tmp_path / "nothing_here"))
    bad_track = points[:1] + [(99, [0, 0, 0], [1, 2, 3], 0.0, [(1234, 0)])]
    _write(str(tmp_path / "bad"), cameras, images, bad_track)
    with pytest.raises(ValueError, match="1234"):
        load_colmap(str(tmp_path / "bad"))
    with pytest.raises(ValueError):
        colmap.camera_params(np.eye(3), "OPENCV")
    # the writer's shape checks come before any device work
    z = torch.zeros
    with pytest.raises(ValueError, match="camera model"):
        colmap.save_colmap(str(tmp_path / "o"), z(2, 3), z(2, 3, dtype=torch.uint8), z(2, 3, dtype=torch.int32), torch.tensor([2]), z(1, 3, 4), z(1, 3, 3),
                           ["a"], (4, 4), camera_model="SIMPLE_RADIAL")
    with pytest.raises(ValueError, match=r"\[P, 3\]"):
        colmap.save_colmap(str(tmp_path / "o"), z(2, 3), z(3, 3, dtype=torch.uint8), z(2, 3, dtype=torch.int32), torch.tensor([2]), z(1, 3, 4), z(1, 3, 3),
                           ["a"], (4, 4))
    with pytest.raises(ValueError, match="image_names"):
        colmap.save_colmap(str(tmp_path / "o"), z(2, 3), z(2, 3, dtype=torch.uint8), z(2, 3, dtype=torch.int32), torch.tensor([2]), z(1, 3, 4), z(1, 3, 3),
                           ["a", "b"], (4, 4))
    with pytest.raises(ValueError, match="depth_conf"):
        colmap.colmap_points_from_depth(z(2, 4, 5), z(2, 5, 4), z(2, 3, 4, 5), z(2, 3, 4), z(2, 3, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        colmap.colmap_points_from_depth(z(2, 4, 5), z(2, 4, 5), z(2, 3, 4, 5), z(2, 3, 4), z(2, 3, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        colmap.save_points_ply(str(tmp_path / "p.ply"), z(2, 3), z(2, 3, dtype=torch.uint8))


def test_quaternion_host_code():
    rng = np.random.default_rng(1)
    for k in range(40):
        R = _rot(0, rng.uniform(-3.2, 3.2)) @ _rot(1, rng.uniform(-3.2, 3.2)) @ _rot(2, rng.uniform(-3.2, 3.2))
        if k < 4:      # the four pivots: rotations by pi about an axis and the identity
            R = [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])][k]
        q = colmap.rotation_to_quaternion(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-15
        assert np.abs(colmap.quaternion_to_rotation(q) - R).max() < 1e-14
        assert np.abs(CH.quat_to_rot(q) - R).max() < 1e-14


def test_header_and_library_sizes():
    """the size calls need no device: they refuse what the kernels cannot index"""
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    assert L.wm_colmap_select_workspace_bytes(32, 518, 518) > 0
    assert L.wm_colmap_select_workspace_bytes(8192, 518, 518) == 0      # 2.2e9 pixels
    assert L.wm_colmap_select_workspace_bytes(0, 4, 4) == 0
    assert L.wm_colmap_pack_workspace_bytes(2 ** 31, 3) == 0 and L.wm_colmap_pack_workspace_bytes(10, 0) == 0
    assert L.wm_colmap_pack_workspace_bytes(0, 1) > 0
    assert L.wm_pack_point_ply_workspace_bytes(2 ** 31) == 0 and L.wm_pack_point_ply_workspace_bytes(-1) == 0
    assert L.wm_pack_point_ply_workspace_bytes(0) > 0
    assert colmap.point_ply_header(3) == CH.ply_bytes(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8))[:-45]
