"""GPU: hunyuanworld_mirror_amd.glb (csrc/glb.hip) against what the reference's create_image_mesh and convert_predictions_to_glb_scene
produced on the CPU (tests/golden/glb_*.npz, written by tools/gen_golden_glb.py with a recording stand-in for trimesh) and, at sizes
without a fixture, against the numpy restatement tests/glb_helper.py, which tests/test_glb_cpu.py pins to the same recordings.

Bounds.  Counts, vertex order, faces and colour bytes are exact; vertices and normals are bit copies.  Every geometry is compared as arrays
with the helper's and as a digest with the reference's record.  The scale: |scale - reference| <= 16 * 2^-24 * max |percentile coordinate|
(each percentile is one interpolation, two fp32 roundings in either implementation; the norm adds three more).  Measured on MI355X: at most 3.4e-06, 0.39 of
its bound (profiles/r20_glb_scene.md).  Camera solids are host fp64 work on that scale: they move by at most 0.12 |scale - reference| (the solid
reaches 0.1 scale along the axis and 0.05 scale across), plus the reference's own fp32 products for radius and height.

Seams of the kernels: a block owns 512 pixels of one view (two rounds of 256, four waves each) and one block scans all block counts with
256 lanes.  37 x 52 and 61 x 83 are 4 and 10 blocks per view with a partial last one; 300 x 300 (176 blocks) and 518 x 518 (525 blocks, more
than 256: every scanning lane owns several) cross the block and scan-level boundaries; 2 x 2 and 1 x 9 are a single partial wave."""
import io
import os

import numpy as np
import pytest
import torch

import glb_helper as GH
from conftest import GOLD
from hunyuanworld_mirror_amd import convert_predictions_to_glb_scene, glb, image_mesh, load_glb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return {n: dict(np.load(os.path.join(GOLD, f"glb_{n}.npz"), allow_pickle=False)) for n in ("mesh", "scene")}


_INPUTS = {}


def inputs(g):
    """the group's predictions, drawn once and never modified: (numpy dict, the same on the device)"""
    if g not in _INPUTS:
        p = GH.make_inputs(g)
        _INPUTS[g] = (p, {k: torch.from_numpy(v).to(DEV) for k, v in p.items()})
    return _INPUTS[g]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_mesh(got: "glb.ImageMesh", pts, img, masks, normals=None):
    """every view of an ImageMesh against the helper: counts, order, faces, bit-equal vertices / normals, equal colour bytes, bounds"""
    S = pts.shape[0]
    assert len(got.vertex_counts) == len(got.face_counts) == S
    assert got.vertices.dtype == torch.float32 and got.colors.dtype == torch.uint8 and got.faces.dtype == torch.int32
    bounds = _np(got.bounds)
    for i in range(S):
        faces, idx = GH.image_mesh_ref(masks[i])
        v, c, n, f = got.view(i)
        assert (got.vertex_counts[i], got.face_counts[i]) == (len(idx), len(faces)), i
        assert np.array_equal(_np(f), faces)
        assert np.array_equal(_bits(_np(v)), _bits(pts[i].reshape(-1, 3)[idx]))
        assert np.array_equal(_np(c)[:, :3], GH.mesh_color_bytes(img[i]).reshape(-1, 3)[idx]) and (_np(c)[:, 3] == 255).all()
        if normals is not None:
            assert np.array_equal(_bits(_np(n)), _bits(normals[i].reshape(-1, 3)[idx]))
        else:
            assert n is None
        if len(idx):
            vv = pts[i].reshape(-1, 3)[idx]
            assert np.array_equal(bounds[i], np.concatenate([vv.min(0), vv.max(0)]))
    assert int(got.vertices.shape[0]) == sum(got.vertex_counts) and int(got.faces.shape[0]) == sum(got.face_counts)


# ------------------------------------------------------------------------------------------------ image_mesh
@pytest.mark.parametrize("g", list(GH.GROUPS))
def test_image_mesh_equals_reference(gold, g):
    """final_mask of every view of the group: the recorded faces and vertex indices of create_image_mesh, as integers"""
    p, d = inputs(g)
    got = image_mesh(d["world_points"], d["images"], d["final_mask"], d["normal"])
    z = gold["mesh"]
    for i in range(GH.GROUPS[g][0]):
        v, c, n, f = got.view(i)
        faces, idx = z[f"{g}_v{i}_faces"], z[f"{g}_v{i}_idx"]
        assert got.vertex_counts[i] == len(idx) and got.face_counts[i] == len(faces)
        assert np.array_equal(_np(f), faces) and _np(f).dtype == np.int32
        assert np.array_equal(_bits(_np(v)), _bits(p["world_points"][i].reshape(-1, 3)[idx]))
    _check_mesh(got, p["world_points"], p["images"], p["final_mask"], p["normal"])


def test_image_mesh_without_mask_and_other_masks():
    p, d = inputs("a")
    got = image_mesh(d["world_points"], d["images"])
    _check_mesh(got, p["world_points"], p["images"], np.ones(p["final_mask"].shape, bool))
    assert got.vertex_counts == [37 * 52] * 3 and got.face_counts == [2 * 36 * 51] * 3
    both = p["final_mask"] & p["sky_mask"]
    _check_mesh(image_mesh(d["world_points"], d["images"], d["final_mask"] & d["sky_mask"]), p["world_points"], p["images"], both)
    _check_mesh(image_mesh(d["world_points"], d["images"], d["sky_mask"]), p["world_points"], p["images"], p["sky_mask"])


@pytest.mark.parametrize("hw", [300, 518])
def test_image_mesh_large_view(hw):
    """one view of 300 x 300 and one of 518 x 518 against the helper: many blocks, and at 518 more blocks than scanning lanes"""
    rng = np.random.default_rng(hw)
    pts = rng.standard_normal((1, hw, hw, 3)).astype(np.float32)
    img = rng.random((1, hw, hw, 3), dtype=np.float32)
    mask = rng.random((1, hw, hw)) < 0.8
    mask[0, -2:, -2:] = True      # a valid quad in the last row and column
    got = image_mesh(torch.from_numpy(pts).to(DEV), torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV))
    _check_mesh(got, pts, img, mask)
    assert got.face_counts[0] >= 2 * 0.25 * (hw - 1) ** 2


def test_mesh_color_chain_on_every_byte_value():
    """the three fp32 roundings on all k / 255, their fp32 neighbours, and values around 1: equal bytes with numpy's chain"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)), np.linspace(0, 1, 4096, dtype=np.float32)])
    vals = np.clip(vals, 0, 1).astype(np.float32)
    n = len(vals) // 3 * 3
    img = vals[:n].reshape(1, 1, n // 3, 3)
    img = np.concatenate([img, img], 1)      # two rows: every pixel is a vertex
    pts = np.zeros_like(img)
    got = image_mesh(torch.from_numpy(pts).to(DEV), torch.from_numpy(img).to(DEV))
    assert np.array_equal(_np(got.colors)[:, :3], GH.mesh_color_bytes(img).reshape(-1, 3))
    _, c, _, _ = glb.pack_points(torch.from_numpy(pts).to(DEV), torch.from_numpy(img).to(DEV))
    assert np.array_equal(_np(c)[:, :3], GH.point_color_bytes(img).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ the scene
def _scale_bound(pct):
    return 16 * 2.0 ** -24 * float(np.abs(pct).max())


@pytest.mark.parametrize("g", list(GH.GROUPS))
def test_scene_every_flag_combination(gold, g):
    """as_mesh x mask_ambiguous x mask_sky_bg x frames all / one, and one frame with normals: the order of the geometries, their arrays, the
    scale, the cameras and the transform against the reference's record; covers the empty case (group c with mask_sky_bg: one white point,
    scale 1) and the views without a valid quad, which are left out."""
    p, d = inputs(g)
    z = gold["scene"]
    for combo in GH.combos(g):
        frames, as_mesh, amb, sky, with_normals = combo
        key = GH.combo_key(g, combo)
        pred = {k: v for k, v in d.items() if with_normals or k != "normal"}
        scene = convert_predictions_to_glb_scene(pred, filter_by_frames=frames, show_camera=True, mask_sky_bg=sky, mask_ambiguous=amb,
                                                 as_mesh=as_mesh)
        rec = [(str(k), int(c[0]), str(dg)) for k, c, dg in zip(z[f"{key}_kinds"], z[f"{key}_counts"], z[f"{key}_digests"])]
        rec = [r for r in rec if r[0] == "camera" or r[1] > 0]      # the reference's zero-vertex meshes are left out
        assert [geo.kind for geo in scene.geometry] == [r[0] for r in rec], key
        exp, kept = GH.expected_geometry(p, *combo)
        body = [geo for geo in scene.geometry if geo.kind != "camera"]
        assert len(body) == len(exp)
        for geo, e, r in zip(body, exp, [r for r in rec if r[0] != "camera"]):
            assert geo.kind == e["kind"] and geo.frame == e["frame"]
            v, c = _np(geo.vertices), _np(geo.colors)
            f = None if geo.faces is None else _np(geo.faces)
            n = None if geo.normals is None else _np(geo.normals)
            assert np.array_equal(_bits(v), _bits(e["vertices"])), key
            assert np.array_equal(c[:, :3], e["colors"]) and (c[:, 3] == 255).all(), key
            assert (f is None) == (e["faces"] is None) and (f is None or np.array_equal(f, e["faces"])), key
            assert (n is None) == (e["normals"] is None) and (n is None or np.array_equal(_bits(n), _bits(e["normals"]))), key
            assert GH.geometry_digest(v, f, c[:, :3], n) == r[2], key
        ref_scale, pct = float(z[f"{key}_scale"]), z[f"{key}_pct"]
        if len(kept) == 0:
            assert scene.scale == 1.0 == ref_scale
            bound = 0.0
        else:
            bound = _scale_bound(pct)
            print(f"{key}: |scale - reference| = {abs(scene.scale - ref_scale):.3e}, bound {bound:.3e}")
            assert abs(scene.scale - ref_scale) <= bound, (key, scene.scale, ref_scale)
        cams = [geo for geo in scene.geometry if geo.kind == "camera"]
        q, t = GH.select(p, frames)
        assert len(cams) == len(z[f"{key}_cam_v"]) == q["camera_poses"].shape[0]
        for i, (cam, rv, rf, rc) in enumerate(zip(cams, z[f"{key}_cam_v"], z[f"{key}_cam_f"], z[f"{key}_cam_c"])):
            tol = 0.12 * bound + 4 * 2.0 ** -24 * 0.12 * ref_scale + 1e-12 * (np.abs(q["camera_poses"][i][:3, 3]).max() + ref_scale)
            assert np.abs(_np(cam.vertices) - rv).max() <= tol, key
            assert np.array_equal(_np(cam.faces), rf)
            assert (_np(cam.colors)[:, :3] == rc).all() and (_np(cam.colors)[:, 3] == 255).all()
        assert scene.transform.dtype == np.float64 and scene.transform.shape == (4, 4)
        assert np.abs(scene.transform - z[f"{key}_transform"]).max() <= 1e-12 * max(1.0, np.abs(z[f"{key}_transform"]).max()), key


def test_scene_inputs_numpy_nchw_and_3x4_poses():
    """numpy predictions, channel-first images and [S,3,4] poses give the same scene; without show_camera there are no cameras; the masks
    are read only where the reference reads them"""
    p, d = inputs("b")
    ref = convert_predictions_to_glb_scene(d, "all", True, False, True, True)
    alt = {"world_points": p["world_points"], "images": np.ascontiguousarray(p["images"].transpose(0, 3, 1, 2)),
           "camera_poses": p["camera_poses"][:, :3], "final_mask": p["final_mask"]}
    got = convert_predictions_to_glb_scene(alt, "All", False, False, True, True)
    assert [g_.kind for g_ in got.geometry] == ["mesh", "mesh"] and [g_.kind for g_ in ref.geometry] == ["mesh", "mesh", "camera", "camera"]
    for a, b in zip(got.geometry, ref.geometry):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.colors, b.colors) and torch.equal(a.faces, b.faces)
    assert np.array_equal(got.transform, ref.transform) and got.scale == ref.scale
    with pytest.raises(KeyError):
        convert_predictions_to_glb_scene(alt, "all", False, True, False, True)      # mask_sky_bg reads sky_mask
    with pytest.raises(ValueError):
        convert_predictions_to_glb_scene({"images": p["images"]})


def test_caller_images_are_not_modified():
    """the reference scales predictions["images"] by 255 in place on every mesh call; the library does not"""
    p, d = inputs("a")
    pred = dict(d)
    pred["images"] = d["images"].clone()
    as_numpy = {k: v.copy() for k, v in p.items()}
    for frames in ("all", GH.frame_selector("a")):
        convert_predictions_to_glb_scene(pred, frames, True, True, True, True)
        convert_predictions_to_glb_scene(as_numpy, frames, True, True, True, True)
    assert torch.equal(pred["images"], d["images"]) and np.array_equal(as_numpy["images"], p["images"])
    assert np.array_equal(_np(d["images"]), p["images"])


# ------------------------------------------------------------------------------------------------ percentiles
@pytest.mark.parametrize("n_rows,keep", [(1, 1.0), (2, 1.0), (21, 1.0), (1000, 0.5), (70001, 0.8), (300000, 0.3)])
def test_percentile_neighbours_equal_partition(n_rows, keep):
    """the two order statistics around each percentile against np.partition's picks on the same rows: exact; signs, ties, denormals and
    several histogram blocks included"""
    rng = np.random.default_rng(n_rows)
    pts = (rng.standard_normal((n_rows, 3)) * np.array([1e-3, 1.0, 1e4])).astype(np.float32)
    pts[::7, 0] = pts[0, 0]                      # ties
    pts[::11, 1] = np.float32(1e-42)            # denormals
    pts[::13, 2] = 0.0
    mask = rng.random(n_rows) < keep
    mask[0] = True
    qs = (0.05, 0.95)
    got, n = glb.percentile_neighbours(torch.from_numpy(pts).to(DEV), torch.from_numpy(mask).to(DEV), qs)
    kept = pts[mask]
    assert n == len(kept)
    for c in range(3):
        for j, q in enumerate(qs):
            k0 = int(np.floor((n - 1) * q))
            k1 = min(k0 + 1, n - 1)
            part = np.partition(kept[:, c], (k0, k1))
            assert got[c, j, 0] == part[k0] and got[c, j, 1] == part[k1], (c, j)
    scale, n2 = glb.percentile_scale(torch.from_numpy(pts).to(DEV), torch.from_numpy(mask).to(DEV))
    ref, pct = GH.reference_scale(kept)
    assert n2 == n and abs(scale - ref) <= _scale_bound(pct), (scale, ref)
    got_all, n_all = glb.percentile_neighbours(torch.from_numpy(pts).to(DEV), None, (0.5,))
    assert n_all == n_rows and got_all[1, 0, 0] == np.partition(pts[:, 1], (n_rows - 1) // 2)[(n_rows - 1) // 2]


def test_percentile_of_nothing():
    pts = torch.zeros((5, 3), device=DEV)
    got, n = glb.percentile_neighbours(pts, torch.zeros(5, dtype=torch.bool, device=DEV), (0.05, 0.95))
    assert n == 0 and np.isnan(got).all()
    assert glb.percentile_scale(pts, torch.zeros(5, dtype=torch.bool, device=DEV)) == (1.0, 0)


# ------------------------------------------------------------------------------------------------ the file
@pytest.mark.parametrize("as_mesh", [True, False])
def test_export_and_load_round_trip(tmp_path, as_mesh):
    """export to a path, to a file object and to bytes give the same file; load_glb returns the scene's arrays and the node matrix"""
    p, d = inputs("a")
    frames = GH.frame_selector("a") if as_mesh else "all"
    scene = convert_predictions_to_glb_scene(d, frames, True, True, as_mesh, as_mesh)
    path = str(tmp_path / "scene.glb")
    scene.export(file_obj=path)
    data = scene.export()
    buf = io.BytesIO()
    scene.export(file_obj=buf)
    assert isinstance(data, bytes) and open(path, "rb").read() == data == buf.getvalue()
    back = load_glb(path)
    assert np.array_equal(back["nodes"][0]["matrix"], scene.transform)
    assert back["nodes"][0]["children"] == list(range(1, len(scene.geometry) + 1))
    assert len(back["primitives"]) == len(scene.geometry) and back["json"]["asset"]["version"] == "2.0"
    for pr, geo in zip(back["primitives"], scene.geometry):
        assert pr["mode"] == (0 if geo.kind == "points" else 4)
        assert np.array_equal(pr["positions"], _np(geo.vertices).astype(np.float32))
        assert np.array_equal(pr["colors"], _np(geo.colors))
        assert (pr["indices"] is None) == (geo.faces is None) and (pr["normals"] is None) == (geo.normals is None)
        if geo.faces is not None:
            assert np.array_equal(pr["indices"], _np(geo.faces))
        if geo.normals is not None:
            assert np.array_equal(_bits(pr["normals"]), _bits(_np(geo.normals)))
    doc = back["json"]
    for m in doc["meshes"]:
        acc = doc["accessors"][m["primitives"][0]["attributes"]["POSITION"]]
        view = doc["bufferViews"][acc["bufferView"]]
        assert acc["count"] > 0 and view["byteOffset"] % 4 == 0 and len(acc["min"]) == len(acc["max"]) == 3
    for pr in back["primitives"]:
        acc = doc["accessors"][doc["meshes"][pr["node"] - 1]["primitives"][0]["attributes"]["POSITION"]]
        assert np.array_equal(np.array(acc["min"], np.float32), pr["positions"].min(0))
        assert np.array_equal(np.array(acc["max"], np.float32), pr["positions"].max(0))
    assert any(geo.normals is not None for geo in scene.geometry) == as_mesh
