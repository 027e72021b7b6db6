"""CPU: the host half of the GLB hand-off (hunyuanworld-mirror_amd/glb.py) and the fixtures behind tests/test_glb_gpu.py: the container
writer and reader, the gist_rainbow table, the camera solid, the frame selector, camera_params.json, and the numpy restatement of the mesh
rule (tests/glb_helper.py) against what the reference produced (tests/golden/glb_*.npz, tools/gen_golden_glb.py)."""
import io
import json
import os
import struct

import numpy as np
import pytest

import glb_helper as GH
from conftest import GOLD


@pytest.fixture(scope="module")
def glb():
    from hunyuanworld_mirror_amd import glb
    return glb


@pytest.fixture(scope="module")
def gold():
    return {n: dict(np.load(os.path.join(GOLD, f"glb_{n}.npz"), allow_pickle=False)) for n in ("mesh", "scene", "colors")}


@pytest.mark.parametrize("g", list(GH.GROUPS))
def test_fixture_inputs_match_their_digest(gold, g):
    p = GH.make_inputs(g)
    assert tuple(gold["mesh"][f"{g}_shape"]) == GH.GROUPS[g] == p["world_points"].shape[:3]
    assert GH.inputs_digest(p) == str(gold["mesh"][f"{g}_digest"]) == str(gold["scene"][f"{g}_digest"])


@pytest.mark.parametrize("g", list(GH.GROUPS))
def test_helper_mesh_rule_equals_reference(gold, g):
    """image_mesh_ref against create_image_mesh's recorded faces and vertex indices; no case is vacuous"""
    p = GH.make_inputs(g)
    for i in range(GH.GROUPS[g][0]):
        faces, idx = GH.image_mesh_ref(p["final_mask"][i])
        assert np.array_equal(faces, gold["mesh"][f"{g}_v{i}_faces"]) and faces.dtype == np.int32
        assert np.array_equal(idx, gold["mesh"][f"{g}_v{i}_idx"])
    for gg, i, which in GH.RANDOM_VIEWS:
        if gg == g:
            m = p[which][i]
            faces, idx = GH.image_mesh_ref(m)
            assert len(faces) / 2 >= 0.25 * (m.shape[0] - 1) * (m.shape[1] - 1) and m.sum() > len(idx)


@pytest.mark.parametrize("g", list(GH.GROUPS))
def test_helper_scene_geometry_equals_reference(gold, g):
    """expected_geometry against the digests of what the reference handed to trimesh, in order, for every flag combination; the
    reference's zero-vertex meshes are the views the library leaves out"""
    p, z = GH.make_inputs(g), gold["scene"]
    for combo in GH.combos(g):
        key = GH.combo_key(g, combo)
        exp, kept = GH.expected_geometry(p, *combo)
        rec = [(str(k), int(c[0]), int(c[1]), str(d)) for k, c, d in zip(z[f"{key}_kinds"], z[f"{key}_counts"], z[f"{key}_digests"])]
        body = [r for r in rec if r[0] != "camera" and r[1] > 0]
        assert [r[0] for r in rec if r[0] == "camera"] == ["camera"] * (1 if combo[0] != "all" else GH.GROUPS[g][0])
        assert [r[0] for r in rec][:len(rec) - sum(r[0] == "camera" for r in rec)].count("camera") == 0, "cameras come last"
        assert [(e["kind"], len(e["vertices"]), 0 if e["faces"] is None else len(e["faces"])) for e in exp] == [r[:3] for r in body], key
        assert [GH.geometry_digest(e["vertices"], e["faces"], e["colors"], e["normals"]) for e in exp] == [r[3] for r in body], key
        assert GH.reference_scale(kept)[0] == float(z[f"{key}_scale"])


def test_gist_rainbow_table_equals_matplotlib_rows(glb, gold):
    assert np.array_equal(glb.gist_rainbow_lut(), gold["colors"]["gist_rainbow"])
    assert glb.camera_color(0, 3) == (255, 0, 40) and glb.camera_color(0, 1) == (255, 0, 40)


def test_camera_colors_equal_reference(glb, gold):
    z = gold["scene"]
    for g, (S, _, _) in GH.GROUPS.items():
        rec = z[GH.combo_key(g, ("all", False, False, False, False)) + "_cam_c"]
        assert [tuple(int(v) for v in r) for r in rec] == [glb.camera_color(i, S) for i in range(S)]


def test_frustum_invariants(glb):
    rng = np.random.default_rng(5)
    pose = np.eye(4)
    pose[:3, :3] = GH._rotation(rng.standard_normal(3), 1.1)
    pose[:3, 3] = (0.4, -1.3, 2.2)
    scale = 3.7
    v, f = glb.camera_frustum(pose, scale)
    assert v.shape == (18, 3) and f.shape == (48, 3) and f.max() == 17
    r, h = 0.05 * scale, 0.1 * scale
    assert np.allclose(v[5], pose[:3, 3], atol=1e-12), "the apex is the camera centre"
    corners = np.array([[sx * r / np.sqrt(2), sy * r / np.sqrt(2), h] for sx in (1, -1) for sy in (1, -1)]) @ pose[:3, :3].T + pose[:3, 3]
    got = v[1:5]
    d = np.abs(got[:, None] - corners[None]).max(-1)
    assert (d.min(1) < 1e-12).all() and sorted(d.argmin(1)) == [0, 1, 2, 3], "the four base corners, as a set"
    assert np.allclose(v[0], pose[:3, :3] @ np.array([0, 0, h]) + pose[:3, 3], atol=1e-12)
    assert np.allclose(v[6:12] - v[0], 0.95 * (v[:6] - v[0]), atol=1e-12), "the second layer: the pyramid x 0.95 about the base centre"
    assert np.allclose(v[12], v[0], atol=1e-12) and np.allclose(v[17], v[5], atol=1e-12), "the third layer turns about the axis"
    cosang = ((v[13:17] - v[0]) * (v[1:5] - v[0])).sum(-1) / r ** 2
    assert np.allclose(cosang, np.cos(np.radians(2.0)), atol=1e-12)
    half = f[:24]
    assert np.array_equal(f[24:], half[:, ::-1]), "every sliver once more with the opposite winding"
    assert (half % 6 != 0).all(), "no sliver touches a layer's base centre: only the four side faces are used"
    # the first six faces are generate_camera_mesh_faces' pattern over the side face (1, 2, 5)
    assert half[:6].tolist() == [[1, 2, 8], [1, 7, 5], [11, 2, 5], [1, 2, 14], [1, 13, 5], [17, 2, 5]]


def test_frustum_equals_reference_construction(glb, gold):
    """camera_frustum against the reference's integrate_camera_into_scene run on the same pyramid.  The reference's radius and height are
    fp32 products of its fp32 scale (relative error 2^-24 each) and scipy's rotation matrices may differ from cos / sin in the last place;
    the coordinates are at most |t| + 0.12 scale: 4 fp32 roundings of the offset and 1e-12 relative for the rest."""
    z = gold["scene"]
    for g in GH.GROUPS:
        p = GH.make_inputs(g)
        key = GH.combo_key(g, ("all", True, False, False, False))
        scale = float(z[f"{key}_scale"])
        for i, (rv, rf) in enumerate(zip(z[f"{key}_cam_v"], z[f"{key}_cam_f"])):
            v, f = glb.camera_frustum(p["camera_poses"][i], scale)
            assert np.array_equal(f, rf)
            tol = 4 * 2.0 ** -24 * 0.12 * scale + 1e-12 * (np.abs(p["camera_poses"][i][:3, 3]).max() + scale)
            assert np.abs(v - rv).max() <= tol, (g, i, np.abs(v - rv).max(), tol)


def test_frame_selector(glb):
    f = glb.parse_frame_selector
    assert f("all") is None and f("All") is None
    assert f("3: name.png") == 3 and f("0: a:b.png") == 0 and f("12") == 12 and f(" 7 : x") == 7
    assert f("name.png") is None and f("") is None and f("ALL") is None and f(None) is None and f(": x") is None


def test_save_camera_params(glb, tmp_path):
    ext = np.arange(32, dtype=np.float32).reshape(2, 4, 4) / 7
    intr = np.arange(18, dtype=np.float64).reshape(2, 3, 3) / 3
    path = glb.save_camera_params(ext, intr, str(tmp_path))
    assert path == os.path.join(str(tmp_path), "camera_params.json")
    text = open(path).read()
    expect = {"num_cameras": 2, "extrinsics": [{"camera_id": i, "matrix": ext[i].tolist()} for i in range(2)],
              "intrinsics": [{"camera_id": i, "matrix": intr[i].tolist()} for i in range(2)]}
    assert text == json.dumps(expect, indent=2)
    assert list(json.loads(text)) == ["num_cameras", "extrinsics", "intrinsics"]


def test_container_round_trip(glb, tmp_path):
    """A GLB assembled from small numpy arrays: header, chunks, padding, alignment, component types, min / max, asset.version; and load_glb
    returns what went in."""
    rng = np.random.default_rng(3)
    mesh = dict(kind="mesh", vertices=rng.standard_normal((5, 3)).astype(np.float32), colors=rng.integers(0, 256, (5, 4)).astype(np.uint8),
                faces=np.array([[0, 1, 2], [0, 2, 3], [2, 3, 4]]), normals=rng.standard_normal((5, 3)).astype(np.float32))
    cloud = dict(kind="points", vertices=rng.standard_normal((7, 3)).astype(np.float32), colors=rng.integers(0, 256, (7, 4)).astype(np.uint8))
    cam = dict(kind="camera", vertices=rng.standard_normal((18, 3)), colors=np.full((18, 4), 255, np.uint8), faces=rng.integers(0, 18, (48, 3)))
    T = rng.standard_normal((4, 4))
    data = glb.glb_from_arrays([mesh, cloud, cam], T)
    magic, version, total = struct.unpack_from("<III", data, 0)
    assert (magic, version, total) == (0x46546C67, 2, len(data)) and data[:4] == b"glTF" and len(data) % 4 == 0
    n_json, t_json = struct.unpack_from("<II", data, 12)
    assert t_json == 0x4E4F534A and n_json % 4 == 0
    js = data[20:20 + n_json]
    doc = json.loads(js)
    assert js.rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode(), "padded with spaces only"
    n_bin, t_bin = struct.unpack_from("<II", data, 20 + n_json)
    assert t_bin == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == len(data)
    assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [{"byteLength": n_bin}] and len(doc["buffers"]) == 1
    for v in doc["bufferViews"]:
        assert v["byteOffset"] % 4 == 0 and v["byteOffset"] + v["byteLength"] <= n_bin and v["buffer"] == 0
    for m, kind in zip(doc["meshes"], ("mesh", "points", "camera")):
        (pr,) = m["primitives"]
        assert pr["mode"] == (0 if kind == "points" else 4)
        pos, col = doc["accessors"][pr["attributes"]["POSITION"]], doc["accessors"][pr["attributes"]["COLOR_0"]]
        assert pos["componentType"] == 5126 and pos["type"] == "VEC3" and len(pos["min"]) == 3 and len(pos["max"]) == 3
        assert col["componentType"] == 5121 and col["type"] == "VEC4" and col["normalized"] is True
        if kind != "points":
            ind = doc["accessors"][pr["indices"]]
            assert ind["componentType"] == 5125 and ind["type"] == "SCALAR" and ind["count"] % 3 == 0
        else:
            assert "indices" not in pr
        if kind == "mesh":
            nrm = doc["accessors"][pr["attributes"]["NORMAL"]]
            assert nrm["componentType"] == 5126 and nrm["type"] == "VEC3"
    assert doc["scenes"] == [{"nodes": [0]}] and doc["nodes"][0]["children"] == [1, 2, 3] and len(doc["nodes"][0]["matrix"]) == 16
    assert all(c["count"] > 0 for c in doc["accessors"])

    path = tmp_path / "x.glb"
    path.write_bytes(data)
    for src in (data, str(path)):
        back = glb.load_glb(src)
        assert np.array_equal(back["nodes"][0]["matrix"], T) and [n["mesh"] for n in back["nodes"]] == [None, 0, 1, 2]
        for pr, geo in zip(back["primitives"], (mesh, cloud, cam)):
            assert np.array_equal(pr["positions"], geo["vertices"].astype(np.float32)) and np.array_equal(pr["colors"], geo["colors"])
            assert (pr["indices"] is None) == ("faces" not in geo) and (pr["normals"] is None) == ("normals" not in geo)
            if "faces" in geo:
                assert np.array_equal(pr["indices"], geo["faces"]) and pr["indices"].dtype == np.uint32
            if "normals" in geo:
                assert np.array_equal(pr["normals"], geo["normals"])
            acc = back["json"]["accessors"][back["json"]["meshes"][pr["node"] - 1]["primitives"][0]["attributes"]["POSITION"]]
            assert np.array_equal(np.array(acc["min"], np.float32), pr["positions"].min(0)) and np.array_equal(np.array(acc["max"], np.float32), pr["positions"].max(0))
    buf = io.BytesIO()
    scene = glb.GLBScene([], np.eye(4), 1.0)
    assert scene.export(file_obj=buf) is None and scene.export() == buf.getvalue() and glb.load_glb(buf.getvalue())["primitives"] == []
    with pytest.raises(ValueError):
        glb.load_glb(data[:-4])


def test_package_exports(glb):
    import hunyuanworld_mirror_amd as pkg
    for name in ("image_mesh", "convert_predictions_to_glb_scene", "GLBScene", "load_glb", "save_camera_params"):
        assert getattr(pkg, name) is getattr(glb, name)


def test_no_cpu_fallback(glb):
    import torch
    with pytest.raises(RuntimeError):
        glb.image_mesh(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3))
