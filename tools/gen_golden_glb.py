"""Writes tests/golden/glb_*.npz by running the REFERENCE's own create_image_mesh and convert_predictions_to_glb_scene
(src/utils/visual_util.py) on the CPU.  Data only; nothing of the reference is copied.

    python tools/gen_golden_glb.py <reference root>

What visual_util.py imports and this machine need not have is replaced in sys.modules by stand-ins: ``cv2`` and ``requests`` are empty
modules (only the sky segmentation and the downloader use them); ``trimesh`` records what ``Scene``, ``Trimesh`` and ``PointCloud`` are
given and computes nothing, and its ``creation.cone`` is the library's own ``glb.cone_pyramid`` (trimesh is absent, so the cone's vertex
order is the library's: what is pinned is the reference's construction AROUND the cone, not trimesh's vertex order).  matplotlib and scipy
are the installed packages.

Inputs: tests/glb_helper.make_inputs (drawn from a seed; the fixture keeps their digest, not the arrays).  View groups 3 x 37 x 52,
2 x 61 x 83, 1 x 2 x 2 and 1 x 1 x 9; masks iid at keep rate 0.8, all true, all false, a checkerboard (no valid quad) and one valid quad in
the last row and column.  Every call gets a fresh copy of the images: the reference scales predictions["images"] by 255 in place on every
mesh call (asserted below), which the library does not reproduce.

Files:
  glb_mesh.npz    per group and view, create_image_mesh(mask=final_mask[view], triangulate=True, return_vertex_indices=True): faces, the
                  vertex pixel indices, and (asserted) vertices and colours that are the rows of the inputs at those indices
  glb_scene.npz   per group and flag combination (glb_helper.combos): the kinds of the geometries in order, their vertex and face counts
                  and a digest of each one's arrays as handed to trimesh (fp32 vertices, int32 faces, uint8 rgb, fp32 normals), the scale,
                  the scene transformation, and the cameras' vertices, faces and colours
  glb_colors.npz  the 256 rows of matplotlib's gist_rainbow (fp64)

Asserted here: per random-mask view at least 25 % of the quads are valid and at least one masked-in pixel is not a vertex; the reference's
two [1, -1, 1] flips return the input bits."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def install_stand_ins():
    from hunyuanworld_mirror_amd import glb

    for name in ("cv2", "requests"):
        sys.modules[name] = types.ModuleType(name)

    class Trimesh:
        def __init__(self, vertices=None, faces=None, vertex_colors=None, vertex_normals=None, process=True):
            self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)
            self.vertex_colors, self.vertex_normals = vertex_colors, vertex_normals
            self.visual = types.SimpleNamespace(face_colors=np.full((len(self.faces), 4), 255, np.uint8))

    class PointCloud:
        def __init__(self, vertices=None, colors=None):
            self.vertices, self.colors = np.asarray(vertices), np.asarray(colors)

    class Scene:
        def __init__(self):
            self.geometry, self.transform = [], None

        def add_geometry(self, g):
            self.geometry.append(g)

        def apply_transform(self, m):
            self.transform = np.array(m)

    def cone(radius, height, sections=None):
        assert sections == 4
        tm.last_cone = (radius, height)
        v, f = glb.cone_pyramid(radius, height)
        return types.SimpleNamespace(vertices=v, faces=f)

    tm = types.ModuleType("trimesh")
    tm.Trimesh, tm.PointCloud, tm.Scene = Trimesh, PointCloud, Scene
    tm.creation = types.SimpleNamespace(cone=cone)
    sys.modules["trimesh"] = tm
    return tm


def main(ref_root):
    import matplotlib
    import glb_helper as GH
    tm = install_stand_ins()
    sys.path.insert(0, ref_root)
    VU = importlib.import_module("src.utils.visual_util")

    np.savez_compressed(os.path.join(GOLD, "glb_colors.npz"), gist_rainbow=matplotlib.colormaps["gist_rainbow"](np.arange(256))[:, :3])

    mesh_store, scene_store = {}, {}
    for g, (S, H, W) in GH.GROUPS.items():
        p = GH.make_inputs(g)
        mesh_store[f"{g}_shape"] = np.array([S, H, W])
        scene_store[f"{g}_digest"] = mesh_store[f"{g}_digest"] = np.array(GH.inputs_digest(p))
        # ---- create_image_mesh itself
        for i in range(S):
            m = p["final_mask"][i]
            faces, v, c, idx = VU.create_image_mesh(p["world_points"][i], p["images"][i], mask=m, triangulate=True, return_vertex_indices=True)
            assert faces.dtype == np.int32 and np.array_equal(v.view(np.uint32), p["world_points"][i].reshape(-1, 3)[idx].view(np.uint32))
            assert np.array_equal(c, p["images"][i].reshape(-1, 3)[idx])
            mesh_store[f"{g}_v{i}_faces"], mesh_store[f"{g}_v{i}_idx"] = faces, idx.astype(np.int32)
        for (gg, i, which) in GH.RANDOM_VIEWS:
            if gg != g:
                continue
            m = p[which][i]
            valid = m[:-1, :-1] & m[1:, :-1] & m[1:, 1:] & m[:-1, 1:]
            _, idx = VU.create_image_mesh(mask=m, triangulate=True, return_vertex_indices=True)
            assert valid.mean() >= 0.25, (g, i, which, valid.mean())
            assert m.sum() > len(idx), "every masked-in pixel is a vertex: the case is vacuous"
            print(f"{g} view {i} {which}: {valid.mean():.3f} of the quads valid, {m.sum() - len(idx)} masked-in pixels are no vertex")
        # ---- the scene, every flag combination
        for combo in GH.combos(g):
            frames, as_mesh, amb, sky, with_normals = combo
            pred = {k: v.copy() for k, v in p.items()}
            if not with_normals:
                del pred["normal"]
            before = pred["images"].copy()
            scene = VU.convert_predictions_to_glb_scene(pred, filter_by_frames=frames, show_camera=True, mask_sky_bg=sky, mask_ambiguous=amb,
                                                        as_mesh=as_mesh)
            if as_mesh:
                assert not np.array_equal(before, pred["images"]), "the reference no longer scales the caller's images in place"
            key = GH.combo_key(g, combo)
            kinds, counts, digests, cam_v, cam_f, cam_c = [], [], [], [], [], []
            for geo in scene.geometry:
                if isinstance(geo, tm.PointCloud):
                    kinds.append("points")
                    counts.append((len(geo.vertices), 0))
                    digests.append(GH.geometry_digest(geo.vertices, None, geo.colors, None))
                elif geo.vertex_colors is not None:
                    kinds.append("mesh")
                    counts.append((len(geo.vertices), len(geo.faces)))
                    assert geo.vertices.dtype == np.float32 and geo.faces.dtype == np.int32 and geo.vertex_colors.dtype == np.uint8
                    digests.append(GH.geometry_digest(geo.vertices, geo.faces, geo.vertex_colors, geo.vertex_normals))
                else:
                    kinds.append("camera")
                    counts.append((len(geo.vertices), len(geo.faces)))
                    digests.append("")
                    cam_v.append(np.asarray(geo.vertices, np.float64))
                    cam_f.append(np.asarray(geo.faces, np.int64))
                    assert (geo.visual.face_colors[:, :3] == geo.visual.face_colors[0, :3]).all()
                    cam_c.append(geo.visual.face_colors[0, :3].astype(np.uint8))
            exp, kept = GH.expected_geometry(p, frames, as_mesh, amb, sky, with_normals)
            _, pct = GH.reference_scale(kept)
            # the helper's restatement (fp32 bit copies of the input rows: the two flips cancel) against what trimesh was handed
            got = [d for d, k, c in zip(digests, kinds, counts) if k != "camera" and c[0] > 0]
            assert got == [GH.geometry_digest(e["vertices"], e["faces"], e["colors"], e["normals"]) for e in exp], key
            scene_store[f"{key}_kinds"] = np.array(kinds)
            scene_store[f"{key}_counts"] = np.array(counts, np.int64).reshape(-1, 2)
            scene_store[f"{key}_digests"] = np.array(digests)
            scene_store[f"{key}_transform"] = np.asarray(scene.transform, np.float64)
            scene_store[f"{key}_cam_v"], scene_store[f"{key}_cam_f"], scene_store[f"{key}_cam_c"] = np.array(cam_v), np.array(cam_f), np.array(cam_c)
            # the scale is the camera base width / 0.05 only up to rounding: recompute it with the reference's own statements
            scene_store[f"{key}_scale"] = np.float64(1.0 if len(kept) == 0 else
                                                     np.linalg.norm(np.percentile(kept, 95, axis=0) - np.percentile(kept, 5, axis=0)))
            assert tm.last_cone == (np.float32(scene_store[f"{key}_scale"]) * 0.05, np.float32(scene_store[f"{key}_scale"]) * 0.1) or len(kept) == 0
            scene_store[f"{key}_pct"] = np.zeros(6) if pct is None else pct.astype(np.float64)
            print(key, kinds.count("mesh"), "meshes", kinds.count("points"), "clouds", kinds.count("camera"), "cameras, kept", len(kept),
                  "scale", float(scene_store[f"{key}_scale"]))
    np.savez_compressed(os.path.join(GOLD, "glb_mesh.npz"), **mesh_store)
    np.savez_compressed(os.path.join(GOLD, "glb_scene.npz"), **scene_store)
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("glb_"):
            print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main(sys.argv[1])
