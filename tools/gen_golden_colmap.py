"""Writes tests/golden/colmap_a.npz: the REFERENCE's own --save_colmap statements (infer.py, the body of `if args.save_colmap:`) with
its own depth_to_world_coords_points, create_pixel_coordinate_grid, create_confidence_mask and build_pycolmap_reconstruction, run on the
CPU in fp64 on fp32-valued inputs, at conf_threshold 0, 30 and 100.  Data only: the inputs and the recorded results.

    python tools/gen_golden_colmap.py <reference root>

Nothing of the reference is copied or imported as a package.  infer.py is parsed with `ast` and the one `if` statement is compiled on its
own; src/models/utils/geometry.py and src/utils/build_pycolmap_recon.py are executed from their files into private namespaces.  `pycolmap`
is replaced by the recording stand-in below, which keeps what it is handed (add_point3D, Point2D, Track.add_element, Camera, Image,
Rigid3d) and computes nothing.  vector_to_camera_matrices is replaced by a stub that hands out this tool's poses and the intrinsics of the
asked image size.

Scene: 3 views of 28 x 42 (H x W), saved images of 59 x 40 (out_w / W = 1.405, out_h / H = 1.43: neither an integer, so the truncation of
the rescaled pixel coordinates matters and an x / y swap shows).  View 1 has no valid depth at all; view 0 has a rectangle of depths <= 0
and a band of confidences <= 1e-5 (0 and 1e-6); view 2 has a few negative depths.  All other confidences are distinct.

Asserted here: for each percentage the K-th and the (K + 1)-th largest confidence differ (only then is the kept set independent of a tie
rule); the fp32 run of the same statements keeps the same points with the same colours and pixel coordinates.

Recorded yardsticks (the bounds of tests/test_colmap_gpu.py are 4 x these):
  err_points      max |point of the reference's fp32 run - point of its fp64 run| over the kept points, the largest of the three runs
                  (p<percent>_err_points: per run)
  err_reproj_px, err_reproj_depth   the kept points of the fp32 run (p = 30) put through the trainer's own projection statements
                  (datasets/colmap.py, `if self.load_depths:`) with fp32 arrays, against the source pixel and the input depth; the fp64 run
                  of the same chain lands on them to ~1e-13, so this is the reference's fp32-vs-fp64 reprojection error."""
import ast
import os
import pathlib
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERCENTS = (0.0, 30.0, 100.0)
S, H, W, OUT_W, OUT_H = 3, 28, 42, 59, 40


# ---------------------------------------------------------------- the recording stand-in for pycolmap
class Track:
    def __init__(self):
        self.elements = []

    def add_element(self, image_id, point2D_idx):
        self.elements.append((int(image_id), int(point2D_idx)))


class _Point3D:
    def __init__(self, xyz, track, color):
        self.xyz, self.track, self.color = np.array(xyz, dtype=np.float64), track, np.array(color)


class Point2D:
    def __init__(self, xy, point3D_id):
        self.xy, self.point3D_id = np.array(xy), int(point3D_id)


class Camera:
    def __init__(self, model, width, height, params, camera_id):
        self.model, self.width, self.height, self.params, self.camera_id = model, int(width), int(height), np.array(params), int(camera_id)


class Rotation3d:
    def __init__(self, matrix):
        self.matrix = np.array(matrix)


class Rigid3d:
    def __init__(self, rotation, translation):
        self.rotation, self.translation = rotation, np.array(translation)


class Image:
    def __init__(self, id, name, camera_id, cam_from_world):
        self.id, self.name, self.camera_id, self.cam_from_world = int(id), name, int(camera_id), cam_from_world
        self.points2D, self.registered = [], None


class Reconstruction:
    def __init__(self):
        self.points3D, self.cameras, self.images = {}, {}, {}

    def add_point3D(self, xyz, track, color):
        pid = len(self.points3D) + 1
        self.points3D[pid] = _Point3D(xyz, track, color)
        return pid

    def add_camera(self, camera):
        self.cameras[camera.camera_id] = camera

    def add_image(self, image):
        self.images[image.id] = image

    def write(self, path):
        pass


def _stand_in():
    m = types.ModuleType("pycolmap")
    for c in (Track, Point2D, Camera, Rotation3d, Rigid3d, Image, Reconstruction):
        setattr(m, c.__name__, c)
    m.ListPoint2D = list
    return m


# ---------------------------------------------------------------- the reference's statements
def _exec_file(path, extra=None):
    ns = dict(extra or {})
    exec(compile(open(path).read(), path, "exec"), ns)
    return ns


def _find_if(tree, test_src, must_call=None):
    """the one ast.If whose test reads `test_src` (and whose body calls the function `must_call`)"""
    found = [n for n in ast.walk(tree) if isinstance(n, ast.If) and ast.unparse(n.test) == test_src]
    if must_call:
        found = [n for n in found if any(isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == must_call for c in ast.walk(n))]
    assert len(found) == 1, (test_src, len(found))
    return found[0]


def _compile_body(node, name):
    return compile(ast.fix_missing_locations(ast.Module(body=node.body, type_ignores=[])), name, "exec")


def _function(tree, name):
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name)
    return compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), name, "exec")


def load_reference(ref_root):
    infer = ast.parse(open(os.path.join(ref_root, "infer.py")).read())
    geo = _exec_file(os.path.join(ref_root, "src", "models", "utils", "geometry.py"))
    sys.modules["pycolmap"] = _stand_in()
    try:
        recon = _exec_file(os.path.join(ref_root, "src", "utils", "build_pycolmap_recon.py"))
    finally:
        del sys.modules["pycolmap"]
    ns = dict(torch=torch, np=np)
    exec(_function(infer, "create_confidence_mask"), ns)
    colmap_py = ast.parse(open(os.path.join(ref_root, "submodules", "gsplat", "examples", "datasets", "colmap.py")).read())
    return dict(block=_compile_body(_find_if(infer, "args.save_colmap", must_call="build_pycolmap_reconstruction"), "reference save_colmap block"),
                depth_to_world_coords_points=geo["depth_to_world_coords_points"], create_pixel_coordinate_grid=geo["create_pixel_coordinate_grid"],
                create_confidence_mask=ns["create_confidence_mask"], build_pycolmap_reconstruction=recon["build_pycolmap_reconstruction"],
                project=_compile_body(_find_if(colmap_py, "self.load_depths"), "reference projection block"))


def run_block(ref, sc, percent, dtype):
    """the `if args.save_colmap:` body on this scene in `dtype` -> its namespace"""
    def vector_to_camera_matrices(_params, image_hw):
        k = sc["K_in"] if tuple(image_hw) == (H, W) else sc["K_out"]
        assert tuple(image_hw) in ((H, W), (OUT_H, OUT_W))
        return sc["w2c"][:, :3, :].to(dtype)[None], k.to(dtype)[None]

    saved = {}
    ns = dict(torch=torch, np=np, print=lambda *a, **k: None, args=types.SimpleNamespace(save_colmap=True, conf_threshold=percent),
              new_width=OUT_W, new_height=OUT_H, H=H, W=W, S=S, vector_to_camera_matrices=vector_to_camera_matrices,
              predictions=dict(camera_params=None, depth=sc["depth"].to(dtype)[None, ..., None], depth_conf=sc["conf"].to(dtype)[None]),
              imgs=sc["images"].to(dtype)[None], processed_image_names=list(sc["names"]), sparse_dir=pathlib.Path("sparse/0"),
              save_points_ply=lambda path, p, c: saved.update(path=str(path), pts=p, cols=c),
              **{k: ref[k] for k in ("depth_to_world_coords_points", "create_pixel_coordinate_grid", "create_confidence_mask",
                                     "build_pycolmap_reconstruction")})
    exec(ref["block"], ns)
    assert saved["pts"] is ns["f_pts"] and saved["cols"] is ns["f_cols"]
    return ns


def reference_projection(ref, points, c2w, K, dtype):
    """the dataset's projection statements for one camera on arrays of `dtype` -> pixels [M,2], depths [M], selector [M]"""
    parser = types.SimpleNamespace(image_names=["img"], point_indices={"img": np.arange(len(points))}, points=points.astype(dtype))
    ns = dict(np=np, torch=torch, self=types.SimpleNamespace(parser=parser, load_depths=True), camtoworlds=c2w.astype(dtype), K=K.astype(dtype), index=0,
              image=np.zeros((H, W, 3), np.float32), data={})
    exec(ref["project"], ns)
    proj, cam = ns["points_proj"], ns["points_cam"]
    assert proj.dtype == dtype
    return proj[:, :2] / proj[:, 2:3], cam[:, 2], ns["selector"]


# ---------------------------------------------------------------- the scene
def scene(seed=17):
    g = torch.Generator().manual_seed(seed)

    def rot(ax, a):
        c, s = np.cos(a), np.sin(a)
        m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
        return torch.tensor(m, dtype=torch.float64)

    w2c = torch.eye(4, dtype=torch.float64).repeat(S, 1, 1)
    for i in range(S):
        a = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.9
        w2c[i, :3, :3] = rot(0, float(a[0])) @ rot(1, float(a[1])) @ rot(2, float(a[2]))
        w2c[i, :3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([1.0, 0.6, 0.8])
    w2c = w2c.float()
    K_in = torch.stack([torch.tensor([[38.0 + i, 0, W / 2 + 0.3 * i], [0, 36.5 - i, H / 2 - 0.2], [0, 0, 1]]) for i in range(S)])
    K_out = K_in.clone()
    K_out[:, 0, :] = (K_in[:, 0, :].double() * (OUT_W / W)).float()
    K_out[:, 1, :] = (K_in[:, 1, :].double() * (OUT_H / H)).float()
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.arange(S, dtype=torch.float32).reshape(S, 1, 1)
    depth = (2.6 + 0.9 * torch.sin(0.21 * xx + 0.17 * yy + ph) + 0.3 * torch.rand(S, H, W, generator=g)).float()
    depth[1] = 0.0                                   # a view without a candidate
    depth[0, 10:15, 20:31] = 0.0
    depth[0, 12, 22:25] = -1.0
    depth[2, 3, 5:9] = -0.5
    conf = (1.0 + 9.0 * torch.rand(S, H, W, generator=g)).float()
    conf[0, 5:8, :] = 0.0
    conf[0, 6, ::2] = 1e-6
    images = torch.rand(S, 3, H, W, generator=g).float()
    return dict(w2c=w2c, K_in=K_in, K_out=K_out, depth=depth, conf=conf, images=images, names=["view_b.png", "view_c.png", "view_a.png"])


def main(ref_root):
    ref = load_reference(ref_root)
    sc = scene()
    out = dict(depth=sc["depth"].numpy(), conf=sc["conf"].numpy(), images=sc["images"].numpy(), w2c=sc["w2c"].numpy(), K_in=sc["K_in"].numpy(),
               K_out=sc["K_out"].numpy(), names=np.array(sc["names"]), out_size=np.array([OUT_W, OUT_H], dtype=np.int64),
               percents=np.array(PERCENTS))
    valid = sc["depth"] > 1e-8
    cand_conf = sc["conf"][valid]
    cand_conf = torch.where(cand_conf <= 1e-5, torch.full_like(cand_conf, float("-inf")), cand_conf)
    srt = torch.sort(cand_conf, descending=True).values
    live = sc["conf"][valid][sc["conf"][valid] > 1e-5]
    assert len(torch.unique(live)) == len(live), "two live confidences are equal"
    for percent in PERCENTS:
        tag = f"p{int(percent)}"
        n64, n32 = run_block(ref, sc, percent, torch.float64), run_block(ref, sc, percent, torch.float32)
        P = len(n64["f_pts"])
        n_valid = int(valid.sum())
        K = max(1, int(np.ceil(n_valid * (100.0 - percent) / 100.0))) if percent > 0 else n_valid
        assert P == K == len(n32["f_pts"]), (P, K)
        assert K == n_valid or float(srt[K - 1]) != float(srt[K]), f"the {K}-th and the next confidence tie at {percent} %"
        assert n64["all_pts"].dtype == torch.float64 and n32["all_pts"].dtype == torch.float32
        for k in ("f_cols", "f_xyf"):
            assert np.array_equal(n64[k], n32[k]), k
        # points: the block casts its result to fp32 for pycolmap; the fp64 values are taken in front of that cast
        pts64 = n64["all_pts"][n64["conf_mask"]].numpy()
        pts32 = n32["all_pts"][n32["conf_mask"]].numpy()
        assert np.array_equal(n32["f_pts"], pts32)
        rec = n64["reconstruction"]
        assert sorted(rec.points3D) == list(range(1, P + 1))
        assert all(np.array_equal(rec.points3D[i + 1].color, n64["f_cols"][i]) for i in range(P))
        tracks = [rec.points3D[i + 1].track.elements for i in range(P)]
        assert all(len(t) == 1 for t in tracks)
        counts = np.array([int((n64["f_xyf"][:, 2] == i).sum()) for i in range(S)], dtype=np.int64)
        p2d = np.concatenate([np.array([[*p.xy, p.point3D_id] for p in rec.images[i + 1].points2D], dtype=np.int64).reshape(-1, 3) for i in range(S)])
        assert [len(rec.images[i + 1].points2D) for i in range(S)] == counts.tolist()
        out.update({f"{tag}_points": pts64, f"{tag}_colors": n64["f_cols"], f"{tag}_xyf": n64["f_xyf"], f"{tag}_counts": counts,
                    f"{tag}_point3D_ids": np.array(sorted(rec.points3D), dtype=np.int64), f"{tag}_tracks": np.array([t[0] for t in tracks], dtype=np.int64).reshape(-1, 2),
                    f"{tag}_points2D": p2d, f"{tag}_K": np.int64(K), f"{tag}_err_points": np.float64(np.abs(pts32.astype(np.float64) - pts64).max())})
        if percent == 30.0:
            cams = [rec.cameras[i + 1] for i in range(S)]
            imgs = [rec.images[i + 1] for i in range(S)]
            out.update(camera_ids=np.array([c.camera_id for c in cams]), camera_models=np.array([c.model for c in cams]),
                       camera_sizes=np.array([[c.width, c.height] for c in cams]), camera_params=np.stack([c.params.astype(np.float64) for c in cams]),
                       image_ids=np.array([im.id for im in imgs]), image_camera_ids=np.array([im.camera_id for im in imgs]),
                       image_names=np.array([im.name for im in imgs]), image_registered=np.array([bool(im.registered) for im in imgs]),
                       image_rotations=np.stack([im.cam_from_world.rotation.matrix.astype(np.float64) for im in imgs]),
                       image_translations=np.stack([im.cam_from_world.translation.astype(np.float64) for im in imgs]))
            # reprojection: the trainer's statements per view, fp32 arrays against the source pixel and the input depth
            px_err = z_err = px_err64 = 0.0
            src = n64["all_xyf"][n64["conf_mask"]].numpy()          # (x, y, view) at H x W, before the rescaling
            for i in range(S):
                rows = np.nonzero(src[:, 2] == i)[0]
                if not len(rows):
                    continue
                c2w = np.linalg.inv(sc["w2c"][i].double().numpy())
                want_z = sc["depth"][i].numpy()[src[rows, 1], src[rows, 0]].astype(np.float64)
                xy, z, sel = reference_projection(ref, pts32[rows], c2w, sc["K_in"][i].numpy(), np.float32)
                # a point of pixel column 0 or row 0 reprojects to 0 +- rounding: its place inside the image bound is not decided in fp32
                assert sel[(src[rows, 0] > 0) & (src[rows, 1] > 0)].all()
                px_err = max(px_err, float(np.abs(xy.astype(np.float64) - src[rows, :2]).max()))
                z_err = max(z_err, float(np.abs(z.astype(np.float64) - want_z).max()))
                xy64, z64, _ = reference_projection(ref, pts64[rows], c2w, sc["K_in"][i].numpy(), np.float64)
                px_err64 = max(px_err64, float(np.abs(xy64 - src[rows, :2]).max()), float(np.abs(z64 - want_z).max()))
            assert px_err64 < 1e-10, px_err64
            out.update(err_reproj_px=np.float64(px_err), err_reproj_depth=np.float64(z_err))
        print(tag, "kept", P, "of", n_valid, "counts", counts.tolist(), "fp32-vs-fp64 point error", float(out[f"{tag}_err_points"]))
    out["err_points"] = np.float64(max(float(out[f"p{int(p)}_err_points"]) for p in PERCENTS))      # the largest of the three runs: the one yardstick
    print("reprojection error of the fp32 chain: pixels", float(out["err_reproj_px"]), "depth", float(out["err_reproj_depth"]))
    path = os.path.join(ROOT, "tests", "golden", "colmap_a.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
