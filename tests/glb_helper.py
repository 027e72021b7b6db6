"""Shared by tools/gen_golden_glb.py and tests/test_glb_*.py: the inputs of the GLB fixtures (drawn from a seed; the fixture stores their
digest), and a numpy restatement of the image-mesh rule and of the scene's geometry, which tests/test_glb_cpu.py pins to what the
reference's create_image_mesh / convert_predictions_to_glb_scene produced (tests/golden/glb_*.npz), so that GPU tests can use it at sizes
that have no fixture."""
import hashlib
import itertools

import numpy as np

GROUPS = {"a": (3, 37, 52), "b": (2, 61, 83), "c": (1, 2, 2), "d": (1, 1, 9)}
SEEDS = {"a": 2026102001, "b": 2026102002, "c": 2026102003, "d": 2026102004}
# per group and view: (final_mask, sky_mask) kinds
MASKS = {"a": [("false", "true"), ("iid", "iid"), ("checker", "true")],
         "b": [("iid", "true"), ("corner", "iid")],
         "c": [("true", "false")],
         "d": [("true", "true")]}
RANDOM_VIEWS = [("a", 1, "final_mask"), ("a", 1, "sky_mask"), ("b", 0, "final_mask"), ("b", 1, "sky_mask")]


def frame_selector(g):
    """the single-frame selector of group g, in app.py's "<index>: <file name>" form"""
    return "1: img_0001.png" if GROUPS[g][0] > 1 else "0: img_0000.png"


def combos(g):
    """(frames, as_mesh, mask_ambiguous, mask_sky_bg, with_normals) of every recorded call"""
    out = [(fr, m, a, s, False) for fr, m, a, s in itertools.product(("all", frame_selector(g)), (True, False), (False, True), (False, True))]
    return out + [(frame_selector(g), True, False, True, True)]


def combo_key(g, combo):
    fr, m, a, s, n = combo
    return f"{g}_{'all' if fr == 'all' else 'one'}_m{int(m)}a{int(a)}s{int(s)}n{int(n)}"


def _mask(kind, H, W, rng):
    if kind == "iid":
        return rng.random((H, W)) < 0.8
    if kind == "true":
        return np.ones((H, W), bool)
    if kind == "false":
        return np.zeros((H, W), bool)
    if kind == "checker":
        yy, xx = np.mgrid[:H, :W]
        return (yy + xx) % 2 == 0
    if kind == "corner":      # one valid quad, in the last row and column, and a few lone pixels
        m = np.zeros((H, W), bool)
        m[-2:, -2:] = True
        m[0, 0] = m[H // 2, W // 2] = m[0, -1] = True
        return m
    raise KeyError(kind)


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_inputs(g):
    """The predictions dict of group g (numpy): world_points, images (in [0, 1], a third of them exact k / 255), normal, camera_poses
    [S,4,4] fp64 with fp32-representable entries, final_mask, sky_mask."""
    S, H, W = GROUPS[g]
    rng = np.random.default_rng(SEEDS[g])
    pts = (rng.standard_normal((S, H, W, 3)) * np.array([2.0, 1.0, 3.0]) + np.array([0.3, -0.2, 4.0])).astype(np.float32)
    img = rng.random((S, H, W, 3), dtype=np.float32)
    k255 = (rng.integers(0, 256, (S, H, W, 3)).astype(np.float32) / np.float32(255))
    img = np.where(rng.random((S, H, W, 3)) < 1 / 3, k255, img).astype(np.float32)
    nrm = rng.standard_normal((S, H, W, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    poses = np.tile(np.eye(4), (S, 1, 1))
    for i in range(S):
        poses[i, :3, :3] = _rotation(rng.standard_normal(3), rng.uniform(-2.5, 2.5))
        poses[i, :3, 3] = rng.uniform(-1.5, 1.5, 3)
    poses = poses.astype(np.float32).astype(np.float64)
    final = np.stack([_mask(MASKS[g][i][0], H, W, rng) for i in range(S)])
    sky = np.stack([_mask(MASKS[g][i][1], H, W, rng) for i in range(S)])
    return {"world_points": pts, "images": img, "normal": nrm, "camera_poses": poses, "final_mask": final, "sky_mask": sky}


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def inputs_digest(p):
    return digest(*(p[k] for k in ("world_points", "images", "normal", "camera_poses", "final_mask", "sky_mask")))


def geometry_digest(vertices, faces, colors_rgb, normals):
    """one geometry as the reference handed it to trimesh: fp32 vertices, int32 faces, uint8 rgb, fp32 normals (absent parts contribute nothing)"""
    parts = [np.asarray(vertices, np.float32)]
    if faces is not None:
        parts.append(np.asarray(faces, np.int32))
    parts.append(np.asarray(colors_rgb, np.uint8))
    if normals is not None:
        parts.append(np.asarray(normals, np.float32))
    return digest(*parts)


# ------------------------------------------------------------------------------------------------ the rules, restated
def image_mesh_ref(mask):
    """mask [H,W] bool -> (faces [F,3] int32, vertex pixel indices [V] ascending).  A quad at p = y W + x is valid when p, p + W,
    p + W + 1, p + 1 are masked in; a pixel is a vertex when it is a corner of a valid quad; faces (a, b, c), (a, c, d) per quad
    (p, p + W, p + W + 1, p + 1) in raster order, through the rank of each pixel among the vertices."""
    H, W = mask.shape
    if H < 2 or W < 2:
        return np.zeros((0, 3), np.int32), np.zeros((0,), np.int64)
    valid = mask[:-1, :-1] & mask[1:, :-1] & mask[1:, 1:] & mask[:-1, 1:]
    used = np.zeros((H, W), bool)
    used[:-1, :-1] |= valid
    used[1:, :-1] |= valid
    used[1:, 1:] |= valid
    used[:-1, 1:] |= valid
    rank = np.cumsum(used.ravel()) - 1
    ys, xs = np.nonzero(valid)
    p = ys * W + xs
    quads = np.stack([rank[p], rank[p + W], rank[p + W + 1], rank[p + 1]], 1)
    faces = quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).astype(np.int32)
    return faces, np.flatnonzero(used.ravel())


def mesh_color_bytes(img):
    """the reference's three fp32 roundings and the truncation: (x * 255) / 255 * 255 -> uint8"""
    x = img.astype(np.float32) * np.float32(255)
    x = x / np.float32(255)
    return (x * np.float32(255)).astype(np.uint8)


def point_color_bytes(img):
    return (img.astype(np.float32) * np.float32(255)).astype(np.uint8)


def flag_mask(p, amb, sky):
    m = np.ones(p["final_mask"].shape, bool)
    if amb:
        m = m & p["final_mask"]
    if sky:
        m = m & p["sky_mask"]
    return m


def select(p, frames):
    """the predictions restricted to the selected frame (kept as a batch of one), and its index or None"""
    if frames in ("all", "All"):
        return p, None
    t = int(frames.split(":")[0])
    return {k: v[t][None] for k, v in p.items()}, t


def expected_geometry(p, frames, as_mesh, amb, sky, with_normals):
    """The point / mesh geometries of the scene in order (cameras excluded, views without a vertex left out):
    dicts kind, frame, vertices fp32, colors uint8 [n,3], faces int32 or None, normals or None; and the flag-filtered points the scale is
    taken over."""
    q, t = select(p, frames)
    fm = flag_mask(q, amb, sky)
    kept = q["world_points"].reshape(-1, 3)[fm.reshape(-1)]
    out = []
    if not as_mesh:
        if len(kept) == 0:
            out.append(dict(kind="points", frame=None, vertices=np.array([[1, 0, 0]], np.float32), colors=np.array([[255, 255, 255]], np.uint8),
                            faces=None, normals=None))
        else:
            out.append(dict(kind="points", frame=None, vertices=kept, colors=point_color_bytes(q["images"]).reshape(-1, 3)[fm.reshape(-1)],
                            faces=None, normals=None))
        return out, kept
    S = q["world_points"].shape[0]
    for i in range(S):
        m = q["final_mask"][i] if t is not None else fm[i]
        faces, idx = image_mesh_ref(m)
        if len(idx) == 0:
            continue
        out.append(dict(kind="mesh", frame=t if t is not None else i, vertices=q["world_points"][i].reshape(-1, 3)[idx],
                        colors=mesh_color_bytes(q["images"][i]).reshape(-1, 3)[idx], faces=faces,
                        normals=q["normal"][i].reshape(-1, 3)[idx] if (with_normals and t is not None) else None))
    return out, kept


def reference_scale(kept):
    """visual_util.py:301-309 on the kept points -> (scale, the six percentile coordinates or None)"""
    if len(kept) == 0:
        return 1.0, None
    lo, hi = np.percentile(kept, 5, axis=0), np.percentile(kept, 95, axis=0)
    return float(np.linalg.norm(hi - lo)), np.concatenate([lo, hi])
