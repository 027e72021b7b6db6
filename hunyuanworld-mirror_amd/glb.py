"""The 3-D view of the reference's demo: ``convert_predictions_to_glb_scene`` (src/utils/visual_util.py:208-469, called by app.py:531-540)
with ``create_image_mesh`` (:109-205), as a glTF 2.0 binary written here, without trimesh, matplotlib or scipy.

* ``image_mesh``: ``create_image_mesh(..., mask=, triangulate=True)`` for all views in one call (csrc/glb.hip): ordered compaction of the
  vertices, faces through a per-pixel remap, uint8 RGBA colours, per-view bounds.  No ``np.unique``, no copy of the points to the host.
* ``convert_predictions_to_glb_scene``: the reference's signature and branches -> ``GLBScene``; the point and mesh geometry is packed on the
  device in the layout of the BIN chunk and comes back in one copy when ``export`` is called.  The scene scale's percentiles are exact order
  statistics found by radix selection on the device and interpolated on the host in fp64.
* ``load_glb``: a host numpy reader of what ``export`` writes.  ``save_camera_params``: the JSON app.py:515 writes beside the GLB.

The kernels have no CPU path: predictions given as numpy arrays are uploaded once to the current HIP device.

Where this differs from the reference, on purpose:

* The caller's ``predictions["images"]`` is NOT modified.  The reference multiplies it by 255 in place on every mesh call
  (visual_util.py:332, :400), so a second call there sees images scaled by 255 again; here every call sees what the caller passed.
* A view whose mesh has no vertex is left out of the scene (a zero-count accessor is invalid glTF).
* Poses are taken to fp64 before ``inv(pose[0])``; the reference inverts in the dtype it is given (fp32 for fp32 poses).
* trimesh is absent, so neither the byte layout of its exporter nor the vertex order of ``trimesh.creation.cone`` is reproduced: the camera
  solid is built on ``cone_pyramid`` below (base centre, four ring vertices, apex), and every camera vertex carries the camera's colour.
* Non-finite kept points are out of contract (the reference's percentiles would be NaN)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

GLB_MAGIC, GLB_JSON, GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}

# matplotlib's gist_rainbow, from its piecewise-linear definition: (x, (r, g, b)) anchors, 256 rows
GIST_RAINBOW_ANCHORS = ((0.000, (1.00, 0.00, 0.16)), (0.030, (1.00, 0.00, 0.00)), (0.215, (1.00, 1.00, 0.00)), (0.400, (0.00, 1.00, 0.00)),
                        (0.586, (0.00, 1.00, 1.00)), (0.770, (0.00, 0.00, 1.00)), (0.954, (1.00, 0.00, 1.00)), (1.000, (1.00, 0.00, 0.75)))


def gist_rainbow_lut() -> np.ndarray:
    """The 256 x 3 fp64 rows of matplotlib's ``gist_rainbow``: the anchors interpolated at linspace(0, 1, 256), as a
    LinearSegmentedColormap builds its table (first and last row are the end anchors)."""
    x = np.array([a[0] for a in GIST_RAINBOW_ANCHORS], np.float64) * 255      # both axes in units of rows, as matplotlib scales them
    xind = 255 * np.linspace(0.0, 1.0, 256)
    ind = np.searchsorted(x, xind)[1:-1]
    dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.empty((256, 3), np.float64)
    for c in range(3):
        y = np.array([a[1][c] for a in GIST_RAINBOW_ANCHORS], np.float64)
        lut[:, c] = np.concatenate([[y[0]], dist * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return np.clip(lut, 0.0, 1.0)


def camera_color(i: int, n: int) -> Tuple[int, int, int]:
    """visual_util.py:444-445: int(255 x) of gist_rainbow(i / n); a float in [0, 1] indexes row int(x 256), 1.0 the last row."""
    row = min(int((i / n) * 256), 255)
    return tuple(int(255 * float(v)) for v in gist_rainbow_lut()[row])


def parse_frame_selector(filter_by_frames) -> Optional[int]:
    """visual_util.py:242-248: "3: name.png" -> 3; "all" / "All" and anything unparseable -> None (all frames)."""
    if filter_by_frames in ("all", "All"):
        return None
    try:
        return int(filter_by_frames.split(":")[0])
    except (ValueError, IndexError, AttributeError):
        return None


# ---------------------------------------------------------------------------------------------- camera solids (host, fp64)
def cone_pyramid(radius: float, height: float) -> Tuple[np.ndarray, np.ndarray]:
    """A 4-section cone along +z: vertex 0 the base centre, 1..4 the ring at angles 0, 90, 180, 270 degrees in z = 0, 5 the apex at
    z = height; 4 base and 4 side triangles, outward winding.  It stands where the reference calls trimesh.creation.cone(r, h, sections=4)."""
    v = np.zeros((6, 3), np.float64)
    for i in range(4):
        a = 0.5 * math.pi * i
        v[1 + i] = (radius * math.cos(a), radius * math.sin(a), 0.0)
    v[5] = (0.0, 0.0, height)
    ring = lambda i: 1 + i % 4
    faces = [(0, ring(i + 1), ring(i)) for i in range(4)] + [(ring(i), ring(i + 1), 5) for i in range(4)]
    return v, np.array(faces, np.int64)


def _rot_z(deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    return m


def _transform_points(m: np.ndarray, p: np.ndarray) -> np.ndarray:
    return p @ m[:3, :3].T + m[:3, 3]


def camera_frustum(pose: np.ndarray, scale: float) -> Tuple[np.ndarray, np.ndarray]:
    """integrate_camera_into_scene + generate_camera_mesh_faces (visual_util.py:471-613) -> (vertices [18,3] fp64, faces [48,3]): three
    layers of the pyramid (as is, x 0.95, rotated 2 degrees about z) of radius 0.05 scale and height 0.1 scale, moved by
    pose @ diag(1,-1,-1,1) @ Rz(45 degrees, tz = -height), so that the apex is the camera centre and the base corners are
    pose (+-r / sqrt 2, +-r / sqrt 2, +height); the sliver faces over the triangles that do not touch vertex 0, each also reversed."""
    r, h = float(scale) * 0.05, float(scale) * 0.1
    cone_v, cone_f = cone_pyramid(r, h)
    rz = _rot_z(45.0)
    rz[2, 3] = -h
    final = np.asarray(pose, np.float64) @ np.diag([1.0, -1.0, -1.0, 1.0]) @ rz
    layers = np.concatenate([cone_v, 0.95 * cone_v, _transform_points(_rot_z(2.0), cone_v)])
    verts = _transform_points(final, layers)
    n = len(cone_v)
    faces = []
    for tri in cone_f:
        if 0 in tri:
            continue
        a, b, c = (int(t) for t in tri)
        for k in (1, 2):
            a2, b2, c2 = a + k * n, b + k * n, c + k * n
            faces += [(a, b, b2), (a, a2, c), (c2, b, c)]
    faces += [(c, b, a) for a, b, c in faces]
    return verts, np.array(faces, np.int64)


# ---------------------------------------------------------------------------------------------- device side
def _gpu(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: pass tensors on a HIP device")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _u8mask(m: Optional[torch.Tensor], shape) -> Optional[torch.Tensor]:
    if m is None:
        return None
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"mask {tuple(m.shape)} does not match {tuple(shape)}")
    return (m != 0).to(torch.uint8).contiguous()


@dataclass
class ImageMesh:
    """What ``image_mesh`` returns.  The views' rows are concatenated, view-major: view i owns vertices
    [vertex_offsets[i], vertex_offsets[i + 1]) and faces [face_offsets[i], face_offsets[i + 1]); face indices are local to the view."""
    vertex_counts: List[int]
    face_counts: List[int]                 # triangles: two per valid quad
    vertices: torch.Tensor                 # [V,3] fp32, bit copies of the input points
    colors: torch.Tensor                   # [V,4] uint8 RGBA, alpha 255
    normals: Optional[torch.Tensor]        # [V,3] fp32 copies, when normals were given
    faces: torch.Tensor                    # [F,3] int32
    bounds: torch.Tensor                   # [S,6] fp32: min xyz, max xyz of each view's vertices
    buffer: torch.Tensor                   # the uint8 buffer the four arrays are views of: positions | colours | normals | faces

    @property
    def vertex_offsets(self) -> List[int]:
        return [0] + list(np.cumsum(self.vertex_counts))

    @property
    def face_offsets(self) -> List[int]:
        return [0] + list(np.cumsum(self.face_counts))

    def view(self, i: int):
        """(vertices, colors, normals or None, faces) of view i"""
        v0, v1 = self.vertex_offsets[i], self.vertex_offsets[i + 1]
        f0, f1 = self.face_offsets[i], self.face_offsets[i + 1]
        return self.vertices[v0:v1], self.colors[v0:v1], None if self.normals is None else self.normals[v0:v1], self.faces[f0:f1]


def image_mesh(points: torch.Tensor, colors: torch.Tensor, mask: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None) -> ImageMesh:
    """``create_image_mesh(points, colors[, normals], mask=mask, triangulate=True)`` (visual_util.py:109-205) for every view at once.
    points, colors (and normals) [S,H,W,3] fp32 on the GPU, mask [S,H,W] bool or None (every pixel).  A quad at pixel p = y W + x is valid
    when p, p + W, p + W + 1, p + 1 are all masked in; a pixel is a vertex when it is a corner of a valid quad; vertices in ascending pixel
    index, faces (a, b, c), (a, c, d) in raster order of the quads, indices local to the view.  Colours are uint8 RGBA by the reference's
    chain trunc(fl32(fl32(fl32(x 255) / 255) 255)).  Synchronises once, to size the output."""
    _gpu(points, "image_mesh")
    if points.dim() != 4 or points.shape[-1] != 3 or tuple(colors.shape) != tuple(points.shape):
        raise ValueError(f"points and colors must both be [S,H,W,3], got {tuple(points.shape)} and {tuple(colors.shape)}")
    dev = points.device
    S, H, W = (int(v) for v in points.shape[:3])
    for t in (colors, mask, normals):
        if t is not None:
            _gpu(t, "image_mesh")
    if normals is not None and tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f"normals {tuple(normals.shape)} do not match points {tuple(points.shape)}")
    p, c = _f32c(points), _f32c(colors)
    nrm = None if normals is None else _f32c(normals)
    m = _u8mask(mask, (S, H, W))
    L = _lib.lib()
    ws_bytes = L.wm_image_mesh_workspace_bytes(S, H, W)
    if ws_bytes == 0:
        raise ValueError(f"{S} views of {H} x {W} are outside what the library takes (S, H, W >= 1, S H W < 2^31)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    nv, nq = (C.c_int64 * (S + 1))(), (C.c_int64 * (S + 1))()
    with torch.cuda.device(dev):
        check(L.wm_image_mesh_count(ptr(m), S, H, W, ptr(ws), ws_bytes, nv, nq, stream(dev)), "wm_image_mesh_count")
        V, Q = int(nv[S]), int(nq[S])
        o_col = 12 * V
        o_nrm = o_col + 4 * V
        o_face = o_nrm + (12 * V if nrm is not None else 0)
        buf = torch.empty(o_face + 24 * Q, device=dev, dtype=torch.uint8)
        verts = buf[:o_col].view(torch.float32).reshape(V, 3)
        rgba = buf[o_col:o_nrm].reshape(V, 4)
        nout = buf[o_nrm:o_face].view(torch.float32).reshape(V, 3) if nrm is not None else None
        faces = buf[o_face:].view(torch.int32).reshape(2 * Q, 3)
        bounds = torch.empty((S, 6), device=dev, dtype=torch.float32)
        check(L.wm_image_mesh_pack(ptr(p), ptr(c), ptr(nrm), ptr(m), S, H, W, ptr(ws), ws_bytes, V, Q, ptr(verts) if V else None,
                                   ptr(rgba) if V else None, ptr(nout) if (V and nout is not None) else None, ptr(faces) if Q else None,
                                   ptr(bounds), stream(dev)), "wm_image_mesh_pack")
    return ImageMesh([int(nv[i]) for i in range(S)], [2 * int(nq[i]) for i in range(S)], verts, rgba, nout, faces, bounds, buf)


def pack_points(points: torch.Tensor, colors: torch.Tensor, mask: Optional[torch.Tensor] = None):
    """The point cloud of visual_util.py:274-298: the rows of points / colors [N,3] with mask set, in order ->
    (vertices [n,3] fp32, colors [n,4] uint8 = trunc(fl32(x 255)) with alpha 255, bounds [6] fp32, the uint8 buffer both are views of).
    N = 0 or nothing kept gives empty tensors.  Synchronises once."""
    _gpu(points, "pack_points")
    dev = points.device
    p, c = _f32c(points).reshape(-1, 3), _f32c(colors).reshape(-1, 3)
    N = int(p.shape[0])
    if c.shape[0] != N:
        raise ValueError(f"{N} points and {c.shape[0]} colours")
    m = _u8mask(None if mask is None else mask.reshape(-1), (N,))
    bounds = torch.empty((6,), device=dev, dtype=torch.float32)
    if N == 0:
        buf = torch.empty(0, device=dev, dtype=torch.uint8)
        return buf.view(torch.float32).reshape(0, 3), buf.reshape(0, 4), bounds, buf
    L = _lib.lib()
    ws_bytes = L.wm_glb_pack_points_workspace_bytes(N)
    if ws_bytes == 0:
        raise ValueError(f"{N} points are outside what the library takes (N < 2^31)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    buf = torch.empty(16 * N, device=dev, dtype=torch.uint8)
    n = C.c_int64(0)
    with torch.cuda.device(dev):
        check(L.wm_glb_pack_points(ptr(p), ptr(c), ptr(m), N, ptr(ws), ws_bytes, ptr(buf), 16 * N, C.byref(n), ptr(bounds), stream(dev)),
              "wm_glb_pack_points")
    n = int(n.value)
    buf = buf[:16 * n]
    return buf[:12 * n].view(torch.float32).reshape(n, 3), buf[12 * n:].reshape(n, 4), bounds, buf


def percentile_neighbours(points: torch.Tensor, mask: Optional[torch.Tensor], quantiles) -> Tuple[np.ndarray, int]:
    """For each column of points [N,3] and each quantile q in [0, 1]: the order statistics of rank floor((n - 1) q) and the next (clipped)
    among the n rows with mask set -> (fp32 array [3, len(quantiles), 2] on the host, n).  Exact (radix selection on the device); with
    n = 0 the array is NaN.  One small copy to the host."""
    _gpu(points, "percentile_neighbours")
    dev = points.device
    p = _f32c(points).reshape(-1, 3)
    N, nq = int(p.shape[0]), len(quantiles)
    m = _u8mask(None if mask is None else mask.reshape(-1), (N,))
    L = _lib.lib()
    ws_bytes = L.wm_masked_percentile_neighbours_workspace_bytes(N, nq)
    if ws_bytes == 0:
        raise ValueError(f"{N} points / {nq} quantiles are outside what the library takes (3 N < 2^31, 1 to 4 quantiles)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.full((3 * nq * 2 + 2,), float("nan"), device=dev, dtype=torch.float32)      # the values, then n as an int64 in the last two words
    q = (C.c_double * nq)(*[float(v) for v in quantiles])
    with torch.cuda.device(dev):
        check(L.wm_masked_percentile_neighbours(ptr(p), ptr(m), N, q, nq, ptr(ws), ws_bytes, ptr(out), ptr(out[3 * nq * 2:]), stream(dev)),
              "wm_masked_percentile_neighbours")
    host = out.cpu().numpy()
    n = int(host[3 * nq * 2:].view(np.int64)[0])
    return host[:3 * nq * 2].reshape(3, nq, 2).copy(), n


def percentile_scale(points: torch.Tensor, mask: Optional[torch.Tensor]) -> Tuple[float, int]:
    """visual_util.py:307-309: |percentile(p, 95, axis=0) - percentile(p, 5, axis=0)| over the masked rows, np.percentile's linear method:
    virtual index (n - 1) q in fp64, the two neighbouring order statistics from the device, the interpolation and the norm in fp64 on the
    host.  -> (scale, n); n = 0 gives the reference's scale 1."""
    qs = (0.05, 0.95)
    nb, n = percentile_neighbours(points, mask, qs)
    if n == 0:
        return 1.0, 0
    nb = nb.astype(np.float64)
    vals = []
    for j, q in enumerate(qs):
        pos = (n - 1) * q
        g = pos - math.floor(pos)
        vals.append(nb[:, j, 0] + (nb[:, j, 1] - nb[:, j, 0]) * g)
    return float(np.linalg.norm(vals[1] - vals[0])), n


# ---------------------------------------------------------------------------------------------- the scene
@dataclass
class GLBGeometry:
    """One geometry of a GLBScene.  kind "mesh" / "points": tensors on the device, views of the scene's packed BIN body.  kind "camera":
    host tensors (18 vertices and 48 faces in fp64 / int64, built on the host)."""
    kind: str
    vertices: torch.Tensor
    colors: torch.Tensor                       # [n,4] uint8
    faces: Optional[torch.Tensor] = None       # [f,3]; None for points
    normals: Optional[torch.Tensor] = None
    bounds: Optional[torch.Tensor] = None      # [6] min xyz, max xyz (device), for packed geometries
    frame: Optional[int] = None                # the view or camera it came from
    body_offsets: Optional[Dict[str, int]] = None      # byte offsets of its arrays in the scene's packed body


class GLBScene:
    """What convert_predictions_to_glb_scene returns.  ``geometry``: the records in the order the reference adds them (the point cloud or
    the views' meshes, then the cameras); ``transform``: the 4 x 4 fp64 scene transformation inv(pose[0]) @ diag(1,-1,-1,1), stored as the
    matrix of the one root node; ``scale``: the camera scale factor.  Vertices stay in world coordinates."""

    def __init__(self, geometry: List[GLBGeometry], transform: np.ndarray, scale: float, body: Optional[torch.Tensor] = None):
        self.geometry, self.transform, self.scale, self.body = geometry, np.asarray(transform, np.float64), float(scale), body

    def export(self, file_obj=None, file_type: str = "glb"):
        """glTF 2.0 binary.  file_obj: a path or a writable binary file, as trimesh's Scene.export takes it (app.py:540), or None, and then
        the bytes are returned.  The packed body is copied from the device once, straight into the file image; the camera solids and the
        JSON are added on the host."""
        if file_type != "glb":
            raise ValueError("only file_type='glb' is written")
        size = 0 if self.body is None else int(self.body.numel())
        assert size % 4 == 0
        packed = [g for g in self.geometry if g.body_offsets is not None]
        bounds = torch.stack([g.bounds for g in packed]).cpu().numpy().astype(np.float64) if packed else None
        chunks, prims, n_packed = [], [], 0
        for g in self.geometry:
            arrays = {}
            if g.body_offsets is not None:
                b = bounds[n_packed]
                n_packed += 1
                n = int(g.vertices.shape[0])
                arrays["POSITION"] = (g.body_offsets["POSITION"], n, 5126, "VEC3", (b[:3], b[3:]))
                arrays["COLOR_0"] = (g.body_offsets["COLOR_0"], n, 5121, "VEC4", None)
                if g.normals is not None:
                    arrays["NORMAL"] = (g.body_offsets["NORMAL"], n, 5126, "VEC3", None)
                if g.faces is not None:
                    arrays["indices"] = (g.body_offsets["indices"], 3 * int(g.faces.shape[0]), 5125, "SCALAR", None)
            else:
                host = {"POSITION": np.ascontiguousarray(g.vertices.cpu().numpy(), np.float32).reshape(-1, 3),
                        "COLOR_0": np.ascontiguousarray(g.colors.cpu().numpy(), np.uint8).reshape(-1, 4)}
                if g.normals is not None:
                    host["NORMAL"] = np.ascontiguousarray(g.normals.cpu().numpy(), np.float32).reshape(-1, 3)
                if g.faces is not None:
                    host["indices"] = np.ascontiguousarray(g.faces.cpu().numpy()).astype(np.uint32).reshape(-1)
                for k, a in host.items():
                    raw = a.tobytes()
                    raw += b"\0" * (-len(raw) % 4)
                    mm = (a.min(0).astype(np.float64), a.max(0).astype(np.float64)) if k == "POSITION" else None
                    ctype, typ = {"POSITION": (5126, "VEC3"), "COLOR_0": (5121, "VEC4"), "NORMAL": (5126, "VEC3"), "indices": (5125, "SCALAR")}[k]
                    arrays[k] = (size, a.shape[0], ctype, typ, mm)
                    chunks.append(raw)
                    size += len(raw)
            prims.append((g, arrays))
        data = _glb_container(_gltf_json(prims, self.transform, size), self.body, b"".join(chunks))
        if file_obj is None:
            return data.tobytes()
        if isinstance(file_obj, (str, os.PathLike)):
            with open(file_obj, "wb") as f:
                f.write(memoryview(data))
        else:
            file_obj.write(memoryview(data))
        return None


def _gltf_json(prims, transform: np.ndarray, bin_bytes: int) -> dict:
    views, accessors, meshes, nodes = [], [], [], []
    item = {5121: 1, 5125: 4, 5126: 4}
    for gi, (g, arrays) in enumerate(prims):
        idx = {}
        for k, (off, count, ctype, typ, mm) in arrays.items():
            assert off % 4 == 0
            views.append({"buffer": 0, "byteOffset": int(off), "byteLength": int(count * item[ctype] * _NCOMP[typ]),
                          "target": 34963 if k == "indices" else 34962})
            acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": int(count), "type": typ}
            if k == "COLOR_0":
                acc["normalized"] = True
            if mm is not None:
                acc["min"], acc["max"] = [float(v) for v in mm[0]], [float(v) for v in mm[1]]
            accessors.append(acc)
            idx[k] = len(accessors) - 1
        prim = {"attributes": {k: v for k, v in idx.items() if k != "indices"}, "mode": 0 if g.kind == "points" else 4}
        if "indices" in idx:
            prim["indices"] = idx["indices"]
        meshes.append({"name": f"{g.kind}_{gi}", "primitives": [prim]})
        nodes.append({"name": f"{g.kind}_{gi}", "mesh": gi})
    root = {"name": "world", "matrix": [float(v) for v in np.asarray(transform, np.float64).T.reshape(-1)]}      # column-major
    if nodes:
        root["children"] = list(range(1, len(nodes) + 1))
    gltf = {"asset": {"version": "2.0", "generator": "hunyuanworld-mirror_amd"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [root] + nodes}
    if meshes:
        gltf.update(meshes=meshes, accessors=accessors, bufferViews=views, buffers=[{"byteLength": int(bin_bytes)}])
    return gltf


def _glb_container(gltf: dict, body: Optional[torch.Tensor], tail: bytes) -> np.ndarray:
    """The file image as a uint8 array: 12-byte header, the JSON chunk padded with spaces to 4, one BIN chunk = the packed body (a uint8
    tensor, copied from its device straight into place) followed by `tail` (both multiples of 4 bytes)"""
    js = json.dumps(gltf, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    n_body = 0 if body is None else int(body.numel())
    n_bin = n_body + len(tail)
    assert n_bin % 4 == 0
    total = 12 + 8 + len(js) + (8 + n_bin if n_bin else 0)
    out = np.empty(total, np.uint8)
    head = struct.pack("<III", GLB_MAGIC, 2, total) + struct.pack("<II", len(js), GLB_JSON) + js
    if n_bin:
        head += struct.pack("<II", n_bin, GLB_BIN)
    out[:len(head)] = np.frombuffer(head, np.uint8)
    if n_body:
        torch.from_numpy(out[len(head):len(head) + n_body]).copy_(body.reshape(-1))
    if tail:
        out[len(head) + n_body:] = np.frombuffer(tail, np.uint8)
    return out


def glb_from_arrays(geometries, transform=None) -> bytes:
    """A GLB from host numpy arrays, through the same writer: geometries is a list of dicts with "kind" ("mesh" / "points" / "camera"),
    "vertices" [n,3], "colors" [n,4] uint8 and optionally "faces" [f,3], "normals" [n,3]."""
    recs = [GLBGeometry(g["kind"], torch.as_tensor(np.asarray(g["vertices"])), torch.as_tensor(np.asarray(g["colors"])),
                        None if g.get("faces") is None else torch.as_tensor(np.asarray(g["faces"])),
                        None if g.get("normals") is None else torch.as_tensor(np.asarray(g["normals"]))) for g in geometries]
    return GLBScene(recs, np.eye(4) if transform is None else transform, 1.0).export()


def load_glb(path_or_bytes) -> dict:
    """Reads a GLB written by ``GLBScene.export`` (host, numpy): {"json": the glTF document, "nodes": [{"name", "matrix" 4 x 4 fp64 or None,
    "mesh", "children"}], "primitives": [{"node", "mode", "positions", "colors", "normals", "indices"}] in node order}.  Accessors are read
    tightly packed (no byteStride, no sparse accessors)."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    data = bytes(data)
    magic, version, total = struct.unpack_from("<III", data, 0)
    if magic != GLB_MAGIC or version != 2 or total != len(data):
        raise ValueError("not a glTF 2.0 binary of the stated length")
    off, doc, body = 12, None, b""
    while off < total:
        n, kind = struct.unpack_from("<II", data, off)
        chunk = data[off + 8:off + 8 + n]
        if kind == GLB_JSON:
            doc = json.loads(chunk.decode("utf-8"))
        elif kind == GLB_BIN:
            body = chunk
        off += 8 + n
    if doc is None:
        raise ValueError("no JSON chunk")

    def read(i):
        if i is None:
            return None
        a = doc["accessors"][i]
        v = doc["bufferViews"][a["bufferView"]]
        if "byteStride" in v or "sparse" in a:
            raise ValueError("strided or sparse accessors are not read")
        dt, nc = _COMPONENT[a["componentType"]], _NCOMP[a["type"]]
        start = v.get("byteOffset", 0) + a.get("byteOffset", 0)
        arr = np.frombuffer(body, dtype=dt, count=a["count"] * nc, offset=start)
        return arr.reshape(a["count"], nc) if nc > 1 else arr

    nodes, prims = [], []
    for ni, nd in enumerate(doc.get("nodes", [])):
        mat = np.array(nd["matrix"], np.float64).reshape(4, 4).T if "matrix" in nd else None
        nodes.append({"name": nd.get("name"), "matrix": mat, "mesh": nd.get("mesh"), "children": nd.get("children", [])})
        if "mesh" in nd:
            for pr in doc["meshes"][nd["mesh"]]["primitives"]:
                at = pr["attributes"]
                idx = read(pr.get("indices"))
                prims.append({"node": ni, "mode": pr.get("mode", 4), "positions": read(at.get("POSITION")), "colors": read(at.get("COLOR_0")),
                              "normals": read(at.get("NORMAL")), "indices": None if idx is None else idx.reshape(-1, 3)})
    return {"json": doc, "nodes": nodes, "primitives": prims}


def _as_device(x, dev):
    if isinstance(x, torch.Tensor):
        return x if x.device.type == "cuda" else x.to(dev)
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def convert_predictions_to_glb_scene(predictions, filter_by_frames="all", show_camera=True, mask_sky_bg=False, mask_ambiguous=False,
                                     as_mesh=True) -> GLBScene:
    """visual_util.py:208-469 with the reference's signature.  predictions: "world_points" [S,H,W,3], "images" [S,H,W,3] or [S,3,H,W],
    "camera_poses" [S,4,4] or [S,3,4] (camera to world), and where the reference reads them "final_mask" / "sky_mask" [S,H,W] and
    "normal" [S,H,W,3]; torch tensors on the GPU or numpy arrays (uploaded once).

    Branch by branch as the reference: the frame selector ("3: name.png" -> frame 3, "all" / unparseable -> all); as_mesh=False: the flattened
    points kept by final_mask (mask_ambiguous) and sky_mask (mask_sky_bg), colours uint8(trunc(x 255)); several frames as meshes: one mesh per
    view under the same two flags; one frame as a mesh: the mask is final_mask of that frame whatever the flags say, and "normal" becomes
    NORMAL.  The scale is the norm of the difference of the per-axis 95th and 5th percentiles of the flag-filtered flattened points, in mesh
    mode too; no such point: one white point [1, 0, 0] and scale 1.  show_camera adds one solid per camera (camera_frustum), coloured
    int(255 gist_rainbow(i / S)).  The transform is inv(pose[0]) @ diag(1,-1,-1,1), pose[0] being the selected frame's in single-frame mode.

    predictions["images"] is not modified (the reference scales it by 255 in place on every mesh call); views without a valid quad are left
    out; see the module docstring for the other deliberate differences."""
    if not isinstance(predictions, dict):
        raise ValueError("predictions must be a dictionary")
    if "world_points" not in predictions:
        raise ValueError("world_points not found in predictions. Pointmap Branch requires 'world_points' key.")
    target = parse_frame_selector(filter_by_frames)
    wp = predictions["world_points"]
    dev = wp.device if isinstance(wp, torch.Tensor) and wp.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    single = target is not None
    sel = (lambda x: x[target][None]) if single else (lambda x: x)
    pts = _f32c(_as_device(sel(wp), dev))
    if pts.dim() != 4 or pts.shape[-1] != 3:
        raise ValueError(f"world_points must be [S,H,W,3], got {tuple(wp.shape)}")
    S, H, W = (int(v) for v in pts.shape[:3])
    img = _as_device(sel(predictions["images"]), dev)
    if img.dim() == 4 and img.shape[1] == 3:      # NCHW, the reference's test
        img = img.permute(0, 2, 3, 1)
    img = _f32c(img)
    if tuple(img.shape) != (S, H, W, 3):
        raise ValueError(f"images {tuple(img.shape)} do not match world_points {tuple(pts.shape)}")
    poses_in = sel(predictions["camera_poses"])
    poses_in = poses_in.detach().cpu().numpy() if isinstance(poses_in, torch.Tensor) else np.asarray(poses_in)
    poses = np.tile(np.eye(4), (poses_in.shape[0], 1, 1))
    poses[:, :poses_in.shape[1], :] = poses_in.astype(np.float64)
    need_final = mask_ambiguous or (as_mesh and single)
    final = _as_device(sel(predictions["final_mask"]), dev) != 0 if need_final else None
    sky = _as_device(sel(predictions["sky_mask"]), dev) != 0 if mask_sky_bg else None
    flag_mask = None
    if mask_ambiguous:
        flag_mask = final
    if mask_sky_bg:
        flag_mask = sky if flag_mask is None else flag_mask & sky
    if flag_mask is not None and tuple(flag_mask.shape) != (S, H, W):
        raise ValueError(f"masks {tuple(flag_mask.shape)} do not match world_points {tuple(pts.shape)}")

    geometry: List[GLBGeometry] = []
    body = None
    if as_mesh:
        scale, n_kept = percentile_scale(pts, flag_mask)
        nrm = None
        if single and predictions.get("normal") is not None:
            nrm = _f32c(_as_device(sel(predictions["normal"]), dev))
        mesh = image_mesh(pts, img, final if single else flag_mask, nrm)
        body = mesh.buffer
        V = int(mesh.vertices.shape[0])
        o_col, o_nrm = 12 * V, 16 * V
        o_face = o_nrm + (12 * V if nrm is not None else 0)
        for i in range(S):
            if mesh.vertex_counts[i] == 0:
                continue
            v, c, n_, f = mesh.view(i)
            v0, f0 = mesh.vertex_offsets[i], mesh.face_offsets[i]
            offs = {"POSITION": 12 * v0, "COLOR_0": o_col + 4 * v0, "indices": o_face + 12 * f0}
            if n_ is not None:
                offs["NORMAL"] = o_nrm + 12 * v0
            geometry.append(GLBGeometry("mesh", v, c, f, n_, mesh.bounds[i], target if single else i, offs))
    else:
        v, c, bounds, buf = pack_points(pts, img, flag_mask)
        n_kept = int(v.shape[0])
        if n_kept == 0:
            scale = 1.0
            geometry.append(GLBGeometry("points", torch.tensor([[1.0, 0.0, 0.0]], device=dev), torch.tensor([[255, 255, 255, 255]], dtype=torch.uint8, device=dev)))
        else:
            scale, _ = percentile_scale(pts, flag_mask)
            body = buf
            geometry.append(GLBGeometry("points", v, c, None, None, bounds, None, {"POSITION": 0, "COLOR_0": 12 * n_kept}))
    if show_camera:
        n_cam = poses.shape[0]
        for i in range(n_cam):
            verts, faces = camera_frustum(poses[i], scale)
            rgba = np.tile(np.array(camera_color(i, n_cam) + (255,), np.uint8), (verts.shape[0], 1))
            geometry.append(GLBGeometry("camera", torch.from_numpy(verts), torch.from_numpy(rgba), torch.from_numpy(faces), frame=target if single else i))
    transform = np.linalg.inv(poses[0]) @ np.diag([1.0, -1.0, -1.0, 1.0])
    return GLBScene(geometry, transform, scale, body)


def save_camera_params(extrinsics, intrinsics, target_dir) -> str:
    """src/utils/save_utils.py:16-50 (app.py:515): camera_params.json with num_cameras and, per camera, camera_id and the matrix as nested
    lists, indent 2.  Host only.  -> the path"""
    ext = extrinsics.detach().cpu().numpy() if isinstance(extrinsics, torch.Tensor) else np.asarray(extrinsics)
    intr = intrinsics.detach().cpu().numpy() if isinstance(intrinsics, torch.Tensor) else np.asarray(intrinsics)
    data = {"num_cameras": int(ext.shape[0]), "extrinsics": [], "intrinsics": []}
    for i in range(ext.shape[0]):
        data["extrinsics"].append({"camera_id": i, "matrix": ext[i].tolist()})
        data["intrinsics"].append({"camera_id": i, "matrix": intr[i].tolist()})
    path = os.path.join(target_dir, "camera_params.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
    return path
