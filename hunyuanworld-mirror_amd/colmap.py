"""The COLMAP half of the hand-off to the post-3DGS trainer: the reference's ``--save_colmap`` branch (infer.py:269-358 with
src/utils/build_pycolmap_recon.py) as ``colmap_points_from_depth`` + ``save_colmap``, the coloured point clouds ``save_scene_ply`` /
``save_points_ply`` (src/utils/save_utils.py:81-130), and the trainer's ``Parser`` (submodules/gsplat/examples/datasets/colmap.py:78-216,
262-273, 344-348) as ``load_colmap``.

The point selection and the per-point bodies of ``images.bin``, ``points3D.bin`` and the PLY files are produced on the device by
libwm_hip.so (csrc/colmap.hip) in the byte order of the files and copied to the host once per file; the headers, the per-image headers
and ``cameras.bin`` (a few dozen bytes per view) are written here.  There is no CPU path for them: tensors that are not on a HIP device
raise RuntimeError.  ``load_colmap`` is host numpy.

The record layouts are restated from COLMAP's published binary format (little-endian, no padding).  pycolmap is not a dependency and
was not available when this was written: byte parity with the files pycolmap itself writes is NOT pinned by any test (the same standing
as plyfile for ``save_gs_ply``); what is pinned is that an independent reader written from the format reads back the reference's
values (tests/test_colmap_gpu.py).

Where this differs from the reference, on purpose:
  * a view without a kept point is still written to ``images.bin``, with zero 2-D points.  The reference leaves such an image
    unregistered, and pycolmap then does not write it; the trainer needs its camera and pose.
  * colours are trunc(clamp(image, 0, 1) * 255); the reference does not clamp, and an out-of-range input is undefined there.
  * the camera-to-world pose used for unprojection is the rigid inverse [R^T | -R^T t] of the given world-to-camera pose, taken in fp64
    and rounded to fp32 once; the reference calls a general fp32 matrix inverse.  The two agree to fp32 rounding for a rotation matrix.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1}
# COLMAP's camera models by id: (name, number of parameters); only the two pinhole models are read
_MODEL_PARAMS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
POINT3D_BYTES, POINT2D_BYTES, PLY_ROW_BYTES = 59, 24, 15      # a points3D.bin record with one track element; an images.bin point; a PLY row
DEPTH_EPS = 1e-8                                               # depth_to_world_coords_points' default


def point_ply_header(num_rows: int) -> bytes:
    """The header plyfile writes for save_scene_ply / save_points_ply's vertex element (float x y z, uchar red green blue)."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {num_rows}", "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    return ("\n".join(lines) + "\n").encode()


def _on_one_gpu(tensors, what: str) -> torch.device:
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move the tensors to a HIP device")
    if any(t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f"{what}: the tensors are on different devices")
    return tensors[0].device


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _host(t: torch.Tensor, nbytes: int) -> np.ndarray:
    """The one device-to-host copy of a finished body."""
    return t[:nbytes].cpu().numpy()


def _w2c_4x4(extrinsics_w2c: torch.Tensor, S: int, what: str) -> torch.Tensor:
    """[S,3,4] or [S,4,4] -> [S,4,4] fp64 on the tensor's device, the last row (0, 0, 0, 1)"""
    if extrinsics_w2c.dim() != 3 or extrinsics_w2c.shape[0] != S or tuple(extrinsics_w2c.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{what}: extrinsics_w2c must be [{S}, 3, 4] or [{S}, 4, 4], got {tuple(extrinsics_w2c.shape)}")
    e = extrinsics_w2c.detach().to(torch.float64)[:, :3, :]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=e.device).expand(S, 1, 4)
    return torch.cat([e, bottom], dim=1)


def colmap_points_from_depth(depth: torch.Tensor, depth_conf: torch.Tensor, images: torch.Tensor, extrinsics_w2c: torch.Tensor,
                             intrinsics: torch.Tensor, conf_threshold_percent: float = 30.0,
                             out_size: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """infer.py:296-335: depth [S,H,W], depth_conf [S,H,W], images [S,3,H,W] in [0,1], extrinsics_w2c [S,3,4] or [S,4,4] (rigid),
    intrinsics [S,3,3] at H x W, out_size = (out_w, out_h) of the saved images (None: (W, H)) ->
    points [P,3] f32, colors [P,3] u8, xyf [P,3] i32 = (trunc(x out_w / W), trunc(y out_h / H), view), counts [S] i64, all on the device.

    A pixel is a candidate when depth > 1e-8; the candidates are ordered view-major and row-major inside a view; of the N_valid candidates
    the K = max(1, ceil(N_valid (100 - p) / 100)) highest confidences are kept (p <= 0: all), conf <= 1e-5 counting as -inf and ties at
    the K-th value going to the lowest candidate index.  The kept candidates keep their order; counts[i] of them belong to view i.  The
    call synchronises the stream once, to size its outputs.  No candidate at all returns empty tensors."""
    if depth.dim() != 3:
        raise ValueError(f"colmap_points_from_depth: depth must be [S, H, W], got {tuple(depth.shape)}")
    S, H, W = (int(v) for v in depth.shape)
    if S < 1 or H < 1 or W < 1:
        raise ValueError(f"colmap_points_from_depth: depth must hold at least one pixel, got {tuple(depth.shape)}")
    if tuple(depth_conf.shape) != (S, H, W):
        raise ValueError(f"colmap_points_from_depth: depth_conf must be [{S}, {H}, {W}], got {tuple(depth_conf.shape)}")
    if tuple(images.shape) != (S, 3, H, W):
        raise ValueError(f"colmap_points_from_depth: images must be [{S}, 3, {H}, {W}], got {tuple(images.shape)}")
    if tuple(intrinsics.shape) != (S, 3, 3):
        raise ValueError(f"colmap_points_from_depth: intrinsics must be [{S}, 3, 3], got {tuple(intrinsics.shape)}")
    out_w, out_h = (W, H) if out_size is None else _size2(out_size, "out_size")
    dev = _on_one_gpu([depth, depth_conf, images, extrinsics_w2c, intrinsics], "colmap_points_from_depth")
    w2c = _w2c_4x4(extrinsics_w2c, S, "colmap_points_from_depth")
    Rt = w2c[:, :3, :3].transpose(1, 2)
    c2w = w2c.clone()
    c2w[:, :3, :3] = Rt
    c2w[:, :3, 3] = -(Rt * w2c[:, None, :3, 3]).sum(-1)
    c2w = c2w.to(torch.float32).contiguous()
    d, cf, im, K = _f32(depth), _f32(depth_conf), _f32(images), _f32(intrinsics)
    L = _lib.lib()
    ws_bytes = L.wm_colmap_select_workspace_bytes(S, H, W)
    if ws_bytes == 0:
        raise ValueError(f"colmap_points_from_depth: {S} x {H} x {W} pixels are outside what the library indexes (2^31)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    n_kept, counts = C.c_int64(0), (C.c_int64 * S)()
    eps, pct = C.c_float(DEPTH_EPS), C.c_double(float(conf_threshold_percent))
    with torch.cuda.device(dev):
        check(L.wm_colmap_select(ptr(d), ptr(cf), S, H, W, eps, pct, ptr(ws), ws_bytes, C.byref(n_kept), counts, stream(dev)), "wm_colmap_select")
        P = int(n_kept.value)
        points = torch.empty((P, 3), device=dev, dtype=torch.float32)
        colors = torch.empty((P, 3), device=dev, dtype=torch.uint8)
        xyf = torch.empty((P, 3), device=dev, dtype=torch.int32)
        if P:
            check(L.wm_colmap_gather(ptr(d), ptr(cf), ptr(im), ptr(c2w), ptr(K), S, H, W, eps, C.c_double(out_w / W), C.c_double(out_h / H), ptr(ws),
                                     ws_bytes, P, ptr(points), ptr(colors), ptr(xyf), stream(dev)), "wm_colmap_gather")
    return points, colors, xyf, torch.tensor(list(counts), dtype=torch.int64, device=dev)


def _size2(v, name: str) -> Tuple[int, int]:
    try:
        a, b = v
        a, b = int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (width, height), got {v!r}") from None
    if a < 1 or b < 1:
        raise ValueError(f"{name} must be positive, got {v!r}")
    return a, b


def rotation_to_quaternion(R: np.ndarray) -> np.ndarray:
    """A 3 x 3 rotation (fp64) -> the unit quaternion (qw, qx, qy, qz), by the branch with the largest pivot; the sign is not pinned."""
    R = np.asarray(R, dtype=np.float64)
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(t))
    s = 2.0 * np.sqrt(max(1.0 + t[k], 1e-300))
    if k == 0:
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def quaternion_to_rotation(q: np.ndarray) -> np.ndarray:
    """(qw, qx, qy, qz) -> 3 x 3, the expression of the trainer's reader (no normalisation)"""
    w, x, y, z = (float(v) for v in q)
    return np.eye(3) + 2.0 * np.array([[-y * y - z * z, x * y - z * w, z * x + y * w],
                                       [x * y + z * w, -x * x - z * z, y * z - x * w],
                                       [z * x - y * w, y * z + x * w, -x * x - y * y]])


def camera_params(K: np.ndarray, camera_model: str) -> np.ndarray:
    """build_pycolmap_recon.py:5-18 on one fp32 intrinsic matrix -> the fp64 parameter list of cameras.bin.  The SIMPLE_PINHOLE focal is
    (fx + fy) / 2 in fp32, widened afterwards, as the reference's numpy takes it."""
    K = np.asarray(K, dtype=np.float32)
    if camera_model == "PINHOLE":
        p = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    elif camera_model == "SIMPLE_PINHOLE":
        p = np.array([(K[0, 0] + K[1, 1]) / np.float32(2), K[0, 2], K[1, 2]])
    else:
        raise ValueError(f"Unsupported camera model: {camera_model}")
    assert p.dtype == np.float32
    return p.astype(np.float64)


def _pack_point_ply(points: torch.Tensor, colors: torch.Tensor, keep: Optional[torch.Tensor], filter_finite: bool, what: str) -> Tuple[torch.Tensor, int]:
    """-> (the rows on the device, the number kept)"""
    dev = _on_one_gpu([points, colors] + ([] if keep is None else [keep]), what)
    N = int(points.shape[0])
    L = _lib.lib()
    ws_bytes = L.wm_pack_point_ply_workspace_bytes(N)
    if ws_bytes == 0:
        raise ValueError(f"{what}: {N} rows are outside what the library packs")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out_bytes = N * PLY_ROW_BYTES
    out = torch.empty(max(out_bytes, 4), device=dev, dtype=torch.uint8)
    n_kept = C.c_int64(0)
    with torch.cuda.device(dev):
        st = L.wm_pack_point_ply(ptr(points if N else None), ptr(colors if N else None), ptr(keep if N else None), int(bool(filter_finite)), N, ptr(ws),
                                 ws_bytes, ptr(out), out_bytes, C.byref(n_kept), stream(dev))
    check(st, "wm_pack_point_ply")
    return out, int(n_kept.value)


def _ply_inputs(points: torch.Tensor, colors: torch.Tensor, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if not isinstance(points, torch.Tensor) or not isinstance(colors, torch.Tensor):
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: pass tensors on a HIP device")
    if points.numel() % 3 or colors.numel() != points.numel():
        raise ValueError(f"{what}: points {tuple(points.shape)} and colours {tuple(colors.shape)} must both hold N x 3 values")
    return _f32(points).reshape(-1, 3), colors.detach().to(torch.uint8).reshape(-1, 3).contiguous()


def _write_point_ply(path, out: torch.Tensor, n: int) -> None:
    with open(os.fspath(path), "wb") as f:
        f.write(point_ply_header(n))
        f.write(memoryview(_host(out, n * PLY_ROW_BYTES)))


def save_points_ply(path, points: torch.Tensor, colors: torch.Tensor) -> None:
    """src/utils/save_utils.py save_points_ply on GPU tensors: every row of points [N,3] and colors [N,3] (cast to u8) as a binary
    little-endian PLY, float x y z and uchar red green blue."""
    p, c = _ply_inputs(points, colors, "save_points_ply")
    out, n = _pack_point_ply(p, c, None, False, "save_points_ply")
    _write_point_ply(path, out, n)


def save_scene_ply(path, points_xyz: torch.Tensor, point_colors: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> None:
    """src/utils/save_utils.py save_scene_ply on GPU tensors: without a mask the rows with a NaN or Inf coordinate are left out, with a
    mask its rows are kept; a result without rows is the single white point at the origin, as in the reference."""
    p, c = _ply_inputs(points_xyz, point_colors, "save_scene_ply")
    keep = None
    if valid_mask is not None:
        if valid_mask.numel() != p.shape[0]:
            raise ValueError(f"save_scene_ply: valid_mask holds {valid_mask.numel()} values for {p.shape[0]} points")
        keep = (valid_mask.detach().reshape(-1) != 0).contiguous()
    out, n = _pack_point_ply(p, c, keep, keep is None, "save_scene_ply")
    if n == 0:
        with open(os.fspath(path), "wb") as f:
            f.write(point_ply_header(1) + struct.pack("<3f3B", 0.0, 0.0, 0.0, 255, 255, 255))
        return
    _write_point_ply(path, out, n)


def save_colmap(sparse_dir, points: torch.Tensor, colors: torch.Tensor, xyf: torch.Tensor, counts: torch.Tensor, extrinsics_w2c: torch.Tensor,
                intrinsics_out: torch.Tensor, image_names: Sequence[str], image_size: Tuple[int, int], camera_model: str = "SIMPLE_PINHOLE",
                write_ply: bool = True) -> None:
    """infer.py:337-358 with build_pycolmap_reconstruction (one camera per image): ``cameras.bin``, ``images.bin``, ``points3D.bin`` and,
    with write_ply, ``points3D.ply`` under sparse_dir (created if missing).

    points [P,3] f32, colors [P,3] u8, xyf [P,3] i32 and counts [S] i64 as colmap_points_from_depth returns them (view-major, counts[i] points
    of view i); extrinsics_w2c [S,3,4] or [S,4,4]; intrinsics_out [S,3,3] at image_size = (out_w, out_h); image_names: S names.

    cameras.bin  u64 S | per view: u32 camera_id = i + 1, i32 model, u64 width, u64 height, the parameters as f64
                 (SIMPLE_PINHOLE: f = (fx + fy) / 2 taken in fp32, cx, cy; PINHOLE: fx, fy, cx, cy); another model raises ValueError
    images.bin   u64 S | per view: u32 image_id = i + 1, f64 qw qx qy qz (unit norm, from the rotation in fp64 on the host), f64 tx ty tz,
                 u32 camera_id, the name and a NUL, u64 counts[i], then per kept point f64 x, f64 y, u64 point3D_id
    points3D.bin u64 P | per point: u64 id = index + 1, 3 x f64 xyz, 3 x u8 rgb, f64 error = -1, u64 track length = 1, u32 image_id,
                 u32 point2D_idx (the index inside the view)
    A view without a kept point is written with zero 2-D points (the reference drops it; the trainer needs its camera).  The per-point
    bodies are packed on the device and copied once per file."""
    if camera_model not in CAMERA_MODELS:
        raise ValueError(f"Unsupported camera model: {camera_model}")
    out_w, out_h = _size2(image_size, "image_size")
    if counts.dim() != 1 or counts.shape[0] < 1:
        raise ValueError(f"save_colmap: counts must be [S], got {tuple(counts.shape)}")
    S = int(counts.shape[0])
    P = int(points.shape[0])
    if tuple(points.shape) != (P, 3) or tuple(colors.shape) != (P, 3) or tuple(xyf.shape) != (P, 3):
        raise ValueError(f"save_colmap: points {tuple(points.shape)}, colors {tuple(colors.shape)} and xyf {tuple(xyf.shape)} must all be [P, 3]")
    if tuple(intrinsics_out.shape) != (S, 3, 3):
        raise ValueError(f"save_colmap: intrinsics_out must be [{S}, 3, 3], got {tuple(intrinsics_out.shape)}")
    names = [os.fsencode(n) if not isinstance(n, bytes) else n for n in image_names]
    if len(names) != S or any(b"\0" in n or not n for n in names):
        raise ValueError(f"save_colmap: image_names must be {S} non-empty names without NUL")
    dev = _on_one_gpu([points, colors, xyf, counts], "save_colmap")
    w2c = _w2c_4x4(extrinsics_w2c, S, "save_colmap").cpu().numpy()
    K = intrinsics_out.detach().to(torch.float32).cpu().numpy()
    cnt = counts.detach().to(torch.int64).contiguous()
    cnt_h = cnt.cpu().numpy()
    if (cnt_h < 0).any() or int(cnt_h.sum()) != P:
        raise ValueError(f"save_colmap: counts sum to {int(cnt_h.sum())} for {P} points")
    pts, col, xy = _f32(points), colors.detach().to(torch.uint8).contiguous(), xyf.detach().to(torch.int32).contiguous()
    L = _lib.lib()
    ws_bytes = L.wm_colmap_pack_workspace_bytes(P, S)
    if ws_bytes == 0:
        raise ValueError(f"save_colmap: {P} points are outside what the library packs")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    b3 = torch.empty(max(P * POINT3D_BYTES, 8), device=dev, dtype=torch.uint8)
    b2 = torch.empty(max(P * POINT2D_BYTES, 8), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(L.wm_colmap_pack(ptr(pts), ptr(col), ptr(xy), ptr(cnt), S, P, ptr(ws), ws_bytes, ptr(b3), P * POINT3D_BYTES, ptr(b2),
                               P * POINT2D_BYTES, stream(dev)), "wm_colmap_pack")
    os.makedirs(os.fspath(sparse_dir), exist_ok=True)
    sparse_dir = os.fspath(sparse_dir)
    with open(os.path.join(sparse_dir, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", S))
        for i in range(S):
            prm = camera_params(K[i], camera_model)
            f.write(struct.pack("<IiQQ", i + 1, CAMERA_MODELS[camera_model], out_w, out_h) + prm.astype("<f8").tobytes())
    body2 = memoryview(_host(b2, P * POINT2D_BYTES))
    with open(os.path.join(sparse_dir, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", S))
        off = 0
        for i in range(S):
            q = rotation_to_quaternion(w2c[i, :3, :3])
            n = int(cnt_h[i])
            f.write(struct.pack("<I7dI", i + 1, *q, *w2c[i, :3, 3], i + 1) + names[i] + b"\0" + struct.pack("<Q", n))
            f.write(body2[off * POINT2D_BYTES:(off + n) * POINT2D_BYTES])
            off += n
    with open(os.path.join(sparse_dir, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", P))
        f.write(memoryview(_host(b3, P * POINT3D_BYTES)))
    if write_ply:
        save_points_ply(os.path.join(sparse_dir, "points3D.ply"), pts, col)


# ---------------------------------------------------------------------------------------------------------------- reading it back
class ColmapModel:
    """The fields of the trainer's Parser that come from the COLMAP model (datasets/colmap.py:248-260, 348), host numpy:

    image_names (sorted), camtoworlds [C,4,4] f64, camera_ids, Ks_dict {camera_id: 3 x 3 f64}, params_dict (empty arrays: pinhole only),
    imsize_dict {camera_id: (width, height)}, points [P,3] f32, points_err [P] f32, points_rgb [P,3] u8, point_indices {name: int32 indices,
    in the file order of the points}, transform (identity), scene_scale.  Beyond the Parser: Ks [C,3,3] (Ks_dict per image), visible() and to()."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def Ks(self):
        ks = [self.Ks_dict[c] for c in self.camera_ids]
        return torch.stack(ks) if ks and isinstance(ks[0], torch.Tensor) else np.stack(ks)

    def visible(self, device=None) -> torch.Tensor:
        """[C,P] bool: row i holds the points of image_names[i]'s list, the mask project_depth_points(..., visible=) takes"""
        Cn, P = len(self.image_names), int(self.points.shape[0])
        vis = np.zeros((Cn, P), dtype=bool)
        for i, name in enumerate(self.image_names):
            idx = self.point_indices.get(name)
            if idx is not None and len(idx):
                vis[i, np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64)] = True
        out = torch.from_numpy(vis)
        return out if device is None else out.to(device)

    def to(self, device) -> "ColmapModel":
        """The arrays as tensors on ``device``: camtoworlds and Ks_dict fp32, points fp32, points_err fp32, points_rgb u8, point_indices int32"""
        def t(a, dtype=None):
            a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            return a.to(device=device, dtype=dtype) if dtype else a.to(device)

        kw = dict(self.__dict__)
        kw["camtoworlds"] = t(self.camtoworlds, torch.float32)
        kw["Ks_dict"] = {k: t(v, torch.float32) for k, v in self.Ks_dict.items()}
        kw["points"], kw["points_err"], kw["points_rgb"] = t(self.points), t(self.points_err), t(self.points_rgb)
        kw["point_indices"] = {k: t(v) for k, v in self.point_indices.items()}
        return ColmapModel(**kw)


def _read_cameras(data: bytes, path: str) -> Dict[int, Tuple[int, int, int, np.ndarray]]:
    (n,), pos, cams = struct.unpack_from("<Q", data, 0), 8, {}
    for _ in range(n):
        cid, model, w, h = struct.unpack_from("<IiQQ", data, pos)
        pos += 24
        if model not in _MODEL_PARAMS:
            raise ValueError(f"{path}: unknown camera model id {model}")
        npar = _MODEL_PARAMS[model][1]
        cams[cid] = (model, w, h, np.frombuffer(data, dtype="<f8", count=npar, offset=pos).copy())
        pos += 8 * npar
    if pos != len(data):
        raise ValueError(f"{path}: {len(data) - pos} bytes behind the last camera")
    return cams


def _read_images(data: bytes, path: str):
    """-> [(image_id, q [4], t [3], camera_id, name)] in file order; the 2-D points are stepped over (the Parser takes the point lists
    from the tracks of points3D.bin), whatever their point3D ids, the invalid id (all ones) included"""
    (n,), pos, out = struct.unpack_from("<Q", data, 0), 8, []
    for _ in range(n):
        vals = struct.unpack_from("<I7dI", data, pos)
        pos += 64
        end = data.index(b"\0", pos)
        name = data[pos:end].decode()
        pos = end + 1
        (n2d,) = struct.unpack_from("<Q", data, pos)
        pos += 8 + POINT2D_BYTES * n2d
        if pos > len(data):
            raise ValueError(f"{path}: image {vals[0]} runs past the end of the file")
        out.append((vals[0], np.array(vals[1:5]), np.array(vals[5:8]), vals[8], name))
    if pos != len(data):
        raise ValueError(f"{path}: {len(data) - pos} bytes behind the last image")
    return out


def _points3d_fixed(data: bytes):
    """Every record of the same length (every track as long as the first): one strided structured read.  None when the file is not of
    that kind: the size does not divide, or the track-length column is not constant."""
    (n,) = struct.unpack_from("<Q", data, 0)
    if n == 0:
        return None
    if (len(data) - 8) % n or (len(data) - 8) // n < 51 or ((len(data) - 8) // n - 51) % 8:
        return None
    T = ((len(data) - 8) // n - 51) // 8
    dt = np.dtype([("id", "<u8"), ("xyz", "<f8", (3,)), ("rgb", "u1", (3,)), ("err", "<f8"), ("len", "<u8"), ("track", "<u4", (T, 2))])
    assert dt.itemsize == 51 + 8 * T
    rec = np.frombuffer(data, dtype=dt, count=n, offset=8)
    if not (rec["len"] == T).all():
        return None
    return rec["id"].copy(), rec["xyz"].copy(), rec["rgb"].copy(), rec["err"].copy(), np.full(n, T, dtype=np.int64), rec["track"].reshape(n * T, 2).copy()


def _points3d_walk(data: bytes, path: str):
    """Tracks of any length: one record after the other"""
    (n,), pos = struct.unpack_from("<Q", data, 0), 8
    head = np.dtype([("id", "<u8"), ("xyz", "<f8", (3,)), ("rgb", "u1", (3,)), ("err", "<f8"), ("len", "<u8")])
    ids, xyz, rgb, err, lens, tracks = np.empty(n, "<u8"), np.empty((n, 3)), np.empty((n, 3), np.uint8), np.empty(n), np.empty(n, np.int64), []
    for i in range(n):
        if pos + 51 > len(data):
            raise ValueError(f"{path}: point {i} runs past the end of the file")
        h = np.frombuffer(data, dtype=head, count=1, offset=pos)[0]
        T = int(h["len"])
        pos += 51
        if pos + 8 * T > len(data):
            raise ValueError(f"{path}: the track of point {i} runs past the end of the file")
        ids[i], xyz[i], rgb[i], err[i], lens[i] = h["id"], h["xyz"], h["rgb"], h["err"], T
        tracks.append(np.frombuffer(data, dtype="<u4", count=2 * T, offset=pos).reshape(T, 2))
        pos += 8 * T
    if pos != len(data):
        raise ValueError(f"{path}: {len(data) - pos} bytes behind the last point")
    return ids, xyz, rgb, err, lens, (np.concatenate(tracks) if tracks else np.empty((0, 2), "<u4"))


def read_points3d(path, force_walk: bool = False):
    """points3D.bin -> (ids [P] u64, xyz [P,3] f64, rgb [P,3] u8, errors [P] f64, track lengths [P], track elements [sum, 2] u32 =
    (image_id, point2D_idx) point after point).  The strided read when it applies, else (or with force_walk) the sequential walk."""
    with open(os.fspath(path), "rb") as f:
        data = f.read()
    if len(data) < 8:
        raise ValueError(f"{path}: not a points3D.bin")
    got = None if force_walk else _points3d_fixed(data)
    return got if got is not None else _points3d_walk(data, os.fspath(path))


def load_colmap(path, factor: int = 1, image_size: Optional[Tuple[int, int]] = None, device=None, normalize: bool = False,
                _force_walk: bool = False) -> ColmapModel:
    """The trainer's Parser on a binary COLMAP model: ``path`` is the data directory (its ``sparse/0`` or ``sparse`` is read, as the Parser
    looks for them) or the model directory itself.  ``factor`` divides the intrinsics and the sizes; ``image_size`` = (width, height) of
    the images actually used rescales them as the Parser does from the first image it loads (None: the sizes of the model).  ``device``:
    return ``.to(device)``.

    Not built, NotImplementedError: a camera model other than SIMPLE_PINHOLE / PINHOLE (the rasteriser is pinhole only),
    ``normalize=True``, and models with ``rigs.bin`` / ``frames.bin``."""
    if normalize:
        raise NotImplementedError("load_colmap: normalize=True (the world normalisation of the Parser) is not built")
    if int(factor) != factor or int(factor) < 1:
        raise ValueError(f"factor must be a positive integer, got {factor!r}")
    factor = int(factor)
    actual = None if image_size is None else _size2(image_size, "image_size")
    path = os.fspath(path)
    model_dir = next((d for d in (os.path.join(path, "sparse", "0"), os.path.join(path, "sparse"), path)
                      if os.path.exists(os.path.join(d, "cameras.bin"))), None)
    if model_dir is None:
        raise FileNotFoundError(f"no cameras.bin under {path}, {os.path.join(path, 'sparse')} or {os.path.join(path, 'sparse', '0')}")
    for extra in ("rigs.bin", "frames.bin"):
        if os.path.exists(os.path.join(model_dir, extra)):
            raise NotImplementedError(f"load_colmap: {extra} (the rig / frame model of newer COLMAP) is not read")

    def read(name):
        with open(os.path.join(model_dir, name), "rb") as f:
            return f.read()

    cams = _read_cameras(read("cameras.bin"), os.path.join(model_dir, "cameras.bin"))
    images = _read_images(read("images.bin"), os.path.join(model_dir, "images.bin"))
    if not images:
        raise ValueError("No images found in COLMAP.")
    bottom = np.array([0, 0, 0, 1]).reshape(1, 4)
    w2c_mats, camera_ids, Ks_dict, params_dict, imsize_dict = [], [], {}, {}, {}
    for _, q, t, cid, _ in images:
        w2c_mats.append(np.concatenate([np.concatenate([quaternion_to_rotation(q), t.reshape(3, 1)], 1), bottom], axis=0))
        camera_ids.append(cid)
        if cid not in cams:
            raise ValueError(f"{model_dir}: an image names camera {cid}, which cameras.bin does not hold")
        model, w, h, prm = cams[cid]
        if model not in (0, 1):
            raise NotImplementedError(f"load_colmap: camera model {_MODEL_PARAMS[model][0]} of camera {cid}: only SIMPLE_PINHOLE and PINHOLE are read")
        fx, fy, cx, cy = (prm[0], prm[0], prm[1], prm[2]) if model == 0 else prm
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        K[:2, :] /= factor
        Ks_dict[cid] = K
        params_dict[cid] = np.empty(0, dtype=np.float32)
        imsize_dict[cid] = (w // factor, h // factor)
    camtoworlds = np.linalg.inv(np.stack(w2c_mats, axis=0))
    image_names = [im[4] for im in images]
    inds = np.argsort(image_names)
    image_names = [image_names[i] for i in inds]
    camtoworlds = camtoworlds[inds]
    camera_ids = [camera_ids[i] for i in inds]

    ids, xyz, rgb, err, lens, tracks = read_points3d(os.path.join(model_dir, "points3D.bin"), force_walk=_force_walk)
    id_to_name = {im[0]: im[4] for im in images}
    point_idx = np.repeat(np.arange(len(ids), dtype=np.int64), lens)
    point_indices: Dict[str, np.ndarray] = {}
    if len(tracks):
        img_ids = tracks[:, 0].astype(np.int64)
        unknown = set(np.unique(img_ids).tolist()) - set(id_to_name)
        if unknown:
            raise ValueError(f"{model_dir}: points3D.bin names images {sorted(unknown)}, which images.bin does not hold")
        order = np.argsort(img_ids, kind="stable")      # per image, the points in file order
        bounds = np.flatnonzero(np.diff(img_ids[order])) + 1
        for run in np.split(order, bounds):
            point_indices[id_to_name[int(img_ids[run[0]])]] = point_idx[run].astype(np.int32)

    if actual is not None:
        colmap_width, colmap_height = imsize_dict[camera_ids[0]]
        s_height, s_width = actual[1] / colmap_height, actual[0] / colmap_width
        for cid, K in Ks_dict.items():
            K[0, :] *= s_width
            K[1, :] *= s_height
            width, height = imsize_dict[cid]
            imsize_dict[cid] = (int(width * s_width), int(height * s_height))
    camera_locations = camtoworlds[:, :3, 3]
    scene_center = np.mean(camera_locations, axis=0)
    scene_scale = float(np.max(np.linalg.norm(camera_locations - scene_center, axis=1)))
    model = ColmapModel(image_names=image_names, camtoworlds=camtoworlds, camera_ids=camera_ids, Ks_dict=Ks_dict, params_dict=params_dict,
                        imsize_dict=imsize_dict, points=xyz.astype(np.float32), points_err=err.astype(np.float32), points_rgb=rgb.astype(np.uint8),
                        point_indices=point_indices, transform=np.eye(4), scene_scale=scene_scale, model_dir=model_dir)
    return model if device is None else model.to(device)
