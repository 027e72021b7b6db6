"""Writing splats out and reading them back: gsplat's ``export_splats`` (gsplat/exporter.py:475-553), the feed-forward hand-off file
``save_gs_ply`` (src/utils/save_utils.py:133-188), the trainer's ``load_gaussian_ply`` (examples/simple_trainer_worldmirror.py:239-277)
and the ``ffgs`` branch of its ``create_splats_with_optimizers`` (:310-372) as ``splats_from_ply``.

The file BODY is produced on the device by libwm_hip.so (csrc/export.hip) in the byte order of the file and copied to the host once;
this module writes the text header in front of it.  There is no CPU path: tensors that are not on a HIP device raise RuntimeError.

Where the reference leaves the result undefined it is defined (include/wm_hip.h): a chunk of ``ply_compressed`` whose minimum equals its
maximum packs that field as 0, an export that keeps no row gives a valid file with zero elements, and a row with a non-finite opacity
is dropped on its own (the reference drops every row).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

FORMATS = {"ply": 0, "splat": 1, "ply_compressed": 2}
CHUNK_PROPERTIES = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x",
                    "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b")
VERTEX_PROPERTIES = ("packed_position", "packed_rotation", "packed_scale", "packed_color")
GS_PLY_ATTRIBUTES = ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                     "rot_0", "rot_1", "rot_2", "rot_3")
OPACITY_THRESHOLD = 1 / 255          # splat2ply_bytes_compressed's default; export_splats never passes another


def ply_header(num_splats: int, K: int) -> bytes:
    """Header of format "ply" (gsplat/exporter.py:388-404) for K higher-order coefficients per channel."""
    names = ["x", "y", "z"] + [f"f_dc_{j}" for j in range(3)] + [f"f_rest_{j}" for j in range(3 * K)] + ["opacity"]
    names += [f"scale_{j}" for j in range(3)] + [f"rot_{j}" for j in range(4)]
    return float_ply_header(num_splats, names)


def float_ply_header(num_rows: int, names) -> bytes:
    """A binary little-endian PLY header with one element, vertex, of float properties."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {num_rows}"] + [f"property float {n}" for n in names] + ["end_header"]
    return ("\n".join(lines) + "\n").encode()


def ply_compressed_header(num_splats: int, K: int) -> bytes:
    """Header of format "ply_compressed" (gsplat/exporter.py:263-275)."""
    n_chunks = num_splats // 256 + (num_splats % 256 != 0)
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {n_chunks}"] + [f"property float {p}" for p in CHUNK_PROPERTIES]
    lines += [f"element vertex {num_splats}"] + [f"property uint {p}" for p in VERTEX_PROPERTIES]
    lines += [f"element sh {num_splats}"] + [f"property uchar f_rest_{j}" for j in range(3 * K)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode()


def _on_one_gpu(tensors, what: str) -> torch.device:
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move the tensors to a HIP device")
    if any(t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f"{what}: the tensors are on different devices")
    return tensors[0].device


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _body(out: torch.Tensor, nbytes: int) -> bytes:
    """The one device-to-host copy of the finished body."""
    return out[:nbytes].cpu().numpy().tobytes()


def export_splats(means: torch.Tensor, scales: torch.Tensor, quats: torch.Tensor, opacities: torch.Tensor, sh0: torch.Tensor,
                  shN: torch.Tensor, format: str = "ply", save_to: Optional[str] = None) -> bytes:
    """gsplat.export_splats: means [N,3], scales [N,3] (log), quats [N,4], opacities [N] (logit), sh0 [N,1,3], shN [N,K,3] on the GPU ->
    the bytes of a "ply", "splat" or "ply_compressed" file, also written to ``save_to`` when given.  Rows with a NaN or Inf anywhere are
    left out; "ply_compressed" also leaves out rows with sigmoid(opacity) <= 1 / 255; "splat" and "ply_compressed" are in Morton order."""
    total_splats = means.shape[0]
    assert means.shape == (total_splats, 3), "Means must be of shape (N, 3)"
    assert scales.shape == (total_splats, 3), "Scales must be of shape (N, 3)"
    assert quats.shape == (total_splats, 4), "Quaternions must be of shape (N, 4)"
    assert opacities.shape == (total_splats,), "Opacities must be of shape (N,)"
    assert sh0.shape == (total_splats, 1, 3), "sh0 must be of shape (N, 1, 3)"
    assert shN.ndim == 3 and shN.shape[0] == total_splats and shN.shape[2] == 3, f"shN must be of shape (N, K, 3), got {shN.shape}"
    if format not in FORMATS:
        raise ValueError(f"Unsupported format: {format}")
    K = int(shN.shape[1])
    if K > 15:
        raise ValueError(f"shN holds {K} coefficients per channel; at most 15 (degree 3) are exported")
    dev = _on_one_gpu([means, scales, quats, opacities, sh0, shN], "export_splats")
    fmt, N = FORMATS[format], int(total_splats)
    L = _lib.lib()
    t = [_f32(x) for x in (means, scales, quats, opacities, sh0, shN)]
    ws_bytes = L.wm_export_splats_workspace_bytes(N, K, fmt)
    out_bytes = L.wm_export_splats_payload_bytes(N, K, fmt)
    if ws_bytes == 0:
        raise ValueError(f"export_splats: {N} splats with K = {K} are outside what the library exports")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.empty(max(out_bytes, 1), device=dev, dtype=torch.uint8)
    n_kept = C.c_int(0)
    with torch.cuda.device(dev):
        st = L.wm_export_splats(*[ptr(x if x.numel() else None) for x in t], N, K, fmt, OPACITY_THRESHOLD, ptr(ws), ws_bytes, ptr(out), out_bytes,
                                C.byref(n_kept), stream(dev))
    check(st, "wm_export_splats")
    n = int(n_kept.value)
    header = {"ply": ply_header, "ply_compressed": ply_compressed_header}.get(format, lambda n_, k_: b"")(n, K)
    data = header + _body(out, L.wm_export_splats_payload_bytes(n, K, fmt))
    if save_to:
        with open(save_to, "wb") as f:
            f.write(data)
    return data


def _pack_rows(columns, keep: Optional[torch.Tensor], N: int, dev: torch.device) -> Tuple[torch.Tensor, int]:
    """columns: (tensor or None, element offset, row stride in elements, transform) -> (out bytes tensor on the device, rows kept)"""
    L = _lib.lib()
    n_cols = len(columns)
    ptrs = (C.c_void_p * n_cols)(*[None if c[0] is None else c[0].data_ptr() + 4 * c[1] for c in columns])
    strides = (C.c_int * n_cols)(*[c[2] for c in columns])
    xfs = (C.c_int * n_cols)(*[c[3] for c in columns])
    ws_bytes = L.wm_pack_rows_workspace_bytes(N)
    if ws_bytes == 0:
        raise ValueError(f"{N} rows are outside what the library packs")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out_bytes = N * n_cols * 4
    out = torch.empty(max(out_bytes, 4), device=dev, dtype=torch.uint8)
    n_kept = C.c_int(0)
    with torch.cuda.device(dev):
        st = L.wm_pack_rows(ptrs, strides, xfs, n_cols, ptr(keep if N else None), N, ptr(ws), ws_bytes, ptr(out), out_bytes, C.byref(n_kept),
                            stream(dev))
    check(st, "wm_pack_rows")
    return out, int(n_kept.value)


def save_gs_ply(path, means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, rgbs: torch.Tensor,
                opacities: torch.Tensor) -> None:
    """src/utils/save_utils.py save_gs_ply: the splats of a forward pass (scales linear, opacities as probabilities, rgbs the degree-0
    coefficients) to the PLY the trainer starts from.  Rows whose largest scale exceeds the 0.95 quantile of the largest scales are left
    out; columns x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3 with zero normals and log scales."""
    dev = _on_one_gpu([means, scales, rotations, rgbs, opacities], "save_gs_ply")
    m, s, q, c, o = (_f32(x.reshape(-1, d) if d else x.reshape(-1)) for x, d in ((means, 3), (scales, 3), (rotations, 4), (rgbs, 3), (opacities, 0)))
    N = int(m.shape[0])
    if not (s.shape[0] == q.shape[0] == c.shape[0] == o.shape[0] == N):
        raise ValueError("save_gs_ply: the tensors hold different numbers of splats")
    if N:
        largest = s.max(dim=-1)[0]
        keep = (largest <= torch.quantile(largest, 0.95, dim=0)).contiguous()
    else:
        keep = None
    NONE, LOG = 0, 1
    cols = [(m, j, 3, NONE) for j in range(3)] + [(None, 0, 0, NONE)] * 3 + [(c, j, 3, NONE) for j in range(3)] + [(o, 0, 1, NONE)]
    cols += [(s, j, 3, LOG) for j in range(3)] + [(q, j, 4, NONE) for j in range(4)]
    out, n = _pack_rows(cols, keep, N, dev)
    with open(os.fspath(path), "wb") as f:
        f.write(float_ply_header(n, GS_PLY_ATTRIBUTES) + _body(out, n * len(cols) * 4))


def _read_float_ply(path) -> Tuple[Dict[str, int], np.ndarray]:
    """A binary little-endian PLY whose first element is `vertex` with float properties only -> ({name: column}, rows [N, columns])"""
    with open(os.fspath(path), "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")[1:]
    body = end + len(b"end_header\n")
    if not lines or lines[0].split() != ["format", "binary_little_endian", "1.0"]:
        raise ValueError(f"{path}: only binary little-endian PLY files are read")
    count, names, in_vertex, seen = None, [], False, False
    for line in lines[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "element":
            if seen:
                break          # elements behind `vertex` are not looked at
            if w[1] != "vertex":
                raise ValueError(f"{path}: the first element must be `vertex`, found `{w[1]}`")
            count, in_vertex, seen = int(w[2]), True, True
        elif w[0] == "property" and in_vertex:
            if len(w) != 3 or w[1] not in ("float", "float32"):
                raise ValueError(f"{path}: vertex property `{' '.join(w[1:])}` is not a float")
            names.append(w[2])
    if count is None:
        raise ValueError(f"{path}: no `vertex` element")
    need = count * len(names) * 4
    if len(data) - body < need:
        raise ValueError(f"{path}: the body holds {len(data) - body} bytes, {count} vertices of {len(names)} floats need {need}")
    rows = np.frombuffer(data, dtype="<f4", count=count * len(names), offset=body).reshape(count, len(names))
    return {n: j for j, n in enumerate(names)}, rows


def load_gaussian_ply(ply_path) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The trainer's load_gaussian_ply: (positions [N,3], sh_features [N,3] = f_dc_*, opacity [N], scales [N,3], rotations [N,4]) as
    stored, fp32 on the host.  Reads what save_gs_ply and export_splats(format="ply") write, and any binary little-endian PLY whose vertex
    properties are all float, in any order and with any further columns."""
    col, rows = _read_float_ply(ply_path)
    rows = torch.from_numpy(rows.astype(np.float32))          # (a copy: the buffer of the file is read-only)

    def take(*names):
        missing = [n for n in names if n not in col]
        if missing:
            raise ValueError(f"{ply_path}: no vertex property {missing}")
        return rows[:, [col[n] for n in names]].contiguous()

    return (take("x", "y", "z"), take("f_dc_0", "f_dc_1", "f_dc_2"), take("opacity")[:, 0].contiguous(),
            take("scale_0", "scale_1", "scale_2"), take("rot_0", "rot_1", "rot_2", "rot_3"))


def splats_from_ply(ply_path, sh_degree: int = 0, opacity: str = "probability", device="cuda") -> Dict[str, torch.Tensor]:
    """The `ffgs` initialisation of the trainer's create_splats_with_optimizers: a PLY of load_gaussian_ply's kind -> the parameter
    tensors means [N,3], scales [N,3] (log, as stored), quats [N,4], opacities [N] (logit), sh0 [N,1,3], shN [N,(L+1)^2-1,3] (zeros) on
    ``device``.  opacity="probability" (a save_gs_ply file) converts with logit(clamp(p, 1e-6, 1 - 1e-6)); opacity="logit" (an
    export_splats file) takes the stored values."""
    if opacity not in ("probability", "logit"):
        raise ValueError(f"opacity must be 'probability' or 'logit', got {opacity!r}")
    if int(sh_degree) < 0:
        raise ValueError(f"sh_degree must be >= 0, got {sh_degree}")
    positions, sh_features, opac, scales, quats = load_gaussian_ply(ply_path)
    if opacity == "probability":
        opac = torch.logit(torch.clamp(opac, 1e-6, 1 - 1e-6))
    N = positions.shape[0]
    colors = torch.zeros((N, (int(sh_degree) + 1) ** 2, 3))
    colors[:, 0, :] = sh_features
    out = {"means": positions, "scales": scales, "quats": quats, "opacities": opac, "sh0": colors[:, :1, :].contiguous(),
           "shN": colors[:, 1:, :].contiguous()}
    return {k: v.to(device) for k, v in out.items()}


def process_ply_to_splat(*args, **kwargs):
    """The demo's own `.splat` writer orders the records by importance (size x opacity), not by Morton code; it is not built.
    export_splats(format="splat") writes gsplat's `.splat`."""
    raise NotImplementedError("process_ply_to_splat (importance-ordered .splat of the demo) is not built; "
                              "use export_splats(..., format='splat') for gsplat's Morton-ordered .splat")
