"""PNG compression of trained splats: ``gsplat.compression.PngCompression`` (submodules/gsplat/gsplat/compression/png_compression.py) as the
trainer's ``Runner.run_compression`` calls it (submodules/gsplat/examples/simple_trainer_worldmirror.py:1293-1307, ``compression = "png"``).

The reference quantises on the host with numpy, clusters the higher SH bands with torchpq (CUDA / cupy) and sorts with PLAS.  Here the min /
max reduction, the quantiser, both decoders, the L1 k-means and the grid sort run in libwm_hip.so (csrc/compress.hip); the host only writes
and reads the files (Pillow for the PNGs, numpy for the npz).  There is no CPU path: a tensor that is not on a HIP device raises RuntimeError.

Pinned to the reference: the file set and layout (``means_l.png`` / ``means_u.png``, ``scales.png``, ``quats.png``, ``opacities.png``,
``sh0.png``, ``shN.npz`` with ``centroids`` u8 and ``labels`` u16, ``<extra>.npz``, ``meta.json`` with ``shape`` / ``dtype`` / ``mins`` /
``maxs`` / ``quantization``), the quantiser's fp32 arithmetic and the fp64 decoders.  Not pinned, because torchpq and PLAS are not
available to compare against: the k-means semantics (stated at ``kmeans_l1``) and the sort (stated at ``sort_splats``)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

KMEANS_DIMS = (9, 24, 45)          # shN of SH degree 1, 2, 3, flattened
KMEANS_MAX_K = 65536
_PNG8 = ("scales", "quats", "opacities", "sh0")
_WHERE = "runs in libwm_hip.so on the GPU"


def log_transform(x: torch.Tensor) -> torch.Tensor:
    """gsplat/utils.py:136-137"""
    return torch.sign(x) * torch.log1p(torch.abs(x))


def inverse_log_transform(y: torch.Tensor) -> torch.Tensor:
    """gsplat/utils.py:140-141"""
    return torch.sign(y) * torch.expm1(torch.abs(y))


# ---------------------------------------------------------------- thin wrappers of the C ABI (no synchronisation in any of them)
def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _minmax(x2d: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    rows, ch = int(x2d.shape[0]), int(x2d.shape[1])
    L = _lib.lib()
    nbytes = L.wm_compress_minmax_workspace_bytes(rows, ch)
    if nbytes == 0:
        raise ValueError(f"compression: a field of {rows} rows x {ch} channels is outside what the library quantises (1..16 channels)")
    ws = torch.empty(nbytes, device=x2d.device, dtype=torch.uint8)
    mm = torch.empty(2 * ch, device=x2d.device, dtype=torch.float32)
    with torch.cuda.device(x2d.device):
        check(L.wm_compress_minmax(ptr(x2d), rows, ch, ptr(ws), nbytes, ptr(mm), ptr(flag), stream(x2d.device)), "wm_compress_minmax")
    return mm


def _quantise(x2d: torch.Tensor, mm: torch.Tensor, bits: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    rows, ch = int(x2d.shape[0]), int(x2d.shape[1])
    lo = torch.empty((rows, ch), device=x2d.device, dtype=torch.uint8)
    hi = torch.empty((rows, ch), device=x2d.device, dtype=torch.uint8) if bits > 8 else None
    with torch.cuda.device(x2d.device):
        check(_lib.lib().wm_compress_quantise(ptr(x2d), rows, ch, ptr(mm), bits, ptr(lo), ptr(hi), stream(x2d.device)), "wm_compress_quantise")
    return lo, hi


def _dequantise(lo: torch.Tensor, hi: Optional[torch.Tensor], mm: torch.Tensor, bits: int) -> torch.Tensor:
    rows, ch = int(lo.shape[0]), int(lo.shape[1])
    out = torch.empty((rows, ch), device=lo.device, dtype=torch.float32)
    with torch.cuda.device(lo.device):
        check(_lib.lib().wm_compress_dequantise(ptr(lo), ptr(hi), rows, ch, ptr(mm), bits, ptr(out), stream(lo.device)), "wm_compress_dequantise")
    return out


def _gather_rows(fields: List[torch.Tensor], idx: torch.Tensor) -> List[torch.Tensor]:
    """out[f][r] = fields[f][idx[r]] for contiguous fields; idx int32 on the device, every value a valid row (the callers build it)."""
    rows = int(idx.shape[0])
    outs = [torch.empty((rows,) + tuple(f.shape[1:]), device=f.device, dtype=f.dtype) for f in fields]
    live = [(f, o) for f, o in zip(fields, outs) if o.numel() > 0]
    L = _lib.lib()
    for at in range(0, len(live), 16):
        part = live[at:at + 16]
        n = len(part)
        src = (C.c_void_p * n)(*[f.data_ptr() for f, _ in part])
        dst = (C.c_void_p * n)(*[o.data_ptr() for _, o in part])
        rb = (C.c_int * n)(*[(f.numel() // f.shape[0]) * f.element_size() for f, _ in part])
        with torch.cuda.device(idx.device):
            check(L.wm_gather_rows(src, dst, rb, n, ptr(idx), rows, stream(idx.device)), "wm_gather_rows")
    return outs


def _to_host(tensors: List[torch.Tensor], dev) -> List[np.ndarray]:
    """Every tensor to pinned host memory on the current stream, then ONE stream synchronisation."""
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
    for h, t in zip(host, tensors):
        h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return [h.numpy() for h in host]


# ---------------------------------------------------------------- k-means
def _kmeans_check(x, n_clusters, max_iter, tol, init) -> Tuple[int, int, int]:
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"kmeans_l1 {_WHERE}: pass a tensor on a HIP device")
    if x.dim() != 2:
        raise ValueError(f"kmeans_l1: x must be [N, D], got {tuple(x.shape)}")
    N, D = int(x.shape[0]), int(x.shape[1])
    if N == 0:
        raise ValueError("kmeans_l1: no rows to cluster")
    if D not in KMEANS_DIMS:
        raise ValueError(f"kmeans_l1: D must be one of {KMEANS_DIMS} (the flattened shN of SH degree 1, 2, 3), got {D}")
    if int(n_clusters) != n_clusters or int(n_clusters) < 1:
        raise ValueError(f"kmeans_l1: n_clusters must be a positive integer, got {n_clusters!r}")
    K = min(int(n_clusters), N)
    if K > KMEANS_MAX_K:
        raise ValueError(f"kmeans_l1: at most {KMEANS_MAX_K} clusters (the labels are stored as uint16), got {K}")
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= 65536:
        raise ValueError(f"kmeans_l1: max_iter must be an integer in 1..65536, got {max_iter!r}")
    if not float(tol) >= 0.0:
        raise ValueError(f"kmeans_l1: tol must be >= 0, got {tol!r}")
    if N > 1 << 30:
        raise ValueError(f"kmeans_l1: {N} rows are outside what the library clusters (N <= 2^30)")
    if init is not None:
        if not isinstance(init, torch.Tensor) or init.dtype != torch.int64 or tuple(init.shape) != (K,):
            raise ValueError(f"kmeans_l1: init must be an int64 tensor of shape [{K}]")
    if x.device.type != "cuda":
        raise RuntimeError(f"kmeans_l1 {_WHERE}: move the tensor to a HIP device")
    return N, D, K


def _kmeans_launch(x: torch.Tensor, K: int, max_iter: int, tol: float, init: Optional[torch.Tensor], generator) -> Dict[str, torch.Tensor]:
    """Everything of kmeans_l1 up to the synchronisation: device tensors labels, labels_last (int32), centroids, errors [max_iter], info [2]."""
    dev = x.device
    N, D = int(x.shape[0]), int(x.shape[1])
    xs = _f32(x)
    if init is None:
        init = torch.randperm(N, generator=generator, device=generator.device if generator is not None else dev)[:K]
    init = init.to(dev).contiguous()
    L = _lib.lib()
    nbytes = L.wm_kmeans_l1_workspace_bytes(N, D, K)
    if nbytes == 0:
        raise ValueError(f"kmeans_l1: N = {N}, D = {D}, K = {K} are outside what the library clusters")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out = {"labels": torch.empty(N, device=dev, dtype=torch.int32), "labels_last": torch.empty(N, device=dev, dtype=torch.int32),
           "centroids": torch.empty((K, D), device=dev, dtype=torch.float32), "errors": torch.zeros(int(max_iter), device=dev, dtype=torch.float64),
           "info": torch.zeros(2, device=dev, dtype=torch.int32)}
    with torch.cuda.device(dev):
        check(L.wm_kmeans_l1(ptr(xs), N, D, K, ptr(init), int(max_iter), float(tol), ptr(ws), nbytes, ptr(out["labels"]), ptr(out["labels_last"]),
                             ptr(out["centroids"]), ptr(out["errors"]), ptr(out["info"]), stream(dev)), "wm_kmeans_l1")
    return out


def _assign(x: torch.Tensor, centroids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Step (1) of an iteration on its own: labels int32 [N] and fp32 distances [N] of x [N, D] against centroids [K, D], both contiguous
    fp32 on the same HIP device.  No synchronisation."""
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(centroids.shape[0])
    labels = torch.empty(N, device=x.device, dtype=torch.int32)
    dist = torch.empty(N, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(_lib.lib().wm_kmeans_l1_assign(ptr(x), N, D, ptr(centroids), K, ptr(labels), ptr(dist), stream(x.device)), "wm_kmeans_l1_assign")
    return labels, dist


def _kmeans_l1(x, n_clusters, *, max_iter=15, tol=1e-4, init=None, generator=None):
    """kmeans_l1 and, as a fourth value, the assignment of the last iteration (int64 [N]): the labels whose member means the centroids are."""
    N, D, K = _kmeans_check(x, n_clusters, max_iter, tol, init)
    out = _kmeans_launch(x, K, int(max_iter), float(tol), init, generator)
    iters, bad_init = (int(v) for v in out["info"].tolist())          # the one synchronisation
    if bad_init:
        raise ValueError(f"kmeans_l1: init holds a row outside 0..{N - 1}")
    return out["labels"].to(torch.int64), out["centroids"], out["errors"][:iters].clone(), out["labels_last"].to(torch.int64)


def kmeans_l1(x: torch.Tensor, n_clusters: int, *, max_iter: int = 15, tol: float = 1e-4, init: Optional[torch.Tensor] = None,
              generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Lloyd's k-means under Manhattan distance on x [N, D] (a HIP device, computed in fp32; D in 9, 24, 45) -> labels int64 [N], centroids
    fp32 [K, D], errors fp64 [iterations run].  It stands where ``torchpq.KMeans(distance="manhattan")`` stands in png_compression.py:361-365;
    torchpq cannot be run beside it, so the semantics are this library's own:

      K            min(n_clusters, N), at most 65536
      start        the rows ``init`` (int64 [K]) or ``torch.randperm(N, generator=generator)[:K]``
      iteration t  (1) every row goes to the centroid of least L1 distance (an fp32 sum over d = 0..D-1), ties to the lowest centroid index;
                   (2) errors[t] = the mean assigned distance; (3) every centroid with members becomes the mean of its members, a centroid
                   with none keeps its value
      stop         after max_iter iterations, or after an iteration t > 0 with |errors[t-1] - errors[t]| <= tol * errors[t-1]
      labels       one more assignment against the final centroids, so the returned labels belong to the returned centroids

    Deterministic: the member sums run in row order in fp64 (stable radix sort of (label, row), rounded once to fp32) and the error is a
    fixed-order fp64 reduction; there are no float atomics, so the same x and init give the same bits.  No [N, K] array exists; the
    workspace is 20 N + 4 K bytes.  The stop rule is evaluated on the device and the call synchronises once, at its end."""
    return _kmeans_l1(x, n_clusters, max_iter=max_iter, tol=tol, init=init, generator=generator)[:3]


# ---------------------------------------------------------------- the grid sort
def _grid_perm(means: torch.Tensor, n: int, flag: torch.Tensor) -> torch.Tensor:
    dev = means.device
    L = _lib.lib()
    nbytes = L.wm_grid_order_workspace_bytes(n)
    if nbytes == 0:
        raise ValueError(f"sort_splats: a grid of side {n} is outside what the library sorts (1..46340)")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    perm = torch.empty(n * n, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(L.wm_grid_order(ptr(means), n, ptr(ws), nbytes, ptr(perm), ptr(flag), stream(dev)), "wm_grid_order")
    return perm


def _check_fields(who: str, splats) -> Tuple[Dict[str, torch.Tensor], int, torch.device]:
    if not isinstance(splats, (Mapping, torch.nn.ParameterDict)):
        raise ValueError(f"{who}: splats must be a dict or ParameterDict of tensors")
    fields = {k: v for k, v in splats.items()}
    if "means" not in fields:
        raise ValueError(f"{who}: splats has no 'means'")
    for k, v in fields.items():
        if not isinstance(v, torch.Tensor):
            raise RuntimeError(f"{who} {_WHERE}: field {k!r} is not a tensor")
        if v.dim() < 1:
            raise ValueError(f"{who}: field {k!r} has no row dimension")
    N = int(fields["means"].shape[0])
    if N == 0:
        raise ValueError(f"{who}: no splats")
    for k, v in fields.items():
        if int(v.shape[0]) != N:
            raise ValueError(f"{who}: field {k!r} has {int(v.shape[0])} rows, means has {N}")
    if tuple(fields["means"].shape) != (N, 3):
        raise ValueError(f"{who}: means must be [N, 3], got {tuple(fields['means'].shape)}")
    dev = fields["means"].device
    for k, v in fields.items():
        if v.device.type != "cuda":
            raise RuntimeError(f"{who} {_WHERE}: move field {k!r} to a HIP device")
        if v.device != dev:
            raise ValueError(f"{who}: field {k!r} is on {v.device}, means on {dev}")
    return {k: v.detach() for k, v in fields.items()}, N, dev


def sort_splats(splats: Dict[str, torch.Tensor], verbose: bool = True) -> Dict[str, torch.Tensor]:
    """A new dict with every field's rows in grid order; N must be a square n^2 and row r = i * n + j of the result is cell (i, j) of the
    n x n images.  It stands where gsplat/compression/sort.py (sort_with_plas) stands in the reference.  PLAS is not built; the order
    here is this library's own and compresses less well than PLAS would:

      1. the 30-bit Morton code of ``splats["means"]`` (compress passes the log-transformed means), 10 bits per axis over the per-axis
         bounding box, floor((x - min) / (max - min) * 1024) held to 0..1023;
      2. a stable radix sort of those codes (equal codes stay in row order);
      3. the i-th splat of that order goes to the grid cell with the i-th smallest 2-D Morton code of (row, col), so that neighbours in
         space are neighbours in both image directions.

    Deterministic: no random shuffle.  The input is not modified.  A NaN or infinite mean raises ValueError (the one synchronisation)."""
    fields, N, dev = _check_fields("sort_splats", splats)
    n = math.isqrt(N)
    if n * n != N:
        raise ValueError(f"sort_splats: the number of splats must be a square, got {N}")
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    perm = _grid_perm(_f32(fields["means"]), n, flag)
    names = list(fields)
    outs = _gather_rows([fields[k].contiguous() for k in names], perm)
    if int(flag.item()):
        raise ValueError("sort_splats: means holds a NaN or infinite value")
    if verbose:
        print(f"sort_splats: {N} splats laid on a {n} x {n} grid in Morton order")
    return dict(zip(names, outs))


# ---------------------------------------------------------------- files
def _write_png(path: str, plane: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(plane[:, :, 0] if plane.shape[2] == 1 else plane).save(path)


def _read_png(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def _dtype_name(t: torch.Tensor) -> str:
    return str(t.dtype).split(".")[1]


class PngCompression:
    """gsplat.compression.PngCompression with the reference's two fields, ``use_sort`` and ``verbose``, and keyword-only ``n_clusters``
    (65536), ``quantization`` (6 bits for the centroids), ``max_iter`` (15), ``tol`` (1e-4) and ``generator`` for the k-means of ``shN``
    (png_compression.py:322-330 has the first two as arguments of ``_compress_kmeans``).

    ``use_sort=True`` means ``sort_splats`` of this module, a deterministic Morton grid order; PLAS is not built.

    Differences from the reference, all deliberate:
      * ``compress`` does not modify the caller's dict.  The reference overwrites ``splats["means"]`` with its log transform and
        ``splats["quats"]`` with the normalised quaternions (:84-85), a side effect on a live ParameterDict.
      * The crop to n^2 = int(N ** 0.5)^2 rows keeps the highest opacities in descending-opacity order, as
        ``argsort(descending=True)[:-n_crop]`` does; ties keep the lower row first (the reference's argsort is unstable, so its ties are
        not defined).  A square N is not cropped and keeps its order.
      * A field with zero elements (``shN`` [N, 0, 3] of a degree-0 model) writes no file, only ``shape`` / ``dtype`` in meta.json, and
        decodes to zeros of that shape.  The reference means to do this but tests ``torch.numel == 0``, which is never true, and its
        decoders return the meta dict.
      * A channel whose values are all equal encodes as code 0 and decodes to its minimum.  The reference computes 0 / 0.
      * The k-means is ``kmeans_l1`` of this module, not torchpq's.
    A NaN or infinite value in a quantised field (or in ``shN``) raises ValueError; it is read from a device flag at the call's one
    synchronisation, before any file is written."""

    def __init__(self, use_sort: bool = True, verbose: bool = True, *, n_clusters: int = 65536, quantization: int = 6, max_iter: int = 15,
                 tol: float = 1e-4, generator: Optional[torch.Generator] = None):
        if int(quantization) != quantization or not 1 <= int(quantization) <= 8:
            raise ValueError(f"PngCompression: quantization must be 1..8 bits (the centroids are stored as uint8), got {quantization!r}")
        self.use_sort, self.verbose = bool(use_sort), bool(verbose)
        self.n_clusters, self.quantization, self.max_iter, self.tol, self.generator = int(n_clusters), int(quantization), int(max_iter), float(tol), generator

    def compress(self, compress_dir: str, splats) -> None:
        """png_compression.py:75-111: ``splats`` is a dict or ParameterDict of tensors on a HIP device with pre-activation values: means
        [N,3], scales, quats, opacities, sh0, shN and any extra fields (extra fields go to ``np.savez_compressed``).  The caller's dict
        and tensors are NOT modified (the reference's are).  Every argument is checked before the first GPU call; the call launches
        everything, synchronises once, and then writes the files."""
        fields, N, dev = _check_fields("PngCompression.compress", splats)
        for k in ("quats", "opacities"):
            if k not in fields:
                raise ValueError(f"PngCompression.compress: splats has no {k!r}")
        if fields["opacities"].dim() != 1:
            raise ValueError(f"PngCompression.compress: opacities must be [N], got {tuple(fields['opacities'].shape)}")
        n = math.isqrt(N)
        for k in ("means",) + _PNG8:
            if k in fields and fields[k].numel() > 0:
                ch = fields[k].numel() // N
                if ch not in (1, 2, 3, 4):
                    raise ValueError(f"PngCompression.compress: {k!r} has {ch} values per splat; a PNG holds 1 to 4 channels")
        km = None
        if "shN" in fields and fields["shN"].numel() > 0:
            km = _kmeans_check(fields["shN"].reshape(N, -1)[:n * n], self.n_clusters, self.max_iter, self.tol, None)
        os.makedirs(compress_dir, exist_ok=True)

        # :84-85, on copies
        work = dict(fields)
        work["means"] = log_transform(_f32(fields["means"]))
        work["quats"] = torch.nn.functional.normalize(fields["quats"], dim=-1)
        work = {k: v.contiguous() for k, v in work.items()}
        names = list(work)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        if n * n != N:      # :88-94 and _crop_n_splats
            keep = torch.sort(work["opacities"], descending=True, stable=True).indices[:n * n].to(torch.int32)
            work = dict(zip(names, _gather_rows([work[k] for k in names], keep)))
            print(f"Warning: Number of Gaussians was not square. Removed {N - n * n} Gaussians.")
        if self.use_sort:
            perm = _grid_perm(work["means"], n, flag)
            work = dict(zip(names, _gather_rows([work[k] for k in names], perm)))

        meta, pending, jobs = {}, [], []      # jobs: (kind, name, indices into pending)
        for name in names:
            v = work[name]
            m = {"shape": list(v.shape), "dtype": _dtype_name(v)}
            meta[name] = m
            if name == "means" or name in _PNG8 or name == "shN":
                if v.numel() == 0:
                    continue
                x = _f32(v).reshape(n * n, -1)
                if name == "shN":
                    _minmax(x.reshape(-1, 1), flag)      # only for the flag
                    out = _kmeans_launch(x, km[2], self.max_iter, self.tol, None, self.generator)
                    cent = out["centroids"]
                    mm = _minmax(cent.reshape(-1, 1), flag)
                    codes, _ = _quantise(cent.reshape(-1, 1), mm, self.quantization)
                    jobs.append(("kmeans", name, len(pending)))
                    pending += [codes.reshape(cent.shape), out["labels"], mm, out["info"], out["errors"]]
                    m["quantization"] = self.quantization
                else:
                    bits = 16 if name == "means" else 8
                    mm = _minmax(x, flag)
                    lo, hi = _quantise(x, mm, bits)
                    jobs.append(("png16" if bits == 16 else "png8", name, len(pending)))
                    pending += [lo.reshape(n, n, -1), mm] + ([hi.reshape(n, n, -1)] if hi is not None else [])
            else:
                jobs.append(("npz", name, len(pending)))
                pending.append(v)
        host = _to_host(pending + [flag], dev)      # the one synchronisation
        if int(host[-1][0]):
            raise ValueError("PngCompression.compress: a quantised field holds a NaN or infinite value")

        for kind, name, at in jobs:
            m = meta[name]
            if kind == "npz":      # _compress_npz
                np.savez_compressed(os.path.join(compress_dir, f"{name}.npz"), arr=host[at])
                continue
            if kind == "kmeans":
                codes, labels, mm, info, errors = host[at:at + 5]
                if self.verbose:
                    print(f"kmeans_l1: {int(info[0])} iterations, mean L1 error {errors[:int(info[0])].tolist()}")
                np.savez_compressed(os.path.join(compress_dir, f"{name}.npz"), centroids=codes, labels=labels.astype(np.uint16))
                m["mins"], m["maxs"] = float(mm[0]), float(mm[1])
                continue
            mm = host[at + 1]
            ch = mm.shape[0] // 2
            m["mins"], m["maxs"] = mm[:ch].tolist(), mm[ch:].tolist()
            if kind == "png16":
                _write_png(os.path.join(compress_dir, f"{name}_l.png"), host[at])
                _write_png(os.path.join(compress_dir, f"{name}_u.png"), host[at + 2])
            else:
                _write_png(os.path.join(compress_dir, f"{name}.png"), host[at])
        for name in names:      # the reference's key order within a field
            m = meta[name]
            meta[name] = {k: m[k] for k in ("shape", "dtype", "mins", "maxs", "quantization") if k in m}
        with open(os.path.join(compress_dir, "meta.json"), "w") as f:
            json.dump(meta, f)

    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, torch.Tensor]:
        """png_compression.py:113-132: the dict of tensors on ``device`` (a HIP device), ``inverse_log_transform`` applied to the means.
        The decoders are the reference's fp64 arithmetic rounded once to the stored dtype's fp32; files written by the reference decode
        to the reference's values."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"PngCompression.decompress {_WHERE}: device must be a HIP device")
        with open(os.path.join(compress_dir, "meta.json")) as f:
            meta = json.load(f)
        splats = {}
        for name, m in meta.items():
            shape, dtype = [int(s) for s in m["shape"]], getattr(torch, m["dtype"])
            if name == "means" or name in _PNG8 or name == "shN":
                if not all(shape):
                    splats[name] = torch.zeros(shape, dtype=dtype, device=dev)
                    continue
            if name == "shN":
                z = np.load(os.path.join(compress_dir, f"{name}.npz"))
                codes, labels = np.ascontiguousarray(z["centroids"], dtype=np.uint8), z["labels"].astype(np.int32).reshape(-1)
                if codes.ndim != 2 or labels.size == 0 or int(labels.max()) >= codes.shape[0]:
                    raise ValueError(f"{name}.npz: labels reach {int(labels.max()) if labels.size else None}, the table has {codes.shape[0]} centroids")
                bits = int(m["quantization"])
                if not 1 <= bits <= 8:
                    raise ValueError(f"meta.json: {name} quantization {bits} is outside 1..8 bits")
                mm = torch.tensor([float(m["mins"]), float(m["maxs"])], dtype=torch.float32, device=dev)
                table = _dequantise(torch.from_numpy(codes).to(dev).reshape(-1, 1), None, mm, bits)
                rows = _gather_rows([table.reshape(codes.shape)], torch.from_numpy(labels).to(dev))[0]
                splats[name] = rows.reshape(shape).to(dtype)
            elif name == "means" or name in _PNG8:
                mins, maxs = np.atleast_1d(m["mins"]), np.atleast_1d(m["maxs"])
                mm = torch.tensor(np.concatenate([mins, maxs]), dtype=torch.float32, device=dev)
                ch = len(mins)
                if name == "means":
                    lo = _read_png(os.path.join(compress_dir, f"{name}_l.png"))
                    hi = _read_png(os.path.join(compress_dir, f"{name}_u.png"))
                    lo_d, hi_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev).reshape(-1, ch) for a in (lo, hi))
                    grid = _dequantise(lo_d, hi_d, mm, 16)
                else:
                    img = _read_png(os.path.join(compress_dir, f"{name}.png"))
                    grid = _dequantise(torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)).to(dev).reshape(-1, ch), None, mm, 8)
                splats[name] = grid.reshape(shape).to(dtype)
            else:      # _decompress_npz
                arr = np.load(os.path.join(compress_dir, f"{name}.npz"))["arr"]
                splats[name] = torch.from_numpy(arr).to(dev).reshape(shape).to(dtype)
        splats["means"] = inverse_log_transform(splats["means"])
        return splats
