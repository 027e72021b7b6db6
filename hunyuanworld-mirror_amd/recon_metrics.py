"""Point-cloud evaluation of a reconstruction on the GPU: accuracy / completeness, normal consistency, Umeyama alignment and ICP.

The reference's README reports accuracy and completeness on 7-Scenes, NRGBD and DTU, but its evaluation code is not released (the
"Evaluation Code" box of its README is unticked), so the semantics here are this library's own.  They follow the protocol the DUSt3R /
Spann3R line of work uses for multi-view reconstruction (mv-recon): the valid pixels of the predicted and the ground-truth point maps,
a Sim(3) alignment by Umeyama's closed form on the pixel correspondences, a point-to-point ICP refinement, then

    accuracy       the mean (and median) distance from every predicted point to its nearest ground-truth point
    completeness   the same from every ground-truth point to its nearest predicted point
    normal consistency   the mean (and median) of |n_a . n_b| over the same nearest pairs, the ABSOLUTE dot product (the sign of an
                   estimated normal carries no information)

The host-side form of this runs on a kd-tree and takes minutes per scene.  Here the nearest-point search is an exact, deterministic
Morton-cell index in libwm_hip.so (csrc/knn.hip: built once over a cloud, queried many times, ICP asks it every iteration) and the
reductions are fp64 sums in a fixed order and exact order statistics (csrc/reconmetrics.hip), so a result is reproducible to the bit.
There is no CPU path: a tensor that is not on a HIP device raises RuntimeError.

Not built: dataset loaders, pose AUC, depth metrics, normal estimation from points, point-to-plane ICP.  Parity with Open3D's ICP and
with any released evaluation script is not pinned: neither was available to compare against."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream

MAX_THRESHOLDS = 16          # include/wm_hip.h WM_STATS_MAX_THRESHOLDS
ALIGN_MODES = ("umeyama+icp", "umeyama", "none")
Transform = Tuple[torch.Tensor, torch.Tensor, torch.Tensor]


def _cloud(x, name: str, what: str, rows: Optional[int] = None, min_rows: int = 0, device: bool = True) -> None:
    """the checks every [N,3] argument gets, in front of the first GPU call; device=False leaves the device to a later _on_gpu, so that a
    call with several arguments refuses a wrong shape or option before it refuses a CPU tensor"""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: {name} must be a tensor on a HIP device")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what}: {name} must be [N, 3], got {tuple(x.shape)}")
    if rows is not None and int(x.shape[0]) != rows:
        raise ValueError(f"{what}: {name} has {int(x.shape[0])} rows, expected {rows}")
    if int(x.shape[0]) < min_rows:
        raise ValueError(f"{what}: {name} needs at least {min_rows} row(s), got {int(x.shape[0])}")
    if int(x.shape[0]) >= 2 ** 31:
        raise ValueError(f"{what}: {name} has {int(x.shape[0])} rows; the library searches fewer than 2^31")
    if device:
        _on_gpu(x, name, what)


def _on_gpu(x, name: str, what: str) -> None:
    if x.device.type != "cuda":
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move {name} to a HIP device")


def _same_device(dev, x, name: str, what: str) -> None:
    if x.device != dev:
        raise RuntimeError(f"{what}: {name} is on {x.device}, expected {dev}")


def _f32(x: torch.Tensor) -> torch.Tensor:
    return x.detach().to(torch.float32).contiguous()


def _thresholds(thresholds, what: str) -> Tuple[float, ...]:
    taus = tuple(float(t) for t in thresholds)
    if len(taus) > MAX_THRESHOLDS:
        raise ValueError(f"{what}: at most {MAX_THRESHOLDS} thresholds, got {len(taus)}")
    if any(not t > 0.0 or t == float("inf") for t in taus):
        raise ValueError(f"{what}: thresholds must be positive and finite, got {taus}")
    return taus


class NearestIndex:
    """The nearest-point index of ``ref`` [N,3] (N >= 1) on a HIP device: built once, queried many times.

    ``query(q)`` returns ``(dist [M] fp32, idx [M] int32)`` for q [M,3] anywhere in space: dist[i] = min_j sqrt(dx^2 + dy^2 + dz^2) on the
    fp32 coordinate differences, every operation rounded on its own (the distance rule of ``knn``), and idx[i] the lowest row of ref
    that attains the minimum.  Exact and deterministic.  A query row with a NaN or infinite coordinate gets dist NaN and idx -1.
    Clouds in another dtype are converted to fp32 first.  ``ref`` (the fp32 copy) stays reachable as ``.ref``.

    A NaN or infinite coordinate in ref raises ValueError; learning that is the one synchronisation of the constructor.  With
    ``check=False`` the constructor does not synchronise, and every query against a non-finite ref answers NaN and -1 on all rows."""

    def __init__(self, ref: torch.Tensor, check: bool = True):
        _cloud(ref, "ref", "NearestIndex", min_rows=1)
        self.ref = _f32(ref)
        self.N = int(ref.shape[0])
        self.device = ref.device
        L = _lib.lib()
        self._bytes = L.wm_nearest_build_workspace_bytes(self.N)
        if self._bytes == 0:
            raise ValueError(f"NearestIndex: {self.N} points are outside what the library searches (1 <= N < 2^31)")
        self._index = torch.empty(self._bytes, device=self.device, dtype=torch.uint8)
        self._flag = torch.empty(1, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(L.wm_nearest_build(ptr(self.ref), self.N, ptr(self._index), self._bytes, ptr(self._flag), stream(self.device)),
                       "wm_nearest_build")
        self._checked = bool(check)
        if check and int(self._flag.item()):          # the one synchronisation
            raise ValueError("NearestIndex: ref holds a NaN or infinite coordinate")

    def query(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _cloud(q, "q", "NearestIndex.query")
        _same_device(self.device, q, "q", "NearestIndex.query")
        M = int(q.shape[0])
        pts = _f32(q)
        if self._checked:
            dist = torch.empty(M, device=self.device, dtype=torch.float32)
            idx = torch.empty(M, device=self.device, dtype=torch.int32)
        else:          # an index over a non-finite ref writes nothing
            dist = torch.full((M,), float("nan"), device=self.device, dtype=torch.float32)
            idx = torch.full((M,), -1, device=self.device, dtype=torch.int32)
        L = _lib.lib()
        ws_bytes = L.wm_nearest_query_workspace_bytes(M)
        ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            check(L.wm_nearest_query(ptr(self._index), self._bytes, self.N, ptr(pts), M, ptr(ws), ws_bytes, ptr(dist), ptr(idx),
                                     stream(self.device)), "wm_nearest_query")
        return dist, idx


def nearest(q: torch.Tensor, ref: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``NearestIndex(ref).query(q)`` in one call (it synchronises once, as the constructor does)."""
    _cloud(ref, "ref", "nearest", min_rows=1, device=False)
    _cloud(q, "q", "nearest", device=False)
    _on_gpu(ref, "ref", "nearest")
    _same_device(ref.device, q, "q", "nearest")
    return NearestIndex(ref).query(q)


def _umeyama_raw(src32: torch.Tensor, dst32: torch.Tensor, mask8: Optional[torch.Tensor], with_scale: bool) -> torch.Tensor:
    """wm_umeyama on prepared tensors: out [16] fp64 = s, R, t, count, source variance, 0"""
    dev, P = src32.device, int(src32.shape[0])
    L = _lib.lib()
    ws_bytes = L.wm_umeyama_workspace_bytes(P)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.empty(16, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(L.wm_umeyama(ptr(src32), ptr(dst32), ptr(mask8), P, 1 if with_scale else 0, ptr(ws), ws_bytes, ptr(out), stream(dev)), "wm_umeyama")
    return out


def umeyama(src: torch.Tensor, dst: torch.Tensor, mask: Optional[torch.Tensor] = None, with_scale: bool = True) -> Transform:
    """The similarity ``(s, R, t)`` that minimises sum |dst_i - (s R src_i + t)|^2 over the pairs mask keeps (all without a mask): Umeyama's
    closed form with the determinant correction, so R is a rotation (det +1) also for a mirrored target.  src, dst [P,3] on a HIP
    device (read as fp32), mask [P] bool or uint8.  Returns fp64 tensors on the device: s 0-d (1 with with_scale=False), R [3,3], t [3].
    Moments and the 3 x 3 decomposition (one-sided Jacobi) run in fp64 in libwm_hip.so; the call does NOT synchronise.  Fewer than three
    kept pairs, or collinear ones, leave the rotation undetermined (no kept pair gives NaNs); nothing is raised for that."""
    _cloud(src, "src", "umeyama", min_rows=1, device=False)
    _cloud(dst, "dst", "umeyama", rows=int(src.shape[0]), device=False)
    _mask_ok(mask, int(src.shape[0]), "umeyama")
    _on_gpu(src, "src", "umeyama")
    _same_device(src.device, dst, "dst", "umeyama")
    m8 = _mask8(mask, int(src.shape[0]), src.device, "umeyama")
    out = _umeyama_raw(_f32(src), _f32(dst), m8, with_scale)
    return out[0], out[1:10].reshape(3, 3), out[10:13]


def _mask_ok(mask, rows: int, what: str) -> None:
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: mask must be a bool or uint8 tensor")
    if mask.numel() != rows:
        raise ValueError(f"{what}: mask has {mask.numel()} elements for {rows} rows")


def _mask8(mask, rows: int, dev, what: str) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    _mask_ok(mask, rows, what)
    if mask.device != dev:
        raise RuntimeError(f"{what}: mask is on {mask.device}, expected {dev}")
    return mask.reshape(-1).contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.reshape(-1).contiguous()


def _identity(dev) -> Transform:
    return (torch.ones((), device=dev, dtype=torch.float64), torch.eye(3, device=dev, dtype=torch.float64),
            torch.zeros(3, device=dev, dtype=torch.float64))


def _check_transform(tr, dev, what: str) -> Transform:
    try:
        s, R, t = tr
    except (TypeError, ValueError):
        raise ValueError(f"{what}: init must be (s, R, t)")
    s = torch.as_tensor(s, dtype=torch.float64, device=dev).reshape(())
    R = torch.as_tensor(R, dtype=torch.float64, device=dev)
    t = torch.as_tensor(t, dtype=torch.float64, device=dev)
    if tuple(R.shape) != (3, 3) or tuple(t.shape) != (3,):
        raise ValueError(f"{what}: init must be (s, R [3,3], t [3]), got R {tuple(R.shape)}, t {tuple(t.shape)}")
    return s, R, t


def apply_transform(x: torch.Tensor, transform: Transform) -> torch.Tensor:
    """s R x + t for x [N,3], taken in fp64 and rounded once to fp32"""
    s, R, t = transform
    return (x.to(torch.float64) @ (s * R).T + t).to(torch.float32)


def icp(src: torch.Tensor, index: NearestIndex, init: Optional[Transform] = None, max_dist: float = 0.1, iters: int = 30,
        tol: Optional[float] = None, with_scale: bool = False) -> Tuple[Transform, torch.Tensor]:
    """Point-to-point ICP of src [P,3] against the cloud of ``index``.  Every iteration transforms src by the current (s, R, t), queries the
    index, keeps the pairs with dist <= max_dist, runs ``umeyama`` from the transformed points to their nearest points on the kept pairs
    and composes the step in front of the current transform.  An iteration with fewer than 3 kept pairs leaves the transform as it is.
    Returns ``((s, R, t), rms)``: fp64 tensors on the device, rms [iterations run] the root mean square distance of the kept pairs each
    iteration started from (0 where none was kept).

    tol=None runs ``iters`` iterations without a host read.  With tol one scalar is read per iteration and the loop ends when
    |rms_k - rms_{k-1}| <= tol * rms_{k-1}.  with_scale=True lets every step rescale (the composed s then drifts from init's)."""
    _cloud(src, "src", "icp", min_rows=1, device=False)
    if not isinstance(index, NearestIndex):
        raise ValueError("icp: index must be a NearestIndex")
    if int(iters) != iters or int(iters) < 0:
        raise ValueError(f"icp: iters must be a non-negative integer, got {iters!r}")
    if not float(max_dist) >= 0.0:
        raise ValueError(f"icp: max_dist must be >= 0, got {max_dist!r}")
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError(f"icp: tol must be >= 0 or None, got {tol!r}")
    _on_gpu(src, "src", "icp")
    _same_device(index.device, src, "src", "icp")
    dev = src.device
    s, R, t = _identity(dev) if init is None else _check_transform(init, dev, "icp")
    src64 = _f32(src).to(torch.float64)
    hist = []
    prev = None
    for _ in range(int(iters)):
        cur = (src64 @ (s * R).T + t).to(torch.float32)
        dist, idx = index.query(cur)
        keep = dist <= float(max_dist)          # False for the NaN of a non-finite row
        dst = index.ref.index_select(0, idx.clamp(min=0).to(torch.int64))
        out = _umeyama_raw(cur, dst, keep.view(torch.uint8), with_scale)
        count = out[13]
        d64 = dist.to(torch.float64)
        rms = torch.sqrt(torch.where(keep, d64 * d64, torch.zeros_like(d64)).sum() / count.clamp(min=1.0))
        ds, dR, dt = out[0], out[1:10].reshape(3, 3), out[10:13]
        ok = count >= 3.0
        s, R, t = torch.where(ok, ds * s, s), torch.where(ok, dR @ R, R), torch.where(ok, ds * (dR @ t) + dt, t)
        hist.append(rms)
        if tol is not None:
            now = float(rms)          # the one host read of the iteration
            if prev is not None and abs(now - prev) <= float(tol) * prev:
                break
            prev = now
    rms_all = torch.stack(hist) if hist else torch.zeros(0, device=dev, dtype=torch.float64)
    return (s, R, t), rms_all


def _direction_stats(dist: torch.Tensor, idx: torch.Tensor, normals_a: Optional[torch.Tensor], normals_b: Optional[torch.Tensor],
                     taus: Sequence[float]) -> torch.Tensor:
    """wm_cloud_stats: out [4 + MAX_THRESHOLDS] fp64 (NaN where nothing is written)"""
    dev, M = dist.device, int(dist.shape[0])
    L = _lib.lib()
    ws_bytes = L.wm_cloud_stats_workspace_bytes(M)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.full((4 + MAX_THRESHOLDS,), float("nan"), device=dev, dtype=torch.float64)
    arr = (C.c_float * max(len(taus), 1))(*taus)
    Nb = int(normals_b.shape[0]) if normals_b is not None else 0
    with torch.cuda.device(dev):
        check(L.wm_cloud_stats(ptr(dist), ptr(idx), M, ptr(normals_a), ptr(normals_b), Nb, arr, len(taus), ptr(ws), ws_bytes, ptr(out),
                               stream(dev)), "wm_cloud_stats")
    return out


def direction_statistics(dist: torch.Tensor, idx: Optional[torch.Tensor] = None, normals_a: Optional[torch.Tensor] = None,
                         normals_b: Optional[torch.Tensor] = None, thresholds: Sequence[float] = ()) -> Dict[str, torch.Tensor]:
    """The statistics of one direction over a ``NearestIndex.query`` result dist [M] fp32, idx [M] int32 (M >= 1): ``mean`` (a fixed-order fp64
    sum), ``median`` (numpy's rule, exact order statistics), ``counts`` [T] = the number of dist < thresholds[k] and, with normals_a [M,3]
    (of the queries) and normals_b [Nb,3] (of the indexed cloud), ``nc_mean`` and ``nc_median`` of |n_a[i] . n_b[idx[i]]|.  fp64 tensors on
    the device; no synchronisation."""
    what = "direction_statistics"
    if not isinstance(dist, torch.Tensor):
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: dist must be a tensor on a HIP device")
    if dist.dim() != 1 or dist.shape[0] < 1 or dist.dtype != torch.float32:
        raise ValueError(f"{what}: dist must be fp32 [M] with M >= 1")
    taus = _thresholds(thresholds, what)
    M = int(dist.shape[0])
    if (normals_a is None) != (normals_b is None):
        raise ValueError(f"{what}: normals come for both clouds or for neither")
    if normals_a is not None:
        _cloud(normals_a, "normals_a", what, rows=M, device=False)
        _cloud(normals_b, "normals_b", what, min_rows=1, device=False)
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or tuple(idx.shape) != (M,):
            raise ValueError(f"{what}: normals need idx int32 [M]")
    if dist.device.type != "cuda":
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move dist to a HIP device")
    for name, x in (("idx", idx), ("normals_a", normals_a), ("normals_b", normals_b)):
        if x is not None:
            _same_device(dist.device, x, name, what)
    na = _f32(normals_a) if normals_a is not None else None
    nb = _f32(normals_b) if normals_b is not None else None
    out = _direction_stats(dist.contiguous(), idx.contiguous() if idx is not None else None, na, nb, taus)
    res = {"mean": out[0], "median": out[1], "counts": out[4:4 + len(taus)]}
    if na is not None:
        res["nc_mean"], res["nc_median"] = out[2], out[3]
    return res


def _check_pair(pred, gt, pred_normals, gt_normals, taus_in, what: str) -> Tuple[float, ...]:
    _cloud(pred, "pred", what, min_rows=1, device=False)
    _cloud(gt, "gt", what, min_rows=1, device=False)
    if (pred_normals is None) != (gt_normals is None):
        raise ValueError(f"{what}: normals come for both clouds or for neither")
    if pred_normals is not None:
        _cloud(pred_normals, "pred_normals", what, rows=int(pred.shape[0]), device=False)
        _cloud(gt_normals, "gt_normals", what, rows=int(gt.shape[0]), device=False)
    taus = _thresholds(taus_in, what)
    _on_gpu(pred, "pred", what)
    _same_device(pred.device, gt, "gt", what)
    if pred_normals is not None:
        _same_device(pred.device, pred_normals, "pred_normals", what)
        _same_device(pred.device, gt_normals, "gt_normals", what)
    return taus


def accuracy_completeness(pred: torch.Tensor, gt: torch.Tensor, pred_normals: Optional[torch.Tensor] = None,
                          gt_normals: Optional[torch.Tensor] = None, thresholds: Sequence[float] = ()) -> Dict[str, torch.Tensor]:
    """pred [Np,3], gt [Ng,3] on a HIP device -> a dict of fp64 tensors on the device, without a host synchronisation:

        acc, acc_med      mean and median distance pred -> nearest gt        comp, comp_med    the same gt -> nearest pred
        chamfer           (acc + comp) / 2
        nc_acc, nc_comp, nc_acc_med, nc_comp_med, nc = (nc_acc + nc_comp) / 2      with both normal sets [Np,3], [Ng,3] (unit vectors): the
                          mean / median of |n . n'| over the nearest pairs of either direction
        precision, recall, fscore      [T], per threshold: the fractions of pred / gt points with a distance < tau, and 2 P R / (P + R)
                          (0 where P + R = 0); present with thresholds

    Nothing is raised for a NaN or infinite coordinate (that would need a host read): the direction it spoils comes out NaN."""
    what = "accuracy_completeness"
    taus = _check_pair(pred, gt, pred_normals, gt_normals, thresholds, what)
    p32, g32 = _f32(pred), _f32(gt)
    pn = _f32(pred_normals) if pred_normals is not None else None
    gn = _f32(gt_normals) if gt_normals is not None else None
    d_acc, i_acc = NearestIndex(g32, check=False).query(p32)
    d_comp, i_comp = NearestIndex(p32, check=False).query(g32)
    a = _direction_stats(d_acc, i_acc, pn, gn, taus)
    c = _direction_stats(d_comp, i_comp, gn, pn, taus)
    res = {"acc": a[0], "acc_med": a[1], "comp": c[0], "comp_med": c[1], "chamfer": (a[0] + c[0]) / 2}
    if pn is not None:
        res.update({"nc_acc": a[2], "nc_acc_med": a[3], "nc_comp": c[2], "nc_comp_med": c[3], "nc": (a[2] + c[2]) / 2})
    if taus:
        P = a[4:4 + len(taus)] / float(p32.shape[0])
        Rc = c[4:4 + len(taus)] / float(g32.shape[0])
        res.update({"precision": P, "recall": Rc, "fscore": torch.where(P + Rc > 0, 2 * P * Rc / (P + Rc).clamp(min=1e-300), torch.zeros_like(P))})
    return res


def _compact(maps, keep: torch.Tensor, n: int, dev) -> Tuple[list, int]:
    """the rows of every [n,3] map where keep is set, in input order (wm_pack_rows: prefix sums, no atomics; one synchronisation)"""
    from .exporter import _pack_rows
    cols = [(m, c, 3, 0) for m in maps for c in range(3)]
    out, kept = _pack_rows(cols, keep, n, dev)
    rows = out[:kept * len(cols) * 4].view(torch.float32).reshape(kept, len(cols))
    return [rows[:, 3 * i:3 * i + 3].contiguous() for i in range(len(maps))], kept


def evaluate_pointmaps(pred_pts: torch.Tensor, gt_pts: torch.Tensor, gt_mask: torch.Tensor, pred_normals: Optional[torch.Tensor] = None,
                       gt_normals: Optional[torch.Tensor] = None, align: str = "umeyama+icp", icp_max_dist: float = 0.1,
                       thresholds: Sequence[float] = (), icp_iters: int = 30) -> Tuple[Dict[str, torch.Tensor], Transform]:
    """The evaluation of predicted point maps pred_pts [S,H,W,3] against gt_pts [S,H,W,3] on the pixels of gt_mask [S,H,W] (bool or uint8):
    the valid pixels of both maps (and of both normal maps [S,H,W,3]) in pixel order, then, by ``align``,

        "none"           nothing
        "umeyama"        ``umeyama`` with scale on the pixel correspondences pred -> gt
        "umeyama+icp"    that, then ``icp`` (no scale, max_dist = icp_max_dist in the units of gt, icp_iters iterations) against the gt cloud

    and ``accuracy_completeness`` of the transformed prediction (its normals rotated by R).  Returns ``(metrics, (s, R, t))``.  The
    compaction synchronises once (its size is a host number); with ICP the index build synchronises once more."""
    what = "evaluate_pointmaps"
    for name, x in (("pred_pts", pred_pts), ("gt_pts", gt_pts), ("gt_mask", gt_mask), ("pred_normals", pred_normals), ("gt_normals", gt_normals)):
        if x is not None and not isinstance(x, torch.Tensor):
            raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: {name} must be a tensor on a HIP device")
    if pred_pts.dim() != 4 or pred_pts.shape[-1] != 3:
        raise ValueError(f"{what}: pred_pts must be [S, H, W, 3], got {tuple(pred_pts.shape)}")
    if gt_pts.shape != pred_pts.shape:
        raise ValueError(f"{what}: gt_pts {tuple(gt_pts.shape)} does not match pred_pts {tuple(pred_pts.shape)}")
    if tuple(gt_mask.shape) != tuple(pred_pts.shape[:3]) or gt_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: gt_mask must be bool or uint8 {tuple(pred_pts.shape[:3])}, got {gt_mask.dtype} {tuple(gt_mask.shape)}")
    if (pred_normals is None) != (gt_normals is None):
        raise ValueError(f"{what}: normals come for both maps or for neither")
    for name, x in (("pred_normals", pred_normals), ("gt_normals", gt_normals)):
        if x is not None and x.shape != pred_pts.shape:
            raise ValueError(f"{what}: {name} {tuple(x.shape)} does not match pred_pts {tuple(pred_pts.shape)}")
    if align not in ALIGN_MODES:
        raise ValueError(f"{what}: align must be one of {ALIGN_MODES}, got {align!r}")
    if not float(icp_max_dist) >= 0.0:
        raise ValueError(f"{what}: icp_max_dist must be >= 0, got {icp_max_dist!r}")
    taus = _thresholds(thresholds, what)
    n = int(gt_mask.numel())
    if n < 1 or n >= 2 ** 31:
        raise ValueError(f"{what}: {n} pixels are outside what the library packs")
    dev = pred_pts.device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move the maps to a HIP device")
    for name, x in (("gt_pts", gt_pts), ("gt_mask", gt_mask), ("pred_normals", pred_normals), ("gt_normals", gt_normals)):
        if x is not None:
            _same_device(dev, x, name, what)
    maps = [_f32(pred_pts).reshape(n, 3), _f32(gt_pts).reshape(n, 3)]
    if pred_normals is not None:
        maps += [_f32(pred_normals).reshape(n, 3), _f32(gt_normals).reshape(n, 3)]
    packed, kept = _compact(maps, _mask8(gt_mask, n, dev, what), n, dev)
    if kept < 1:
        raise ValueError(f"{what}: gt_mask keeps no pixel")
    pred, gt = packed[0], packed[1]
    pn, gn = (packed[2], packed[3]) if pred_normals is not None else (None, None)
    transform = _identity(dev)
    if align != "none":
        out = _umeyama_raw(pred, gt, None, True)
        transform = (out[0], out[1:10].reshape(3, 3), out[10:13])
        if align == "umeyama+icp":
            transform, _ = icp(pred, NearestIndex(gt), init=transform, max_dist=icp_max_dist, iters=icp_iters, with_scale=False)
        pred = apply_transform(pred, transform)
        if pn is not None:
            pn = (pn.to(torch.float64) @ transform[1].T).to(torch.float32)
    return accuracy_completeness(pred, gt, pn, gn, taus), transform
