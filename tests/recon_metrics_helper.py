"""Brute-force restatements of the point-cloud evaluation (hunyuanworld_mirror_amd.recon_metrics), independent of the library: the yardsticks of
tests/test_recon_metrics_gpu.py, themselves checked on hand-computed cases by tests/test_recon_metrics_cpu.py.

    nearest_bruteforce   min_j of (dx dx + dy dy) + dz dz over ALL j, element-wise torch CPU ops (each rounded on its own, nothing fused) in
                         fp32 or fp64, and the LOWEST row that attains the minimum (where(mask, arange, N).min, not a tie-dependent argmin)
    umeyama_np           Umeyama's closed form through numpy's fp64 SVD
    icp_ref              the ICP loop over the brute-force search, in either dtype
    direction_stats_np / accuracy_completeness_ref   the metrics in fp64 on given distances"""
import numpy as np
import torch

U32 = 2.0 ** -24


def nearest_bruteforce(q, ref, dtype=torch.float32, chunk=512):
    """q [M,3], ref [N,3] (numpy) -> (d2 [M] the minimum SQUARED distance in dtype, idx [M] int64 the lowest row attaining it), numpy"""
    q = torch.as_tensor(np.ascontiguousarray(q)).to(dtype)
    r = torch.as_tensor(np.ascontiguousarray(ref)).to(dtype)
    N = r.shape[0]
    rows = torch.arange(N, dtype=torch.int64)[None, :]
    d2s, idxs = [], []
    for a in range(0, q.shape[0], chunk):
        c = q[a:a + chunk]
        dx = c[:, None, 0] - r[None, :, 0]
        dy = c[:, None, 1] - r[None, :, 1]
        dz = c[:, None, 2] - r[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        m = d2.min(dim=1).values
        idxs.append(torch.where(d2 == m[:, None], rows, torch.full_like(rows, N)).min(dim=1).values)
        d2s.append(m)
    if not d2s:
        return np.zeros(0, np.float64 if dtype == torch.float64 else np.float32), np.zeros(0, np.int64)
    return torch.cat(d2s).numpy(), torch.cat(idxs).numpy()


def two_nearest_gap(q, ref):
    """fp64: the smallest relative difference (d_2 - d_1) / d_2 between the distances to the nearest and the second-nearest row, over q"""
    q = torch.as_tensor(np.asarray(q, np.float64))
    r = torch.as_tensor(np.asarray(ref, np.float64))
    d = torch.cdist(q, r)
    two = torch.topk(d, 2, dim=1, largest=False).values
    return float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())


def umeyama_np(src, dst, with_scale=True):
    """fp64: (s, R [3,3], t [3]) minimising sum |dst - (s R src + t)|^2, R a rotation (Umeyama 1991, eqs. 39-42)"""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    cov = b.T @ a / len(src)
    var = (a * a).sum() / len(src)
    U, S, Vt = np.linalg.svd(cov)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    s = float((S * d).sum() / var) if with_scale else 1.0
    return s, R, md - s * R @ ms


def cov_singular_values(src, dst):
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    return np.linalg.svd((dst - dst.mean(0)).T @ (src - src.mean(0)) / len(src), compute_uv=False)


def apply(tr, x):
    s, R, t = tr
    return s * np.asarray(x, np.float64) @ np.asarray(R).T + np.asarray(t)


def icp_ref(src, ref, init=None, max_dist=0.1, iters=30, with_scale=False, dtype=torch.float32):
    """Point-to-point ICP of src against ref (both numpy fp32 values).  dtype is the precision of the transformed points and of the search:
    fp32 rounds the transformed points to fp32 as the library does, fp64 keeps everything in fp64.  The Umeyama step is fp64 either way.
    Returns ((s, R, t), rms list, the smallest two-nearest gap met)."""
    np_t = np.float32 if dtype == torch.float32 else np.float64
    s, R, t = (1.0, np.eye(3), np.zeros(3)) if init is None else (float(init[0]), np.asarray(init[1], np.float64), np.asarray(init[2], np.float64))
    src64 = np.asarray(src, np.float64)
    ref_t = np.asarray(ref).astype(np_t)
    rms, gap = [], np.inf
    for _ in range(iters):
        cur = apply((s, R, t), src64).astype(np_t)
        d2, idx = nearest_bruteforce(cur, ref_t, dtype)
        dist = np.sqrt(d2)
        keep = dist <= np_t(max_dist)
        gap = min(gap, two_nearest_gap(cur, ref_t))
        n = int(keep.sum())
        rms.append(float(np.sqrt((dist[keep].astype(np.float64) ** 2).sum() / max(n, 1))))
        if n >= 3:
            ds, dR, dt = umeyama_np(cur[keep], ref_t[idx[keep]], with_scale)
            s, R, t = ds * s, dR @ R, ds * dR @ t + dt
    return (s, R, t), rms, gap


def transform_error(a, b, extent):
    """max(|dR|, |ds| / s, |dt| / extent) between two (s, R, t)"""
    return max(float(np.abs(np.asarray(a[1]) - np.asarray(b[1])).max()), abs(float(a[0]) - float(b[0])) / abs(float(b[0])),
               float(np.abs(np.asarray(a[2]) - np.asarray(b[2])).max()) / extent)


def direction_stats_np(dist, idx=None, normals_a=None, normals_b=None, thresholds=()):
    """fp64 statistics of fp32 distances: mean, np.median, counts of dist < tau (tau as fp32), and with normals the mean / median of the
    absolute dot products taken in fp64"""
    d = np.asarray(dist, np.float32)
    out = {"mean": float(d.astype(np.float64).mean()), "median": float(np.median(d.astype(np.float64))),
           "counts": [int((d < np.float32(t)).sum()) for t in thresholds]}
    if normals_a is not None:
        nc = np.abs((np.asarray(normals_a, np.float64) * np.asarray(normals_b, np.float64)[idx]).sum(1))
        out["nc_mean"], out["nc_median"] = float(nc.mean()), float(np.median(nc))
    return out


def accuracy_completeness_ref(pred, gt, pred_normals=None, gt_normals=None, thresholds=()):
    """the dict of recon_metrics.accuracy_completeness as Python floats / lists, on fp32 brute-force distances"""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    d2a, ia = nearest_bruteforce(pred, gt)
    d2c, ic = nearest_bruteforce(gt, pred)
    a = direction_stats_np(np.sqrt(d2a), ia, pred_normals, gt_normals, thresholds)
    c = direction_stats_np(np.sqrt(d2c), ic, gt_normals, pred_normals, thresholds)
    res = {"acc": a["mean"], "acc_med": a["median"], "comp": c["mean"], "comp_med": c["median"], "chamfer": (a["mean"] + c["mean"]) / 2}
    if pred_normals is not None:
        res.update({"nc_acc": a["nc_mean"], "nc_acc_med": a["nc_median"], "nc_comp": c["nc_mean"], "nc_comp_med": c["nc_median"],
                    "nc": (a["nc_mean"] + c["nc_mean"]) / 2})
    if len(thresholds):
        P = [k / len(pred) for k in a["counts"]]
        R = [k / len(gt) for k in c["counts"]]
        res.update({"precision": P, "recall": R, "fscore": [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, R)]})
    return res


def ulp32(x):
    """the spacing of fp32 at |x| (numpy), at least the smallest denormal"""
    x = np.abs(np.asarray(x, np.float32))
    return np.maximum(np.spacing(x).astype(np.float64), 2.0 ** -149)
