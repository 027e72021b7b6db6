"""Times of the point-cloud evaluation (hunyuanworld_mirror_amd.recon_metrics) on the GPU: the nearest-point index (build and query, each way
between two clouds of N points, on a depth-map-like cloud and on a uniform cube) and one full evaluate_pointmaps on 8 x 518^2 maps with
"umeyama+icp", each beside the same result from torch ops on the same GPU: chunked torch.cdist(...).min, the yardstick that
profiles/r18_knn_init.md used for knn.  Prints one JSON line per measurement.

    build / query   NearestIndex(ref) and index.query(q): two warm-ups, then --rounds timings with a host clock around a device synchronise;
                    median and spread (min .. max) in ms.  The build's time includes its one synchronisation (the non-finite flag).
    cdist           chunked torch.cdist(q, ref).min(1) for the first --cdist-m queries against the WHOLE ref (all of them would take minutes at
                    10^6), with the index queried for the same rows beside it; the results are compared.
    sample_check    1024 sampled rows by plain element-wise torch, ((q[:, None] - ref[None]) ** 2).sum(-1).min(1).sqrt(), timed twice: the
                    second yardstick, and the judge between the other two (cdist's answers have been seen to be wrong at these shapes)
    evaluate        evaluate_pointmaps(pred, gt, mask, normals, align="umeyama+icp"): one warm-up, --eval-rounds timings.  Its torch yardstick
                    is an extrapolation and labelled so: the cdist time of --cdist-m rows, scaled to one pass over all rows, times the 32
                    searches the call makes (30 ICP iterations, accuracy, completeness).

    python tools/bench_recon_metrics.py [--rounds 7] [--n 100000 1000000] [--clouds depth uniform] [--cdist-m 100000] [--views 8]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
from bench_knn import SIZE, _one, _stats, depth_cloud, uniform_cloud  # noqa: E402


def cdist_nearest(q, ref):
    chunk = max(64, min(2048, (1 << 28) // ref.shape[0]))          # about 1 GiB of distances at a time
    d = torch.empty(q.shape[0], device=q.device, dtype=q.dtype)
    i = torch.empty(q.shape[0], device=q.device, dtype=torch.int64)
    for s in range(0, q.shape[0], chunk):
        m = torch.cdist(q[s:s + chunk], ref, compute_mode="donot_use_mm_for_euclid_dist").min(dim=1)
        d[s:s + chunk], i[s:s + chunk] = m.values, m.indices
    return d, i


def depth_maps(S, seed):
    """gt point maps [S,518,518,3] and unit normals of a smooth depth surface seen from S cameras on an arc"""
    g = torch.Generator().manual_seed(seed)
    coarse = 1.5 + 2.5 * torch.rand(S, 1, 9, 9, generator=g)
    depth = torch.nn.functional.interpolate(coarse, size=(SIZE, SIZE), mode="bilinear", align_corners=True)[:, 0].double()
    v, u = torch.meshgrid(torch.arange(SIZE, dtype=torch.float64), torch.arange(SIZE, dtype=torch.float64), indexing="ij")
    cam = torch.stack([(u - SIZE / 2) / 400.0 * depth, (v - SIZE / 2) / 400.0 * depth, depth], -1)
    out = []
    for k in range(S):
        a = 0.6 * (k / max(S - 1, 1) - 0.5)
        R = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float64)
        out.append(cam[k] @ R.T + torch.tensor([-3.0 * np.sin(a), 0.05 * k, 3.0 - 3.0 * np.cos(a)], dtype=torch.float64))
    pts = torch.stack(out)
    n = torch.randn(S, SIZE, SIZE, 3, generator=g).double()
    return pts.float(), (n / n.norm(dim=-1, keepdim=True)).float(), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--eval-rounds", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--clouds", nargs="+", default=["depth", "uniform"], choices=["depth", "uniform"])
    ap.add_argument("--cdist-m", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon_metrics needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    per_row_cdist = None
    for kind in a.clouds:
        for N in a.n:
            make = depth_cloud if kind == "depth" else uniform_cloud
            ref = make(N, seed=N % 1000 + 7)[0].to(dev)
            if kind == "depth":          # a second sampling of the same surfaces: what a prediction is to its ground truth
                g = torch.Generator().manual_seed(5)
                q = (ref.cpu()[torch.randperm(N, generator=g)] + 0.01 * torch.randn(N, 3, generator=g)).to(dev)
            else:
                q = make(N, seed=N % 1000 + 8)[0].to(dev)
            for _ in range(2):
                index = wm.NearestIndex(ref)
                index.query(q)
            tb = [_one(lambda: wm.NearestIndex(ref))[0] for _ in range(a.rounds)]
            tq = [_one(lambda: index.query(q))[0] for _ in range(a.rounds)]
            back = wm.NearestIndex(q)
            back.query(ref)
            tq2 = [_one(lambda: back.query(ref))[0] for _ in range(a.rounds)]
            ext = (ref.max(0).values - ref.min(0).values).cpu().tolist()
            line = dict(tool="bench_recon_metrics", tag=a.tag, what="nearest", cloud=kind, N=N, M=N, extent=[round(e, 2) for e in ext],
                        build_ms=_stats(tb), query_ms=_stats(tq), query_back_ms=_stats(tq2))
            m = min(a.cdist_m, N)
            if m > 0:
                qs = q[:m].contiguous()
                cdist_nearest(qs[:4096], ref)
                rc = [_one(lambda: cdist_nearest(qs, ref)) for _ in range(2)]
                rk = [_one(lambda: index.query(qs)) for _ in range(a.rounds)]
                tc, tk, (dc, ic), (dk, ik) = [r[0] for r in rc], [r[0] for r in rk], rc[-1][1], rk[-1][1]
                rel = ((dk.double() - dc.double()).abs() / dc.double().clamp(min=1e-30)).max()
                line["prefix"] = dict(M=m, cdist_min_ms=_stats(tc), query_ms=_stats(tk), max_rel_diff=float(rel),
                                      rows_agree=float((ik.long() == ic).double().mean()))
                # both against plain element-wise torch on a sample of rows (256 at a time: [256, N, 3] differences)
                pick = torch.randperm(m, generator=torch.Generator().manual_seed(1))[:1024].to(dev)
                plain = lambda: torch.cat([((qs[pick[s:s + 256], None, :] - ref[None, :, :]) ** 2).sum(-1).min(dim=1).values.sqrt()  # noqa: E731
                                           for s in range(0, 1024, 256)])
                plain()
                rp = [_one(plain) for _ in range(2)]
                db = rp[-1][1]
                line["sample_check"] = dict(rows=1024, elementwise_min_ms=_stats([r[0] for r in rp]), query_max_rel_diff=float(((dk[pick].double() - db.double()).abs() / db.double().clamp(min=1e-30)).max()),
                                            cdist_max_rel_diff=float(((dc[pick].double() - db.double()).abs() / db.double().clamp(min=1e-30)).max()))
                if kind == "depth" and N == max(a.n):
                    per_row_cdist = min(tc) / m
            print(json.dumps(line), flush=True)
            del ref, q, index, back
    S = a.views
    gt, gn, g = depth_maps(S, seed=3)
    ang = 0.4
    R0 = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=torch.float32)
    pred = (1.3 * (gt + 0.005 * torch.randn(gt.shape, generator=g)) @ R0.T + torch.tensor([0.5, -1.0, 2.0])).contiguous()
    pn = (gn @ R0.T).contiguous()
    mask = torch.rand(S, SIZE, SIZE, generator=g) > 0.3
    gt, gn, pred, pn, mask = (x.to(dev) for x in (gt, gn, pred, pn, mask))
    run = lambda: wm.evaluate_pointmaps(pred, gt, mask, pn, gn, align="umeyama+icp", icp_max_dist=0.1, thresholds=(0.02, 0.05))  # noqa: E731
    metrics, (s, R, t) = run()
    te = [_one(run)[0] for _ in range(a.eval_rounds)]
    kept = int(mask.sum())
    line = dict(tool="bench_recon_metrics", tag=a.tag, what="evaluate_pointmaps", views=S, size=SIZE, kept=kept, align="umeyama+icp",
                evaluate_ms=_stats(te), acc=float(metrics["acc"]), comp=float(metrics["comp"]), nc=float(metrics["nc"]),
                fscore=metrics["fscore"].tolist(), scale=float(s), scale_expected=1 / 1.3)
    if per_row_cdist is not None:
        line["torch_cdist_extrapolated_ms"] = round(per_row_cdist * kept * (kept / max(a.n)) * 32, 1)
        line["torch_cdist_extrapolation"] = f"min cdist ms per query row at N={max(a.n)} x kept rows x (kept / N) x 32 searches"
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
