"""Time of knn(points, 4), the neighbour search of the trainer's splat initialisation (simple_trainer_worldmirror.py:334-337), at the sizes
save_colmap hands over: N = 1.49 M (8 views of 518 x 518 at conf_threshold 30 %) and 5.96 M (32 views).

Clouds (seeded, generated on the host, the same points for every form)
    depth     S views of 518 x 518 pixels unprojected from a smooth random depth (a bilinearly upsampled 9 x 9 grid of depths in 1.5 .. 4,
              one per view), the cameras on an arc around the scene, a random N of the pixels kept, and 0.1 % of the kept points pushed
              out along their ray by a factor of 10 .. 100: dense surfaces and a few far outliers in one bounding box
    uniform   N points uniform in the unit cube

Forms
    knn       hunyuanworld_mirror_amd.knn(points, 4): the device search, its one synchronisation (the non-finite flag) inside
    host      the reference's knn on the same points: the copy to the host and scikit-learn's kd-tree (utils.py:141-145), when
              scikit-learn is installed; ONE run (it takes seconds to a minute), and only up to --host-max points
    cdist     chunked torch.cdist + topk on the GPU, at --cdist-n points (a prefix of the same cloud; the full sizes would take minutes),
              with knn on the same prefix beside it

knn is warmed up twice, then timed --rounds times with a host clock around a device synchronise; median and spread (min .. max) in ms.
Where the host form ran, the largest relative difference between its distances and knn's is reported (it should be a few 2^-24).
One JSON line per cloud and size.  No time is gated.

    python tools/bench_knn.py [--rounds 7] [--n 1490000 5960000] [--clouds depth uniform] [--host-max 1490000] [--cdist-n 200000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hunyuanworld_mirror_amd as wm  # noqa: E402

SIZE = 518


def _one(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3), runs=len(ts))


def depth_cloud(N, seed):
    """-> [N,3] f32 and the number of views"""
    S = int(np.ceil(N / (0.7 * SIZE * SIZE)))
    g = torch.Generator().manual_seed(seed)
    coarse = 1.5 + 2.5 * torch.rand(S, 1, 9, 9, generator=g)
    depth = torch.nn.functional.interpolate(coarse, size=(SIZE, SIZE), mode="bilinear", align_corners=True)[:, 0].double()
    f, c = 400.0, SIZE / 2
    v, u = torch.meshgrid(torch.arange(SIZE, dtype=torch.float64), torch.arange(SIZE, dtype=torch.float64), indexing="ij")
    cam = torch.stack([(u - c) / f * depth, (v - c) / f * depth, depth], -1)          # [S,H,W,3]
    pts = []
    for i in range(S):
        a = 0.6 * (i / max(S - 1, 1) - 0.5)
        R = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float64)
        t = torch.tensor([-3.0 * np.sin(a), 0.05 * i, 3.0 - 3.0 * np.cos(a)], dtype=torch.float64)
        centre = t
        p = cam[i].reshape(-1, 3) @ R.T + t
        pts.append((p, centre))
    keep = torch.randperm(S * SIZE * SIZE, generator=g)[:N].sort().values
    allp = torch.cat([p for p, _ in pts])[keep]
    centres = torch.cat([c_.expand(SIZE * SIZE, 3) for _, c_ in pts])[keep]
    out = torch.randperm(N, generator=g)[:N // 1000]
    factor = 10.0 + 90.0 * torch.rand(len(out), 1, generator=g).double()
    allp[out] = centres[out] + (allp[out] - centres[out]) * factor
    return allp.float().contiguous(), S


def uniform_cloud(N, seed):
    return torch.rand(N, 3, generator=torch.Generator().manual_seed(seed)).contiguous(), 0


def host_knn(x_host, K):
    """utils.py:141-145"""
    from sklearn.neighbors import NearestNeighbors
    x_np = x_host.numpy()
    model = NearestNeighbors(n_neighbors=K, metric="euclidean").fit(x_np)
    distances, _ = model.kneighbors(x_np)
    return torch.from_numpy(distances).to(x_host)


def cdist_knn(x, K, chunk=2048):
    out = torch.empty((x.shape[0], K), device=x.device, dtype=x.dtype)
    for s in range(0, x.shape[0], chunk):
        d = torch.cdist(x[s:s + chunk], x, compute_mode="donot_use_mm_for_euclid_dist")
        out[s:s + chunk] = torch.topk(d, K, dim=1, largest=False, sorted=True).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, nargs="+", default=[1_490_000, 5_960_000])
    ap.add_argument("--clouds", nargs="+", default=["depth", "uniform"], choices=["depth", "uniform"])
    ap.add_argument("--host-max", type=int, default=1_490_000)
    ap.add_argument("--cdist-n", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    for kind in a.clouds:
        for N in a.n:
            x_host, S = (depth_cloud if kind == "depth" else uniform_cloud)(N, seed=N % 1000 + 7)
            x = x_host.to(dev)
            for _ in range(2):
                got = wm.knn(x, a.k)
            times = [_one(lambda: wm.knn(x, a.k))[0] for _ in range(a.rounds)]
            ext = (x.max(0).values - x.min(0).values).cpu().tolist()
            line = dict(tool="bench_knn", tag=a.tag, cloud=kind, N=N, K=a.k, views=S, extent=[round(e, 2) for e in ext], knn_ms=_stats(times))
            if have_sklearn and N <= a.host_max:
                t0 = time.perf_counter()
                ref = host_knn(x_host, a.k)
                line["host_sklearn_ms_one_run"] = round((time.perf_counter() - t0) * 1e3, 1)
                r, g_ = ref.double(), got.cpu().double()
                nz = r > 0
                line["max_rel_diff_to_host"] = float(((g_ - r).abs()[nz] / r[nz]).max())
                line["zeros_agree"] = bool(torch.equal(g_ == 0, r == 0))
            else:
                line["host_sklearn_ms_one_run"] = None if have_sklearn else "scikit-learn not installed"
            n2 = min(a.cdist_n, N)
            if n2 > 0:
                xs = x[:n2].contiguous()
                cdist_knn(xs[:4096].contiguous(), a.k)          # warm-up of the two ops
                wm.knn(xs, a.k)
                tc = [_one(lambda: cdist_knn(xs, a.k))[0] for _ in range(2)]
                tk = [_one(lambda: wm.knn(xs, a.k))[0] for _ in range(a.rounds)]
                line["prefix"] = dict(N=n2, cdist_topk_ms=_stats(tc), knn_ms=_stats(tk))
            print(json.dumps(line), flush=True)
            del x, got


if __name__ == "__main__":
    main()
