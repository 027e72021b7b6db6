"""torch / numpy restatements of what hunyuanworld_mirror_amd.compression computes on the GPU, for tests/test_compress_cpu.py (which pins
them to the reference's recorded files, tests/golden/compress_a/) and tests/test_compress_gpu.py (which holds the kernels against them).
Everything here runs on the CPU."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_a")
PNG_FIELDS = ("means", "scales", "quats", "opacities", "sh0")


def log_transform(x):
    return torch.sign(x) * torch.log1p(torch.abs(x))


def inverse_log_transform(y):
    return torch.sign(y) * torch.expm1(torch.abs(y))


def crop_indices(opacities):
    """The rows kept by the crop to n^2 = int(N ** 0.5)^2, in descending-opacity order, ties to the lower row; all rows in their own
    order when N is a square."""
    N = opacities.shape[0]
    n = math.isqrt(N)
    if n * n == N:
        return torch.arange(N)
    return torch.sort(opacities, descending=True, stable=True).indices[:n * n]


def preprocess(splats):
    """log transform, normalisation and crop of a dict of CPU tensors -> (new dict, n)"""
    out = dict(splats)
    out["means"] = log_transform(splats["means"].float())
    out["quats"] = torch.nn.functional.normalize(splats["quats"], dim=-1)
    keep = crop_indices(out["opacities"])
    return {k: v[keep] for k, v in out.items()}, math.isqrt(splats["means"].shape[0])


def quantise(x2d, bits):
    """x2d [rows, C] fp32 -> (codes uint16 [rows, C], mins fp32 [C], maxs fp32 [C]); every operation in fp32, rint half to even; a channel
    with max == min encodes as 0"""
    x = x2d.float().numpy()
    mins, maxs = x.min(axis=0), x.max(axis=0)
    rng = (maxs - mins).astype(np.float32)
    safe = np.where(rng == 0, np.float32(1), rng).astype(np.float32)
    norm = ((x - mins).astype(np.float32) / safe).astype(np.float32)
    q = np.round((norm * np.float32(2 ** bits - 1)).astype(np.float32))
    q = np.where(rng == 0, np.float32(0), q)
    return q.astype(np.uint16), mins, maxs


def dequantise(codes, mins, maxs, bits):
    """the reference's fp64 decoder: codes / (2^bits - 1) * double(float(max - min)) + double(min), rounded once to fp32"""
    mins, maxs = np.asarray(mins, np.float32), np.asarray(maxs, np.float32)
    rng = (maxs - mins).astype(np.float32).astype(np.float64)
    return (codes.astype(np.float64) / float(2 ** bits - 1) * rng + mins.astype(np.float64)).astype(np.float32)


def dequantise_kmeans(codes, labels, mn, mx, bits):
    table = dequantise(codes, np.float32(mn), np.float32(mx), bits)
    return table[labels.astype(np.int64)]


def l1_distances(x, c, chunk=2048):
    """fp64 [N, K] L1 distances of fp64 rows x [N, D] and centroids c [K, D]"""
    return torch.cat([torch.cdist(x[i:i + chunk], c, p=1) for i in range(0, x.shape[0], chunk)])


def kmeans_l1_ref(x, n_clusters, init, max_iter=15, tol=1e-4):
    """kmeans_l1 as the package states it, in fp64 -> (labels, centroids fp64, errors fp64, labels of the last iteration)"""
    x = x.double()
    N = x.shape[0]
    K = min(int(n_clusters), N)
    cent = x[init[:K]].clone()
    errors = []
    last = None
    for t in range(max_iter):
        d = l1_distances(x, cent)
        best, last = d.min(dim=1)          # the first minimum: the lowest index
        errors.append(float(best.sum() / N))
        sums = torch.zeros_like(cent).index_add_(0, last, x)
        cnt = torch.bincount(last, minlength=K)
        has = cnt > 0
        cent[has] = sums[has] / cnt[has].unsqueeze(1).double()
        if t > 0 and abs(errors[t - 1] - errors[t]) <= tol * errors[t - 1]:
            break
    labels = l1_distances(x, cent).argmin(dim=1)
    return labels, cent, torch.tensor(errors, dtype=torch.float64), last


def _part1by2(v):
    v = v & 0x3ff
    v = (v ^ (v << 16)) & 0xff0000ff
    v = (v ^ (v << 8)) & 0x0300f00f
    v = (v ^ (v << 4)) & 0x030c30c3
    v = (v ^ (v << 2)) & 0x09249249
    return v


def _part1by1(v):
    v = v & 0xffff
    v = (v ^ (v << 8)) & 0x00ff00ff
    v = (v ^ (v << 4)) & 0x0f0f0f0f
    v = (v ^ (v << 2)) & 0x33333333
    v = (v ^ (v << 1)) & 0x55555555
    return v


def grid_perm(means):
    """perm [n^2] int64: the row of means [n^2, 3] (fp32) that goes to every cell of the grid, as sort_splats states it"""
    N = means.shape[0]
    n = math.isqrt(N)
    assert n * n == N
    x = means.float()
    lo, hi = x.min(dim=0).values, x.max(dim=0).values
    length = hi - lo
    length = torch.where(length > 0, length, torch.ones_like(length))
    q = torch.floor((x - lo) / length * 1024.0).clamp(0, 1023).to(torch.int64)
    keys = (_part1by2(q[:, 2]) << 2) | (_part1by2(q[:, 1]) << 1) | _part1by2(q[:, 0])
    order = torch.sort(keys, stable=True).indices
    c = torch.arange(N)
    ckeys = (_part1by1(c // n) << 1) | _part1by1(c % n)
    cells = torch.sort(ckeys, stable=True).indices
    perm = torch.empty(N, dtype=torch.int64)
    perm[cells] = order
    return perm


def scene(N, degree=0, seed=0, with_row=True):
    """a random scene of CPU tensors with distinct opacities; ``row`` (int32 [N]) stores the row number"""
    g = torch.Generator().manual_seed(seed)
    s = {
        "means": 3.0 * torch.randn(N, 3, generator=g),
        "scales": torch.randn(N, 3, generator=g) - 4.0,
        "quats": torch.randn(N, 4, generator=g),
        "opacities": (torch.randperm(N, generator=g).float() + 0.25) / N * 8.0 - 4.0,
        "sh0": torch.randn(N, 1, 3, generator=g) * 0.6,
    }
    if degree is not None:
        nb = (degree + 1) ** 2 - 1
        g2 = torch.Generator().manual_seed(seed + 1)
        proto = torch.randn(40, nb * 3, generator=g2) * 0.3      # clustered, as trained higher bands are
        pick = torch.randint(0, 40, (N,), generator=g2)
        s["shN"] = (proto[pick] + 0.03 * torch.randn(N, nb * 3, generator=g2)).reshape(N, nb, 3)
    if with_row:
        s["row"] = torch.arange(N, dtype=torch.int32)
    return s


def coherent_scene(n, seed=0):
    """n^2 points on a smooth surface with attributes that are smooth functions of position, presented in random order"""
    g = torch.Generator().manual_seed(seed)
    u, v = torch.meshgrid(torch.linspace(0, 1, n), torch.linspace(0, 1, n), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    z = torch.sin(3.0 * u) * torch.cos(2.0 * v)
    s = {
        "means": torch.stack([4 * u - 2, 4 * v - 2, z], dim=1),
        "scales": torch.stack([-4 + u, -4 + v, -5 + 0.5 * z], dim=1),
        "quats": torch.stack([1 + 0.2 * u, 0.3 * v, 0.3 * z, 0.2 * u * v], dim=1),
        "opacities": 2.0 * torch.sin(2.0 * u + v),
        "sh0": torch.stack([u, v, 0.5 + 0.5 * z], dim=1).reshape(-1, 1, 3),
        "row": torch.arange(n * n, dtype=torch.int32),
    }
    shuffle = torch.randperm(n * n, generator=g)
    return {k: t[shuffle].contiguous() for k, t in s.items()}


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def planes_of(splats_cpu):
    """{field: (codes uint16 [n, n, C], mins, maxs)} of the PNG fields of a dict of CPU tensors, after preprocess()"""
    pre, n = preprocess(splats_cpu)
    out = {}
    for k in PNG_FIELDS:
        if k in pre:
            codes, mins, maxs = quantise(pre[k].reshape(n * n, -1), 16 if k == "means" else 8)
            out[k] = (codes.reshape(n, n, -1), mins, maxs)
    return out, pre, n


def reference_planes(directory, n):
    """the same layout from the PNG files of a directory"""
    out = {}
    for k in PNG_FIELDS:
        if k == "means":
            lo = read_png(os.path.join(directory, "means_l.png")).astype(np.uint16)
            hi = read_png(os.path.join(directory, "means_u.png")).astype(np.uint16)
            out[k] = ((hi << 8) + lo).reshape(n, n, -1)
        elif os.path.exists(os.path.join(directory, f"{k}.png")):
            out[k] = read_png(os.path.join(directory, f"{k}.png")).astype(np.uint16).reshape(n, n, -1)
    return out
