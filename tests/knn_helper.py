"""An fp64 brute-force restatement of the k nearest neighbours of a cloud within itself (the reference's knn, submodules/gsplat/examples/
utils.py:141-145, which asks scikit-learn's kd-tree): all pairwise coordinate differences, the distances, the K smallest per row.
Independent of hunyuanworld_mirror_amd; pinned against scikit-learn's recorded fp64 distances by tests/test_knn_cpu.py and the yardstick
for generated inputs in tests/test_knn_gpu.py."""
import os

import numpy as np
import torch

from conftest import ROOT

U = 2.0 ** -24                    # fp32 unit roundoff
DIST_REL = 4 * 2.0 ** -23         # |got - ref64| <= DIST_REL * ref64: about twice the derived 3.5 u + u (tests/test_knn_gpu.py)


def load_golden(name="a"):
    """tests/golden/knn_<name>.npz (tools/gen_golden_knn.py) as a dict, with dist64_k4 = the first four columns of dist64_k16"""
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", f"knn_{name}.npz")))
    z["dist64_k4"] = z["dist64_k16"][:, :4]
    return z


def knn_bruteforce(x, K, chunk=1024):
    """x [N,3] (any float dtype, taken to fp64 exactly) -> (dist [N,K] fp64 ascending, idx [N,K] int64), the point itself included"""
    x = torch.as_tensor(np.asarray(x)).to(torch.float64)
    N = x.shape[0]
    dist, idx = torch.empty((N, K), dtype=torch.float64), torch.empty((N, K), dtype=torch.int64)
    for s in range(0, N, chunk):
        diff = x[s:s + chunk, None, :] - x[None, :, :]
        d = torch.sqrt((diff * diff).sum(-1))
        v, i = torch.topk(d, K, dim=1, largest=False, sorted=True)
        dist[s:s + chunk], idx[s:s + chunk] = v, i
    return dist.numpy(), idx.numpy()


def scales_from_dist(dist4, init_scale):
    """simple_trainer_worldmirror.py:335-337 on [N,4] distances, in the dtype given -> [N]"""
    d = torch.as_tensor(dist4)
    dist2_avg = (d[:, 1:] ** 2).mean(dim=-1)
    return torch.log(torch.sqrt(dist2_avg) * init_scale).numpy()


def dist_excess(got, ref64):
    """max over the entries of |got - ref64| / (DIST_REL ref64), zeros of the reference having to be exact zeros -> a value <= 1 passes"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    zero = ref64 == 0
    if (got[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(got - ref64)[~zero] / (DIST_REL * ref64[~zero])).max())


def scales_excess(got, ref):
    """|got - ref| <= 8 2^-23 + 2^-23 |ref|, -inf exactly where the reference has it -> max of the ratio; <= 1 passes"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ninf = np.isneginf(ref)
    if not np.array_equal(np.isneginf(got), ninf) or not np.isfinite(got[~ninf]).all():
        return float("inf")
    if ninf.all():
        return 0.0
    return float((np.abs(got[~ninf] - ref[~ninf]) / (8 * 2.0 ** -23 + 2.0 ** -23 * np.abs(ref[~ninf]))).max())
