"""GPU: hunyuanworld_mirror_amd.splat_init (csrc/knn.hip): knn, knn_scales and create_splats_with_optimizers against scikit-learn's recorded
fp64 distances and the reference's recorded scales (tests/golden/knn_a.npz, tools/gen_golden_knn.py) and, for generated clouds, against
the fp64 brute force of tests/knn_helper.py (pinned to the recording by tests/test_knn_cpu.py).

Bounds, derived and not measured.
  distances  A difference-form fp32 distance sqrt(dx^2 + dy^2 + dz^2) rounds in the subtraction, the square, two additions and the root,
             each by at most u = 2^-24 relative: 3.5 u in all; the reference's own rounding of its fp64 result to fp32 adds u.  The k-th
             smallest of values each perturbed by a factor (1 +- d) is within (1 +- d) of the k-th smallest.  Bound: |got - ref64| <=
             4 2^-23 ref64 (knn_helper.DIST_REL), about twice the derived error; a zero of the reference must be an exact zero.
  scales     log(sqrt(mean(d^2)) s): the argument carries the relative error of the distances plus three roundings, the logarithm turns
             a relative error into an absolute one and rounds once more.  Bound: |got - ref| <= 8 2^-23 + 2^-23 |ref|
             (knn_helper.scales_excess); -inf exactly where the reference has it.
Measured on MI355X, as the largest ratio error / bound over the cases of this file (each test prints its own): distances 0.325 (the golden
cloud at K = 16; 2.6 u relative), scales 0.590 (the golden cloud at init_scale 0.5); zeros exact and -inf in place everywhere.

Shapes.  The query kernel runs one query per lane in blocks of 256, so 257 and 4097 points cross a block with a one-lane tail; N = K and
N = 1 have no K-th sorted neighbour on either side and start at the root level, N = 5 has one at its two end positions only; K = 4, 8 and
16 are the three list sizes the kernel is built for, K = 3 and K = 9 sit inside a larger list.  Identical points, a line, a plane and the
lattices are the bounding boxes without extent along one or more axes and the distances that tie exactly on cell faces.  Cells of more than
48 points, which the kernel takes apart instead of scanning, are met by the golden cloud's outliers (their coarse cells hold the dense
cluster) and, at the finest level where nothing is left to take apart, by the 299-point cluster."""
import functools
import os

import numpy as np
import pytest
import torch

import knn_helper as KH
from hunyuanworld_mirror_amd import (create_splats_with_optimizers, knn, knn_scales, photometric_loss, rasterization, rgb_to_sh, save_gs_ply,
                                     splats_from_ply)
from hunyuanworld_mirror_amd.colmap import ColmapModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return KH.load_golden("a")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _report(what, ratio):
    print(f"[knn] {what}: error / bound = {ratio:.3f}")
    return ratio


# ---------------------------------------------------------------- 1. the golden cloud
@pytest.mark.parametrize("K", [4, 16])
def test_golden_distances(gold, K):
    got = knn(_gpu(gold["points"]), K)
    assert got.shape == (3000, K) and got.dtype == torch.float32 and got.device == torch.device(DEV)
    got = got.cpu().numpy()
    assert _report(f"golden K={K}", KH.dist_excess(got, gold[f"dist64_k{K}"])) <= 1.0
    assert (np.diff(got, axis=1) >= 0).all() and (got[:, 0] == 0).all()
    dup = gold["dup_rows"]
    ref = gold[f"dist64_k{K}"]
    assert (ref[dup, 1] == 0).all() and np.array_equal(got[dup] == 0, ref[dup] == 0)


@pytest.mark.parametrize("name,init_scale", [("scales_1", 1.0), ("scales_05", 0.5)])
def test_golden_scales(gold, name, init_scale):
    got = knn_scales(_gpu(gold["points"]), init_scale)
    assert got.shape == (3000, 3) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    assert _report(name, KH.scales_excess(got[:, 0], gold[name])) <= 1.0
    assert np.isneginf(got[gold["dup_rows"], 0]).all()


# ---------------------------------------------------------------- 2. indices
@pytest.mark.parametrize("K", [4, 16])
def test_indices(gold, K):
    x = gold["points"]
    dist, idx = knn(_gpu(x), K, return_indices=True)
    assert idx.shape == (3000, K) and idx.dtype == torch.int64
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < 3000
    x64 = x.astype(np.float64)
    pair = np.sqrt(((x64[:, None, :] - x64[idx]) ** 2).sum(-1))
    assert KH.dist_excess(dist, pair) <= 1.0
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()      # distinct in every row
    alone = dist[:, 1] != 0
    assert np.array_equal(idx[alone, 0], np.flatnonzero(alone))


# ---------------------------------------------------------------- 3. seams and degenerate shapes
def _lattice():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def _cloud(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("uniform"):
        return rng.uniform(-1.0, 1.0, (int(name[7:]), 3)).astype(np.float32)
    if name == "identical":
        return np.tile(np.array([[0.25, -3.0, 7.5]], np.float32), (300, 1))
    if name == "zeros":
        return np.zeros((300, 3), np.float32)
    if name == "line":
        return (rng.uniform(0.0, 1.0, (500, 1)) * np.array([1.0, 2.0, -3.0]) + 5.0).astype(np.float32)
    if name == "plane":
        p = rng.uniform(-4.0, 4.0, (500, 3)).astype(np.float32)
        p[:, 2] = 0.0
        return p
    if name == "lattice":
        return _lattice()
    if name == "lattice_shifted":
        return ((_lattice() + np.float32(1e4)) * np.float32(1e-2)).astype(np.float32)
    if name == "cluster_outlier":
        c = rng.uniform(0.0, 1e-3, (299, 3))
        return np.concatenate([c, [[1e3, 0.0, 0.0]]]).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the fp64 brute force of a generated cloud, once: its 16 (or N) nearest, of which a case takes the first K columns"""
    x = _cloud(name)
    return KH.knn_bruteforce(x, min(16, len(x)))[0]


CASES = [("uniform4", 4), ("uniform1", 1), ("uniform5", 4), ("uniform257", 4), ("uniform4097", 4), ("uniform4097", 16), ("uniform257", 3),
         ("uniform257", 8), ("uniform257", 9), ("identical", 4), ("zeros", 4), ("line", 4), ("plane", 4), ("lattice", 4), ("lattice", 8),
         ("lattice_shifted", 4), ("cluster_outlier", 4)]


@pytest.mark.parametrize("name,K", CASES)
def test_seams_and_degenerate_clouds(name, K):
    x = _cloud(name)
    ref = _reference(name)[:, :K]
    dist, idx = knn(_gpu(x), K, return_indices=True)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert dist.shape == ref.shape
    assert _report(f"{name} K={K}", KH.dist_excess(dist, ref)) <= 1.0
    assert (np.diff(dist, axis=1) >= 0).all() and (dist[:, 0] == 0).all()
    assert idx.min() >= 0 and idx.max() < len(x)
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()
    if name == "lattice":          # integer coordinates: every square is exact, so the distances are the correctly rounded roots
        assert np.array_equal(dist, np.sqrt((ref ** 2).round()).astype(np.float32))
        assert (dist[:, 1] == 1.0).all() and set(np.unique(dist)) <= {0.0, 1.0, np.float32(np.sqrt(2.0)), np.float32(np.sqrt(3.0))}
    if name in ("identical", "zeros"):
        assert (dist == 0).all()
    if name == "cluster_outlier":
        assert (idx[299, 1:] < 299).all() and idx[299, 0] == 299          # the outlier's neighbours are the cluster
        assert (idx[:299] != 299).all()                                    # and nobody in the cluster has the outlier


# ---------------------------------------------------------------- 4. determinism
def test_repeatable_and_permutation_equivariant():
    x = _cloud("uniform4097")
    ref = _reference("uniform4097")[:, :5]
    assert (np.diff(ref, axis=1) > 1e-5 * ref[:, 1:]).all()          # no ties in this cloud, in fp32 either: the indices are unique
    xt = _gpu(x)
    d0, i0 = knn(xt, 4, return_indices=True)
    d1, i1 = knn(xt, 4, return_indices=True)
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(i0, i1)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(x))).to(DEV)
    dp, ip = knn(xt[perm].contiguous(), 4, return_indices=True)
    assert torch.equal(dp.view(torch.int32), d0[perm].view(torch.int32))
    assert torch.equal(perm[ip], i0[perm])


# ---------------------------------------------------------------- 5. errors
def test_errors_leave_the_device_usable(gold):
    x = _gpu(gold["points"][:100])
    for K in (0, 17, 101):
        with pytest.raises(ValueError):
            knn(x, K)
    with pytest.raises(ValueError):
        knn(x[:, :2].contiguous(), 4)
    for bad in (float("nan"), float("inf"), float("-inf")):
        y = x.clone()
        y[37, 1] = bad
        with pytest.raises(ValueError):
            knn(y, 4)
        with pytest.raises(ValueError):
            knn_scales(y)
    got = knn(x, 4).cpu().numpy()
    ref, _ = KH.knn_bruteforce(gold["points"][:100], 4)
    assert KH.dist_excess(got, ref) <= 1.0


# ---------------------------------------------------------------- 6. create_splats_with_optimizers
def _parser(gold, device=None):
    rgb = np.random.default_rng(3).integers(0, 256, (3000, 3), dtype=np.uint8)
    m = ColmapModel(points=gold["points"], points_rgb=rgb)
    return (m if device is None else ColmapModel(points=_gpu(m.points), points_rgb=_gpu(rgb))), rgb


def _check_optimizers(splats, opts, lrs, BS):
    assert sorted(opts) == sorted(splats.keys()) == sorted(lrs)
    for name, opt in opts.items():
        assert type(opt) is torch.optim.Adam and len(opt.param_groups) == 1
        g = opt.param_groups[0]
        assert g["name"] == name and len(g["params"]) == 1 and g["params"][0] is splats[name]
        assert g["lr"] == lrs[name] * np.sqrt(BS) and g["eps"] == 1e-15 / np.sqrt(BS)
        assert g["betas"] == (1 - BS * (1 - 0.9), 1 - BS * (1 - 0.999))


@pytest.mark.parametrize("on_device,batch_size", [(False, 1), (True, 4)])
def test_create_splats_sfm(gold, on_device, batch_size):
    parser, rgb = _parser(gold, DEV if on_device else None)
    splats, opts = create_splats_with_optimizers(parser, init_type="sfm", batch_size=batch_size, scene_scale=1.7, device=DEV)
    assert isinstance(splats, torch.nn.ParameterDict) and all(p.device == torch.device(DEV) and p.requires_grad for p in splats.values())
    lrs = dict(means=1.6e-4 * 1.7, scales=5e-3, quats=1e-3, opacities=5e-2, sh0=2.5e-3, shN=2.5e-3 / 20)
    _check_optimizers(splats, opts, lrs, batch_size)
    assert np.array_equal(splats["means"].detach().cpu().numpy(), gold["points"])
    sc = splats["scales"].detach().cpu().numpy()
    assert sc.shape == (3000, 3) and np.array_equal(sc[:, 0], sc[:, 1]) and np.array_equal(sc[:, 0], sc[:, 2])
    assert KH.scales_excess(sc[:, 0], gold["scales_1"]) <= 1.0
    want_sh0 = rgb_to_sh(_gpu(rgb / 255.0).float())          # (rgb_to_sh itself is held to the reference's values in test_knn_cpu.py)
    assert splats["sh0"].shape == (3000, 1, 3) and torch.equal(splats["sh0"].detach()[:, 0, :], want_sh0)
    assert splats["shN"].shape == (3000, 15, 3) and not splats["shN"].detach().any()
    op = splats["opacities"].detach().cpu()
    assert op.shape == (3000,) and bool((op == op[0]).all()) and abs(float(op[0]) - np.log(0.1 / 0.9)) < 1e-6
    # (logit(0.1) in fp32: three roundings of the argument, 3 u = 1.8e-7 absolute behind the logarithm, and the logarithm's own few ulps of 2.2)
    q = splats["quats"].detach()
    assert q.shape == (3000, 4) and bool((q >= 0).all()) and bool((q < 1).all()) and float(q.std()) > 0.2


def test_create_splats_sfm_world_split(gold):
    parser, _ = _parser(gold)
    full, _ = create_splats_with_optimizers(parser, device=DEV, init_scale=0.5, sh_degree=1)
    assert KH.scales_excess(full["scales"].detach().cpu().numpy()[:, 0], gold["scales_05"]) <= 1.0
    assert full["shN"].shape == (3000, 3, 3)
    ranks = [create_splats_with_optimizers(parser, device=DEV, init_scale=0.5, sh_degree=1, world_rank=r, world_size=2) for r in (0, 1)]
    for r, (s, o) in enumerate(ranks):
        assert s["means"].shape == (1500, 3) and s["quats"].shape == (1500, 4) and s["opacities"].shape == (1500,)
        for name in ("means", "scales", "sh0"):          # the kNN ran on the full cloud: the scales are the full cloud's rows
            assert torch.equal(s[name].detach(), full[name].detach()[r::2]), name
        assert o["means"].param_groups[0]["lr"] == 1.6e-4 * np.sqrt(2) and o["means"].param_groups[0]["betas"] == (1 - 2 * (1 - 0.9), 1 - 2 * (1 - 0.999))


def test_create_splats_random():
    g = torch.Generator(device=DEV).manual_seed(11)
    splats, opts = create_splats_with_optimizers(None, init_type="random", init_num_pts=5000, init_extent=2.0, scene_scale=1.5, sh_degree=2,
                                                 device=DEV, generator=g)
    m = splats["means"].detach()
    assert m.shape == (5000, 3) and float(m.abs().max()) <= 3.0 and float(m.abs().max()) > 2.9 and float(m.min()) < -2.9
    assert torch.equal(splats["scales"].detach(), knn_scales(m, 1.0)) and bool(torch.isfinite(splats["scales"]).all())
    sh0 = splats["sh0"].detach() * 0.28209479177387814 + 0.5
    assert splats["sh0"].shape == (5000, 1, 3) and float(sh0.min()) > -1e-6 and float(sh0.max()) < 1 + 1e-6
    assert splats["shN"].shape == (5000, 8, 3) and len(opts) == 6
    g2 = torch.Generator(device=DEV).manual_seed(11)
    again, _ = create_splats_with_optimizers(None, init_type="random", init_num_pts=5000, init_extent=2.0, scene_scale=1.5, sh_degree=2,
                                             device=DEV, generator=g2)
    assert all(torch.equal(again[k].detach(), splats[k].detach()) for k in splats.keys())


def _small_ply(tmp_path):
    g = torch.Generator().manual_seed(2)
    N = 400
    means = torch.randn(N, 3, generator=g).to(DEV)
    scales = (0.01 + 0.05 * torch.rand(N, 3, generator=g)).to(DEV)
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1).to(DEV)
    rgbs = torch.randn(N, 3, generator=g).to(DEV)
    opac = (0.05 + 0.9 * torch.rand(N, generator=g)).to(DEV)
    path = os.path.join(str(tmp_path), "gs.ply")
    save_gs_ply(path, means, scales, quats, rgbs, opac)
    return path


def test_create_splats_ffgs(tmp_path):
    path = _small_ply(tmp_path)
    want = splats_from_ply(path, sh_degree=3, device=DEV)
    splats, opts = create_splats_with_optimizers(None, init_type="ffgs", ply_path=path, device=DEV)
    assert sorted(splats.keys()) == sorted(want) and len(opts) == 6
    n = want["means"].shape[0]
    assert 0 < n < 400
    for k, v in want.items():
        assert torch.equal(splats[k].detach(), v), k
    half, _ = create_splats_with_optimizers(None, init_type="ffgs", ply_path=path, device=DEV, world_rank=1, world_size=2)
    for k, v in want.items():
        assert torch.equal(half[k].detach(), v[1::2]), k


def test_create_splats_feature_dim(gold):
    parser, rgb = _parser(gold)
    splats, opts = create_splats_with_optimizers(parser, feature_dim=32, device=DEV)
    assert sorted(splats.keys()) == sorted(["means", "scales", "quats", "opacities", "features", "colors"]) and "sh0" not in splats
    _check_optimizers(splats, opts, dict(means=1.6e-4, scales=5e-3, quats=1e-3, opacities=5e-2, features=2.5e-3, colors=2.5e-3), 1)
    f = splats["features"].detach()
    assert f.shape == (3000, 32) and bool((f >= 0).all()) and bool((f < 1).all())
    assert torch.equal(splats["colors"].detach(), torch.logit(_gpu(rgb / 255.0).float()))


def test_one_training_step_from_sfm_splats():
    """sfm splats of a 2000-point cloud -> rasterization at 2 views of 64 x 64 -> photometric_loss -> backward -> every optimiser steps"""
    rng = np.random.default_rng(8)
    pts = (rng.uniform(-1.0, 1.0, (2000, 3)) * [1.0, 1.0, 0.5] + [0.0, 0.0, 3.0]).astype(np.float32)
    parser = ColmapModel(points=pts, points_rgb=rng.integers(0, 256, (2000, 3), dtype=np.uint8))
    splats, opts = create_splats_with_optimizers(parser, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    assert bool(torch.isfinite(splats["scales"]).all())
    viewmats = torch.eye(4, device=DEV).repeat(2, 1, 1)
    viewmats[1, 0, 3] = 0.2
    Ks = torch.tensor([[60.0, 0.0, 32.0], [0.0, 60.0, 32.0], [0.0, 0.0, 1.0]], device=DEV).repeat(2, 1, 1)
    colors = torch.cat([splats["sh0"], splats["shN"]], 1)
    render, alphas, info = rasterization(splats["means"], splats["quats"], torch.exp(splats["scales"]), torch.sigmoid(splats["opacities"]), colors,
                                         viewmats, Ks, 64, 64, sh_degree=3)
    assert render.shape == (2, 64, 64, 3) and float(alphas.detach().max()) > 0
    target = torch.rand(2, 64, 64, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    loss, _, _ = photometric_loss(render, target)
    before = {k: v.detach().clone() for k, v in splats.items()}
    loss.backward()
    for opt in opts.values():
        opt.step()
        opt.zero_grad(set_to_none=True)
    assert all(bool(torch.isfinite(v).all()) for v in splats.values())
    assert not torch.equal(splats["means"].detach(), before["means"]) and not torch.equal(splats["sh0"].detach(), before["sh0"])
