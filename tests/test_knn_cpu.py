"""CPU: the yardsticks of tests/test_knn_gpu.py and the argument checks of hunyuanworld_mirror_amd.splat_init, none of which needs a GPU.

tests/knn_helper.py (fp64 brute force) is held against scikit-learn's recorded fp64 distances (tests/golden/knn_a.npz, written by
tools/gen_golden_knn.py from the reference's own knn and rgb_to_sh); the recorded scales follow from the recorded distances by the
statements of simple_trainer_worldmirror.py:335-337; create_splats_with_optimizers refuses what it does not build before it touches a
device; knn has no CPU path."""
import numpy as np
import pytest
import torch

import knn_helper as KH
from hunyuanworld_mirror_amd import create_splats_with_optimizers, knn, knn_scales, rgb_to_sh, splat_init


@pytest.fixture(scope="module")
def gold():
    return KH.load_golden("a")


def test_golden_composition(gold):
    pts = gold["points"]
    assert pts.shape == (3000, 3) and pts.dtype == np.float32 and np.isfinite(pts).all()
    far = np.all(pts == np.array([1000.0, -1000.0, 500.0], np.float32), axis=1)
    assert far.sum() == 10
    same_as_0 = np.all(pts == pts[0], axis=1)
    assert same_as_0.sum() == 6
    assert np.array_equal(np.flatnonzero(far | same_as_0), gold["dup_rows"])
    assert float(gold["brute_err"]) < 1e-12


@pytest.mark.parametrize("K", [4, 16])
def test_helper_matches_recorded_fp64_distances(gold, K):
    dist, idx = KH.knn_bruteforce(gold["points"], K)
    ref = gold[f"dist64_k{K}"]
    assert np.abs(dist - ref).max() <= 1e-12 * ref.max() and (np.abs(dist - ref) <= 1e-12 * ref).all()
    assert (dist[:, 0] == 0).all() and (np.diff(dist, axis=1) >= 0).all()
    x = gold["points"].astype(np.float64)
    assert np.allclose(np.sqrt(((x[:, None, :] - x[idx]) ** 2).sum(-1)), dist, rtol=1e-14, atol=0)      # (another summation order)
    assert (dist[gold["dup_rows"], 1] == 0).all()
    # the reference's own fp32 result is its fp64 distances rounded once
    if K == 4:
        assert np.array_equal(gold["knn4_ref"], ref.astype(np.float32))


def test_recorded_scales_follow_from_recorded_distances(gold):
    for name, s in (("scales_1", 1.0), ("scales_05", 0.5)):
        assert np.array_equal(KH.scales_from_dist(gold["knn4_ref"], s), gold[name])                       # the same fp32 statements
        assert KH.scales_excess(gold[name], KH.scales_from_dist(gold["dist64_k4"], s)) <= 1.0              # and the fp64 ones, within the bound
    ninf = np.isneginf(gold["scales_1"])
    assert np.array_equal(np.flatnonzero(ninf), gold["dup_rows"])      # every duplicated point here has at least three twins


def test_excess_measures():
    ref = np.array([[0.0, 1.0, 2.0]])
    assert KH.dist_excess(ref.astype(np.float32), ref) == 0.0
    assert KH.dist_excess(np.array([[1e-30, 1.0, 2.0]]), ref) == float("inf")          # a zero must be exact
    assert 0.9 < KH.dist_excess(np.array([[0.0, 1.0 + 0.95 * KH.DIST_REL, 2.0]]), ref) < 1.0
    assert KH.dist_excess(np.array([[0.0, 1.0, 2.0 * (1 + 1.1 * KH.DIST_REL)]]), ref) > 1.0
    s = np.array([-np.inf, -3.0])
    assert KH.scales_excess(s, s) == 0.0
    assert KH.scales_excess(np.array([-1e30, -3.0]), s) == float("inf")
    assert KH.scales_excess(np.array([-np.inf, -3.0 + 12 * 2.0 ** -23]), s) > 1.0


def test_rgb_to_sh_matches_reference(gold):
    assert torch.equal(rgb_to_sh(torch.from_numpy(gold["rgb"])), torch.from_numpy(gold["sh"]))


def test_knn_has_no_cpu_path(gold):
    x = torch.from_numpy(gold["points"])
    with pytest.raises(RuntimeError):
        knn(x, 4)
    with pytest.raises(RuntimeError):
        knn_scales(x)
    with pytest.raises(RuntimeError):
        knn(gold["points"], 4)          # not a tensor


def test_knn_argument_checks_come_first():
    """shape and K are refused as ValueError whatever the device"""
    x = torch.zeros(10, 3)
    for bad_k in (0, 17, 11, 2.5):
        with pytest.raises(ValueError):
            knn(x, bad_k)
    with pytest.raises(ValueError):
        knn(torch.zeros(10, 2), 4)
    with pytest.raises(ValueError):
        knn(torch.zeros(30), 4)


class _Parser:
    points = np.zeros((8, 3), np.float32)
    points_rgb = np.zeros((8, 3), np.uint8)


def test_create_splats_rejects_before_any_gpu_call(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU call in front of the argument checks")

    monkeypatch.setattr(splat_init, "knn", no_gpu)
    monkeypatch.setattr(splat_init, "splats_from_ply", no_gpu)
    monkeypatch.setattr(splat_init._lib, "lib", no_gpu)
    monkeypatch.setattr(torch, "rand", no_gpu)
    for arg in ("sparse_grad", "visible_adam"):
        with pytest.raises(NotImplementedError) as e:
            create_splats_with_optimizers(_Parser(), **{arg: True})
        assert arg in str(e.value)
    with pytest.raises(ValueError, match="Please specify a correct init_type: sfm, random, or ffgs"):
        create_splats_with_optimizers(_Parser(), init_type="colmap")
    with pytest.raises(ValueError, match="ply_path must be provided when using ffgs initialization"):
        create_splats_with_optimizers(None, init_type="ffgs")
    with pytest.raises(ValueError):
        create_splats_with_optimizers(None, init_type="sfm")
    with pytest.raises(ValueError):
        create_splats_with_optimizers(_Parser(), world_rank=2, world_size=2)
    with pytest.raises(ValueError):
        create_splats_with_optimizers(None, init_type="random", init_num_pts=3)


def test_signature_is_the_reference_s_plus_generator():
    import inspect
    p = inspect.signature(create_splats_with_optimizers).parameters
    want = dict(init_type="sfm", init_num_pts=100_000, init_extent=3.0, init_opacity=0.1, init_scale=1.0, means_lr=1.6e-4, scales_lr=5e-3,
                opacities_lr=5e-2, quats_lr=1e-3, sh0_lr=2.5e-3, shN_lr=2.5e-3 / 20, scene_scale=1.0, sh_degree=3, sparse_grad=False,
                visible_adam=False, batch_size=1, feature_dim=None, device="cuda", world_rank=0, world_size=1, ply_path=None, generator=None)
    assert list(p) == ["parser"] + list(want)
    assert {k: p[k].default for k in want} == want
