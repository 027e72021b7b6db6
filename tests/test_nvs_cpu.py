"""CPU: the novel-view path's goldens (tools/gen_golden_nvs.py: the reference's own code on fp32-valued inputs) against the torch
restatement of tests/nvs_helper.py, and the argument checks of hunyuanworld_mirror_amd.nvs, which come before the first GPU call."""
import numpy as np
import pytest
import torch

import nvs_helper as NH


@pytest.mark.parametrize("name", NH.MASK_SCENES + NH.HAND_SCENES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_reproduces_the_golden_masks(name, dtype):
    """equal to the reference's fp64 mask on every non-marginal pixel, in fp64 and in fp32; the stored marginal flags are the helper's"""
    z = NH.load(name)
    NH.assert_mask(NH.in_frustum_mask(*NH.scene_tensors(z, dtype)).numpy(), z, name)
    NH.assert_mask(z["mask32"], z, name + " (the reference in fp32)")
    assert np.array_equal(NH.marginal_pixels(*NH.scene_tensors(z)).numpy(), z["marginal"])
    if name in NH.MASK_SCENES:
        assert z["marginal"].sum() <= NH.MAX_MARGINAL * z["marginal"].size


def test_golden_scene_shapes_and_hand_cases():
    shapes = {"a": (2, 3, 2, 37, 45), "b": (1, 2, 3, 19, 70), "c": (1, 1, 1, 5, 7), "d": (1, 1, 2, 16, 16)}
    for name, (B, V1, V2, H, W) in shapes.items():
        z = NH.load(name)
        assert z["depth_1"].shape == (B, V1, H, W) and z["depth_2"].shape == (B, V2, H, W) and z["mask64"].shape == (B, V1, H, W)
        assert z["depth_1"].dtype == np.float32 and (z["depth_1"] == 0).any()
    z = NH.load("hand_split")   # x = 1: inside view A's frustum only, matching in view B only, through a footprint over B's border
    t = NH.scene_tensors(z, torch.float64)
    p2d, zc = NH.project(t[0], t[1], t[2], t[4], t[5])
    s = NH.sample(t[3], p2d)
    px, close = p2d[0, 0, :, 1:, 1, 0], torch.isclose(zc, s, atol=1e-1)[0, 0, :, 1:, 1]
    assert (px[0] > 0).all() and (px[1] < 0).all() and (px[1] > -0.5).all()
    assert not close[0].any() and close[1].all() and z["mask64"][0, 0, 1:, 1].all()
    z = NH.load("hand_nan")
    assert np.isnan(z["depth_1"]).sum() == 1 and np.isnan(z["depth_2"]).sum() == 1
    assert not z["mask64"][0, 0, 3, 3] and not z["mask64"][0, 0, 5:7, 5:7].any() and z["mask64"][0, 0, 4, 4]


def test_fp64_matrices_of_the_binding_reproduce_the_projection():
    """the binding's K1^-1 and c2w_2^-1 c2w_1 (nvs.frustum_matrices) give the restatement's projected points"""
    from hunyuanworld_mirror_amd import nvs
    z = NH.load("a")
    d1, K1, c1, d2, K2, c2 = NH.scene_tensors(z, torch.float64)
    kinv, rel = nvs.frustum_matrices(K1.float(), c1.float(), c2.float())
    assert kinv.dtype == torch.float64 and rel.shape == (2, 3, 2, 3, 4)
    h, w = d1.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    cam = torch.einsum("bvij,hwj->bvhwi", kinv, torch.stack([xs, ys, torch.ones_like(xs)], -1)) * d1[..., None]
    p = torch.einsum("bvuij,bvhwj->bvuhwi", rel[..., :3], cam) + rel[..., 3][:, :, :, None, None]
    p2d = torch.einsum("buij,bvuhwj->bvuhwi", K2, p / p[..., 2:])[..., :2]
    ref2d, refz = NH.project(d1, K1, c1, K2, c2)
    ok = torch.isfinite(ref2d).all(-1) & (refz.abs() > 1e-2)
    assert (p2d - ref2d)[ok].abs().max() < 1e-9 and (p[..., 2] - refz)[ok].abs().max() < 1e-12


def test_filter_restatement_reproduces_the_reference_index_sets():
    z = NH.load("filter")
    names = sorted(k[:-5] for k in z if k.endswith("_conf"))
    assert names == ["cap", "k1", "p0", "p30", "p333"]
    for n in names:
        p, cap = float(z[n + "_params"][0]), int(z[n + "_params"][1])
        got = NH.filter_indices(z[n + "_conf"], p, cap)
        assert np.array_equal(got, z[n + "_kept"]), n
        assert got.shape[1] == NH.keep_count(z[n + "_conf"].shape[1], p, cap)
    assert z["k1_kept"].shape[1] == 1 and z["cap_kept"].shape[1] == 100 and z["p333_kept"].shape[1] == 667


def test_filter_restatement_tie_and_nan_rules():
    conf = np.array([[0.5, 0.9, 0.5, np.nan, 0.5, 1e-6, np.inf, 0.5]], np.float32)
    assert NH.filter_indices(conf, 50.0, 100).tolist() == [[0, 1, 3, 6]]        # NaN, +inf, 0.9, then the first of the four 0.5
    assert NH.filter_indices(conf, 25.0, 100).tolist() == [[0, 1, 2, 3, 4, 6]]  # ties to the lowest indices
    assert NH.filter_indices(conf, 0.0, 3).tolist() == [[1, 3, 6]]
    from hunyuanworld_mirror_amd import nvs
    for n, p, cap in ((1000, 33.3, 5_000_000), (7, 0.0, 3), (5, 100.0, 9), (4099, 30.0, 100)):
        assert nvs.filter_keep_count(n, p, cap) == NH.keep_count(n, p, cap)


def test_scale_factor_restatement():
    z = NH.load("scale")
    S = int(z["S"])
    a, c = torch.from_numpy(z["all_c2w"]).double(), torch.from_numpy(z["ctx_c2w"]).double()
    sf = NH.translation_scale(c, a, S)
    eps = np.finfo(np.float64).eps
    assert np.abs(sf.numpy() - z["scale_factor"]).max() <= 4 * eps * np.abs(z["scale_factor"]).max()
    scaled = a.clone()
    scaled[..., :3, 3] = scaled[..., :3, 3] * sf
    assert np.abs(scaled.numpy() - z["scaled_c2w"]).max() <= 8 * eps * np.abs(z["scaled_c2w"]).max()
    from hunyuanworld_mirror_amd import nvs
    assert torch.equal(nvs.translation_scale(c, a, S), sf)


# ------------------------------------------------------------------------------------------------ argument errors, no GPU needed
def _views(n=3, h=6, w=5):
    return {"depthmap": torch.ones(1, n, h, w), "camera_intrinsics": torch.eye(4)[None, None].repeat(1, n, 1, 1),
            "camera_pose": torch.eye(4)[None, None].repeat(1, n, 1, 1)}


def test_mask_argument_errors_come_before_the_gpu():
    from hunyuanworld_mirror_amd import calculate_in_frustum_mask, calculate_unprojected_mask
    d, K, P = torch.ones(1, 2, 6, 5), torch.eye(3)[None, None].repeat(1, 2, 1, 1), torch.eye(4)[None, None].repeat(1, 2, 1, 1)
    with pytest.raises(ValueError):
        calculate_in_frustum_mask(d[0], K, P, d, K, P)
    with pytest.raises(ValueError):
        calculate_in_frustum_mask(d, K[:, :1], P, d, K, P)
    with pytest.raises(ValueError):
        calculate_in_frustum_mask(d, K, P[..., :3, :], d, K, P)
    with pytest.raises(ValueError):
        calculate_in_frustum_mask(d, K, P, d[..., :4], K, P)
    with pytest.raises(ValueError):
        calculate_in_frustum_mask(d, K, P, d[:, :0], K[:, :0], P[:, :0])
    with pytest.raises(RuntimeError):
        calculate_in_frustum_mask(d, K, P, d, K, P)                   # well-formed, but on the CPU: there is no CPU path
    v = _views()
    for bad in (0, 3, 4, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            calculate_unprojected_mask(v, bad)
    with pytest.raises(ValueError):
        calculate_unprojected_mask({k: x for k, x in v.items() if k != "camera_pose"}, 1)
    with pytest.raises(RuntimeError):
        calculate_unprojected_mask(v, 2)                               # 4x4 intrinsics are cut to 3x3, then the device is refused


def test_filter_and_forward_argument_errors_come_before_the_gpu():
    from hunyuanworld_mirror_amd import WMConfig, WorldMirror, apply_confidence_filter
    sp = {"means": torch.zeros(1, 10, 3), "weights": torch.zeros(1, 10)}
    with pytest.raises(ValueError):
        apply_confidence_filter(sp, torch.zeros(1, 9))
    with pytest.raises(ValueError):
        apply_confidence_filter({"means": torch.zeros(10, 3)}, torch.zeros(10))
    with pytest.raises(RuntimeError):
        apply_confidence_filter(sp, torch.zeros(1, 2, 5))
    m = WorldMirror(arch=WMConfig.tiny())
    r = m.gs_renderer
    assert (r.enable_conf_filter, r.conf_threshold_percent, r.max_gaussians) == (False, 30.0, 5_000_000)
    assert r.apply_confidence_filter(sp, torch.zeros(1, 10)) is sp     # filter off: untouched, as rasterization.py:260-261
    m._handle = object()                                               # stands in for a device handle: the checks below come first
    img = torch.rand(1, 3, 3, 70, 56)
    for bad in (0, 4, 2.0, "2"):
        with pytest.raises(ValueError):
            m({"img": img, "context_nums": bad})
    m._comm = (0, 2)
    with pytest.raises(NotImplementedError):
        m({"img": img, "context_nums": 2})
    r.enable_conf_filter = True
    with pytest.raises(NotImplementedError):
        m({"img": img})
    m._handle = None
    with pytest.raises(ValueError):
        r.render(torch.rand(1, 3, 70, 56), {})
    with pytest.raises(ValueError):
        r.render(img, {"camera_poses": torch.eye(4)[None, None], "camera_intrs": torch.eye(3)[None, None]}, {"context_nums": 5})
