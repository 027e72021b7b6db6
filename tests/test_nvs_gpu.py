"""GPU: the novel-view path (hunyuanworld_mirror_amd/nvs.py, csrc/frustum.hip, the count form of the select, context_nums in
WorldMirror.forward, gs_renderer.render).

Mask: equal to the reference's fp64 golden (tools/gen_golden_nvs.py) on every pixel that is not marginal there (tests/nvs_helper.py:
a threshold decision within 2^-10 of its threshold cannot be compared across arithmetic orders; at most 0.1 % of a scene), identical
bits on a repeat, a strided input against its contiguous copy, the context views in reversed order.
Filter: the kept rows are the reference's index set, in input order, for every tensor of the dict; ties to the lowest indices.
Forward and render: bit-for-bit against the plain forward's rows, prune_gs and rasterize_batches called directly."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import nvs_helper as NH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLAT_KEYS = ("means", "quats", "scales", "opacities", "sh", "weights")


def same(a, b):
    """bit-for-bit (NaN-proof), same shape"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ mask
@pytest.mark.parametrize("name", NH.MASK_SCENES + NH.HAND_SCENES)
def test_mask_equals_the_golden_off_the_marginal_pixels(name):
    from hunyuanworld_mirror_amd import calculate_in_frustum_mask
    z = NH.load(name)
    t = NH.scene_tensors(z, device=DEV)
    got = calculate_in_frustum_mask(*t)
    assert got.dtype == torch.bool and got.shape == z["mask64"].shape
    g = got.cpu().numpy()
    print(f"nvs_{name}: true {g.mean():.1%} (golden {z['mask64'].mean():.1%}), differs on {int((g != z['mask64']).sum())} pixels, "
          f"{int(z['marginal'].sum())} marginal")
    NH.assert_mask(g, z, name)
    assert torch.equal(calculate_in_frustum_mask(*t), got), "not the same bits on a repeat"
    d1, K1, c1, d2, K2, c2 = t                                   # the context views in reversed order: the same mask
    assert torch.equal(calculate_in_frustum_mask(d1, K1, c1, d2.flip(1), K2.flip(1), c2.flip(1)), got)


def test_mask_strided_input_equals_its_contiguous_copy():
    from hunyuanworld_mirror_amd import calculate_in_frustum_mask, calculate_unprojected_mask
    z = NH.load("a")
    d1, K1, c1, d2, K2, c2 = NH.scene_tensors(z, device=DEV)
    want = calculate_in_frustum_mask(d1, K1, c1, d2, K2, c2)
    big1 = torch.full((2, 3, 40, 2 * 45 + 3), 7.0, device=DEV)
    big1[..., 2:39, 1:91:2] = d1
    big2 = torch.zeros((2, 45, 2, 37), device=DEV)
    big2[:] = d2.permute(0, 3, 1, 2)
    s1, s2 = big1[..., 2:39, 1:91:2], big2.permute(0, 2, 3, 1)
    assert not s1.is_contiguous() and not s2.is_contiguous() and torch.equal(s1, d1) and torch.equal(s2, d2)
    assert torch.equal(calculate_in_frustum_mask(s1, K1, c1, s2, K2, c2), want)
    # calculate_unprojected_mask (frustum.py:7-23): context views first, 4x4 intrinsics cut to 3x3
    K4 = torch.eye(4, device=DEV).repeat(2, 5, 1, 1)
    K4[..., :3, :3] = torch.cat([K2, K1], 1)
    views = {"depthmap": torch.cat([d2, d1], 1), "camera_intrinsics": K4, "camera_pose": torch.cat([c2, c1], 1)}
    assert torch.equal(calculate_unprojected_mask(views, 2), want)


def test_mask_entry_refuses_bad_arguments_before_launching():
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    d = torch.ones(1, 1, 4, 4, device=DEV)
    k, r, m = torch.eye(3, device=DEV).reshape(1, 1, 3, 3), torch.eye(4, device=DEV)[:3].reshape(1, 1, 1, 3, 4), torch.zeros(16, device=DEV, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(d), p(d), p(k), p(r), p(k), 1, 1, 1, 4, 4, p(m), None]
    assert L.wm_in_frustum_mask(*args) == 0
    for i in (0, 1, 2, 3, 4, 10):
        bad = list(args)
        bad[i] = None
        assert L.wm_in_frustum_mask(*bad) == 1, i
    for i in (5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = 0
        assert L.wm_in_frustum_mask(*bad) == 1, i
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ filter
def _splats(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    sp = {"means": torch.randn(B, N, 3, generator=g), "quats": torch.randn(B, N, 4, generator=g), "scales": torch.rand(B, N, 3, generator=g),
          "opacities": torch.rand(B, N, generator=g), "sh": torch.randn(B, N, 1, 3, generator=g), "weights": torch.rand(B, N, generator=g)}
    sp = {k: v.to(DEV) for k, v in sp.items()}
    sp["gs_feats"] = torch.arange(5, device=DEV)
    return sp


def _check_filter(sp, conf, p, cap, kept):
    from hunyuanworld_mirror_amd import apply_confidence_filter
    out = apply_confidence_filter(sp, torch.from_numpy(conf).to(DEV), p, cap)
    idx = torch.from_numpy(kept).to(DEV)                       # ascending: the input order
    assert set(out) == set(sp) and out["gs_feats"] is sp["gs_feats"]
    for k in SPLAT_KEYS:
        want = torch.stack([sp[k][b][idx[b]] for b in range(idx.shape[0])])
        assert same(out[k], want), k


@pytest.mark.parametrize("case", ["p30", "p0", "cap", "k1", "p333"])
def test_filter_keeps_the_reference_set_in_input_order(case):
    """B = 2 (p30, cap), the max_gaussians cap, p = 0, K = 1, p = 33.3 (the count in double); N = 4099 spans two blocks of the select"""
    z = NH.load("filter")
    conf, kept = z[case + "_conf"], z[case + "_kept"]
    p, cap = float(z[case + "_params"][0]), int(z[case + "_params"][1])
    _check_filter(_splats(*conf.shape, seed=len(case)), conf, p, cap, kept)


def test_filter_tie_rule_nan_and_shaped_confidences():
    conf = np.array([[0.5, 0.9, 0.5, np.nan, 0.5, 1e-6, np.inf, 0.5]], np.float32)
    sp = _splats(1, 8, 3)
    for p, cap in ((50.0, 100), (25.0, 100), (0.0, 3), (0.0, 100)):
        _check_filter(sp, conf, p, cap, NH.filter_indices(conf, p, cap))
    from hunyuanworld_mirror_amd import apply_confidence_filter
    out = apply_confidence_filter(sp, torch.from_numpy(conf).to(DEV).reshape(1, 2, 2, 2), 50.0, 100)     # [B, S, H, W] as the forward gives it
    assert same(out["means"], sp["means"][:, [0, 1, 3, 6]])
    n = 3 * 4096 + 5                                           # one value everywhere: the first K rows, across the select's blocks
    sp = _splats(1, n, 4)
    _check_filter(sp, np.full((1, n), 2.0, np.float32), 30.0, 5000, np.arange(5000)[None])


# ------------------------------------------------------------------------------------------------ context_nums, render
@pytest.fixture(scope="module")
def scene():
    from conftest import load_golden
    from hunyuanworld_mirror_amd import WorldMirror
    cfg, views, flags, _, _ = load_golden("tiny_3v_70x56_pose_ray")
    cfg = dataclasses.replace(cfg, enable_gs=True)
    m = WorldMirror(arch=cfg).init_synthetic_weights().to(DEV)
    tv = {k: torch.from_numpy(v).to(DEV) for k, v in views.items()}
    plain = m(tv, flags)
    ctx2 = m({**tv, "context_nums": 2}, flags)
    torch.cuda.synchronize()
    return types_ns(m=m, cfg=cfg, tv=tv, flags=flags, plain=plain, ctx2=ctx2, H=70, W=56)


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def _same_tree(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return same(a, b)


def test_context_nums_builds_splats_from_the_context_views_only(scene):
    from hunyuanworld_mirror_amd.worldmirror import prune_gs
    s, rows = scene, 2 * scene.H * scene.W
    assert set(s.ctx2) == set(s.plain)
    for k in SPLAT_KEYS:
        assert s.plain["splats_raw"][k].shape[1] == 3 * s.H * s.W
        assert same(s.ctx2["splats_raw"][k], s.plain["splats_raw"][k][:, :rows]), k
    assert _same_tree(s.ctx2["splats"], prune_gs({k: s.plain["splats_raw"][k][:, :rows] for k in SPLAT_KEYS}))
    assert s.ctx2["splats"]["means"][0].shape[0] < s.plain["splats"]["means"][0].shape[0]
    for k in s.plain:
        if k not in ("splats", "splats_raw"):
            assert _same_tree(s.ctx2[k], s.plain[k]), k
    assert _same_tree(s.m({**s.tv, "context_nums": 3}, s.flags), s.plain)
    for bad in (0, 4):
        with pytest.raises(ValueError):
            s.m({**s.tv, "context_nums": bad}, s.flags)


def test_context_nums_on_a_sharded_handle_raises(scene):
    from hunyuanworld_mirror_amd import WorldMirror, _lib
    L = _lib.lib()
    grp = C.c_void_p(L.wm_local_group_create(2))
    m = WorldMirror(arch=scene.cfg).init_synthetic_weights().to(DEV).shard_local(grp, 0, 2)
    with pytest.raises(NotImplementedError):
        m({**scene.tv, "context_nums": 2}, scene.flags)
    m.gs_renderer.enable_conf_filter = True
    with pytest.raises(NotImplementedError):
        m(scene.tv, scene.flags)
    del m
    L.wm_local_group_destroy(grp)


def test_forward_confidence_filter_runs_in_front_of_prune(scene):
    from hunyuanworld_mirror_amd import apply_confidence_filter
    from hunyuanworld_mirror_amd.worldmirror import prune_gs
    s, r = scene, scene.m.gs_renderer
    r.enable_conf_filter, r.conf_threshold_percent = True, 40.0
    try:
        got = s.m({**s.tv, "context_nums": 2}, s.flags)
    finally:
        r.enable_conf_filter, r.conf_threshold_percent = False, 30.0
    assert _same_tree(got["splats_raw"], s.ctx2["splats_raw"])
    kept = apply_confidence_filter(s.ctx2["splats_raw"], s.plain["depth_conf"][:, :2], 40.0)
    assert kept["means"].shape[1] == NH.keep_count(2 * s.H * s.W, 40.0, 5_000_000)
    assert _same_tree(got["splats"], prune_gs(kept))


def test_render_equals_direct_rasterisation_for_every_chunk_size(scene):
    from hunyuanworld_mirror_amd import calculate_unprojected_mask
    s, r = scene, scene.m.gs_renderer
    views = {**s.tv, "context_nums": 2}
    sp = s.ctx2["splats"]
    c, d, a = r.rasterizer.rasterize_batches(sp["means"], sp["quats"], sp["scales"], sp["opacities"], sp["sh"], s.ctx2["camera_poses"],
                                             s.ctx2["camera_intrs"], width=s.W, height=s.H, sh_degree=0)
    outs = [r.render(s.tv["img"], dict(s.ctx2), views, chunk_size=cs) for cs in (1, 2, 4)]
    for o in outs:
        assert o["rendered_colors"].shape == (1, 3, s.H, s.W, 3) and o["rendered_depths"].shape == (1, 3, s.H, s.W, 1)
        assert same(o["rendered_colors"], c) and same(o["rendered_depths"], d) and same(o["rendered_alphas"], a)
        assert same(o["gt_colors"], s.tv["img"].permute(0, 1, 3, 4, 2))
        assert same(o["rendered_extrinsics"], s.ctx2["camera_poses"]) and same(o["rendered_intrinsics"], s.ctx2["camera_intrs"])
        assert o["splats"] is sp
        assert o["valid_masks"].shape == (1, 1, s.H, s.W) and torch.equal(o["valid_masks"], calculate_unprojected_mask(s.tv, 2))
    assert "rendered_colors" not in s.ctx2                      # the test's own copy was filled, not the fixture
    o = r.render(s.tv["img"], dict(s.ctx2), {"context_nums": 2})
    assert "valid_masks" not in o and same(o["rendered_colors"], c)
    o = r.render(s.tv["img"], dict(s.plain))                    # no views: every view is a context view
    assert "valid_masks" not in o and o["rendered_colors"].shape == (1, 3, s.H, s.W, 3)


def test_render_with_context_predictions_rescales_cameras_and_rebuilds_means(scene):
    from hunyuanworld_mirror_amd import depth_to_world_coords_points
    s, r = scene, scene.m.gs_renderer
    ctx = s.m({k: v[:, :2] for k, v in s.tv.items()}, s.flags)         # the two-view forward of the same inputs
    r.enable_prune = False
    try:
        o = r.render(s.tv["img"], dict(s.ctx2), {**s.tv, "context_nums": 2}, context_predictions=ctx)
    finally:
        r.enable_prune = True
    # the scale factor of rasterization.py:194-202 in fp64 (the restatement); the fp32 evaluation rounds each of the two 6-term means,
    # the sum with 1e-6, the quotient and the product: <= (6 + 6 + 3) eps32 relative to sum |t| / |sum t| of each mean
    pa, pc = s.ctx2["camera_poses"].double().cpu(), ctx["camera_poses"].double().cpu()
    sf = NH.translation_scale(pc, pa, 2)
    cond = sum(float(t[:, :2, :3, 3].abs().sum() / t[:, :2, :3, 3].sum().abs()) for t in (pa, pc))
    tol = 16 * 2.0 ** -24 * (cond + 1)
    want = pa[..., :3, 3] * sf
    got = o["rendered_extrinsics"].double().cpu()
    print("scale factor", float(sf), "cond", cond, "max rel err", float(((got[..., :3, 3] - want).abs() / want.abs().clamp_min(1e-30)).max()), "tol", tol)
    assert ((got[..., :3, 3] - want).abs() <= tol * want.abs()).all()
    assert same(o["rendered_extrinsics"][..., :3, :3], s.ctx2["camera_poses"][..., :3, :3]) and same(o["rendered_extrinsics"][..., 3, :], s.ctx2["camera_poses"][..., 3, :])
    assert same(s.ctx2["camera_poses"], s.plain["camera_poses"])        # the prediction itself is not written to
    pts, _, _ = depth_to_world_coords_points(s.ctx2["gs_depth"][:, :2].reshape(2, s.H, s.W), ctx["camera_poses"].reshape(2, 4, 4),
                                             ctx["camera_intrs"].reshape(2, 3, 3))
    assert same(o["splats"]["means"], pts.reshape(1, 2 * s.H * s.W, 3))
    for k in SPLAT_KEYS[1:]:
        assert same(o["splats"][k], s.ctx2["splats_raw"][k]), k
    assert o["rendered_colors"].shape == (1, 3, s.H, s.W, 3) and o["valid_masks"].shape == (1, 1, s.H, s.W)
