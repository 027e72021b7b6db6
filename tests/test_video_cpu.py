"""CPU: the fly-through video's restatement (tests/video_helper.py) against the reference's recorded results (tests/golden/video_*.npz,
tools/gen_golden_video.py), the public camera paths on CPU tensors, the colour table and the argument errors of
hunyuanworld_mirror_amd.video.  No GPU.

The reference casts its cameras to fp32 in front of the rasteriser (render_utils.py:245), so the recorded paths are fp32 numbers: ext32 from
an fp32 run (the restatement in fp32 follows the same operations), ext64r from an fp64 run rounded once by that cast (the restatement in
fp64, rounded the same way, may differ by one fp32 ulp where the two fp64 values straddle a rounding boundary)."""
import sys

import numpy as np
import pytest
import torch

import video_helper as VH


def _ulp_of_max(a):
    return float(np.spacing(np.float32(np.abs(a).max())))


def test_helper_paths_reproduce_the_reference():
    z = VH.load_golden("traj")
    n = int(z["n"])
    e32, i32 = VH.interpolated_traj(z["c2w"], z["K"], n, torch.float32)
    e64, i64 = VH.interpolated_traj(z["c2w"], z["K"], n, torch.float64)
    S = z["c2w"].shape[1]
    assert tuple(e32.shape) == (1, (S - 1) * (n + 1), 4, 4) and tuple(e32.shape[1:]) == tuple(z["ext32"].shape)
    for got, ref in ((e32[0], z["ext32"]), (i32[0], z["int32"]), (e64[0].float(), z["ext64r"]), (i64[0].float(), z["int64r"])):
        err = float(np.abs(got.numpy().astype(np.float64) - ref).max())
        print("path: max |helper - reference|", err, "ulp of the largest entry", _ulp_of_max(ref))
        assert err <= _ulp_of_max(ref)
    # fp64 round-off proper: the fp64 restatement against itself is exact, against the fp32-rounded record it is half an ulp
    assert VH.max_rel(e64[0].numpy(), z["ext64r"]) <= 2.0 ** -24
    delta = torch.from_numpy(z["wob_means"])[0].median(dim=0).values.norm(dim=-1)[None]
    we, wi = VH.wobble_traj(z["wob_c2w"], z["wob_K"], z["wob_ext"].shape[0], delta, torch.float32)
    assert np.abs(we[0].numpy() - z["wob_ext"]).max() <= _ulp_of_max(z["wob_ext"]) and np.array_equal(wi[0].numpy(), z["wob_int"])


def test_path_fixture_takes_every_branch():
    z = VH.load_golden("traj")
    R = torch.from_numpy(z["c2w"][0, :, :3, :3])
    assert sorted(set(VH.quat_branch(R))) == [1, 2, 3, 4]
    q = VH.quat_from_rot(R.double())
    dots = (q[:-1] * q[1:]).sum(-1)
    assert bool((dots.abs() > 0.9995).any()) and bool((dots < 0).any()) and bool((dots.abs() < 0.9995).any())


def test_helper_effect_reproduces_the_reference_in_fp64():
    z = VH.load_golden("effect")
    worst = 0.0
    for ti, t_n in enumerate(VH.T_CASES):
        for ig in (0, 1):
            got = VH.spread_effect(z["means"], z["scales"], z["opacities"], z["colors"], z["random_vals"], t_n, bool(ig), torch.float64)
            for k in ("means", "scales", "opacities", "colors", "flag"):
                worst = max(worst, VH.max_rel(got[k].numpy(), z[f"t{ti}_i{ig}_{k}"]))
    print("effect: worst relative error of the fp64 restatement", worst)
    assert worst <= 1e-14
    # the cases cover the wave before it starts, in flight and saturated
    assert z["t0_i0_flag"].min() == 1.0 and 0 < (z["t3_i0_flag"] < 0.99).mean() < 1 and z["t5_i0_flag"].max() == 0.0


def test_helper_depth_vis_and_bytes_reproduce_the_reference_video():
    z, lut = VH.load_golden("frames"), VH.load_golden("turbo")["lut"]
    F = z["depth"].shape[0]
    dep = np.stack([lut[VH.turbo_rows(VH.depth_vis_x(z["depth"][f], torch.float32)[0].numpy())] for f in range(F)])
    rgb = (torch.from_numpy(z["rgb"]).clamp(0, 1) * 255).to(torch.uint8).numpy()
    loop = lambda v: np.concatenate([v, v[::-1][1:-1]], axis=0)
    assert np.array_equal(loop(dep), z["video_depth"]) and np.array_equal(loop(rgb), z["video_rgb"])
    assert (z["depth"] == 0).mean() > 0.02          # holes are there


def test_turbo_table_is_matplotlibs():
    from hunyuanworld_mirror_amd import video
    lut = VH.load_golden("turbo")["lut"]
    got = video.turbo_lut().numpy()
    assert got.dtype == np.uint8 and got.shape == (256, 3) and np.array_equal(got, lut)


@pytest.mark.parametrize("name", ["fx_a", "fx_b"])
def test_helper_schedule_reproduces_the_reference(name):
    z = VH.load_golden(name)
    sched, seen, _, _ = VH.golden_schedule(z)
    assert [s[2] for s in sched] == list(z["t"][:, 0]) and len(sched) == z["ext"].shape[0]
    kept = sum(1 for s in sched if s[3])
    assert 2 * kept - 2 == int(z["n_video"])
    assert np.abs(seen - 0.01).min() > 1e-4 and np.abs(z["stats"][:, 1] - 0.01).min() > 1e-4
    if name == "fx_b":      # the bookkeeping is exercised: t comes back
        assert max(s[2] for s in sched) > sched[-1][2]


def test_public_paths_on_cpu_tensors():
    """the yardstick of test_bilagrid_gpu.py: the restatement's own fp32-against-fp64 error on the same inputs, times 4, never less
    than one ulp"""
    import hunyuanworld_mirror_amd as wm
    z = VH.load_golden("traj")
    n = int(z["n"])
    c2w, K = torch.from_numpy(z["c2w"]), torch.from_numpy(z["K"])
    ext, ints = wm.interpolate_trajectory(c2w, K, n)
    e32, i32 = VH.interpolated_traj(z["c2w"], z["K"], n, torch.float32)
    e64, i64 = VH.interpolated_traj(z["c2w"], z["K"], n, torch.float64)
    assert ext.dtype == torch.float32 and tuple(ext.shape[1:]) == tuple(z["ext32"].shape) and tuple(ints.shape[1:]) == tuple(z["int32"].shape)
    for tag, got, f32, ref, gold in (("ext", ext, e32, e64, z["ext32"]), ("int", ints, i32, i64, z["int32"])):
        yard = max(VH.max_rel(f32.numpy(), ref.numpy()), VH.ULP)
        err = VH.max_rel(got.numpy(), ref.numpy())
        print(f"{tag}: yardstick {yard:.3e} public {err:.3e} ratio {err / yard:.2f}; against the fp32 record {VH.max_rel(got[0].numpy(), gold):.3e}")
        assert err <= VH.FACTOR * yard and VH.max_rel(got[0].numpy(), gold) <= VH.FACTOR * yard
    # camera i itself is emitted unchanged and the last camera is not emitted
    assert torch.equal(ext[0, ::n + 1], c2w[0, :-1]) and not bool((ext[0] == c2w[0, -1]).all(dim=(-1, -2)).any())
    delta = torch.from_numpy(z["wob_means"])[0].median(dim=0).values.norm(dim=-1)[None]
    nums = z["wob_ext"].shape[0]
    we, wi = wm.wobble_trajectory(torch.from_numpy(z["wob_c2w"]), torch.from_numpy(z["wob_K"]), nums, delta)
    w32, _ = VH.wobble_traj(z["wob_c2w"], z["wob_K"], nums, delta, torch.float32)
    w64, _ = VH.wobble_traj(z["wob_c2w"], z["wob_K"], nums, delta, torch.float64)
    yard = max(VH.max_rel(w32.numpy(), w64.numpy()), VH.ULP)
    assert VH.max_rel(we.numpy(), w64.numpy()) <= VH.FACTOR * yard and np.array_equal(wi[0].numpy(), z["wob_int"])
    # the quaternion helpers round-trip
    R = c2w[0, :, :3, :3]
    back = wm.quaternion_to_rotation_matrix(wm.rotation_matrix_to_quaternion(R))
    assert float((back - R).abs().max()) < 1e-5
    q = wm.rotation_matrix_to_quaternion(R)
    assert torch.allclose(wm.slerp_quaternions(q, q, 0.3), q, atol=1e-6)


def test_argument_errors(monkeypatch):
    import hunyuanworld_mirror_amd as wm
    sc = VH.effect_scene(16, 1)
    g = {k: torch.from_numpy(v) for k, v in sc.items() if k != "random_vals"}
    fx = wm.GSEffects(0.0, 10.0, random_vals=torch.from_numpy(sc["random_vals"]))
    with pytest.raises(NotImplementedError, match="effect_type"):
        fx.apply_effect(g, 1.0, effect_type=1)
    with pytest.raises(RuntimeError, match="GPU"):
        fx.apply_effect(g, 1.0, effect_type=2)
    with pytest.raises(RuntimeError, match="GPU"):
        wm.depth_frames(torch.ones(2, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        wm.rgb_frames(torch.ones(2, 4, 4, 3))
    c2w, K = torch.eye(4).repeat(1, 3, 1, 1), torch.eye(3).repeat(1, 3, 1, 1)

    class NoRenderer:
        def __getattr__(self, name):
            raise AssertionError("the renderer was touched before the arguments were checked")

    for mod in ("moviepy", "moviepy.editor"):
        monkeypatch.setitem(sys.modules, mod, None)      # import of either now raises ImportError
    with pytest.raises(ImportError, match="moviepy"):
        wm.render_interpolated_video(NoRenderer(), {}, c2w, K, (4, 4), "/nonexistent/out")
    with pytest.raises(ValueError, match="save_mode"):
        wm.render_interpolated_frames(NoRenderer(), {}, c2w, K, (4, 4), save_mode="neither")
    with pytest.raises(NotImplementedError, match="effect_type"):
        wm.render_interpolated_frames(NoRenderer(), {}, c2w, K, (4, 4), effects=fx, effect_type=1)
    with pytest.raises(ValueError):
        wm.interpolate_trajectory(c2w[:, :1], K[:, :1], 4)
