"""CPU: the restatement tests/eval_helper.py against the reference's own numbers (tests/golden/eval_*.npz, written by
tools/gen_golden_eval.py), the guard on the scenes, and what hunyuanworld_mirror_amd.metrics refuses before it touches a GPU."""
import os

import numpy as np
import pytest
import torch

import eval_helper as EH
from conftest import GOLD


def _gold(name):
    return dict(np.load(os.path.join(GOLD, f"eval_{name}.npz"), allow_pickle=False))


@pytest.mark.parametrize("name", ["a", "b"])
def test_helper_color_correct_matches_reference_fp64(name):
    z = _gold(name)
    img, ref = torch.from_numpy(z["img"]), torch.from_numpy(z["ref"])
    info = {}
    got = EH.color_correct(img.double(), ref.double(), info=info)
    err = float((got - torch.from_numpy(z["cc64"])).abs().max())
    print(f"scene {name}: restatement against the reference's fp64 {err:.3e}, smallest eigenvalue ratio {info['ratio_genuine']:.3e}")
    assert err <= 1e-12
    assert info["ratio_spurious"] == 0.0 and info["ratio_genuine"] > EH.CUTOFF      # full rank: nothing was dropped
    assert abs(info["ratio_genuine"] - float(z["ratio_genuine"])) <= 1e-6 * float(z["ratio_genuine"])
    # the reference's composition restated (lstsq), in fp64 the same result, in fp32 the reference's own fp32 error
    err_l = float((EH.color_correct_lstsq(img.double(), ref.double()) - torch.from_numpy(z["cc64"])).abs().max())
    assert err_l <= 1e-12
    e32 = EH.e32_of(img, ref)
    print(f"scene {name}: e32 fixture {float(z['e32']):.3e}, restated {e32:.3e}")
    assert 0.25 * float(z["e32"]) <= e32 <= 4.0 * float(z["e32"])


@pytest.mark.parametrize("name", ["a", "b"])
def test_scene_is_the_fixture_and_passes_the_guard(name):
    z = _gold(name)
    sc = EH.make_inputs(name)
    assert sc["seed"] == int(z["seed"]) and sc["e32"] == float(z["e32"])
    B, H, W, _ = EH.SCENES[name]
    img, ref = EH.draw_scene(B, H, W, sc["seed"])
    assert np.array_equal(img.numpy(), z["img"]) and np.array_equal(ref.numpy(), z["ref"])      # the fixture's inputs are the seed's
    assert np.array_equal(sc["img"].numpy(), z["img"]) and np.array_equal(sc["ref"].numpy(), z["ref"])
    assert sc["margin"] >= EH.GUARD_FACTOR * float(z["e32"])
    assert abs(sc["margin"] - float(z["margin"])) <= 1e-12
    # ref is 8-bit, so eps sits half a level from every value
    k = sc["ref"].double() * 255
    assert float((k - k.round()).abs().max()) < 1e-4


def test_guard_sees_a_value_at_a_threshold():
    img, ref = EH.draw_scene(1, 11, 11, 300)
    assert EH.guard_margin(img, ref) > 1e-4
    bad = img.clone()
    bad[0, 3, 4, 1] = EH.EPS + 1e-6
    assert EH.guard_margin(bad, ref) <= 1.1e-6
    bad_ref = ref.clone()
    bad_ref[0, 5, 5, 2] = 1 - EH.EPS
    assert EH.guard_margin(img, bad_ref) <= 1e-7


def test_cutoff_lies_between_the_recorded_ratios():
    z = dict(np.load(os.path.join(GOLD, "eval_ratios.npz"), allow_pickle=False))
    assert float(z["cutoff"]) == EH.CUTOFF
    assert z["ratio_spurious"].max() < 1e-3 * EH.CUTOFF and EH.CUTOFF < 1e-3 * z["ratio_genuine"].min()
    src = open(os.path.join(os.path.dirname(GOLD), "..", "hunyuanworld-mirror_amd", "csrc", "evalmetrics.hip")).read()
    assert "CC_CUTOFF = 1e-10" in src and EH.CUTOFF == 1e-10
    design = open(os.path.join(os.path.dirname(GOLD), "..", "DESIGN.md")).read()
    assert "1e-10" in design and f"{z['ratio_genuine'].min():.1e}" in design and f"{z['ratio_spurious'].max():.1e}" in design


def test_degenerate_systems_get_the_minimum_norm_solution():
    """grey input: rank 3; the projection recovers a per-channel quadratic of the grey value.  A saturated channel: w = 0, a zero channel."""
    g = torch.Generator().manual_seed(5)
    v = (0.1 + 0.8 * torch.rand(1, 20, 20, 1, generator=g)).float().double()
    grey = v.repeat(1, 1, 1, 3)
    ref = torch.cat([0.9 * v ** 2 + 0.05, 0.8 * v, 0.3 * v ** 2 + 0.5 * v + 0.1], dim=-1)
    info = {}
    got = EH.color_correct(grey, ref, info=info)
    assert float((got - ref).abs().max()) <= 1e-12 and 0 < info["ratio_spurious"] < 1e-13
    sat = EH.draw_scene(1, 20, 20, 6)[0].double()
    sat[..., 1] = 1.0
    out = EH.color_correct(sat, EH.draw_scene(1, 20, 20, 6)[1].double())
    assert torch.isfinite(out).all() and float(out[..., 1].abs().max()) == 0.0


def test_canvas_and_psnr_match_the_trainer_statements():
    z = _gold("frame")
    colors = torch.from_numpy(z["colors"])
    pixels = torch.from_numpy(z["pixels_u8"]).to(torch.float32) / 255.0
    assert np.array_equal(EH.canvas_bytes(colors, pixels), z["canvas"])
    got = EH.psnr64(colors, pixels)
    assert abs(got - float(z["psnr"])) <= 4 * np.finfo(np.float64).eps * abs(got)
    each = EH.psnr64(colors, pixels, per_image=True)
    assert np.abs(each - z["psnr_each"]).max() <= 4 * np.finfo(np.float64).eps * np.abs(each).max()


def test_exports():
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import bilagrid, metrics
    for n in ("color_correct", "psnr", "ssim", "eval_metrics", "Evaluator", "PeakSignalNoiseRatio", "StructuralSimilarityIndexMeasure"):
        assert getattr(wm, n) is getattr(metrics, n), n
    assert bilagrid.color_correct is metrics.color_correct
    assert "``color_correct`` (an evaluation-time" not in bilagrid.__doc__


def test_refusals_without_a_gpu():
    from hunyuanworld_mirror_amd import metrics as M
    img, ref = torch.rand(2, 12, 12, 3), torch.rand(2, 12, 12, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.color_correct(img, ref)
    with pytest.raises(NotImplementedError, match="3 channels"):
        M.color_correct(torch.rand(5, 4), torch.rand(5, 4))
    with pytest.raises(ValueError, match="channels must match"):
        M.color_correct(torch.rand(5, 3), torch.rand(5, 4))
    with pytest.raises(ValueError, match="one shape"):
        M.color_correct(torch.rand(5, 3), torch.rand(6, 3))
    with pytest.raises(ValueError, match="num_iters"):
        M.color_correct(img, ref, num_iters=-1)
    for eps in (0.0, 0.5, -0.1, 0.7):
        with pytest.raises(ValueError, match="eps"):
            M.color_correct(img, ref, eps=eps)
    with pytest.raises(TypeError, match="floating"):
        M.color_correct((img * 255).to(torch.uint8), ref)
    with pytest.raises(ValueError, match="per_image"):
        M.color_correct(torch.rand(5, 3), torch.rand(5, 3), per_image=True)
    with pytest.raises(ValueError, match="empty"):
        M.color_correct(torch.rand(0, 3), torch.rand(0, 3))
    a, b = torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 12)
    for fn in (M.psnr, M.ssim):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(a, b)
        with pytest.raises(ValueError, match="3 channels"):
            fn(torch.rand(1, 4, 12, 12), torch.rand(1, 4, 12, 12))
        with pytest.raises(ValueError, match="one shape"):
            fn(a, torch.rand(1, 3, 12, 13))
        with pytest.raises(ValueError, match="data_range"):
            fn(a, b, data_range=0.0)
        with pytest.raises(TypeError):
            fn(a.numpy(), b)
    with pytest.raises(ValueError, match="11 x 11"):
        M.ssim(torch.rand(1, 3, 10, 12), torch.rand(1, 3, 10, 12))
    with pytest.raises(RuntimeError, match="HIP device"):
        M.eval_metrics(img, ref)
    with pytest.raises(ValueError, match="3 channels"):
        M.eval_metrics(torch.rand(1, 12, 12, 4), torch.rand(1, 12, 12, 4))
    with pytest.raises(ValueError, match="11 x 11"):
        M.eval_metrics(torch.rand(1, 12, 10, 3), torch.rand(1, 12, 10, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        M.Evaluator(device="cpu")
    # the torchmetrics objects: per-call value only
    for cls in (M.PeakSignalNoiseRatio, M.StructuralSimilarityIndexMeasure):
        m = cls(data_range=1.0)
        assert m.to("cuda:0") is m
        with pytest.raises(NotImplementedError, match="update"):
            m.update(a, b)
        with pytest.raises(NotImplementedError, match="compute"):
            m.compute()
        with pytest.raises(NotImplementedError, match="reduction"):
            cls(data_range=1.0, reduction="sum")
        with pytest.raises(RuntimeError, match="HIP device"):
            m(a, b)


def test_entries_refuse_bad_arguments_before_any_launch():
    """status WM_ERR_INVALID (non-zero) from the C entries, with null streams and host pointers that are never dereferenced"""
    import ctypes as C
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    assert L.wm_eval_frame_workspace_bytes(1, 518, 518) == 8 * ((518 * 518 + 1023) // 1024)
    assert L.wm_eval_frame_workspace_bytes(0, 5, 5) == 0 and L.wm_eval_frame_workspace_bytes(70000, 5, 5) == 0
    assert L.wm_eval_frame_workspace_bytes(1, 40000, 40000) == 0
    assert L.wm_color_correct_workspace_bytes(1, 518 * 518) == 8 * (195 * ((518 * 518 + 511) // 512 + 1) + 30)
    assert L.wm_color_correct_workspace_bytes(0, 10) == 0 and L.wm_color_correct_workspace_bytes(1, 0) == 0
    assert L.wm_color_correct_workspace_bytes(1, 2 ** 31) == 0
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    q = C.c_void_p(buf.ctypes.data + 16384)
    st4 = (C.c_int64 * 4)(48, 12, 3, 1)
    assert L.wm_eval_frame(None, st4, p, st4, 1, 4, 4, 1, 1.0, None, None, None, None, p, 4096, None) != 0
    assert L.wm_eval_frame(p, st4, p, st4, 1, 4, 4, 1, 1.0, None, None, None, None, p, 4, None) != 0          # workspace too small
    assert L.wm_eval_frame(p, st4, p, st4, 1, 4, 4, 1, 0.0, None, None, None, None, p, 4096, None) != 0       # data_range
    assert L.wm_eval_frame(p, st4, p, st4, 1, 4, 4, 0, 1.0, None, q, None, None, p, 4096, None) != 0          # canvas without clamp
    assert L.wm_color_correct(p, p, 1, 16, 5, 0.5 / 255, p, q, 8192, None) != 0                                # out overlaps img
    assert L.wm_color_correct(p, p, 1, 16, -1, 0.5 / 255, q, q, 8192, None) != 0
    assert L.wm_color_correct(p, p, 1, 16, 5, 0.5, q, q, 8192, None) != 0
    assert L.wm_color_correct(p, p, 1, 16, 5, 0.5 / 255, q, q, 8, None) != 0
