"""The trainer's evaluation on the GPU (wm_eval_frame, wm_color_correct through hunyuanworld_mirror_amd.metrics) against the fp64
restatement tests/eval_helper.py, which tests/test_eval_cpu.py pins to the reference's own numbers (tests/golden/eval_*.npz).

color_correct: max |gpu - fp64 helper| <= 4 e32, e32 = the reference's own fp32-against-fp64 error on the same scene (from the fixture;
computed from the restated composition where there is none).  The kernel rounds img_mat to fp32 once per iteration as the fp32
reference does and forms everything else in fp64, so it should sit inside the reference's fp32 error; 4 is the project's usual margin.
Largest ratio measured on MI355X: 0.22 (fixture a; 0.21 on fixture b, 0.19 at 11 x 11, 0.04 at 300 x 301, 0.14 on the pair;
profiles/r21_eval_metrics.md).

Sizes, by the seam each crosses (colour correction: blocks of 512 pixels staged in two rounds of 256, their partials added in block
order with the loads of 16 blocks in flight; eval frame: blocks of 1024 pixels, whose partials the finishing block takes 256 at a time):
  11 x 11     the SSIM minimum; one block, one partial round (121 pixels: a full wave and a partial one)
  37 x 52     1924 pixels: 4 colour blocks, the last with one full and one partial round; 2 frame blocks
  61 x 83     5063 pixels: 10 colour blocks (fewer than one group of 16), the last partial; 5 frame blocks, the last partial
  300 x 301   177 colour blocks: 11 groups of 16 partials and a remainder of one, the last block a partial first round; 89 frame blocks
  518 x 518   (PSNR only) 263 frame blocks: more partials than the finishing block's 256 lanes take in one step
  [2,37,52,3] as one system (3848 pixels) and per_image (the image index on the grid's second dimension)"""
import json
import os

import numpy as np
import pytest
import torch

import eval_helper as EH

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _dev():
    return torch.device("cuda:0")


def _M():
    from hunyuanworld_mirror_amd import metrics
    return metrics


def _cc(img, ref, **kw):
    out = _M().color_correct(img.to(_dev()), ref.to(_dev()), **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.cpu().reshape(-1).numpy().view(np.uint8), b.cpu().reshape(-1).numpy().view(np.uint8))


@pytest.mark.parametrize("name", ["a", "b", "min", "big", "pair"])
def test_color_correct_within_the_reference_fp32_error(name):
    sc = EH.make_inputs(name)
    want = EH.color_correct(sc["img"].double(), sc["ref"].double())
    got = _cc(sc["img"], sc["ref"])
    assert got.dtype == torch.float32 and got.shape == sc["img"].shape and torch.isfinite(got).all()
    err = float((got.double() - want).abs().max())
    print(f"color_correct {name} {tuple(sc['img'].shape)}: e32 {sc['e32']:.3e} gpu {err:.3e} ratio {err / sc['e32']:.3f}")
    assert err <= FACTOR * sc["e32"]
    if "cc64" in sc:        # and against the reference's own fp64 output
        assert float((got.double() - sc["cc64"]).abs().max()) <= FACTOR * sc["e32"]


@pytest.mark.parametrize("iters", [1, 2])
def test_color_correct_fewer_iterations(iters):
    sc = EH.make_inputs("a")
    e32 = EH.e32_of(sc["img"], sc["ref"], num_iters=iters)
    want = EH.color_correct(sc["img"].double(), sc["ref"].double(), num_iters=iters)
    err = float((_cc(sc["img"], sc["ref"], num_iters=iters).double() - want).abs().max())
    print(f"color_correct a, {iters} iterations: e32 {e32:.3e} gpu {err:.3e} ratio {err / e32:.3f}")
    assert err <= FACTOR * e32


def test_color_correct_zero_iterations_returns_the_input():
    sc = EH.make_inputs("min")
    img = sc["img"].to(_dev())
    assert _M().color_correct(img, sc["ref"].to(_dev()), num_iters=0) is img


def test_color_correct_per_image_equals_single_calls():
    sc = EH.make_inputs("pair")
    both = _cc(sc["img"], sc["ref"], per_image=True)
    one = _cc(sc["img"], sc["ref"])
    for b in range(2):
        single = _cc(sc["img"][b], sc["ref"][b])
        assert _bits(both[b], single), b
        want = EH.color_correct(sc["img"][b].double(), sc["ref"][b].double())
        assert float((both[b].double() - want).abs().max()) <= FACTOR * sc["e32"]
    assert not _bits(both, one)          # two fits are not the joint fit


def test_color_correct_strided_view_and_repeat_are_bit_identical():
    sc = EH.make_inputs("b")
    dev = _dev()
    four = torch.cat([sc["img"], torch.full_like(sc["img"][..., :1], 7.0)], dim=-1).to(dev)
    view = four[..., :3]
    assert not view.is_contiguous()
    ref = sc["ref"].to(dev)
    a = _M().color_correct(view, ref)
    b = _M().color_correct(sc["img"].to(dev), ref)
    c = _M().color_correct(sc["img"].to(dev), ref)
    torch.cuda.synchronize()
    assert _bits(a, b) and _bits(b, c)
    # other dtypes come back in their own
    h = _M().color_correct(sc["img"].to(dev).double(), ref.double())
    assert h.dtype == torch.float64 and _bits(h.float(), b)


def test_color_correct_grey_image_is_projected():
    """rank 3 of 10: a per-channel quadratic of the grey value is recovered to the fp32 rounding of ref (8 * 2^-24 on values in [0, 1])"""
    g = torch.Generator().manual_seed(11)
    v = (0.1 + 0.8 * torch.rand(1, 37, 52, 1, generator=g)).float()
    img = v.repeat(1, 1, 1, 3).contiguous()
    vd = v.double()
    ref = torch.cat([0.9 * vd ** 2 + 0.05, 0.8 * vd, 0.3 * vd ** 2 + 0.5 * vd + 0.1], dim=-1).float()
    got = _cc(img, ref)
    err = float((got.double() - ref.double()).abs().max())
    print(f"grey image: max |corrected - ref| {err:.3e} (bound {8 * 2.0 ** -24:.3e})")
    assert torch.isfinite(got).all() and err <= 8 * 2.0 ** -24


def test_color_correct_saturated_channel_gives_a_zero_channel():
    sc = EH.make_inputs("a")
    img = sc["img"].clone()
    img[..., 1] = 1.0
    got = _cc(img, sc["ref"])
    assert torch.isfinite(got).all()
    assert float(got[..., 1].abs().max()) == 0.0
    assert float(got[..., 0].max()) > 0.5 and float(got[..., 2].max()) > 0.5 and float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def _psnr_gpu(colors, pixels, **kw):
    out = _M().psnr(colors.to(_dev()).permute(0, 3, 1, 2), pixels.to(_dev()).permute(0, 3, 1, 2), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.dim() == 0
    return float(out)


@pytest.mark.parametrize("shape", [(1, 11, 11), (2, 37, 52), (1, 61, 83), (1, 518, 518)])
def test_psnr_matches_fp64(shape):
    colors, pixels = EH.frame_inputs(*shape, seed=sum(shape))
    clamped = torch.clamp(colors, 0, 1)
    for tag, c in (("clamped", clamped), ("raw", colors)):
        want = EH.psnr64(c, pixels, clamp=False)
        got = _psnr_gpu(c, pixels)
        print(f"psnr {shape} {tag}: fp64 {want:.9f} gpu {got:.9f} |diff| / |psnr| {abs(got - want) / abs(want):.3e}")
        assert abs(got - want) <= 2 * 2.0 ** -24 * abs(want)
    # contiguous [B,3,H,W] input: the same bits as the permuted channels-last view
    nchw = clamped.permute(0, 3, 1, 2).contiguous().to(_dev())
    got_c = _M().psnr(nchw, pixels.permute(0, 3, 1, 2).contiguous().to(_dev()))
    assert float(got_c) == _psnr_gpu(clamped, pixels)
    want = EH.psnr64(colors, pixels, data_range=2.0)
    assert abs(_psnr_gpu(clamped, pixels, data_range=2.0) - want) <= 2 * 2.0 ** -24 * abs(want)


def test_psnr_identical_images_is_inf():
    _, pixels = EH.frame_inputs(1, 12, 13, 3)
    assert _psnr_gpu(pixels, pixels) == float("inf")
    M = _M()
    m = M.PeakSignalNoiseRatio(data_range=1.0).to(_dev())
    s = M.StructuralSimilarityIndexMeasure(data_range=1.0).to(_dev())
    p = pixels.to(_dev()).permute(0, 3, 1, 2)
    assert float(m(p, p)) == float("inf") and abs(float(s(p, p)) - 1.0) <= 1e-6


def test_frame_fixture_canvas_and_psnr():
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_frame.npz"), allow_pickle=False))
    colors = torch.from_numpy(z["colors"])
    pixels = torch.from_numpy(z["pixels_u8"]).to(torch.float32) / 255.0
    M = _M()
    res = M.eval_metrics(colors.to(_dev()), pixels.to(_dev()), canvas=True)
    each = M.eval_metrics(colors.to(_dev()), pixels.to(_dev()), canvas=False, per_image=True)
    torch.cuda.synchronize()
    assert res["canvas"].dtype == torch.uint8 and np.array_equal(res["canvas"].cpu().numpy(), z["canvas"])
    assert "canvas" not in each and each["psnr"].shape == (2,) and each["ssim"].shape == (2,)
    assert abs(float(res["psnr"]) - float(z["psnr"])) <= 2 * 2.0 ** -24 * float(z["psnr"])
    assert np.abs(each["psnr"].cpu().numpy().astype(np.float64) - z["psnr_each"]).max() <= 2 * 2.0 ** -24 * z["psnr_each"].max()
    for b in range(2):     # a per-image value is the single call's, bit for bit
        single = M.eval_metrics(colors[b:b + 1].to(_dev()), pixels[b:b + 1].to(_dev()), canvas=False)
        assert _bits(each["psnr"][b], single["psnr"]) and _bits(each["ssim"][b], single["ssim"])


def test_canvas_all_levels_and_out_of_range_colors():
    """16 x 16 holding all 256 levels as k / 255.0f, and colors with 1.0, 0.0, -0.3, 1.7: bytes exactly as (canvas * 255).astype(uint8)"""
    k = torch.arange(256, dtype=torch.float32).reshape(1, 16, 16, 1)
    pixels = (k / 255.0).repeat(1, 1, 1, 3).contiguous()
    colors = pixels.flip(1).clone()
    colors[0, 0, 0:4, 0] = torch.tensor([1.0, 0.0, -0.3, 1.7])
    colors[0, 1, 0:4, 2] = torch.tensor([1.7, -0.3, 0.0, 1.0])
    want = EH.canvas_bytes(colors, pixels)
    res = _M().eval_metrics(colors.to(_dev()), pixels.to(_dev()))
    torch.cuda.synchronize()
    got = res["canvas"].cpu().numpy()
    assert got.shape == (1, 16, 32, 3) and np.array_equal(got, want)
    assert tuple(got[0, 0, 16:20, 0]) == (255, 0, 0, 255)
    # on-device pixels (uint8 / 255.0 as the trainer forms them on its device) truncate from whatever fp32 value the division gave
    dpix = torch.arange(256, dtype=torch.uint8, device=_dev()).reshape(1, 16, 16, 1).repeat(1, 1, 1, 3) / 255.0
    res = _M().eval_metrics(dpix.flip(2), dpix)
    torch.cuda.synchronize()
    assert np.array_equal(res["canvas"].cpu().numpy(), EH.canvas_bytes(dpix.flip(2).cpu(), dpix.cpu()))


def test_ssim_is_fused_ssim_on_the_clamped_images():
    from hunyuanworld_mirror_amd import fused_ssim
    M = _M()
    for shape in ((1, 11, 11), (2, 37, 52)):
        colors, pixels = EH.frame_inputs(*shape, seed=9)
        c = torch.clamp(colors, 0, 1).to(_dev()).permute(0, 3, 1, 2)
        p = pixels.to(_dev()).permute(0, 3, 1, 2)
        want = fused_ssim(c, p, padding="valid", train=False)
        assert _bits(M.ssim(c, p), want)
        assert _bits(M.StructuralSimilarityIndexMeasure(data_range=1.0)(c, p), want)
        assert abs(float(M.ssim(c * 4.0, p * 4.0, data_range=4.0)) - float(want)) <= 1e-5
    with pytest.raises(ValueError, match="11 x 11"):
        M.ssim(torch.rand(1, 3, 10, 11, device=_dev()), torch.rand(1, 3, 10, 11, device=_dev()))


@pytest.mark.parametrize("per_image", [False, True])
def test_eval_metrics_equals_the_separate_calls(per_image):
    M = _M()
    sc = EH.make_inputs("pair")
    dev = _dev()
    pixels = sc["ref"].to(dev)
    # an RGB+ED render: the colours are channels 0:3 of a [B,H,W,4] tensor, unclamped (a few values pushed outside [0, 1])
    raw = sc["img"].clone()
    raw[:, 0, :5, :] = torch.tensor([-0.3, 1.7, 1.2])
    render = torch.cat([raw, torch.full_like(raw[..., :1], 3.0)], dim=-1).to(dev)
    res = M.eval_metrics(render[..., :3], pixels, color_corrected=True, canvas=True, per_image=per_image)
    torch.cuda.synchronize()
    assert set(res) == {"psnr", "ssim", "cc_psnr", "cc_ssim", "canvas"}
    clamped = torch.clamp(raw, 0, 1).to(dev)
    cc = M.color_correct(clamped, pixels, per_image=per_image)
    groups = [slice(b, b + 1) for b in range(2)] if per_image else [slice(0, 2)]
    for key, x in (("psnr", clamped), ("ssim", clamped), ("cc_psnr", cc), ("cc_ssim", cc)):
        fn = M.psnr if key.endswith("psnr") else M.ssim
        want = [fn(x[g].permute(0, 3, 1, 2), pixels[g].permute(0, 3, 1, 2)) for g in groups]
        want = torch.stack(want) if per_image else want[0]
        assert _bits(res[key], want), key
    assert np.array_equal(res["canvas"].cpu().numpy(), EH.canvas_bytes(raw, sc["ref"]))
    plain = M.eval_metrics(render[..., :3], pixels, canvas=False, per_image=per_image)
    assert set(plain) == {"psnr", "ssim"} and _bits(plain["psnr"], res["psnr"]) and _bits(plain["ssim"], res["ssim"])


def test_evaluator_over_three_views(tmp_path):
    from PIL import Image
    M = _M()
    dev = _dev()
    H, W = 23, 31
    views, renders = [], []
    for i in range(3):
        colors, pixels = EH.frame_inputs(1, H, W, 40 + i)
        v = {"camtoworld": torch.eye(4), "K": torch.eye(3), "image": torch.round(pixels[0] * 255).to(torch.uint8)}
        if i == 1:
            mask = torch.ones(H, W, dtype=torch.bool)
            mask[:7, :9] = False
            v["mask"] = mask
        if i == 2:
            v["image"] = v["image"].float()        # float in 0-255 is taken too
        views.append(v)
        renders.append(torch.cat([colors, torch.full_like(colors[..., :1], 2.0)], dim=-1))
    calls = []

    def render_fn(camtoworlds, Ks, width, height, masks):
        assert camtoworlds.shape == (1, 4, 4) and Ks.shape == (1, 3, 3) and (width, height) == (W, H) and camtoworlds.device == dev
        calls.append(masks)
        return renders[len(calls) - 1].to(dev), None, None

    out = str(tmp_path / "run")
    stats = M.Evaluator(dev).evaluate(render_fn, views, use_bilateral_grid=True, num_gs=1234, out_dir=out, stage="val", step=30)
    assert set(stats) == {"psnr", "ssim", "cc_psnr", "cc_ssim", "ellipse_time", "num_GS"}
    assert stats["num_GS"] == 1234 and stats["ellipse_time"] > 0 and calls[0] is None and calls[1] is not None and calls[2] is None
    each = []
    for i, v in enumerate(views):
        colors = renders[i][..., :3].clone()
        if "mask" in v:
            colors[0][~v["mask"]] = 0
        pixels = (v["image"].to(dev)[None] / 255.0)
        each.append(M.eval_metrics(colors.to(dev), pixels, color_corrected=True))
    for k in ("psnr", "ssim", "cc_psnr", "cc_ssim"):
        assert stats[k] == torch.stack([e[k] for e in each]).mean().item(), k
    assert sorted(os.listdir(os.path.join(out, "renders"))) == [f"val_step30_{i:04d}.png" for i in range(3)]
    assert os.listdir(os.path.join(out, "stats")) == ["val_step0030.json"]
    assert json.load(open(os.path.join(out, "stats", "val_step0030.json"))) == stats
    for i in range(3):
        png = np.asarray(Image.open(os.path.join(out, "renders", f"val_step30_{i:04d}.png")))
        assert png.shape == (H, 2 * W, 3) and np.array_equal(png, each[i]["canvas"][0].cpu().numpy())
    png = np.asarray(Image.open(os.path.join(out, "renders", "val_step30_0001.png")))
    assert not png[:7, W:W + 9].any() and png[:7, :9].any()          # the masked-out render is black, the ground truth is not
    plain = M.Evaluator(dev).evaluate(lambda c, k, w, h, m: renders[0].to(dev), views[:1])
    assert set(plain) == {"psnr", "ssim", "ellipse_time", "num_GS"} and plain["num_GS"] == 0
