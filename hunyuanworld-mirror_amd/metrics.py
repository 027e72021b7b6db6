"""Evaluation of the reference's "Post 3DGS Optimization" trainer (gsplat's simple_trainer_worldmirror.py, Runner.eval :1005-1091) over the
C ABI entries ``wm_eval_frame`` and ``wm_color_correct`` (hand-written HIP, csrc/evalmetrics.hip) and the SSIM kernel of
``losses.fused_ssim``.  What the trainer takes from torchmetrics and examples/lib_bilagrid.py:

    self.psnr = PeakSignalNoiseRatio(data_range=1.0).to(self.device)
    self.ssim = StructuralSimilarityIndexMeasure(data_range=1.0).to(self.device)
    colors = torch.clamp(colors, 0.0, 1.0); canvas = (cat([pixels, colors], dim=2) * 255).astype(np.uint8)
    metrics["psnr"].append(self.psnr(colors_p, pixels_p)); metrics["ssim"].append(self.ssim(colors_p, pixels_p))
    cc_colors = color_correct(colors, pixels)

``eval_metrics`` is those lines for one batch in one launch sequence without a host synchronisation; ``Evaluator`` is the loop around
them.  SSIM is the 11 x 11 Gaussian (sigma 1.5) structural similarity averaged over the map cropped by 5 on every side: the value
``fused_ssim(..., padding="valid", train=False)`` computes.  ``color_correct`` solves its least-squares systems as masked normal equations
with a minimum-norm pseudo-inverse: on full-rank systems it is the reference's result, on rank-deficient ones (a grey image, a saturated
channel) it is the unique projection where the reference's depends on the LAPACK driver or asserts.  No CPU fallback:
tensors must live on a HIP device."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from typing import Callable, Dict, Iterable, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream
from .losses import fused_ssim

_DEFAULT_EPS = 0.5 / 255


def _need_gpu(what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"{what} takes torch tensors, got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: move the tensors to a HIP device")
    if any(t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f"{what}: the tensors are on different devices: {[str(t.device) for t in tensors]}")


def _check_pair(what, a, b, layout):
    """a, b: floating [B,H,W,3] (layout "bhwc") or [B,3,H,W] ("bchw") of one shape"""
    for t in (a, b):
        if not torch.is_tensor(t):
            raise TypeError(f"{what} takes torch tensors, got {type(t).__name__}")
        if not t.dtype.is_floating_point:
            raise TypeError(f"{what} takes floating-point images, got {t.dtype}")
    ch = 3 if layout == "bhwc" else 1
    want = "[B, H, W, 3]" if layout == "bhwc" else "[B, 3, H, W]"
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"{what} takes two {want} tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[ch] != 3:
        raise ValueError(f"{what} is built for 3 channels ({want}), got {tuple(a.shape)}")
    if min(a.shape) < 1:
        raise ValueError(f"{what}: empty image {tuple(a.shape)}")


def _check_range(data_range):
    if not isinstance(data_range, (int, float)) or isinstance(data_range, bool) or not data_range > 0:
        raise ValueError(f"data_range must be a positive number (a (min, max) pair is not built), got {data_range!r}")


def _strides4(t):
    return (C.c_int64 * 4)(*t.stride())


def _eval_frame(colors, pixels, clamp, data_range, want_clamped, want_canvas, per_image):
    """colors, pixels: fp32 [B,H,W,3] views of any strides on one HIP device -> (psnr 0-d or [B], clamped or None, canvas or None)"""
    L = _lib.lib()
    B, H, W, _ = (int(x) for x in colors.shape)
    dev = colors.device
    psnr = torch.empty((B,) if per_image else (), device=dev, dtype=torch.float32)
    clamped = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32) if want_clamped else None
    canvas = torch.empty((B, H, 2 * W, 3), device=dev, dtype=torch.uint8) if want_canvas else None
    need = L.wm_eval_frame_workspace_bytes(B, H, W)
    if need == 0:
        raise ValueError(f"eval frame: a batch of {B} images of {H} x {W} is beyond what the kernel indexes (B <= 65535, 6 H W < 2^31)")
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        st = L.wm_eval_frame(ptr(colors), _strides4(colors), ptr(pixels), _strides4(pixels), B, H, W, 1 if clamp else 0, float(data_range),
                             ptr(clamped), ptr(canvas), None if per_image else ptr(psnr), ptr(psnr) if per_image else None, ptr(ws),
                             ws.numel() * 8, stream(dev))
    check(st, "wm_eval_frame")
    return psnr, clamped, canvas


def _f32(t):
    return t.detach() if t.dtype == torch.float32 else t.detach().to(torch.float32)


def psnr(preds: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """torchmetrics' peak_signal_noise_ratio for the trainer's call: preds, target [B,3,H,W] (any strides) -> 0-d fp32 tensor,
    10 log10(data_range^2 / mse) over the whole batch, the mean squared error taken in fp64 in a fixed order; +inf for identical images.
    Nothing is clamped."""
    _check_pair("psnr", preds, target, "bchw")
    _check_range(data_range)
    _need_gpu("psnr", preds, target)
    return _eval_frame(_f32(preds).permute(0, 2, 3, 1), _f32(target).permute(0, 2, 3, 1), False, data_range, False, False, False)[0]


def ssim(preds: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Structural similarity for the trainer's call: preds, target [B,3,H,W] -> 0-d fp32 tensor.  11 x 11 Gaussian window of sigma 1.5,
    C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2, the mean of the map cropped by 5 on every side: fused_ssim(preds / data_range,
    target / data_range, padding="valid", train=False), the same kernel.  Images below 11 x 11 raise ValueError."""
    _check_pair("ssim", preds, target, "bchw")
    _check_range(data_range)
    if preds.shape[2] < 11 or preds.shape[3] < 11:
        raise ValueError(f"ssim needs at least 11 x 11 pixels (the cropped map would be empty), got {preds.shape[2]} x {preds.shape[3]}")
    _need_gpu("ssim", preds, target)
    a, b = _f32(preds), _f32(target)
    if data_range != 1.0:                     # SSIM is invariant under a common scale once C1, C2 scale with it
        a, b = a * (1.0 / data_range), b * (1.0 / data_range)
    return fused_ssim(a, b, padding="valid", train=False)


class _Metric:
    """The part of a torchmetrics metric object that Runner.eval uses: construct, .to(device), call on one batch."""
    _fn: Callable = None
    _name = ""

    def __init__(self, data_range: float = 1.0, **kwargs):
        if kwargs:
            raise NotImplementedError(f"{self._name}({', '.join(sorted(kwargs))}=...) is not built: only data_range is")
        _check_range(data_range)
        self.data_range = data_range

    def to(self, *args, **kwargs):
        return self

    def __call__(self, preds, target):
        return type(self)._fn(preds, target, self.data_range)

    forward = __call__

    def update(self, *args, **kwargs):
        raise NotImplementedError(f"{self._name}.update is not built: call the object on each batch, it returns that batch's value")

    def compute(self):
        raise NotImplementedError(f"{self._name}.compute is not built: call the object on each batch, it returns that batch's value")

    def reset(self):
        raise NotImplementedError(f"{self._name}.reset is not built: the object keeps no state")


class PeakSignalNoiseRatio(_Metric):
    _fn = staticmethod(psnr)
    _name = "PeakSignalNoiseRatio"


class StructuralSimilarityIndexMeasure(_Metric):
    _fn = staticmethod(ssim)
    _name = "StructuralSimilarityIndexMeasure"


def _check_cc(img, ref, num_iters, eps):
    for t in (img, ref):
        if not torch.is_tensor(t):
            raise TypeError(f"color_correct takes torch tensors, got {type(t).__name__}")
        if not t.dtype.is_floating_point:
            raise TypeError(f"color_correct takes floating-point images, got {t.dtype}")
    if img.dim() < 1 or ref.dim() < 1 or img.shape[-1] != ref.shape[-1]:
        raise ValueError(f"img's and ref's channels must match, got {tuple(img.shape)} and {tuple(ref.shape)}")
    if img.shape[-1] != 3:
        raise NotImplementedError(f"color_correct is built for 3 channels, got {img.shape[-1]}")
    if img.shape != ref.shape:
        raise ValueError(f"img and ref must have one shape, got {tuple(img.shape)} and {tuple(ref.shape)}")
    if img.numel() == 0:
        raise ValueError(f"color_correct: empty image {tuple(img.shape)}")
    if not isinstance(num_iters, int) or isinstance(num_iters, bool) or num_iters < 0:
        raise ValueError(f"num_iters must be an integer >= 0, got {num_iters!r}")
    if not (isinstance(eps, (int, float)) and 0.0 < eps < 0.5):
        raise ValueError(f"eps must lie in (0, 0.5), got {eps!r}")


def _color_correct(img32, ref32, nsys, num_iters, eps):
    """img32, ref32: contiguous fp32 of nsys * P * 3 values on one HIP device -> corrected, same shape"""
    L = _lib.lib()
    P = img32.numel() // (3 * nsys)
    dev = img32.device
    need = L.wm_color_correct_workspace_bytes(nsys, P)
    if need == 0:
        raise ValueError(f"color_correct: {nsys} systems of {P} pixels are beyond what the kernel indexes (65535 systems, 2^31 - 1 pixels)")
    out = torch.empty_like(img32)
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        st = L.wm_color_correct(ptr(img32), ptr(ref32), nsys, P, num_iters, float(eps), ptr(out), ptr(ws), ws.numel() * 8, stream(dev))
    check(st, "wm_color_correct")
    return out


def color_correct(img: torch.Tensor, ref: torch.Tensor, num_iters: int = 5, eps: float = _DEFAULT_EPS, per_image: bool = False) -> torch.Tensor:
    """lib_bilagrid.color_correct for 3 channels: warp img [..., 3] towards ref by num_iters quadratic colour fits over the pixels that
    are unclipped in img, in the current estimate and in ref.  All leading dimensions form one system (the reference's reshape([-1, 3]));
    per_image=True fits each img[b] of a [B, ..., 3] batch on its own, in the same launches.  Result: img's shape and dtype.
    num_iters = 0 returns img.  No host synchronisation."""
    _check_cc(img, ref, num_iters, eps)
    if per_image and img.dim() < 3:
        raise ValueError(f"per_image needs a leading batch dimension ([B, ..., 3]), got {tuple(img.shape)}")
    _need_gpu("color_correct", img, ref)
    if num_iters == 0:
        return img
    nsys = int(img.shape[0]) if per_image else 1
    out = _color_correct(_f32(img).contiguous(), _f32(ref).contiguous(), nsys, num_iters, eps)
    return out.to(img.dtype)


def _ssim_each(a_p, b_p, per_image):
    if not per_image:
        return fused_ssim(a_p, b_p, padding="valid", train=False)
    return torch.stack([fused_ssim(a_p[i:i + 1], b_p[i:i + 1], padding="valid", train=False) for i in range(a_p.shape[0])])


def eval_metrics(colors: torch.Tensor, pixels: torch.Tensor, *, color_corrected: bool = False, canvas: bool = True,
                 per_image: bool = False) -> Dict[str, torch.Tensor]:
    """Runner.eval's per-batch lines (:1040-1060) fused.  colors [B,H,W,3]: the render, unclamped, possibly a strided channel view
    (renders[..., :3] of an RGB+ED render); pixels [B,H,W,3] in [0, 1].  -> {"psnr", "ssim"} (+ {"cc_psnr", "cc_ssim"} with
    color_corrected: the metrics of color_correct(clamped colors, pixels)), 0-d fp32 device tensors over the batch, or [B] with per_image
    (colour correction per image too); with canvas also "canvas": uint8 [B,H,2W,3], pixels left, clamped colors right, bytes as
    (canvas * 255).astype(np.uint8).  No host synchronisation."""
    _check_pair("eval_metrics", colors, pixels, "bhwc")
    if colors.shape[1] < 11 or colors.shape[2] < 11:
        raise ValueError(f"eval_metrics needs at least 11 x 11 pixels (SSIM's cropped map would be empty), got {colors.shape[1]} x {colors.shape[2]}")
    _need_gpu("eval_metrics", colors, pixels)
    c32, p32 = _f32(colors), _f32(pixels)
    ps, clamped, cv = _eval_frame(c32, p32, True, 1.0, True, bool(canvas), per_image)
    p_p = p32.permute(0, 3, 1, 2)
    out = {"psnr": ps, "ssim": _ssim_each(clamped.permute(0, 3, 1, 2), p_p, per_image)}
    if color_corrected:
        B = int(c32.shape[0])
        cc = _color_correct(clamped, p32.contiguous(), B if per_image else 1, 5, _DEFAULT_EPS)
        out["cc_psnr"] = _eval_frame(cc, p32, False, 1.0, False, False, per_image)[0]
        out["cc_ssim"] = _ssim_each(cc.permute(0, 3, 1, 2), p_p, per_image)
    if canvas:
        out["canvas"] = cv
    return out


class Evaluator:
    """Runner.eval without the dataset plumbing: render every view, clamp, write the canvas, collect the metrics, average, write the stats.

        ev = Evaluator(device="cuda:0")
        stats = ev.evaluate(render_fn, views, use_bilateral_grid=True, num_gs=len(splats["means"]), out_dir=result_dir, step=3000)

    render_fn(camtoworlds [1,4,4], Ks [1,3,3], width, height, masks or None) -> the render [1,H,W,>=3] (channels 0:3 are the colours) or a
    tuple whose first item is it, as Runner.rasterize_splats.  A view is a dict with "camtoworld" [4,4], "K" [3,3], "image" [H,W,3]
    (uint8, or float in 0-255) and optionally "mask" [H,W] bool; a leading batch dimension of 1 (a DataLoader's) is accepted."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the evaluation runs in libwm_hip.so on the GPU: give a HIP device")

    @staticmethod
    def _batched(t, dims):
        return t if t.dim() == dims + 1 else t.unsqueeze(0)

    @torch.no_grad()
    def evaluate(self, render_fn: Callable, views: Iterable[dict], *, use_bilateral_grid: bool = False, num_gs: Optional[int] = None,
                 out_dir: Optional[str] = None, stage: str = "val", step: int = 0) -> Dict[str, float]:
        dev = self.device
        if out_dir is not None:
            from PIL import Image
            os.makedirs(os.path.join(out_dir, "renders"), exist_ok=True)
            os.makedirs(os.path.join(out_dir, "stats"), exist_ok=True)
        ellipse_time = 0.0
        metrics: Dict[str, list] = {}
        canvases = []
        n = 0
        for i, data in enumerate(views):
            camtoworlds = self._batched(torch.as_tensor(data["camtoworld"]), 2).to(dev)
            Ks = self._batched(torch.as_tensor(data["K"]), 2).to(dev)
            pixels = self._batched(torch.as_tensor(data["image"]), 3).to(dev) / 255.0
            masks = self._batched(torch.as_tensor(data["mask"]), 2).to(dev) if "mask" in data else None
            height, width = pixels.shape[1:3]
            torch.cuda.synchronize(dev)
            tic = time.time()
            colors = render_fn(camtoworlds, Ks, width, height, masks)
            if isinstance(colors, (tuple, list)):
                colors = colors[0]
            if masks is not None:
                colors[~masks] = 0                     # Runner.rasterize_splats :644
            torch.cuda.synchronize(dev)
            ellipse_time += max(time.time() - tic, 1e-10)
            res = eval_metrics(colors[..., :3], pixels, color_corrected=use_bilateral_grid, canvas=out_dir is not None)
            for k in ("psnr", "ssim", "cc_psnr", "cc_ssim"):
                if k in res:
                    metrics.setdefault(k, []).append(res[k])
            if out_dir is not None:
                canvases.append(res["canvas"])
            n += 1
        if n == 0:
            raise ValueError("evaluate: no views")
        stats = {k: torch.stack(v).mean().item() for k, v in metrics.items()}
        stats.update({"ellipse_time": ellipse_time / n, "num_GS": int(num_gs) if num_gs is not None else 0})
        if out_dir is not None:
            for i, cv in enumerate(canvases):
                Image.fromarray(cv[0].cpu().numpy()).save(os.path.join(out_dir, "renders", f"{stage}_step{step}_{i:04d}.png"))
            with open(os.path.join(out_dir, "stats", f"{stage}_step{step:04d}.json"), "w") as f:
                json.dump(stats, f)
        return stats
