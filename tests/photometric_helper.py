"""TEST INFRASTRUCTURE ONLY (not a test file): a differentiable torch restatement of the L1 + SSIM photometric loss
(include/wm_hip.h, wm_photometric_loss), in any float dtype, that the loss tests differentiate with autograd.

The definition is the published one fused_ssim implements: an 11-tap Gaussian window (sigma 1.5, normalised), five depthwise
filters with zero padding 5, C1 = 0.01^2, C2 = 0.03^2.  Two spellings of the filter, which tests/test_photometric_cpu.py holds
together: FORM "conv2d" = one F.conv2d(..., groups=C) with the 2-D window, FORM "separable" = two 1-D passes."""
from __future__ import annotations

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS, PAD, SIGMA = 11, 5, 1.5
FORMS = ("conv2d", "separable")


def window(dtype, device="cpu"):
    x = torch.arange(TAPS, dtype=torch.float64) - TAPS // 2
    g = torch.exp(-(x * x) / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(device=device, dtype=dtype)


def gauss(x, form="conv2d"):
    """depthwise zero-padded 11 x 11 Gaussian filter of [B,C,H,W]"""
    C = x.shape[1]
    g = window(x.dtype, x.device)
    if form == "conv2d":
        w2 = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)
        return F.conv2d(x, w2, padding=PAD, groups=C)
    assert form == "separable", form
    h = F.conv2d(x, g.reshape(1, 1, 1, TAPS).repeat(C, 1, 1, 1), padding=(0, PAD), groups=C)
    return F.conv2d(h, g.reshape(1, 1, TAPS, 1).repeat(C, 1, 1, 1), padding=(PAD, 0), groups=C)


def ssim_map(a, b, form="conv2d"):
    """the "same" map, [B,C,H,W]"""
    mu1, mu2 = gauss(a, form), gauss(b, form)
    s1 = gauss(a * a, form) - mu1 * mu1
    s2 = gauss(b * b, form) - mu2 * mu2
    s12 = gauss(a * b, form) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def loss(a, b, padding="valid", lam=0.2, form="conv2d"):
    """-> (loss, l1, ssim), 0-d: loss = (1 - lam) l1 + lam (1 - ssim)"""
    m = ssim_map(a, b, form)
    if padding == "valid":
        m = m[:, :, PAD:-PAD, PAD:-PAD]
    else:
        assert padding == "same", padding
    ssim = m.mean()
    l1 = (a - b).abs().mean()
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


def gradients(a, b, padding, lam, dtype, form="conv2d"):
    """a, b: the test's tensors as they are (fp32 inputs go to the fp64 run unchanged, so both see the same signs of a - b).
    -> dict: ssim, l1, loss (Python floats), grad_loss, grad_ssim (d / d a, tensors of dtype)"""
    x = a.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = b.detach().cpu().to(dtype)
    tot, l1, ssim = loss(x, y, padding, lam, form)
    (g_loss,) = torch.autograd.grad(tot, x, retain_graph=True)
    (g_ssim,) = torch.autograd.grad(ssim, x)
    return {"ssim": float(ssim.detach()), "l1": float(l1.detach()), "loss": float(tot.detach()), "grad_loss": g_loss, "grad_ssim": g_ssim}
