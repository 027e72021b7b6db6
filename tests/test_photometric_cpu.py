"""CPU: pins tests/photometric_helper.py (the fp64 restatement the GPU loss tests compare against) and the host side of the
photometric-loss C ABI (include/wm_hip.h: wm_photometric_loss and its two companions).  No GPU needed."""
import ctypes as C
import os

import pytest
import torch

import photometric_helper as PH
from conftest import ROOT

LIB = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(LIB)


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    b = torch.rand(*shape, generator=g, dtype=torch.float64)
    a = (b + 0.1 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return a, b


def test_the_two_forms_agree_in_fp64():
    for shape in ((1, 1, 11, 13), (1, 3, 7, 9), (2, 3, 29, 41)):
        a, b = _pair(shape)
        m0, m1 = PH.ssim_map(a, b, "conv2d"), PH.ssim_map(a, b, "separable")
        assert float((m0 - m1).abs().max()) < 1e-12
        for padding in ("same", "valid") if min(shape[2:]) >= 11 else ("same",):
            r0 = PH.gradients(a, b, padding, 0.2, torch.float64, "conv2d")
            r1 = PH.gradients(a, b, padding, 0.2, torch.float64, "separable")
            for k in ("ssim", "l1", "loss"):
                assert abs(r0[k] - r1[k]) < 1e-12, (shape, padding, k)
            for k in ("grad_loss", "grad_ssim"):
                assert float((r0[k] - r1[k]).abs().max()) < 1e-12, (shape, padding, k)


def test_identical_images_give_one_and_no_ssim_gradient():
    a, _ = _pair((1, 2, 17, 19), 1)
    for form in PH.FORMS:
        for padding in ("same", "valid"):
            r = PH.gradients(a, a.clone(), padding, 0.2, torch.float64, form)
            assert abs(r["ssim"] - 1.0) < 1e-12 and r["l1"] == 0.0
            # ssim(a, b) <= 1 with equality at a == b: a maximum, so the gradient vanishes there
            assert float(r["grad_ssim"].abs().max()) < 1e-12


def test_constant_images_closed_form_in_valid_mode():
    alpha, beta = 0.3, 0.7
    a = torch.full((1, 2, 15, 14), alpha, dtype=torch.float64)
    b = torch.full((1, 2, 15, 14), beta, dtype=torch.float64)
    want = (2 * alpha * beta + PH.C1) / (alpha * alpha + beta * beta + PH.C1)     # the variance factor is C2 / C2
    for form in PH.FORMS:
        _, l1, ssim = PH.loss(a, b, "valid", 0.2, form)
        assert abs(float(ssim) - want) < 1e-12 and abs(float(l1) - (beta - alpha)) < 1e-15


def test_autograd_matches_central_differences():
    a, b = _pair((1, 2, 13, 12), 2)
    h = 1e-5
    for form in PH.FORMS:
        for padding in ("same", "valid"):
            r = PH.gradients(a, b, padding, 0.2, torch.float64, form)
            fd_loss, fd_ssim = torch.zeros_like(a), torch.zeros_like(a)
            flat = a.reshape(-1)
            for i in range(flat.numel()):
                p, m = flat.clone(), flat.clone()
                p[i] += h
                m[i] -= h
                lp, _, sp = PH.loss(p.reshape(a.shape), b, padding, 0.2, form)
                lm, _, sm = PH.loss(m.reshape(a.shape), b, padding, 0.2, form)
                fd_loss.reshape(-1)[i] = (lp - lm) / (2 * h)
                fd_ssim.reshape(-1)[i] = (sp - sm) / (2 * h)
            for got, fd in ((r["grad_loss"], fd_loss), (r["grad_ssim"], fd_ssim)):
                rel = float((got - fd).norm() / fd.norm())
                assert rel < 1e-6, (form, padding, rel)


def test_valid_is_same_cropped_by_five():
    a, b = _pair((2, 3, 23, 31), 3)
    for form in PH.FORMS:
        m = PH.ssim_map(a, b, form)[:, :, 5:-5, 5:-5]
        assert m.shape[2:] == (13, 21)
        assert abs(float(m.mean()) - float(PH.loss(a, b, "valid", 0.2, form)[2])) < 1e-15
        assert abs(float(PH.ssim_map(a, b, form).mean()) - float(PH.loss(a, b, "same", 0.2, form)[2])) < 1e-15


def test_library_exports_the_three_symbols(L):
    for n in ("wm_photometric_loss_workspace_bytes", "wm_photometric_loss", "wm_photometric_loss_backward"):
        assert hasattr(L, n), n
    from hunyuanworld_mirror_amd import _lib
    assert {"wm_photometric_loss_workspace_bytes", "wm_photometric_loss", "wm_photometric_loss_backward"} <= set(_lib.EXPORTS)


def test_workspace_grows_with_every_size(L):
    f = L.wm_photometric_loss_workspace_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * 4
    base = f(2, 3, 40, 50)
    assert base >= 3 * 4 * 2 * 3 * 40 * 50          # the three fp32 derivative maps
    assert f(3, 3, 40, 50) > base and f(2, 4, 40, 50) > base and f(2, 3, 41, 50) > base and f(2, 3, 40, 51) > base
    assert f(0, 3, 40, 50) == 0 and f(2, 3, -1, 50) == 0
    small = L.wm_photometric_loss_forward_workspace_bytes
    small.restype, small.argtypes = C.c_size_t, [C.c_int] * 4
    assert 0 < small(2, 3, 40, 50) < base - 3 * 4 * 2 * 3 * 40 * 50 + 256     # the per-tile partials alone, no derivative maps
    assert small(3, 3, 40, 50) > small(2, 3, 40, 50) and small(2, 3, 400, 50) > small(2, 3, 40, 50) and small(0, 3, 40, 50) == 0


def test_argument_checks_come_before_any_launch(L):
    """Null images stand in for device pointers: every one of these is refused on its sizes alone."""
    f = L.wm_photometric_loss
    f.restype = C.c_int
    i64p, vp, i32 = C.POINTER(C.c_int64), C.c_void_p, C.c_int
    f.argtypes = [vp, i64p, vp, i64p, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.c_size_t, vp]
    st = (C.c_int64 * 4)(3 * 16 * 16, 16 * 16, 16, 1)
    fake = C.c_void_p(256)       # never dereferenced: the call returns before anything is launched
    WM_ERR_INVALID = 1
    big = 1 << 30
    assert f(fake, st, fake, st, 0, 3, 16, 16, 0, 0, fake, fake, fake, big, None) == WM_ERR_INVALID
    assert f(fake, st, fake, st, 1, 3, 16, -2, 0, 0, fake, fake, fake, big, None) == WM_ERR_INVALID
    assert f(fake, st, fake, st, 1, 3, 10, 40, 1, 0, fake, fake, fake, big, None) == WM_ERR_INVALID      # valid below 11 pixels
    assert f(fake, st, fake, st, 1, 3, 40, 10, 1, 0, fake, fake, fake, big, None) == WM_ERR_INVALID
    assert f(fake, st, fake, st, 1, 3, 16, 16, 0, 1, fake, fake, fake, 64, None) == WM_ERR_INVALID       # workspace too small for the maps
    small = L.wm_photometric_loss_forward_workspace_bytes
    small.restype, small.argtypes = C.c_size_t, [C.c_int] * 4
    assert f(fake, st, fake, st, 1, 3, 16, 16, 0, 0, fake, fake, fake, small(1, 3, 16, 16) - 1, None) == WM_ERR_INVALID   # and for the partials alone


def test_fused_ssim_has_no_cpu_fallback():
    import hunyuanworld_mirror_amd as wm
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError):
        wm.fused_ssim(a, b)
    with pytest.raises(RuntimeError):
        wm.photometric_loss(a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1))
    with pytest.raises(ValueError):
        wm.fused_ssim(a, b, padding="reflect")
    with pytest.raises(ValueError):
        wm.fused_ssim(a, b[:, :2])
    with pytest.raises(ValueError):
        wm.fused_ssim(a[:, :, :10], b[:, :, :10], padding="valid")
