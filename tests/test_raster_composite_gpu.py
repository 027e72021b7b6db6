"""All three instantiations of raster_composite_kernel<PX,PY> (csrc/raster.hip: 1, 2 and 4 pixels per lane, tuning key raster_ppl) and the
compositing backward (csrc/raster_bwd_composite.h) against the fp64 torch restatement tests/raster_modes_helper.py, per pixel, on the
scenes of tests/raster_composite_helper.py: list lengths 0 to 7 with empty tiles between full ones, bit-equal depths, two cameras
with different lists, saturation exits on either half of the unrolled loop / at the last entry / with entries left / never, images
from 1 x 1 up with regions outside the image and lanes with one pixel inside, and a 1024 x 1024 two-camera scene that the launcher
itself sends to the 4-pixel kernel.  tests/test_raster_composite_cpu.py proves those properties and that every threshold margin clears
the fp32 error of what it decides, so nothing here allows for a flipped decision.

Forward bound, per output and per pixel (CH.bounds): |GPU - fp64| <= max(4 e32, 16 eps (Lmax + 1) scale), e32 the fp32 helper's max-abs
error on the same scene, 16 eps the rounding count of an alpha (tests/test_raster_modes_gpu.py), Lmax the longest list, scale 1 for
alpha, the largest colour for rgb, the largest depth for the accumulated depth; expected depth where fp64 alpha > 1e-3, the analytic
terms carried through the division.  Outputs are filled with NaN first (the _opt entry of the C ABI): every pixel is written, and where
the fp64 alpha is exactly zero the GPU's outputs are exact zeros or exactly the background.
Gradient yardstick: that of test_raster_modes_gpu._check_grads, e64 <= 4 e32 and e64 < 1e-3 in rel-L2.

Measured on an MI355X, the same to two digits under raster_ppl 1, 2 and 4 (largest e32 / smallest bound / largest GPU error of a group):
  lists (3 scenes)   rgb 2.0e-6 / 1.5e-5 / 2.1e-6   alpha 2.3e-6 / 1.5e-5 / 2.3e-6   expected depth 1.3e-5 / 4.5e-5 / 1.2e-5   accumulated 3.9e-6 / 3.1e-5 / 4.1e-6
  sat (5 scenes)     rgb 1.6e-6 / 2.5e-5 / 1.5e-6   alpha 3.1e-8 / 2.5e-5 / 3.1e-8   expected depth 1.7e-6 / 9.0e-5 / 1.6e-6   accumulated 1.6e-6 / 7.7e-5 / 1.6e-6
  edge (9 sizes)     rgb 1.0e-7 / 8.6e-6 / 9.4e-8   alpha 3.5e-8 / 9.5e-6 / 3.5e-8   expected depth 2.2e-7 / 3.9e-5 / 1.8e-7
  default, untuned   rgb 9.1e-6 / 3.7e-5 / 9.1e-6   alpha 1.1e-5 / 4.4e-5 / 1.1e-5   expected depth 6.5e-5 / 2.6e-4 / 6.4e-5   accumulated 5.7e-5 / 2.3e-4 / 5.7e-5
  gradients: e64 / e32 at most 1.67 (opacities, seven wide Gaussians), 1.57 (backgrounds, no wide ones), otherwise at most 1.34; e32 from
  7e-8 (backgrounds) to 8e-5
The GPU's error is the fp32 helper's nearly everywhere: both are carried by the projection's roundings, which the two share in kind.
A kernel trace of these calls names raster_composite_kernel<1, 1>, <2, 1> and <2, 2> under raster_ppl 1, 2 and 4, <2, 1> for an untuned
small scene and <2, 2> for the untuned 1024 x 1024 one; on the first list scene the three gave the same bits.
The three kernels are not compared with one another bit for bit: a sub-expression shared between a lane's pixels can change which
multiplies the compiler fuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_composite_helper as CH
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PPL = [1, 2, 4]


class _raster_ppl:
    """wm_set_tuning(b"raster_ppl", v) for the block; the key is process-wide, so it goes back to -1 (unset) whatever happens inside"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from hunyuanworld_mirror_amd import _lib
        if self.v is not None:
            assert _lib.lib().wm_set_tuning(b"raster_ppl", int(self.v)) == 0

    def __exit__(self, *exc):
        from hunyuanworld_mirror_amd import _lib
        _lib.lib().wm_set_tuning(b"raster_ppl", -1)


def _tensors(name):
    return {k: torch.from_numpy(v).to(DEV) for k, v in CH.scene(name)[0].items()}


def _forward(name, mode, ppl):
    """wm_rasterize_splats_opt into NaN-filled outputs -> rgb [C,H,W,3], depth [C,H,W,1], alpha [C,H,W,1] (torch, on the GPU)"""
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    inp, _, W, H = CH.scene(name)
    t = _tensors(name)
    N, V = len(inp["means"]), len(inp["viewmats"])
    bg = torch.from_numpy(CH.backgrounds(V)).to(DEV) if mode == "bg_D" else None
    opts = _lib.wm_raster_options(0, int(CH.MODES[mode]["depth_mode"] == "D"), 0.3, 0.01, 1e10, 0.0, None if bg is None else bg.data_ptr())
    out = [torch.full((V, H, W, ch), float("nan"), device=DEV) for ch in (3, 1, 1)]
    cap = 1 << 16
    ws = torch.empty(L.wm_rasterize_workspace_bytes(N, V, W, H, cap), device=DEV, dtype=torch.uint8)
    n = C.c_ulonglong(0)
    p = _lib.ptr
    with _raster_ppl(ppl):
        st = L.wm_rasterize_splats_opt(p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(t["colors"]), 0, 0, 0, None, N, p(t["viewmats"]),
                                       p(t["Ks"]), V, W, H, C.byref(opts), p(out[0]), p(out[1]), p(out[2]), None, p(ws), ws.numel(), cap, C.byref(n),
                                       _lib.stream(DEV))
        torch.cuda.synchronize()
    assert st == 0 and n.value == int(CH.list_lengths(name).sum()), (st, n.value)      # the GPU's lists have the designed total length
    return out


def _check_forward(name, mode, got, tag):
    """every pixel written, exact values outside every footprint, and the per-pixel bound of the module docstring on all three outputs"""
    rgb, dep, al = (o.double().cpu().numpy() for o in got)
    (r64, d64, a64), _ = CH.reference(name, mode, torch.float64)
    b = CH.bounds(name, mode)
    assert np.isfinite(rgb).all() and np.isfinite(dep).all() and np.isfinite(al).all(), "a pixel was not written"
    empty = a64[..., 0] == 0
    if empty.any():
        V = rgb.shape[0]
        want = np.broadcast_to(CH.backgrounds(V).astype(np.float64)[:, None, None, :], rgb.shape) if mode == "bg_D" else np.zeros_like(rgb)
        assert np.array_equal(rgb[empty], want[empty]) and not al[empty].any() and not dep[empty].any()
    m = b["depth_mask"]
    err = {"rgb": np.abs(rgb - r64), "alpha": np.abs(al - a64), "depth": np.where(m, np.abs(dep - d64), 0.0)}
    worst = {k: float(v.max()) for k, v in err.items()}
    print(f"{name} {mode} {tag}: Lmax {b['lmax']}  e32 " + " ".join(f"{k} {v:.3e}" for k, v in b["e32"].items()) +
          f"  bound rgb {b['tol']['rgb']:.3e} alpha {b['tol']['alpha']:.3e} depth {float(b['depth_tol'][m].min()):.3e}" +
          "  GPU " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, tol in (("rgb", b["tol"]["rgb"]), ("alpha", b["tol"]["alpha"]), ("depth", b["depth_tol"])):
        over = err[k] > tol
        if over.any():
            at = np.unravel_index(np.argmax(err[k] - tol), err[k].shape)
            raise AssertionError(f"{name} {mode} {tag}: {k} at (camera, row, column, channel) {at}: error {err[k][at]:.3e} over the bound "
                                 f"{float(np.broadcast_to(tol, err[k].shape)[at]):.3e}; {int(over.sum())} pixels over")


# ------------------------------------------------------------------------------------------------ forward, the three kernels
@pytest.mark.parametrize("ppl", PPL)
@pytest.mark.parametrize("name", CH.LISTS + CH.SAT)
def test_gpu_lists_and_saturation_per_pixel(name, ppl):
    for mode in CH.MODES:
        _check_forward(name, mode, _forward(name, mode, ppl), f"raster_ppl {ppl}")


@pytest.mark.parametrize("ppl", PPL)
@pytest.mark.parametrize("name", CH.EDGE)
def test_gpu_image_edges_per_pixel(name, ppl):
    _check_forward(name, "plain", _forward(name, "plain", ppl), f"raster_ppl {ppl}")


def test_gpu_tuning_key_does_not_stay_set():
    """after a block under _raster_ppl the launcher chooses again: the 2-pixel kernel's bits on a small scene (same kernel, same bits)"""
    name = CH.LISTS[0]
    chosen = _forward(name, "plain", None)
    forced = _forward(name, "plain", 2)
    after = _forward(name, "plain", None)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(chosen, forced, after))
    for ppl in (1, 4):          # for the record only (no assertion either way): how many floats the other two kernels round differently
        other = _forward(name, "plain", ppl)
        print(f"raster_ppl {ppl} against 2: {sum(int((a != b).sum()) for a, b in zip(chosen, other))} of {sum(a.numel() for a in chosen)} floats differ")


# ------------------------------------------------------------------------------------------------ forward, the launcher's own choice
def test_gpu_default_selection_per_pixel_and_bitwise():
    """8192 tile-camera pairs with no tuning set: the path of the real workload, against the fp64 helper; forced to 4 pixels per lane it is
    the same kernel and gives the same bits, as does a repeat of the untuned run"""
    chosen = _forward(CH.DEFAULT, "plain", None)
    _check_forward(CH.DEFAULT, "plain", chosen, "no tuning")
    forced, again = _forward(CH.DEFAULT, "plain", 4), _forward(CH.DEFAULT, "plain", None)
    for a, b, c in zip(chosen, forced, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    _check_forward(CH.DEFAULT, "bg_D", _forward(CH.DEFAULT, "bg_D", None), "no tuning")


# ------------------------------------------------------------------------------------------------ backward
RENDER_MODE = {"plain": "RGB+ED", "bg_D": "RGB+D"}


def _gradients(name, mode, ppl):
    """rasterization() forward under raster_ppl = ppl (None: the launcher's choice), backward under the seeded cotangents -> dict of
    gradients (numpy fp64)"""
    from hunyuanworld_mirror_amd import rasterization
    inp, _, W, H = CH.scene(name)
    t = _tensors(name)
    for k in CH.NAMES:
        t[k].requires_grad_(True)
    kw = {}
    if mode == "bg_D":
        kw["backgrounds"] = torch.from_numpy(CH.backgrounds(len(inp["viewmats"]))).to(DEV).requires_grad_(True)
    with _raster_ppl(ppl):
        rc, al, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], W, H,
                                  render_mode=RENDER_MODE[mode], **kw)
        torch.cuda.synchronize()
    cot = [torch.from_numpy(c).to(DEV) for c in CH.cotangents(name)]
    ((rc[..., :3] * cot[0]).sum() + (rc[..., 3:] * cot[1]).sum() + (al * cot[2]).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: t[k].grad.double().cpu().numpy() for k in CH.NAMES}
    if mode == "bg_D":
        grads["backgrounds"] = kw["backgrounds"].grad.double().cpu().numpy()
    return grads


def _check_grads(name, mode, gg, tag):
    g64, g32 = CH.reference_gradients(name, mode, torch.float64), CH.reference_gradients(name, mode, torch.float32)
    res = {k: (rel_l2(g32[k], g64[k]), rel_l2(gg[k], g64[k])) for k in g64}
    for k, (e32, e64) in res.items():
        print(f"{name} {mode} {tag} grad {k}: e32 {e32:.3e} e64 {e64:.3e}")
    assert set(gg) == set(g64)
    for k, (e32, e64) in res.items():
        assert np.isfinite(gg[k]).all()
        assert e64 <= 4 * e32 and e64 < 1e-3, (k, e32, e64)


@pytest.mark.parametrize("mode", list(CH.MODES))
@pytest.mark.parametrize("name", CH.LISTS + CH.SAT)
def test_gpu_backward_on_short_lists_and_early_exits(name, mode):
    """default tuning: means, quats, scales, opacities, colours (and backgrounds in mode bg_D) against the helper's autograd"""
    _check_grads(name, mode, _gradients(name, mode, None), "default tuning")


@pytest.mark.parametrize("ppl", PPL)
@pytest.mark.parametrize("name", CH.LISTS + CH.SAT)
def test_gpu_backward_after_each_forward_kernel(name, ppl):
    """the backward reads the forward's depth and alpha: after a forward by each of the three kernels it meets the same yardstick"""
    _check_grads(name, "bg_D", _gradients(name, "bg_D", ppl), f"forward raster_ppl {ppl}")
    _check_grads(name, "plain", _gradients(name, "plain", ppl), f"forward raster_ppl {ppl}")
