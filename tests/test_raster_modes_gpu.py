"""gsplat.rasterization's call on the GPU: hunyuanworld_mirror_amd.rasterization(), Rasterizer's new keywords and the _opt entries of
the C ABI (antialiased mode, eps2d, near / far plane, radius_clip, backgrounds, the five render modes) against the fp64 torch
restatement tests/raster_modes_helper.py (pinned by tests/test_raster_modes_cpu.py) and against the entries without options.

Yardsticks are those of the existing rasteriser tests: the forward thresholds of test_gpu_rasterizer_matches_oracle_and_reference_projection
(tests/test_raster.py), the gradient yardstick of test_gpu_gradient_parity (tests/test_raster_backward_gpu.py): with e32 = rel-L2(helper
fp32, helper fp64) and e64 = rel-L2(GPU, helper fp64), e64 <= 4 e32 and e64 < 1e-3.

Threshold margins: the helper reports in fp64, per kind of threshold, how close any decided quantity comes to it.  A decision can differ
between an fp32 and the fp64 evaluation only where the margin is below the fp32 error of the decided quantity, so MARGIN_FLOORS holds that
error per kind (eps = 2^-23; an alpha carries about 16 roundings from the inputs, counted in test_gpu_antialiased_closed_form):
  alpha_threshold  16 eps / 255 = 7.5e-9;   alpha_cap  16 eps x 1 = 1.9e-6
  stop             the transmittance at the stop is a product of factors 1 - alpha_i with sum -log(1 - alpha_i) = log(1e4) = 9.2; each alpha's
                   16 eps relative error moves the product by about 16 eps x 9.2 relative, plus one rounding per factor (some 20 factors):
                   170 eps x 1e-4 = 2.0e-9
  tile             a tile edge is (mean +- radius) / 16, at most 7 tiles here, 4 roundings: 4 eps x 7 = 3.3e-6
The integer radius itself (the "radius" margin) has no floor: the forward tests allow ceil() flips by their mismatch share, as the existing
ones do.  The existing raster tests make no such check on these scenes (their one margin assertion, > 1e-3, is on the finite-difference
scene), so this is the stricter reading.  Checked on the CPU beforehand: the 600-Gaussian scene meets every floor as it is in all three
configurations used (antialiased: alpha_threshold 1.75e-8, stop 1.75e-7); the 1500-Gaussian scene does not in antialiased mode
(alpha_threshold 5.81e-10), so its opacities are nudged: opacities x (1 + 0.01 u), u uniform in [-1, 1) from OPACITY_SEED; seeds 1 to
SEED_1500 - 1 each miss a floor, SEED_1500 is the first that meets all."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import raster_modes_helper as RM
from conftest import GOLD, rel_l2

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]
NAMES = RM.NAMES
EPS32 = 2.0 ** -23
MARGIN_FLOORS = {"alpha_threshold": 16 * EPS32 / 255, "alpha_cap": 16 * EPS32, "stop": 170 * EPS32 * 1e-4, "tile": 4 * EPS32 * 7}
SEED_1500 = 86
OPACITY_SEED = {"raster_600g_2c_80x56": 0, "raster_1500g_3c_100x70": SEED_1500}      # 0: the scene's opacities as they are
CUT = dict(eps2d=0.1, near_plane=2.0, far_plane=4.5)
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    inp["colors"] = z["in_sh"][:, 0]
    if OPACITY_SEED[name]:
        g = torch.Generator().manual_seed(OPACITY_SEED[name])
        op = torch.from_numpy(inp["opacities"])
        inp["opacities"] = (op * (1 + 0.01 * (2 * torch.rand(len(op), generator=g) - 1))).clamp(0, 1).numpy()
    return inp, int(z["width"]), int(z["height"]), np.load(os.path.join(GOLD, name.replace("raster_", "raster_modes_") + ".npz"))


def _bg(C_):
    return np.array([[0.1, 0.5, 0.9], [1.0, 0.0, 0.25], [0.3, 0.7, 0.2]], np.float32)[:C_]


def _cot(name, seed=3):
    inp, W, H, _ = _load(name)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(inp["viewmats"].shape[0], H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]


# the helper's configurations: (options of RM.rasterize, with backgrounds?)
CONFIGS = {"aa": (dict(antialiased=True), False), "bg": (dict(), True), "cut_d_bg": (dict(depth_mode="D", **CUT), True)}


@functools.lru_cache(maxsize=None)
def _ref(name, config, dtype):
    """the helper's outputs and gradients, computed once per (scene, configuration, dtype) and shared; fp64 runs also give the margins"""
    inp, W, H, _ = _load(name)
    opts, with_bg = CONFIGS[config]
    opts = dict(opts, backgrounds=_bg(inp["viewmats"].shape[0])) if with_bg else dict(opts)
    margins = {} if dtype == torch.float64 else None
    outs, grads = RM.gradients(inp, _cot(name), True, W, H, dtype, margins=margins, **opts)
    return outs, grads, margins


def _gpu(name, cot=None, info=False, **kw):
    """rasterization() on the scene (colours as degree-0 SH, as the helper's is_sh) -> outputs (rgb, depth or None, alpha), gradients"""
    from hunyuanworld_mirror_amd import rasterization
    inp, W, H, _ = _load(name)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    if kw.get("backgrounds") is not None:
        kw["backgrounds"] = torch.from_numpy(kw["backgrounds"]).to(DEV).requires_grad_(True)
    rc, al, inf = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :], t["viewmats"], t["Ks"], W, H,
                                sh_degree=0, **kw)
    outs = [rc[..., :3], rc[..., 3:], al] if rc.shape[-1] == 4 else [rc, None, al] if rc.shape[-1] == 3 else [None, rc, al]
    grads = None
    if cot is not None:
        loss = sum((o * torch.from_numpy(c).to(DEV)).sum() for o, c in zip(outs, cot) if o is not None)
        loss.backward()
        grads = {k: t[k].grad.double().cpu().numpy() for k in NAMES}
        if kw.get("backgrounds") is not None:
            grads["backgrounds"] = kw["backgrounds"].grad.double().cpu().numpy()
    torch.cuda.synchronize()
    res = [None if o is None else o.detach().cpu().numpy() for o in outs], grads
    return (*res, inf) if info else res


def _check_forward(name, got, want, tag):
    """assertions and thresholds of test_gpu_rasterizer_matches_oracle_and_reference_projection"""
    (rgb, dep, al), (r0, d0, a0) = got, want
    m = a0 > 1e-3
    print(name, tag, "rgb", rel_l2(rgb, r0), np.abs(rgb - r0).max(), "alpha", rel_l2(al, a0), "depth", rel_l2(dep[m], d0[m]))
    assert np.isfinite(rgb).all() and np.isfinite(dep).all() and np.isfinite(al).all()
    assert rel_l2(rgb, r0) < 2e-4 and np.abs(rgb - r0).max() < 2e-2
    assert rel_l2(al, a0) < 2e-4
    assert rel_l2(dep[m], d0[m]) < 2e-4


def _check_grads(name, config, gg, keys=NAMES):
    _, g64, margins = _ref(name, config, torch.float64)
    _, g32, _ = _ref(name, config, torch.float32)
    print(name, config, "margins", margins)
    assert all(margins[k] >= floor for k, floor in MARGIN_FLOORS.items()), (margins, MARGIN_FLOORS)
    res = {k: (rel_l2(g32[k], g64[k]), rel_l2(gg[k], g64[k])) for k in keys}
    for k, (e32, e64) in res.items():
        print(f"{name} {config} grad {k}: e32 {e32:.3e} e64 {e64:.3e}")
    for k, (e32, e64) in res.items():
        assert np.isfinite(gg[k]).all()
        assert e64 <= 4 * e32 and e64 < 1e-3, (k, e32, e64)


# ------------------------------------------------------------------------------------------------ 1. defaults change nothing
def _exact_cameras(C_):
    """camera-to-world matrices whose inverse, and the inverse of that, are exact in fp32 (identity rotation, dyadic translations), so that
    rasterization(viewmats = inv(c2w)) and Rasterizer(camtoworlds = c2w) hand the kernels the same bits, camera positions included"""
    c2w = torch.eye(4).repeat(C_, 1, 1)
    c2w[1:, :3, 3] = torch.tensor([[0.125, -0.0625, 0.25], [-0.25, 0.125, 0.0625]])[:C_ - 1]
    return c2w.to(DEV)


def _default_case(kind, name=CASES[0]):
    inp, W, H, _ = _load(name)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    g = torch.Generator().manual_seed(7)
    if kind == "colors":
        col, deg = torch.rand(len(inp["means"]), 3, generator=g).to(DEV), None
    elif kind == "sh0":
        col, deg = t["colors"][:, None, :].contiguous(), 0
    else:
        col, deg = ((torch.rand(len(inp["means"]), 9, 3, generator=g) - 0.5) * 0.6).to(DEV), 2
    return t, col, deg, W, H


@pytest.mark.parametrize("kind", ["colors", "sh0", "sh2"])
def test_gpu_defaults_change_nothing(kind):
    """rasterization(..., render_mode="RGB+ED") with gsplat's defaults against Rasterizer().rasterize_splats: the same bits in rgb / depth /
    alpha, the five gradients, means2d.grad / .absgrad, and the camera gradient (at the camera-to-world matrices both calls start from) for
    colours [N,3] and sh_degree 0.  With sh_degree 2 the camera positions reach the two calls' graphs by different torch operations
    (a slice of camtoworlds; the inverse of viewmats), which round differently in torch, not in the kernels.  The issue asks for torch.equal
    on the camera gradient there too; through Python that cannot hold for any implementation that follows the issue's own
    campos = inv(viewmats)[:, :3, 3], so this one assertion is weaker than the issue's text: rel-L2 < 1e-5 here (fp32 rounding of two 4 x 4
    products), and the bitwise comparison of v_viewmats and v_campos is made where the kernels' outputs can be seen directly, at the C ABI
    (test_gpu_opt_entries_with_default_options_equal_the_entries_without)."""
    from hunyuanworld_mirror_amd import Rasterizer, rasterization
    t, col, deg, W, H = _default_case(kind)
    cot = [torch.from_numpy(c).to(DEV) for c in _cot(CASES[0], 5)]
    runs = []
    for new in (False, True):
        leaves = [t[k].clone().requires_grad_(True) for k in NAMES[:4]] + [col.clone().requires_grad_(True)]
        c2w = _exact_cameras(t["viewmats"].shape[0]).requires_grad_(True)
        if new:
            rc, al, info = rasterization(*leaves, torch.linalg.inv(c2w), t["Ks"], W, H, sh_degree=deg, render_mode="RGB+ED", absgrad=True)
            outs = (rc[..., :3], rc[..., 3:], al)
        else:
            *outs, info = Rasterizer(camera_grad=True).rasterize_splats(*leaves, c2w, t["Ks"], W, H, sh_degree=deg, return_info=True, absgrad=True)
        info["means2d"].retain_grad()
        sum((o * c).sum() for o, c in zip(outs, cot)).backward()
        torch.cuda.synchronize()
        runs.append(([o.detach() for o in outs], [x.grad for x in leaves], info["means2d"].grad, info["means2d"].absgrad, c2w.grad, info))
    old, new = runs
    assert all(torch.equal(a, b) for a, b in zip(old[0], new[0]))
    assert all(a is not None and torch.equal(a, b) for a, b in zip(old[1], new[1]))
    assert torch.equal(old[2], new[2]) and torch.equal(old[3], new[3]) and float(old[3].abs().sum()) > 0
    assert torch.equal(old[5]["radii"], new[5]["radii"]) and torch.equal(old[5]["means2d"], new[5]["means2d"])
    assert {k: v for k, v in old[5].items() if k not in ("means2d", "radii")} == {k: v for k, v in new[5].items() if k not in ("means2d", "radii")}
    assert float(old[4].abs().sum()) > 0
    if kind == "sh2":
        assert rel_l2(new[4].double().cpu().numpy(), old[4].double().cpu().numpy()) < 1e-5
    else:
        assert torch.equal(old[4], new[4])


def test_gpu_opt_entries_with_default_options_equal_the_entries_without():
    """wm_rasterize_splats_opt / _backward_opt with null options and with a struct of the defaults, against wm_rasterize_splats_sh /
    _backward_sh (SH degree 2, every optional output) and wm_rasterize_splats / _backward (colours [N,3]): every output the same bits,
    v_viewmats and v_campos included; wm_rasterize_means2d works on the workspace the _opt forward left."""
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    t, sh, _, W, H = _default_case("sh2")
    N, V = int(t["means"].shape[0]), int(t["viewmats"].shape[0])
    c2w = _exact_cameras(V)
    vm, campos = torch.linalg.inv(c2w).contiguous(), c2w[:, :3, 3].contiguous()
    col = torch.rand(N, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    cot = [torch.from_numpy(c).to(DEV).contiguous() for c in _cot(CASES[0], 5)]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap = 1 << 18
    defaults = _lib.wm_raster_options(0, 0, 0.3, 0.01, 1e10, 0.0, None)

    def run(entry, degree):
        colors, K = (sh, 9) if degree else (col, 0)
        o = [torch.full((V, H, W, 3), float("nan"), device=DEV), torch.full((V, H, W), float("nan"), device=DEV), torch.full((V, H, W), float("nan"), device=DEV)]
        radii = torch.zeros((V, N, 2), device=DEV, dtype=torch.int32)
        ws = torch.empty(L.wm_rasterize_workspace_bytes(N, V, W, H, cap), device=DEV, dtype=torch.uint8)
        n = C.c_ulonglong(0)
        head = (p(t["means"]), p(t["quats"]), p(t["scales"]), p(t["opacities"]), p(colors))
        ftail = (p(o[0]), p(o[1]), p(o[2]), p(radii), p(ws), ws.numel(), cap, C.byref(n), stream)
        opt = None if entry == "null" else C.byref(defaults)
        if entry in ("null", "struct"):
            st = L.wm_rasterize_splats_opt(*head, 0, K, degree, p(campos) if degree else None, N, p(vm), p(t["Ks"]), V, W, H, opt, *ftail)
        elif degree:
            st = L.wm_rasterize_splats_sh(*head, K, degree, p(campos), N, p(vm), p(t["Ks"]), V, W, H, *ftail)
        else:
            st = L.wm_rasterize_splats(*head, 0, N, p(vm), p(t["Ks"]), V, W, H, *ftail)
        assert st == 0, (entry, st)
        m2 = torch.empty((V, N, 2), device=DEV)
        assert L.wm_rasterize_means2d(p(ws), ws.numel(), N, V, W, H, cap, p(radii), p(m2), stream) == 0
        g = [torch.empty_like(t["means"]), torch.empty_like(t["quats"]), torch.empty_like(t["scales"]), torch.empty_like(t["opacities"]),
             torch.empty_like(colors)]
        want_cam = bool(degree)           # the plain entry has no camera outputs
        v2d, v2a = (torch.empty((V, N, 2), device=DEV), torch.empty((V, N, 2), device=DEV)) if want_cam else (None, None)
        v_vm, v_cp = (torch.empty((V, 4, 4), device=DEV), torch.empty((V, 3), device=DEV)) if want_cam else (None, None)
        nn = int(n.value)
        mid = (N, p(vm), p(t["Ks"]), V, W, H)
        btail = (p(ws), ws.numel(), cap, nn, None, p(o[1]), None, p(cot[0]), p(cot[1]), p(cot[2]), *[p(x) for x in g])
        if entry in ("null", "struct"):
            gws = torch.empty(L.wm_rasterize_backward_workspace_bytes_opt(N, V, W, H, nn, int(want_cam), int(want_cam), degree, int(want_cam), 0),
                              device=DEV, dtype=torch.uint8)
            st = L.wm_rasterize_splats_backward_opt(*head, 0, K, degree, p(campos) if degree else None, *mid, opt, *btail, p(v2d), p(v2a),
                                                    int(want_cam), p(v_vm), p(v_cp), None, p(gws), gws.numel(), stream)
        elif degree:
            gws = torch.empty(L.wm_rasterize_backward_workspace_bytes_sh(N, V, W, H, nn, 1, 1, 1), device=DEV, dtype=torch.uint8)
            st = L.wm_rasterize_splats_backward_sh(*head, K, degree, p(campos), *mid, *btail, p(v2d), p(v2a), 1, p(v_vm), p(v_cp), p(gws),
                                                   gws.numel(), stream)
        else:
            gws = torch.empty(L.wm_rasterize_backward_workspace_bytes(N, V, W, H, nn), device=DEV, dtype=torch.uint8)
            st = L.wm_rasterize_splats_backward(*head, 0, *mid, *btail, p(gws), gws.numel(), stream)
        torch.cuda.synchronize()
        assert st == 0, (entry, st)
        return [*o, radii, m2, *g] + ([v2d, v2a, v_vm, v_cp] if want_cam else []), nn

    for degree in (2, 0):
        base, n0 = run("old", degree)
        assert n0 > 0 and all(torch.isfinite(x.float()).all() for x in base)
        for entry in ("null", "struct"):
            got, n1 = run(entry, degree)
            assert n1 == n0 and len(got) == len(base)
            for i, (a, b) in enumerate(zip(base, got)):
                assert torch.equal(a, b), (degree, entry, i)


# ------------------------------------------------------------------------------------------------ 2. / 3. antialiased
@pytest.mark.parametrize("name", CASES)
def test_gpu_antialiased_forward(name):
    _, _, _, gz = _load(name)
    (rgb, ed, al), _, info = _gpu(name, None, info=True, rasterize_mode="antialiased", render_mode="RGB+ED")
    radii = info["radii"].cpu().numpy()
    assert (radii != gz["default_radii"]).any(-1).mean() < 2e-3          # a ceil() may flip on a last-bit difference
    _check_forward(name, (rgb, ed, al), _ref(name, "aa", torch.float64)[0], "antialiased")
    # and it is not the classic image
    (rgb_c, _, _), _ = _gpu(name, None, render_mode="RGB+ED")
    assert rel_l2(rgb, rgb_c) > 1e-3


@pytest.mark.parametrize("name", CASES)
def test_gpu_antialiased_gradients(name):
    """seeded cotangents on all three outputs; opacity seed: none for the 600-Gaussian scene, SEED_1500 for the other (module docstring)"""
    _, gg = _gpu(name, _cot(name), rasterize_mode="antialiased", render_mode="RGB+ED")
    _check_grads(name, "aa", gg)


def test_gpu_antialiased_rasterizer_class_is_the_same_render():
    from hunyuanworld_mirror_amd import Rasterizer
    name = CASES[0]
    inp, W, H, _ = _load(name)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    rgb, ed, al = Rasterizer(rasterization_mode="antialiased").rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :],
                                                                                torch.linalg.inv(t["viewmats"]), t["Ks"], W, H, sh_degree=0)
    _check_forward(name, (rgb.cpu().numpy(), ed.cpu().numpy(), al.cpu().numpy()), _ref(name, "aa", torch.float64)[0], "Rasterizer(antialiased)")


# ------------------------------------------------------------------------------------------------ 4. closed form
@pytest.mark.parametrize("eps2d", [0.3, 0.1])
def test_gpu_antialiased_closed_form(eps2d):
    """One isotropic Gaussian of scale s on the optical axis of one 32 x 32 camera at depth z, focal f: sigma2 = (f s / z)^2, comp = sigma2 /
    (sigma2 + eps2d); the centre pixel's alpha = min(0.999, o comp exp(-d^2 / (2 (sigma2 + eps2d)))) with d the half-pixel offset; d sum(alpha)
    / d opacity = sum over unskipped, uncapped pixels of comp exp(-...).
    Bound: K eps_fp32 per term, K = 32 = twice the roundings counted along the expression in fp32 (2-D covariance 4, both determinants 6, ratio
    and square root 2 (halved by the root), opacity product 1, conic 1, exponent 5 roundings scaled by the exponent's size, the fast exp 3,
    final product 1: about 16).  The centre alpha is one term: 32 eps_fp32 |alpha|; the gradient: 32 eps_fp32 x number of summed terms x |sum|."""
    from hunyuanworld_mirror_amd import rasterization
    W = H = 32
    f, z0, s3, o = 40.0, 2.0, 0.05, 0.8
    means = torch.tensor([[0.0, 0.0, z0]], device=DEV); quats = torch.tensor([[1.0, 0, 0, 0]], device=DEV)
    scales = torch.full((1, 3), s3, device=DEV); opac = torch.tensor([o], device=DEV, requires_grad=True)
    col = torch.tensor([[0.7, 0.2, 0.5]], device=DEV)
    K = torch.tensor([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]], device=DEV)
    rgb, al, _ = rasterization(means, quats, scales, opac, col, torch.eye(4, device=DEV)[None], K, W, H, eps2d=eps2d, rasterize_mode="antialiased")
    al.sum().backward()
    torch.cuda.synchronize()
    s2 = (f * s3 / z0) ** 2
    comp = s2 / (s2 + eps2d)
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    e = np.exp(-((px - W / 2) ** 2 + (py - H / 2) ** 2) / (2 * (s2 + eps2d)))
    want_alpha = min(0.999, o * comp * np.exp(-0.5 / (2 * (s2 + eps2d))))
    got_alpha = float(al.detach()[0, H // 2, W // 2, 0])
    use = (o * comp * e >= 1 / 255.0) & (o * comp * e <= 0.999)
    n_terms = int(use.sum())
    want, got = float((comp * e[use]).sum()), float(opac.grad[0])
    print(f"eps2d {eps2d}: centre alpha {got_alpha} expected {want_alpha} ({abs(got_alpha - want_alpha) / want_alpha / EPS32:.1f} eps); "
          f"d sum(alpha) / d opacity {got} expected {want} over {n_terms} terms ({abs(got - want) / want / EPS32:.1f} eps)")
    assert 20 < n_terms < 100
    assert abs(got_alpha - want_alpha) <= 32 * EPS32 * want_alpha
    assert abs(got - want) <= 32 * EPS32 * n_terms * want


# ------------------------------------------------------------------------------------------------ 5. backgrounds
def test_gpu_backgrounds_forward_and_their_gradient():
    name = CASES[0]
    inp, W, H, _ = _load(name)
    bg = _bg(inp["viewmats"].shape[0])
    cot = _cot(name)
    (rgb, ed, al), _ = _gpu(name, None, render_mode="RGB+ED")
    (rgb_b, ed_b, al_b), gb = _gpu(name, cot, render_mode="RGB+ED", backgrounds=bg)
    assert np.array_equal(ed, ed_b) and np.array_equal(al, al_b)            # the depth channel gets no background
    tr, ta, tb = torch.from_numpy(rgb), torch.from_numpy(al), torch.from_numpy(bg)
    prod = tb[:, None, None, :] * (1 - ta)
    want = (tr + prod).numpy()
    # the kernel adds bg (1 - alpha) by one fused multiply-add, torch by a rounded product and a rounded sum: the sums before the last
    # rounding differ by at most half an ulp of the (smaller) product, so the two results are the same or neighbouring floats: one ulp
    tol = np.spacing(np.maximum(np.abs(want), np.abs(rgb_b)).astype(np.float32))
    assert (np.abs(rgb_b - want) <= tol).all(), float((np.abs(rgb_b - want) / tol).max())
    assert np.abs(rgb_b - rgb).max() > 0.05
    # backgrounds.grad = sum over pixels of v_rgb (1 - alpha), from the GPU's own alpha in fp64.  The kernel forms 1 - alpha and the product
    # in fp32 (half an ulp each: eps_fp32 per term), adds in fp64 and rounds the sum once (half an ulp): 2 eps_fp32 x the sum of the terms'
    # magnitudes bounds all three
    terms = cot[0].astype(np.float64) * (1.0 - al.astype(np.float64))
    want_g, mag = terms.sum((1, 2)), np.abs(terms).sum((1, 2))
    print("backgrounds.grad", gb["backgrounds"].tolist(), "expected", want_g.tolist())
    assert (np.abs(gb["backgrounds"] - want_g) <= 2 * EPS32 * mag).all()
    assert np.abs(want_g).min() > 1e-3


def test_gpu_background_gradients_in_the_kernel_and_by_torch_ops():
    """the five splat gradients with backgrounds in the kernel, and by the route "outputs of the Rasterizer without options + torch ops +
    autograd" on the GPU: two fp32 routes to the helper's fp64 value, each under the 4 e32 yardstick"""
    from hunyuanworld_mirror_amd import Rasterizer
    name = CASES[0]
    inp, W, H, _ = _load(name)
    bg, cot = _bg(inp["viewmats"].shape[0]), _cot(name)
    _, g_kernel = _gpu(name, cot, render_mode="RGB+ED", backgrounds=bg)
    _check_grads(name, "bg", g_kernel, keys=NAMES + ("backgrounds",))
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    tb = torch.from_numpy(bg).to(DEV).requires_grad_(True)
    rgb, ed, al = Rasterizer().rasterize_splats(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :], torch.linalg.inv(t["viewmats"]),
                                                t["Ks"], W, H, sh_degree=0)
    outs = (rgb + tb[:, None, None, :] * (1 - al), ed, al)
    sum((o * torch.from_numpy(c).to(DEV)).sum() for o, c in zip(outs, cot)).backward()
    g_torch = {k: t[k].grad.double().cpu().numpy() for k in NAMES}
    g_torch["backgrounds"] = tb.grad.double().cpu().numpy()
    _check_grads(name, "bg", g_torch, keys=NAMES + ("backgrounds",))
    for k in NAMES:
        print(f"kernel route against torch route, {k}: {rel_l2(g_kernel[k], g_torch[k]):.3e}")


def test_gpu_backgrounds_on_an_empty_scene():
    """no visible Gaussian (all beyond the far plane): the image is the background exactly, alpha and depth exact zeros, backgrounds.grad the sum
    of v_rgb (cotangents in quarters, so that every order of summation gives the same fp64 sum) and every splat gradient exactly zero"""
    from hunyuanworld_mirror_amd import rasterization
    name = CASES[0]
    inp, W, H, _ = _load(name)
    V = inp["viewmats"].shape[0]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    tb = torch.from_numpy(_bg(V)).to(DEV).requires_grad_(True)
    rc, al, info = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :], t["viewmats"], t["Ks"], W, H, sh_degree=0,
                                 near_plane=0.001, far_plane=0.002, backgrounds=tb, render_mode="RGB+ED")
    assert int(info["radii"].abs().sum()) == 0
    assert torch.equal(rc[..., :3], tb.detach()[:, None, None, :].expand(V, H, W, 3))
    assert float(rc[..., 3].abs().max()) == 0.0 and float(al.abs().max()) == 0.0
    g = torch.Generator().manual_seed(4)
    v = [(torch.randint(-8, 9, (V, H, W, ch), generator=g).float() / 4).to(DEV) for ch in (4, 1)]
    ((rc * v[0]).sum() + (al * v[1]).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(tb.grad, v[0][..., :3].double().sum((1, 2)).float())
    for k in NAMES:
        assert t[k].grad is not None and float(t[k].grad.abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------ 6. render modes
def test_gpu_render_modes():
    from hunyuanworld_mirror_amd import rasterization
    name = CASES[0]
    inp, W, H, _ = _load(name)
    V = inp["viewmats"].shape[0]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"][:, None, :], t["viewmats"], t["Ks"], W, H)
    out = {m: rasterization(*args, sh_degree=0, render_mode=m, rasterize_mode="antialiased") for m in ("RGB", "D", "ED", "RGB+D", "RGB+ED")}
    assert {m: tuple(o[0].shape) for m, o in out.items()} == {"RGB": (V, H, W, 3), "D": (V, H, W, 1), "ED": (V, H, W, 1), "RGB+D": (V, H, W, 4),
                                                              "RGB+ED": (V, H, W, 4)}
    assert all(tuple(o[1].shape) == (V, H, W, 1) and torch.equal(o[1], out["RGB"][1]) for o in out.values())
    assert torch.equal(out["RGB"][0], out["RGB+D"][0][..., :3]) and torch.equal(out["RGB"][0], out["RGB+ED"][0][..., :3])
    assert torch.equal(out["D"][0], out["RGB+D"][0][..., 3:]) and torch.equal(out["ED"][0], out["RGB+ED"][0][..., 3:])
    al, d, ed = out["RGB"][1], out["D"][0], out["ED"][0]
    assert float((d - ed).abs().max()) > 1e-3
    m = al > 1e-3
    assert rel_l2((d[m] / al[m]).cpu().numpy(), ed[m].cpu().numpy()) < 1e-6      # one division's rounding apart
    # with backgrounds the depth channels are the same bits, the colours are not
    bg = torch.from_numpy(_bg(V)).to(DEV)
    for mode in ("RGB+D", "RGB+ED"):
        rc, al_b, _ = rasterization(*args, sh_degree=0, render_mode=mode, rasterize_mode="antialiased", backgrounds=bg)
        assert torch.equal(rc[..., 3:], out[mode][0][..., 3:]) and torch.equal(al_b, al) and not torch.equal(rc[..., :3], out[mode][0][..., :3])


# ------------------------------------------------------------------------------------------------ 6. / 7. accumulated depth, planes, eps2d
def test_gpu_cut_planes_eps2d_accumulated_depth_and_backgrounds_against_the_helper():
    """(eps2d, near, far) = (0.1, 2.0, 4.5) — planes that cut through the scene, the fixtures' second setting — with render_mode "RGB+D" and
    backgrounds: forward and gradients (the accumulated depth's included, through the seeded depth cotangent) against the helper"""
    name = CASES[0]
    inp, W, H, gz = _load(name)
    bg = _bg(inp["viewmats"].shape[0])
    got, gg, info = _gpu(name, _cot(name), info=True, render_mode="RGB+D", backgrounds=bg, **CUT)
    assert (info["radii"].cpu().numpy() != gz["cut_radii"]).any(-1).mean() < 2e-3
    want = _ref(name, "cut_d_bg", torch.float64)[0]
    _check_forward(name, got, want, "cut planes, RGB+D, backgrounds")
    _check_grads(name, "cut_d_bg", gg, keys=NAMES + ("backgrounds",))


@pytest.mark.parametrize("name", CASES)
def test_gpu_cut_planes_radii(name):
    inp, W, H, gz = _load(name)
    _, _, info = _gpu(name, None, info=True, **CUT)
    radii = info["radii"].cpu().numpy()
    assert (radii != gz["cut_radii"]).any(-1).mean() < 2e-3
    n_vis, n_def = int((radii > 0).all(-1).sum()), int(gz["default_visible"])
    assert n_def / 3 < n_vis < n_def and abs(n_vis - int(gz["cut_visible"])) <= 0.002 * n_def + 4


def test_gpu_radius_clip():
    """radius_clip between the scene's smallest and median radius: the visible set is the helper's (the scene's radii keep 4.3e-4 away from
    an integer: no ceil() flips between fp32 and fp64)"""
    name = CASES[0]
    inp, W, H, gz = _load(name)
    r0 = torch.from_numpy(gz["default_radii"])
    big = r0.max(-1).values[(r0 > 0).all(-1)]
    clip = float((big.min() + big.median()) // 2)
    assert big.min() <= clip < big.median()
    t = {k: torch.from_numpy(inp[k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    want = RM.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H, radius_clip=clip)[0].numpy()
    _, _, info = _gpu(name, None, info=True, radius_clip=clip)
    radii = info["radii"].cpu().numpy()
    assert np.array_equal((radii > 0).all(-1), (want > 0).all(-1)) and (radii != want).any(-1).mean() < 2e-3
    assert 0 < int(((gz["default_radii"] > 0).all(-1) & ~(radii > 0).all(-1)).sum())
    _, _, info0 = _gpu(name, None, info=True, radius_clip=0.0)
    assert (info0["radii"].cpu().numpy() != gz["default_radii"]).any(-1).mean() < 2e-3


# ------------------------------------------------------------------------------------------------ 8. surface
@pytest.mark.parametrize("sh_degree", [0, 3])
def test_gpu_trainer_call_and_strategy(sh_degree):
    """the reference trainer's call (simple_trainer_worldmirror.py:619-642 with :741-752's keywords, default config) as it stands"""
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import rasterization
    inp, width, height, _ = _load(CASES[0])
    g = torch.Generator().manual_seed(9)
    N = len(inp["means"])
    f = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k])).float()
    params = torch.nn.ParameterDict({"means": f("means"), "scales": torch.log(f("scales")), "quats": f("quats"), "opacities": torch.logit(f("opacities").clamp(1e-4, 1 - 1e-4)),
                                     "sh0": f("colors")[:, None, :], "shN": (torch.rand(N, 15, 3, generator=g) - 0.5) * 0.2}).to(DEV)
    optimizers = {k: torch.optim.Adam([params[k]], lr=1e-3) for k in params}
    camtoworlds, Ks = torch.linalg.inv(f("viewmats")).to(DEV), f("Ks").to(DEV)
    strategy = wm.DefaultStrategy(verbose=False)
    strategy.check_sanity(params, optimizers)
    state = strategy.initialize_state(scene_scale=1.0)
    means, quats, scales, opacities = params["means"], params["quats"], torch.exp(params["scales"]), torch.sigmoid(params["opacities"])
    colors = torch.cat([params["sh0"], params["shN"]], 1)
    kwargs = dict(sh_degree=sh_degree, near_plane=0.01, far_plane=1e10, render_mode="RGB")
    render_colors, render_alphas, info = rasterization(
        means=means,
        quats=quats,
        scales=scales,
        opacities=opacities,
        colors=colors,
        viewmats=torch.linalg.inv(camtoworlds),  # [C, 4, 4]
        Ks=Ks,  # [C, 3, 3]
        width=width,
        height=height,
        packed=False,
        absgrad=False,
        sparse_grad=False,
        rasterize_mode="classic",
        distributed=False,
        camera_model="pinhole",
        with_ut=False,
        with_eval3d=False,
        **kwargs,
    )
    V = camtoworlds.shape[0]
    assert render_colors.shape == (V, height, width, 3) and render_alphas.shape == (V, height, width, 1)
    assert set(info) >= {"means2d", "radii", "width", "height", "n_cameras", "gaussian_ids"} and info["gaussian_ids"] is None
    loss = (render_colors - 0.5).abs().mean()
    strategy.step_pre_backward(params, optimizers, state, 0, info)
    loss.backward()
    assert info["means2d"].grad is not None and info["means2d"].grad.shape == (V, N, 2) and float(info["means2d"].grad.abs().sum()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in params.items() if k != "shN" or sh_degree)
    assert float(params["shN"].grad.abs().sum()) > 0 if sh_degree else params["shN"].grad is None or float(params["shN"].grad.abs().sum()) == 0
    strategy.step_post_backward(params, optimizers, state, 0, info)
    assert state["count"] is not None and float(state["count"].sum()) > 0


def test_gpu_invalid_options_surface_as_runtime_error():
    from hunyuanworld_mirror_amd import Rasterizer, rasterization
    inp, W, H, _ = _load(CASES[0])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], W, H)
    for kw in (dict(eps2d=-0.1), dict(near_plane=2.0, far_plane=1.0), dict(radius_clip=-1.0)):
        with pytest.raises(RuntimeError):
            rasterization(*args, **kw)
        with pytest.raises(RuntimeError):
            Rasterizer().rasterize_splats(*args[:5], torch.linalg.inv(t["viewmats"]), t["Ks"], W, H, **kw)
    with pytest.raises(TypeError):
        Rasterizer().rasterize_splats(*args[:5], torch.linalg.inv(t["viewmats"]), t["Ks"], W, H, render_mode="RGB")
    with pytest.raises(NotImplementedError):
        rasterization(*args, packed=True)
    # the keywords reach rasterize_batches too
    bg = torch.from_numpy(_bg(t["viewmats"].shape[0])).to(DEV)
    c2w = torch.linalg.inv(t["viewmats"])
    a = Rasterizer().rasterize_batches([t["means"]], [t["quats"]], [t["scales"]], [t["opacities"]], [t["colors"]], c2w[None], t["Ks"][None], W, H,
                                       backgrounds=bg, eps2d=0.1)
    b = Rasterizer().rasterize_splats(*args[:5], c2w, t["Ks"], W, H, backgrounds=bg, eps2d=0.1)
    assert all(torch.equal(x[0], y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 9. reproducibility
def test_gpu_backward_twice_on_one_forward_is_bitwise_the_same():
    from hunyuanworld_mirror_amd import rasterization
    name = CASES[0]
    inp, W, H, _ = _load(name)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(DEV) for k, v in inp.items()}
    leaves = [t[k].requires_grad_(True) for k in NAMES[:4]] + [t["colors"][:, None, :].clone().requires_grad_(True)]
    vm = t["viewmats"].clone().requires_grad_(True)
    bg = torch.from_numpy(_bg(vm.shape[0])).to(DEV).requires_grad_(True)
    rc, al, info = rasterization(*leaves, vm, t["Ks"], W, H, sh_degree=0, rasterize_mode="antialiased", backgrounds=bg, render_mode="RGB+ED",
                                 absgrad=True, **CUT)
    cot = [torch.from_numpy(c).to(DEV) for c in _cot(name)]
    loss = (rc[..., :3] * cot[0]).sum() + (rc[..., 3:] * cot[1]).sum() + (al * cot[2]).sum()
    wrt = leaves + [vm, bg, info["means2d"]]
    first = torch.autograd.grad(loss, wrt, retain_graph=True)
    abs1 = info["means2d"].absgrad.clone()
    second = torch.autograd.grad(loss, wrt, retain_graph=True)
    torch.cuda.synchronize()
    assert all(a is not None and torch.isfinite(a).all() and float(a.abs().sum()) > 0 for a in first)
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(abs1, info["means2d"].absgrad)
