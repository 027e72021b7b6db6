"""CPU: tests/densify_helper.py (the torch restatement the GPU tests compare with) reproduces the REFERENCE's DefaultStrategy on the
fixtures tests/golden/densify_*.npz (tools/gen_golden_densify.py: gsplat's own code, CPU, fp64), and the new C ABI names are
declared, bound and exported."""
import ctypes as C
import os

import pytest
import torch

import densify_helper as DH
from conftest import ROOT

SCENES, KEYS, load_scene, helper_state = DH.SCENES, DH.KEYS, DH.load_scene, DH.helper_state


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", SCENES)
def test_helper_reproduces_the_reference(name):
    z, cfg = load_scene(name)
    step, scene = int(z["step"]), float(z["scene_scale"])
    g2, cnt, rs = helper_state(z, torch.float64)
    assert relmax(g2, torch.from_numpy(z["state_grad2d"])) < 1e-12
    assert torch.equal(cnt, torch.from_numpy(z["state_count"]))
    if rs is not None:
        assert torch.equal(rs, torch.from_numpy(z["state_radii"]))
    p = {k: torch.from_numpy(z["in_" + k]).double() for k in KEYS}
    mg = DH.margins(g2, cnt, rs, p["scales"], p["opacities"], cfg, step, scene)
    assert min(mg.values()) > 1e-4, mg                      # fp32 rounding cannot flip a decision
    src, kind, rank, counts = DH.plan(g2, cnt, rs, p["scales"], p["opacities"], cfg, step, scene)
    assert list(counts) == [int(x) for x in z["counts"]]
    assert min(counts[:3]) > 0 and all(int((kind == k).sum()) > 0 for k in range(4))
    noise = torch.from_numpy(z["noise"])
    assert noise.shape == (2, counts[1], 3)
    child = kind >= DH.SPLIT0
    for k in KEYS:
        mode = DH.gather_mode(k, cfg["revised_opacity"])
        got = DH.gather(p[k], src, kind, rank, mode, torch.float64, p["quats"], p["scales"], noise)
        want = torch.from_numpy(z["out_" + k])
        assert got.shape == want.shape, k
        computed = child if mode != "copy" else torch.zeros_like(child)
        assert torch.equal(got[~computed], want[~computed]), k          # structure and copied values: exact
        if computed.any():
            assert relmax(got[computed], want[computed]) < 1e-12, k
        for mk in ("m", "v"):
            got_m = DH.gather(torch.from_numpy(z[f"in_{mk}_{k}"]).double(), src, kind, rank, "zero_new", torch.float64)
            assert torch.equal(got_m, torch.from_numpy(z[f"out_{mk}_{k}"])), (k, mk)
            assert float(got_m[kind != DH.KEEP].abs().max()) == 0.0


NEW_EXPORTS = ["wm_rasterize_backward_workspace_bytes_ex", "wm_rasterize_splats_backward_ex", "wm_rasterize_means2d", "wm_densify_accumulate",
               "wm_densify_plan_workspace_bytes", "wm_densify_plan", "wm_densify_gather"]


def test_new_exports_and_strategy_surface():
    from hunyuanworld_mirror_amd import _lib
    import hunyuanworld_mirror_amd as wm
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(lib)
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and hasattr(L, n) and (n + "(") in hdr, n
    L.wm_densify_plan_workspace_bytes.restype = C.c_size_t
    L.wm_densify_plan_workspace_bytes.argtypes = [C.c_size_t]
    assert L.wm_densify_plan_workspace_bytes(1000) >= 2 * 1001 * 20
    L.wm_rasterize_backward_workspace_bytes_ex.restype = C.c_size_t
    L.wm_rasterize_backward_workspace_bytes_ex.argtypes = [C.c_int] * 4 + [C.c_size_t, C.c_int]
    L.wm_rasterize_backward_workspace_bytes.restype = C.c_size_t
    L.wm_rasterize_backward_workspace_bytes.argtypes = [C.c_int] * 4 + [C.c_size_t]
    n = 12800
    assert L.wm_rasterize_backward_workspace_bytes_ex(10, 2, 64, 48, n, 0) == L.wm_rasterize_backward_workspace_bytes(10, 2, 64, 48, n) == 256 + 40 * n
    assert L.wm_rasterize_backward_workspace_bytes_ex(10, 2, 64, 48, n, 1) == 256 + 48 * n
    s = wm.DefaultStrategy()
    for k, v in DH.DEFAULTS.items():
        assert getattr(s, k) == v, k
    assert s.verbose is False and s.key_for_gradient == "means2d"
    st = wm.DefaultStrategy(refine_scale2d_stop_iter=5).initialize_state(2.0)
    assert st == {"grad2d": None, "count": None, "scene_scale": 2.0, "radii": None}
    assert "radii" not in s.initialize_state()
    with pytest.raises(NotImplementedError):
        s.step_post_backward({}, {}, {}, 1, {}, packed=True)
    with pytest.raises(NotImplementedError):
        wm.DefaultStrategy(key_for_gradient="gradient_2dgs").step_pre_backward({}, {}, {}, 1, {})
    p = {k: torch.nn.Parameter(torch.zeros(3, 3)) for k in ("means", "scales", "quats")}
    with pytest.raises(AssertionError):
        s.check_sanity(p, {k: torch.optim.Adam([v]) for k, v in p.items()})     # opacities missing
