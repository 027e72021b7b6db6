"""Rasteriser backward, CPU side: the fp64 torch restatement the GPU gradients are compared with (tests/raster_grad_helper.py)
is itself pinned — forward to the oracle, projection gradients to the reference's own gsplat torch implementation
(tests/golden/raster_grad_*.npz, tools/gen_raster_grad_golden.py), all gradients to central finite differences — and the
library's backward entry points and kernels are checked at build level (exports, registers, scalar loads, no CAS loop)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import raster_grad_helper as RG
from conftest import GOLD, ROOT, rel_l2
from oracle import raster_ref as R

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]
CSRC = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")


def _load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    inp = {k: z["in_" + k] for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    inp["colors"] = z["in_sh"][:, 0]
    return z, inp, int(z["width"]), int(z["height"])


@pytest.mark.parametrize("name", CASES)
def test_helper_forward_matches_oracle(name):
    z, s, W, H = _load(name)
    t = {k: torch.from_numpy(v).double() for k, v in s.items()}
    with torch.no_grad():
        rgb, ed, al = RG.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], True, t["viewmats"], t["Ks"], W, H)
    r0, e0, a0, _ = R.rasterize(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"], s["viewmats"], s["Ks"], W, H)
    rgb, ed, al = rgb.numpy(), ed.numpy(), al.numpy()
    print(name, "rgb", rel_l2(rgb, r0), np.abs(rgb - r0).max(), "alpha", rel_l2(al, a0))
    assert rel_l2(rgb, r0) < 2e-4 and np.abs(rgb - r0).max() < 2e-2
    assert rel_l2(al, a0) < 2e-4
    m = a0 > 1e-3
    assert rel_l2(ed[m], e0[m]) < 2e-4


@pytest.mark.parametrize("name", CASES)
def test_helper_projection_gradients_match_gsplat_torch(name):
    z, s, W, H = _load(name)
    gz = np.load(os.path.join(GOLD, name.replace("raster_", "raster_grad_") + ".npz"))
    t = {k: torch.from_numpy(s[k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    for k in ("means", "quats", "scales"):
        t[k].requires_grad_(True)
    radii, m2, depths, conics, _ = RG.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H)
    assert np.array_equal(radii.numpy(), z["ref_radii"])
    loss = (m2 * torch.from_numpy(gz["cot_means2d"])).sum() + (depths * torch.from_numpy(gz["cot_depths"])).sum() + \
           (conics * torch.from_numpy(gz["cot_conics"])).sum()
    g = torch.autograd.grad(loss, [t["means"], t["quats"], t["scales"]])
    for k, gi in zip(("means", "quats", "scales"), g):
        e = rel_l2(gi.numpy(), gz["grad_" + k])
        print(name, k, e)
        assert e < 1e-9, (k, e)


def fd_scene(seed=0, N=40, C=2, W=32, H=24):
    """Wide, faint Gaussians in front of two cameras: every pixel sees every Gaussian well above the 1/255 skip and below the
    0.999 cap, and the transmittance never comes near the 1e-4 stop, so the render is smooth in every parameter."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    f = 30.0
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([1.6, 1.2]), 2.0 + u(N, 1)], 1)
    quats = torch.randn(N, 4, generator=g, dtype=torch.float64)
    scales = 1.3 + 0.9 * u(N, 3)
    opac = 0.03 + 0.05 * u(N)
    colors = u(N, 3)
    vm = torch.eye(4, dtype=torch.float64).repeat(C, 1, 1)
    vm[1, :3, :3] = torch.tensor([[np.cos(0.1), 0, np.sin(0.1)], [0, 1, 0], [-np.sin(0.1), 0, np.cos(0.1)]])
    vm[1, :3, 3] = torch.tensor([0.1, -0.05, 0.2])
    K = torch.tensor([[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], dtype=torch.float64).repeat(C, 1, 1)
    return dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors, viewmats=vm, Ks=K), W, H


def test_helper_gradients_match_finite_differences():
    s, W, H = fd_scene()
    names = ("means", "quats", "scales", "opacities", "colors")
    margins = {}
    g = torch.Generator().manual_seed(1)
    cot = [torch.randn(2, H, W, ch, generator=g, dtype=torch.float64) for ch in (3, 1, 1)]

    def loss_of(t, m=None):
        outs = RG.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], False, t["viewmats"], t["Ks"], W, H, margins=m)
        return sum((o * c).sum() for o, c in zip(outs, cot))

    t = {k: v.clone().requires_grad_(k in names) for k, v in s.items()}
    loss = loss_of(t, margins)
    print("threshold margins", margins)
    assert set(margins) >= {"alpha_threshold", "alpha_cap", "stop", "radius"}
    assert all(v > 1e-3 for v in margins.values()), margins     # no pixel within 1e-3 of a threshold
    grads = torch.autograd.grad(loss, [t[k] for k in names])
    h = 1e-6
    with torch.no_grad():
        for k, ga in zip(names, grads):
            fd = torch.zeros_like(ga).reshape(-1)
            base = s[k].reshape(-1)
            for i in range(base.numel()):
                lp = []
                for sgn in (1.0, -1.0):
                    x = base.clone()
                    x[i] += sgn * h
                    lp.append(loss_of({**s, k: x.reshape(s[k].shape)}))
                fd[i] = (lp[0] - lp[1]) / (2 * h)
            e = rel_l2(ga.reshape(-1).numpy(), fd.numpy())
            print("finite differences", k, e)
            assert e < 1e-6, (k, e)


def test_backward_entry_points_exported_and_declared():
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(lib)
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    from hunyuanworld_mirror_amd import _lib
    for n in ("wm_rasterize_splats_backward", "wm_rasterize_backward_workspace_bytes"):
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert "UNTOUCHED between that forward and this call" in hdr      # the workspace contract is part of the interface
    L.wm_rasterize_backward_workspace_bytes.restype = C.c_size_t
    L.wm_rasterize_backward_workspace_bytes.argtypes = [C.c_int] * 4 + [C.c_size_t]
    a, b = L.wm_rasterize_backward_workspace_bytes(100, 2, 64, 48, 0), L.wm_rasterize_backward_workspace_bytes(100, 2, 64, 48, 1000)
    assert b - a >= 1000 * 40 and a > 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_raster_backward_kernels_resources_and_scalar_loads(tmp_path):
    """Both backward kernels keep everything in registers; the compositing backward, like the forward, gets the Gaussian of a
    step through scalar loads (no per-lane record loads in its loops), sums across lanes by DPP, touches no LDS, and the file
    holds no compare-and-swap loop (and no atomics at all: every pair record has one writer)."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = [f.replace("$(ARCH)", "gfx950") for f in line.split("=", 1)[1].split() if not f.startswith("$(")]
    asm = tmp_path / "raster_bwd.s"
    r = subprocess.run(["hipcc", *flags, "-x", "hip", "--cuda-device-only", "-S", os.path.join(CSRC, "raster_bwd.hip"), "-o", str(asm),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        for kern in ("raster_composite_bwd_kernel", "raster_project_bwd_kernel"):
            if kern in name:
                seen.add(kern)
                get = lambda key: int(re.search(key + r": (\d+)", b).group(1))
                assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0, b[:400]
    assert seen == {"raster_composite_bwd_kernel", "raster_project_bwd_kernel"}
    text = open(asm).read()
    assert "cmpswap" not in text and "atomic" not in text
    kernels = re.findall(r"^(_ZN\S*raster_composite_bwd_kernel\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(kernels) == 1
    body = kernels[0][1].split("\n")
    lines = [l.strip() for l in body if l.strip() and not l.strip().startswith(";")]
    assert not [l for l in lines if l.startswith("ds_") or l.startswith("s_barrier") or l.startswith("scratch_")]
    assert sum(l.startswith("v_add_f32_dpp") for l in lines) >= 40 and sum(l.startswith("s_load_dwordx") for l in lines) >= 4
    marks = [i for i, l in enumerate(body) if "Loop Header" in l]
    assert len(marks) >= 2      # the front-to-back and the back-to-front walk
    # inside the loops (from the first loop header to the last store of a pair record) no vector load: records come by s_load
    last_store = max(i for i, l in enumerate(body) if l.strip().startswith("global_store_dword"))
    loop = [l.strip() for l in body[min(marks):last_store]]
    first_bwd = next(i for i, l in enumerate(loop) if l.startswith("v_add_f32_dpp"))
    bwd_loop = loop[first_bwd - 200 if first_bwd > 200 else 0:]
    assert any(l.startswith("s_load_dwordx") for l in loop)
    assert not [l for l in bwd_loop if l.startswith(("global_load", "buffer_load", "flat_load"))], "a per-lane load in the back-to-front walk"
