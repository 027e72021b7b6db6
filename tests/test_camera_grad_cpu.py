"""Camera-pose gradients, CPU side: the yardstick of the GPU tests (tests/raster_grad_helper.py differentiated with respect to
viewmats) is pinned to the reference's own gsplat torch projection, pose.CameraOptModule to the reference trainer's module (recorded
results: tests/golden/camera_grad_*.npz, pose_adjust.npz, tools/gen_camera_grad_golden.py), and the new entry points and kernel
instantiations are checked at build level (exports, registers).  Measured values: profiles/r09_camera_gradients.md."""
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

CASES = ["raster_600g_2c_80x56", "raster_1500g_3c_100x70"]
CSRC = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")


@pytest.mark.parametrize("name", CASES)
def test_helper_viewmats_gradient_matches_gsplat_torch(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    gz = np.load(os.path.join(GOLD, name.replace("raster_", "raster_grad_") + ".npz"))
    want = np.load(os.path.join(GOLD, name.replace("raster_", "camera_grad_") + ".npz"))["grad_viewmats"]
    t = {k: torch.from_numpy(z["in_" + k]).double() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    t["viewmats"].requires_grad_(True)
    radii, m2, depths, conics, _ = RG.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], int(z["width"]), int(z["height"]))
    assert np.array_equal(radii.numpy(), z["ref_radii"])
    loss = (m2 * torch.from_numpy(gz["cot_means2d"])).sum() + (depths * torch.from_numpy(gz["cot_depths"])).sum() + \
           (conics * torch.from_numpy(gz["cot_conics"])).sum()
    (gv,) = torch.autograd.grad(loss, [t["viewmats"]])
    e = rel_l2(gv.numpy(), want)
    print(name, "viewmats gradient, helper against gsplat torch:", e)
    assert want.shape == gv.shape and float(np.abs(want[:, :3]).min()) > 0 and np.all(want[:, 3] == 0)
    assert e < 1e-12, e


def _pose_fixture():
    z = np.load(os.path.join(GOLD, "pose_adjust.npz"))
    from hunyuanworld_mirror_amd import CameraOptModule
    m = CameraOptModule(z["weight"].shape[0]).double()
    with torch.no_grad():
        m.embeds.weight.copy_(torch.from_numpy(z["weight"]))
    return z, m


def test_camera_opt_module_matches_the_reference_trainers():
    z, m = _pose_fixture()
    ids = torch.from_numpy(z["embed_ids"])
    assert len(set(ids.tolist())) < len(ids)                  # an image used twice: its row gets both gradients
    out = m(torch.from_numpy(z["camtoworlds"]), ids)
    (gw,) = torch.autograd.grad((out * torch.from_numpy(z["cotangent"])).sum(), [m.embeds.weight])
    e_out, e_grad = rel_l2(out.detach().numpy(), z["out"]), rel_l2(gw.numpy(), z["grad_weight"])
    print("CameraOptModule against the reference: output", e_out, "embeds.weight gradient", e_grad)
    assert out.dtype == torch.float64 and e_out < 1e-12 and e_grad < 1e-12
    # batch dimensions in front: [2,3,4,4] poses with [2,3] ids
    out2 = m(torch.from_numpy(z["camtoworlds"]).reshape(2, 3, 4, 4), ids.reshape(2, 3))
    assert torch.equal(out2.reshape(-1, 4, 4), out)
    with pytest.raises(ValueError):
        m(torch.from_numpy(z["camtoworlds"]), ids[:-1])


def test_camera_opt_module_zero_init_and_state_dict():
    z, m = _pose_fixture()
    c2w = torch.from_numpy(z["camtoworlds"])
    m.zero_init()
    assert torch.equal(m(c2w, torch.from_numpy(z["embed_ids"])), c2w)
    sd = m.state_dict()
    assert sorted(sd) == ["embeds.weight", "identity"]
    assert tuple(sd["embeds.weight"].shape) == (5, 9) and tuple(sd["identity"].shape) == (6,)
    torch.manual_seed(0)
    m.random_init(0.1)
    assert 0.02 < float(m.embeds.weight.detach().std()) < 0.3
    from hunyuanworld_mirror_amd import CameraOptModule
    fresh = CameraOptModule(5)
    fresh.load_state_dict({k: v.float() for k, v in sd.items()})      # a checkpoint's pose_adjust entry loads as it is
    assert fresh.embeds.weight.dtype == torch.float32


def test_camera_entry_points_exported_and_declared():
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    for n in ("wm_rasterize_splats_backward_cam", "wm_rasterize_backward_workspace_bytes_cam"):
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in _lib.EXPORTS and getattr(L, n).argtypes, n
    # the declared parameter list and the ctypes one have the same length; v_viewmats sits behind want_absgrad
    decl = re.search(r"wm_status wm_rasterize_splats_backward_cam\((.*?)\);", hdr, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == len(L.wm_rasterize_splats_backward_cam.argtypes) == 34
    assert params[29] == "int want_absgrad" and params[30] == "float* v_viewmats"
    size_ex, size_cam = L.wm_rasterize_backward_workspace_bytes_ex, L.wm_rasterize_backward_workspace_bytes_cam
    for N, V, n, ab in ((65, 2, 0, 0), (65, 2, 300, 1), (1500, 3, 4000, 0), (4 * 518 * 518, 4, 3_000_000, 1)):
        waves = (N + 63) // 64
        assert size_cam(N, V, 100, 70, n, ab) >= size_ex(N, V, 100, 70, n, ab) + 96 * V * waves      # 12 fp64 partials per wave per camera
    assert size_ex(100, 2, 64, 48, 1000, 0) == L.wm_rasterize_backward_workspace_bytes(100, 2, 64, 48, 1000)      # the old sizes stay


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_project_backward_instantiations_stay_in_registers(tmp_path):
    """raster_project_bwd_kernel<REC, M2D, CAM>: the three instantiations from before the camera gradient and the three with it keep
    everything in registers (no scratch, no spills) at four waves per SIMD, and so does the reducer.  VGPRs without / with CAM:
    <10,0> 107 / 118, <10,1> 109 / 120, <12,1> 109 / 120."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = [f.replace("$(ARCH)", "gfx950") for f in line.split("=", 1)[1].split() if not f.startswith("$(")]
    r = subprocess.run(["hipcc", *flags, "-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, "raster_bwd.hip"), "-o", str(tmp_path / "r.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        m = re.search(r"raster_project_bwd_kernelILi(\d+)ELb(\d)ELb(\d)E", name)
        key = tuple(int(x) for x in m.groups()) if m else "reduce" if "raster_cam_reduce_kernel" in name else None
        if key is None:
            continue
        seen[key] = get(r"VGPRs")
        print(key, "VGPRs", get(r"VGPRs"), "SGPRs", get(r"TotalSGPRs"), "occupancy", get(r"Occupancy \[waves/SIMD\]"))
        assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0, b[:400]
        assert get(r"VGPRs") <= 128 and get(r"Occupancy \[waves/SIMD\]") >= 4, b[:400]
    assert set(seen) == {(10, 0, 0), (10, 1, 0), (12, 1, 0), (10, 0, 1), (10, 1, 1), (12, 1, 1), "reduce"}, seen
