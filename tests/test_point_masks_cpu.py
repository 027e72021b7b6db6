"""CPU: the point-cloud filter mask API is exported and declared, refuses CPU tensors, and its fixture is self-consistent."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

NEW = ("wm_depth_edge", "wm_normals_edge", "wm_point_filter_mask_workspace_bytes", "wm_point_filter_mask")


def test_new_symbols_are_exported_and_declared():
    import hunyuanworld_mirror_amd as pkg
    from hunyuanworld_mirror_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    declared = set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared and n in _lib.EXPORTS, n
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(lib)
    for n in NEW:
        getattr(L, n)
    for f in ("depth_edge", "normals_edge", "filter_points_mask"):
        assert callable(getattr(pkg, f)), f
    assert _lib.lib().wm_point_filter_mask_workspace_bytes(32, 518, 518) > 0


def test_mirrors_raise_on_cpu_tensors():
    from hunyuanworld_mirror_amd import depth_edge, filter_points_mask, normals_edge
    d, n = torch.rand(2, 9, 11), torch.rand(2, 9, 11, 3)
    with pytest.raises(RuntimeError):
        depth_edge(d, rtol=0.03)
    with pytest.raises(RuntimeError):
        normals_edge(n, 5.0)
    with pytest.raises(RuntimeError):
        filter_points_mask(d, d, n)
    with pytest.raises(ValueError):
        depth_edge(d, rtol=0.03, kernel_size=4)
    with pytest.raises(ValueError):
        normals_edge(n, 5.0, kernel_size=9)


def test_fixture_is_self_consistent():
    from test_point_masks import load_fixture
    z = load_fixture()    # also checks the decoded inputs against the generator's digest
    pct = float(z["params"][0])
    assert os.path.getsize(os.path.join(GOLD, "point_masks.npz")) <= 512 << 10
    for g in "abc":
        conf = z[f"{g}_conf"]
        S, H, W = conf.shape
        thr = np.array([np.quantile(conf[i], pct / 100.0) for i in range(S)], np.float32)
        assert np.array_equal(thr, z[f"thr_{g}"], equal_nan=True)
        cm = conf >= thr[:, None, None]
        de, ne = z[f"case_{g}_depth_k3_nomask_rtol"], z[f"case_{g}_normals_k3_nomask"]
        assert z[f"case_{g}_app_c0e0"].all()
        assert np.array_equal(z[f"case_{g}_app_c1e0"], cm)
        assert np.array_equal(z[f"case_{g}_app_c0e1"], ~(de & ne))
        final = z[f"case_{g}_app_c1e1"]
        assert not (final & ~cm).any()          # the edge step only removes points
        assert final.sum() < cm.sum()
        for k, v in z.items():
            if k.startswith(f"case_{g}_"):
                assert v.shape == (S, H, W) and v.dtype == np.bool_, k
                assert z["band_" + k[5:]].shape == v.shape, k
