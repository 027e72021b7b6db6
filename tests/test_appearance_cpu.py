"""The appearance module, CPU side: the torch restatement tests/appearance_helper.py against the reference's own fp64 numbers
(tests/golden/appearance_*.npz from tools/gen_golden_appearance.py), the fixtures' ReLU margin, the module's parameter names, the
library's exports, the kernels' resource figures, and what the module refuses."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import appearance_helper as AH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")


def _built_library():
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(lib)


def _inputs(z):
    state = {k[6:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state.")}
    ids = torch.from_numpy(z["embed_ids"]) if bool(z["has_ids"]) else None
    return state, torch.from_numpy(z["features"]), ids, torch.from_numpy(z["dirs"]), torch.from_numpy(z["v_out"]), int(z["degree"])


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_the_reference_in_fp64(name):
    z = AH.load_golden(name)
    state, features, ids, dirs, v_out, degree = _inputs(z)
    assert all(t.dtype == torch.float32 for t in (features, dirs, v_out, *state.values()))
    got = AH.gradients(state, features, ids, dirs, v_out, degree, torch.float64)
    for k in ("out", "v_features", "v_dirs"):
        err = AH.max_rel(got[k].numpy(), z[k])
        print(name, k, err)
        assert z[k].dtype == np.float64 and err <= 1e-12, (k, err)
    for k in AH.KEYS:
        ref = z["grad." + k]
        if name == "b" and k == "embeds.weight":
            assert not ref.any() and not got[k].any()                     # embed_ids None: no embedding takes part
            continue
        err = AH.max_rel(got[k].numpy(), ref)
        print(name, k, err)
        assert err <= 1e-12, (k, err)
    if name == "a":
        assert not z["grad.embeds.weight"][[1, 2, 3]].any() and z["grad.embeds.weight"][[0, 4]].any()
    else:
        assert not z["grad.color_head.0.weight"][:, 48 + 4:].any() and not z["grad.color_head.0.weight"][:, :16].any()


@pytest.mark.parametrize("name", ["a", "b"])
def test_no_pre_activation_sits_on_the_relu_kink(name):
    z = AH.load_golden(name)
    state, features, ids, dirs, _, degree = _inputs(z)
    lo, err = AH.relu_margin(state, features, ids, dirs, degree)
    print(name, "smallest |pre-activation|", lo, "fp32 error", err, "stored margin", float(z["margin"]))
    assert lo >= float(z["margin"]) and lo >= 16 * err


def test_state_dict_keys_and_shapes_are_the_reference_modules():
    from hunyuanworld_mirror_amd import AppearanceOptModule
    z = AH.load_golden("a")
    m = AppearanceOptModule(5, 32, 16, 3)
    sd = m.state_dict()
    assert list(sd) == list(AH.KEYS)
    for k in AH.KEYS:
        assert tuple(sd[k].shape) == z["state." + k].shape and sd[k].dtype == torch.float32, k
    m.load_state_dict({k: torch.from_numpy(z["state." + k]) for k in AH.KEYS})
    assert isinstance(m.embeds, torch.nn.Embedding) and isinstance(m.color_head, torch.nn.Sequential)
    assert AppearanceOptModule(2, 32, sh_degree=1).color_head[0].weight.shape == (64, 16 + 32 + 4)


def test_library_exports_the_appearance_entries():
    from hunyuanworld_mirror_amd import _lib
    L = _built_library()
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    for sym in ("wm_appearance_forward", "wm_appearance_backward", "wm_appearance_backward_workspace_bytes"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and (sym + "(") in hdr, sym


def _blocks(L, N, C_):
    """the backward's grid size, read back from the workspace size: blocks x (7428 + 256 C) floats + one reduced set + C x 64 floats, each
    part rounded up to 256 bytes"""
    L.wm_appearance_backward_workspace_bytes.restype = ctypes.c_size_t
    L.wm_appearance_backward_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    al = lambda x: (x + 255) // 256 * 256
    total = L.wm_appearance_backward_workspace_bytes(N, C_)
    rest = total - al(7428 * 4) - al(C_ * 64 * 4)
    for b in range(1, 4097):
        if al(b * 7428 * 4) + al(b * 4 * C_ * 64 * 4) == rest:
            return b
    raise AssertionError((N, C_, total))


def test_python_constants_are_the_kernels_and_the_grid_depends_on_n_alone():
    """appearance.TILE / MAX_BLOCKS restate csrc/wm_kernels.h (a test sizes its scene by them), and the persistent grid is
    min(tiles, MAX_BLOCKS)-shaped: ceil(tiles / ceil(tiles / MAX_BLOCKS)) blocks, whatever C is"""
    from hunyuanworld_mirror_amd import appearance as A
    hdr = open(os.path.join(CSRC, "wm_kernels.h")).read()
    assert int(re.search(r"WM_APPEARANCE_TILE = (\d+)", hdr).group(1)) == A.TILE
    assert int(re.search(r"WM_APPEARANCE_MAX_BLOCKS = (\d+)", hdr).group(1)) == A.MAX_BLOCKS
    L = _built_library()
    for N in (1, A.TILE, A.TILE + 1, A.MAX_BLOCKS * A.TILE, A.MAX_BLOCKS * A.TILE + 1, 2 * A.MAX_BLOCKS * A.TILE - 3 * A.TILE + 37, 5 * A.MAX_BLOCKS * A.TILE):
        tiles = -(-N // A.TILE)
        per_block = -(-tiles // A.MAX_BLOCKS)
        for C_ in (1, 3):
            assert _blocks(L, N, C_) == -(-tiles // per_block), (N, C_)


def test_refused_configurations_name_the_argument():
    from hunyuanworld_mirror_amd import AppearanceOptModule
    for kw, word in ((dict(feature_dim=16), "feature_dim"), (dict(embed_dim=8), "embed_dim"), (dict(mlp_width=32), "mlp_width"),
                     (dict(mlp_depth=3), "mlp_depth"), (dict(sh_degree=4), "sh_degree")):
        args = dict(n=3, feature_dim=32)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            AppearanceOptModule(**args)
    m = AppearanceOptModule(3, 32, sh_degree=2)
    with pytest.raises(NotImplementedError, match="sh_degree"):
        m(torch.zeros(4, 32), None, torch.ones(2, 4, 3), 3)
    with pytest.raises(NotImplementedError, match="feature_dim"):
        m(torch.zeros(4, 16), None, torch.ones(2, 4, 3), 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(4, 32), None, torch.ones(2, 4, 3), 1)           # CPU tensors: no fallback
    with pytest.raises(ValueError):
        m(torch.zeros(5, 32), None, torch.ones(2, 4, 3), 1)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_appearance_kernels_use_no_scratch(tmp_path):
    """The backward keeps dW2 and dW1's feature and basis columns, 128 accumulator registers per lane, over its whole run beside the
    activations of the pair in flight; a form that kept the feature share of layer 1 as well, or selected between two elements of the
    basis array, went to scratch.  Resource figures only: no kernel of the file may spill or use scratch, the two hot ones in any of the four degrees."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = [f.replace("$(ARCH)", "gfx950") for f in line.split("=", 1)[1].split() if not f.startswith("$(")]
    r = subprocess.run(["hipcc", *flags, "-x", "hip", "-c", os.path.join(CSRC, "appearance.hip"), "-o", str(tmp_path / "a.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {"appearance_fwd_kernel": 0, "appearance_bwd_kernel": 0, "appearance_reduce_kernel": 0, "appearance_finalize_kernel": 0}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        for kind in seen:
            if kind in name:
                seen[kind] += 1
                print(name, "VGPRs", get(r"VGPRs"), "AGPRs", get(r"AGPRs"), "occupancy", get(r"Occupancy \[waves/SIMD\]"), "LDS", get(r"LDS Size \[bytes/block\]"))
                assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0, b[:600]
    assert seen == {"appearance_fwd_kernel": 4, "appearance_bwd_kernel": 4, "appearance_reduce_kernel": 1, "appearance_finalize_kernel": 1}
