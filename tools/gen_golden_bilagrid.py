"""Writes tests/golden/bilagrid_*.npz: the REFERENCE's own bilateral-grid slice and total variation (gsplat's examples/lib_bilagrid.py),
run on the CPU in fp64 on fp32-valued inputs.  Data only: inputs, the sliced rgb, grids.grad and rgb.grad for a stored upstream
gradient, the total variation of the grids and its gradient.

    python tools/gen_golden_bilagrid.py <reference gsplat examples dir>

lib_bilagrid imports tensorly at module level (only its CP-decomposed 4-D grid uses it); where tensorly is absent a stub module with a
no-op set_backend stands in.  The module builds fp32 grids: .double() on it converts the grids and the grey-weight buffer.

Scenes
  a   3 grids of 5 x 4 x 3 (Wg, Hg, L), 2 images of 33 x 18 as 4-D [B, h, w, .] input, xy uniform in [0, 1], ids [2, 0] (grid 1 unused), rgb
      uniform in [-0.15, 1.15] (a few per cent of the samples clamp in z), grids identity + 0.2 randn.  One file.
  b   2 grids of the default 16 x 16 x 8, 3 rows of 70 * 45 samples as 3-D [B, n, .] input, ids [1, 1, 0] (grid 1 named twice), xy
      uniform in [-0.1, 1.1] (x / y clamp too).  Three files (_in, _out, _grad) to keep each within a few hundred KB.
Asserted here and again by tests/test_bilagrid_cpu.py: no sample lies within 1e-4 grid units of a cell boundary on any axis (the
interpolant has kinks there; fp32 rounding must not be able to change a sample's cell).  A scene that violates it gets another seed."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bilagrid_helper as BH  # noqa: E402

MARGIN = 1e-4


def load_reference(examples_dir):
    try:
        import tensorly  # noqa: F401
    except ImportError:
        stub = types.ModuleType("tensorly")
        stub.set_backend = lambda *a, **k: None
        sys.modules["tensorly"] = stub
    sys.path.insert(0, examples_dir)
    import lib_bilagrid
    return lib_bilagrid


def scene_a(seed):
    g = torch.Generator().manual_seed(seed)
    G, Wg, Hg, L, C, H, W = 3, 5, 4, 3, 2, 18, 33
    grids = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(1, 12, 1, 1, 1).repeat(G, 1, L, Hg, Wg)
    grids = grids + 0.2 * torch.randn(grids.shape, generator=g)
    xy = torch.rand(C, H, W, 2, generator=g)       # (the pixel-centre meshgrid of a 33-wide image puts its middle column exactly on a cell boundary)
    rgb = torch.rand(C, H, W, 3, generator=g) * 1.3 - 0.15
    v_out = torch.randn(C, H, W, 3, generator=g)
    return dict(grids=grids, xy=xy, rgb=rgb, v_out=v_out, ids=torch.tensor([2, 0]))


def scene_b(seed):
    g = torch.Generator().manual_seed(seed)
    G, Wg, Hg, L, C, n = 2, 16, 16, 8, 3, 70 * 45
    grids = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(1, 12, 1, 1, 1).repeat(G, 1, L, Hg, Wg)
    grids = grids + 0.2 * torch.randn(grids.shape, generator=g)
    xy = torch.rand(C, n, 2, generator=g) * 1.2 - 0.1
    rgb = torch.rand(C, n, 3, generator=g) * 1.3 - 0.15
    v_out = torch.randn(C, n, 3, generator=g)
    return dict(grids=grids, xy=xy, rgb=rgb, v_out=v_out, ids=torch.tensor([1, 1, 0]))


def run(lib, sc):
    G, _, L, Hg, Wg = sc["grids"].shape
    bil = lib.BilateralGrid(G, grid_X=Wg, grid_Y=Hg, grid_W=L).double()
    assert bil.grids.shape == sc["grids"].shape and bil.grids.dtype == torch.float64
    with torch.no_grad():
        bil.grids.copy_(sc["grids"].double())
    rgb = sc["rgb"].double().requires_grad_(True)
    out = lib.slice(bil, sc["xy"].double(), rgb, sc["ids"].unsqueeze(-1))["rgb"]
    assert out.dtype == torch.float64 and out.shape == rgb.shape
    (out * sc["v_out"].double()).sum().backward()
    res = dict(out=out.detach(), v_grids=bil.grids.grad.clone(), v_rgb=rgb.grad.clone())
    bil.grids.grad = None
    tv = lib.total_variation_loss(bil.grids)
    tv.backward()
    res.update(tv=tv.detach(), tv_grad=bil.grids.grad.clone())
    return res


def main():
    lib = load_reference(sys.argv[1])
    gold = os.path.join(ROOT, "tests", "golden")
    for name, make in (("a", scene_a), ("b", scene_b)):
        for seed in range(20000):
            sc = make(seed)
            margin = BH.boundary_margin(sc["grids"].shape, sc["xy"], sc["rgb"])
            if min(margin) >= MARGIN:
                break
        else:
            raise SystemExit(f"scene {name}: no seed keeps every sample {MARGIN} grid units from the cell boundaries")
        res = run(lib, sc)
        clamped = float(BH.z_clamped(sc["grids"].shape, sc["rgb"]).double().mean())
        print(f"scene {name}: seed {seed}, margin (x, y, z) {margin}, {100 * clamped:.1f} % of the samples clamp in z, tv {float(res['tv']):.6f}")
        inputs = {k: sc[k].numpy() for k in ("grids", "xy", "rgb", "v_out")}
        inputs["ids"] = sc["ids"].numpy().astype(np.int64)
        inputs["seed"] = np.int64(seed)
        outs = {k: res[k].numpy() for k in ("out", "v_rgb")}
        grads = {"v_grids": res["v_grids"].numpy(), "tv": res["tv"].numpy()}
        if name == "a":
            grads["tv_grad"] = res["tv_grad"].numpy()        # (b's would be another 390 KB; its value is kept)
            np.savez(os.path.join(gold, "bilagrid_a.npz"), **inputs, **outs, **grads)
        else:
            np.savez(os.path.join(gold, "bilagrid_b_in.npz"), **inputs)
            np.savez(os.path.join(gold, "bilagrid_b_out.npz"), **outs)
            np.savez(os.path.join(gold, "bilagrid_b_grad.npz"), **grads)


if __name__ == "__main__":
    main()
