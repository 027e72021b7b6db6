"""tests/bilagrid_helper.py (the torch restatement of the bilateral-grid slice and of the total variation that the GPU tests use as
reference and yardstick) in fp64 against tests/golden/bilagrid_*.npz: the reference's own lib_bilagrid run in fp64 on the same
fp32-valued inputs (tools/gen_golden_bilagrid.py).  The same arithmetic in the same precision: agreement is at fp64 rounding."""
import numpy as np
import pytest
import torch

import bilagrid_helper as BH

TOL = 2e-14       # relative to the largest element: a few hundred fp64 ulps for sums of 8 to ~10^4 terms in another order


@pytest.mark.parametrize("name", ["a", "b"])
def test_helper_matches_the_reference_in_fp64(name):
    z = BH.load_golden(name)
    t = {k: torch.from_numpy(z[k]) for k in ("grids", "xy", "rgb", "v_out")}
    ids = torch.from_numpy(z["ids"])
    got = BH.gradients(t["grids"], t["xy"], t["rgb"], ids, t["v_out"], torch.float64)
    for k in ("out", "v_grids", "v_rgb"):
        assert got[k].shape == z[k].shape
        e = BH.max_rel(got[k].numpy(), z[k])
        print(f"scene {name} {k}: max error relative to the largest element {e:.2e}")
        assert e <= TOL, (k, e)
    tv = BH.tv_gradients(t["grids"], torch.float64)
    assert abs(float(tv["tv"]) - float(z["tv"])) <= TOL * abs(float(z["tv"]))
    if "tv_grad" in z:
        assert BH.max_rel(tv["v_x"].numpy(), z["tv_grad"]) <= TOL


@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_scenes_are_what_the_tests_rely_on(name):
    """No sample within 1e-4 grid units of a cell boundary (fp32 rounding cannot move a sample into another cell); some samples clamp
    in z; scene a leaves grid 1 unused (its gradient is exactly zero), scene b names grid 1 twice and clamps in x and y too."""
    z = BH.load_golden(name)
    xy, rgb = torch.from_numpy(z["xy"]), torch.from_numpy(z["rgb"])
    assert z["grids"].dtype == np.float32 and xy.dtype == torch.float32 and rgb.dtype == torch.float32 and z["out"].dtype == np.float64
    margin = BH.boundary_margin(z["grids"].shape, xy, rgb)
    assert min(margin) >= 1e-4, margin
    clamped = BH.z_clamped(z["grids"].shape, rgb)
    assert 0.005 < float(clamped.double().mean()) < 0.1
    if name == "a":
        assert z["ids"].tolist() == [2, 0] and z["grids"].shape == (3, 12, 3, 4, 5) and z["rgb"].shape == (2, 18, 33, 3)
        assert not z["v_grids"][1].any() and z["v_grids"][0].any() and z["v_grids"][2].any()
    else:
        assert z["ids"].tolist() == [1, 1, 0] and z["grids"].shape == (2, 12, 8, 16, 16) and z["rgb"].shape == (3, 70 * 45, 3)
        assert float(xy.min()) < 0 and float(xy.max()) > 1


def test_helper_total_variation_of_small_and_degenerate_shapes():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 12, 2, 3, 4, generator=g, dtype=torch.float64)
    want = sum(((x.narrow(a, 1, x.shape[a] - 1) - x.narrow(a, 0, x.shape[a] - 1)) ** 2).sum() / (x[0].numel() // x.shape[a] * (x.shape[a] - 1))
               for a in (2, 3, 4)) / 2
    assert abs(float(BH.total_variation(x)) - float(want)) < 1e-14
    assert float(BH.total_variation(torch.ones(1, 12, 1, 1, 1, dtype=torch.float64))) == 0.0     # no differences along any axis
