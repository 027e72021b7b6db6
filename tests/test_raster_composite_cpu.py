"""The scenes of tests/raster_composite_helper.py have the properties tests/test_raster_composite_gpu.py relies on — conditions, checked
where they can be run without a GPU: the designed list lengths, every fp64 threshold margin above the fp32 error of the decided quantity
(so no GPU assertion needs an allowance for a flipped decision), the closing steps that put the forward's exits on both halves of its
unrolled loop and the backward's `++k; break` at, before and beyond the end of a list, and images that change by more than ten GPU
tolerances when a list loses an entry or has two entries swapped."""
import numpy as np
import pytest
import torch

import raster_composite_helper as CH

SMALL = CH.LISTS + CH.SAT + CH.EDGE


@pytest.mark.parametrize("name", SMALL)
def test_list_lengths_are_the_designed_ones(name):
    _, design, W, H = CH.scene(name)
    lens = CH.list_lengths(name)
    assert np.array_equal(lens, design), (lens, design)
    if name in CH.LISTS + CH.SAT:
        base = lens - lens.min()
        assert set(base.ravel().tolist()) == set(range(8))          # lengths 0 to 7 (over the wide ones) all occur
        assert base[0, 0] == 0 and base[0, 1] == 1 and base[0, CH.TIE_TILE] == 4 and base[0, 7] == 7 and base[0, 9] == 1   # empty between full
    if lens.shape[0] == 2:                                          # the second camera's lists differ and start at non-zero offsets
        assert not np.array_equal(lens[0], lens[1]) and CH.projected(name)["offs"][lens.shape[1]] > 0


def test_default_scene_takes_the_launcher_s_own_choice():
    _, _, W, H = CH.scene(CH.DEFAULT)
    lens = CH.list_lengths(CH.DEFAULT)
    assert lens.shape == (2, 4096) and lens.size >= 8192            # raster.hip: 4 pixels per lane from 8192 tile-camera pairs up
    print("pairs", int(lens.sum()), "longest list", int(lens.max()), "non-empty tiles", int((lens > 0).sum()))
    assert (int(lens.sum()), int(lens.max()), int((lens > 0).sum())) == (8049, 6, 4868)
    assert lens[0, 3584:].sum() > 0 and lens[1, 3584:].sum() > 0    # tile indices with the top bits set, and the camera bit, are in the sort keys
    assert not np.array_equal(lens[0], lens[1])


@pytest.mark.parametrize("name", SMALL + [CH.DEFAULT])
def test_margins_meet_the_floors(name):
    _, _, W, H = CH.scene(name)
    _, margins = CH.reference(name, "plain", torch.float64)
    floors = CH.floors(W)
    if name == CH.DEFAULT:
        issue, floors = floors, CH.default_floors(int(CH.projected(name)["radii"].max()))
        assert all(floors[k] >= v for k, v in issue.items())          # nothing below what every scene is held to
    print(name, "margins", margins, "floors", floors)
    for k, floor in floors.items():
        assert margins.get(k, float("inf")) >= floor, (k, margins, floors)


@pytest.mark.parametrize("name", SMALL)
def test_walk_model_is_the_fp64_helper(name):
    """the numpy walk over the lists of oracle.raster_ref.isect_tiles gives the image of RM.rasterize (the masked, loop-free formulation):
    what the model says about closing steps is about the reference the GPU is compared with"""
    rgb, dep, al, _ = CH.walk(name)
    (r64, d64, a64), _ = CH.reference(name, "bg_D", torch.float64)
    bg = CH.backgrounds(rgb.shape[0]).astype(np.float64)
    assert np.abs(rgb + bg[:, None, None, :] * (1 - al[..., None]) - r64).max() < 1e-13
    assert np.abs(dep - d64[..., 0]).max() < 1e-13 and np.abs(al - a64[..., 0]).max() < 1e-13


@pytest.mark.parametrize("ppl", [1, 2, 4])
def test_closing_steps_cover_both_halves_the_last_entry_and_beyond(ppl):
    """over the regions of the kernel with `ppl` pixels per lane in the scenes with wide Gaussians: the last pixel of a region closes at
    even and at odd steps (the A and the B half of the forward's unrolled loop), at the last entry of its list, with at least three
    entries left (both sets of the pipeline hold requested records at the exit), and never (the list runs out first)"""
    closings = []
    for name in CH.SAT:
        closings += CH.region_closings(name, CH.walk(name)[3], ppl)
    closed = [(L, k) for L, k in closings if k >= 0]
    assert {k % 2 for _, k in closed} == {0, 1}
    assert any(k == L - 1 for L, k in closed)
    assert any(L - 1 - k >= 3 for L, k in closed)
    assert any(k < 0 for _, k in closings)
    assert any(0 < L - 1 - k < 3 for L, k in closed)               # and one or two left, between the two


@pytest.mark.parametrize("name", [n for n in CH.SAT if not n.startswith("sat5")])
def test_pixels_of_a_region_close_at_different_steps(name):
    """under five wide Gaussians single pixels stop part-way through their lists, at a small one, before their region does: the lanes of a
    wave, and the pixels of a lane (horizontal and vertical neighbours), do not all close together"""
    close = CH.walk(name)[3]
    C, H, W = close.shape
    assert (close[:, :, 0:W - 1:2] != close[:, :, 1:W:2]).any() and (close[:, 0:H - 1:2] != close[:, 1:H:2]).any()
    per_tile_spread = [len(np.unique(close[c, y:y + 16, x:x + 16])) for c in range(C) for y in range(0, H, 16) for x in range(0, W, 16)]
    assert max(per_tile_spread) >= 3


def _distance(name, mutated, true, b):
    """of a mutated walk from the true one, in GPU tolerances of the plain configuration"""
    return max(np.abs(mutated[0] - true[0]).max() / b["tol"]["rgb"], np.abs(mutated[2] - true[2]).max() / b["tol"]["alpha"])


@pytest.mark.parametrize("name", CH.LISTS + CH.SAT)
def test_detection_power(name):
    """A list that loses an entry, or has two overlapping entries swapped, gives an image further than 10 x the GPU tolerance from the true
    one, so the GPU comparison would see either.  In the longest list (tile 7: 7 small Gaussians, all within 1.5 px of the tile centre, in
    front of the wide ones, which overlap everything): every single drop and every swap of neighbours among the 7 small ones and, with wide
    ones, the first three of those; the rest is printed (behind four wide ones an entry weighs 1.6e-3 and less: from a few dozen tolerances
    down to none behind the closing one).  The swap of two of the tied four is asserted where they sit behind two wide ones at most
    (no wide ones, and five); with six and seven they sit behind five, or behind the closing one."""
    p = CH.projected(name)
    true = CH.walk(name)
    b = CH.bounds(name, "plain")
    lens = CH.list_lengths(name)[0]
    n_wide, tile = int(lens.min()), int(lens.argmax())
    L = int(lens[tile])
    assert L >= 3
    drops = [_distance(name, CH.walk(name, *CH.drop_entry(p["vals"], p["offs"], tile, i)), true, b) for i in range(L)]
    swaps = [_distance(name, CH.walk(name, *CH.swap_entries(p["vals"], p["offs"], tile, i, i + 1)), true, b) for i in range(L - 1)]
    print(name, "tolerances", b["tol"], "\n  drop of entry i, in tolerances:", ["%.3g" % d for d in drops], "\n  swap of i, i + 1:", ["%.3g" % d for d in swaps])
    upto = L if n_wide == 0 else 10
    assert min(drops[:upto]) > 10 and min(swaps[:upto - 1]) > 10
    if n_wide <= 5:
        tied = [i for i, g in enumerate(p["vals"][p["offs"][CH.TIE_TILE]:p["offs"][CH.TIE_TILE + 1]]) if CH.scene(name)[0]["scales"][g, 0] < 1]
        assert len(tied) == 4
        d = _distance(name, CH.walk(name, *CH.swap_entries(p["vals"], p["offs"], CH.TIE_TILE, tied[0], tied[1])), true, b)
        print("  swap of two of the tied four:", "%.3g" % d)
        assert d > 10


@pytest.mark.parametrize("mode", list(CH.MODES))
@pytest.mark.parametrize("name", CH.LISTS + CH.SAT)
def test_gradient_yardstick_has_a_scale(name, mode):
    """the GPU gradients are held to e64 <= 4 e32, e32 = rel-L2(fp32 helper, fp64 helper).  That asks for fp32 accuracy only where e32 is
    itself at least the resolution of fp32: below eps = 2^-23 it is the luck of the helper's last rounding (a gradient vector carried by a
    few wide Gaussians, each a sum over a flat image, comes out at 1e-8), which no fp32 kernel can be asked to repeat.  Every splat gradient
    of every scene the GPU test differentiates has e32 >= eps.  The backgrounds' gradient is a plain sum over the pixels that the kernel adds
    in fp64 and rounds once (tests/test_raster_modes_gpu.py): half an ulp, at most eps / 2, which 4 e32 covers from e32 >= eps / 8."""
    g64, g32 = CH.reference_gradients(name, mode, torch.float64), CH.reference_gradients(name, mode, torch.float32)
    e32 = {k: float(np.linalg.norm(g32[k] - g64[k]) / np.linalg.norm(g64[k])) for k in g64}
    print(name, mode, {k: "%.2e" % v for k, v in e32.items()})
    assert set(e32) == set(CH.NAMES) | ({"backgrounds"} if mode == "bg_D" else set())
    assert min(e32[k] for k in CH.NAMES) >= CH.EPS32 and e32.get("backgrounds", 1e-6) >= CH.EPS32 / 8
    assert max(e32.values()) < 2.5e-4                                              # and 4 e32 stays under the yardstick's 1e-3


def test_the_tied_four_are_listed_in_index_order_not_colour_order():
    name = "lists_80x48"
    p = CH.projected(name)
    ids = p["vals"][p["offs"][CH.TIE_TILE]:p["offs"][CH.TIE_TILE + 1]]
    inp = CH.scene(name)[0]
    assert len(np.unique(inp["means"][ids, 2].view(np.uint32))) == 1              # bit-equal depths
    assert np.array_equal(ids, np.sort(ids))                                      # stable: index order
    red = inp["colors"][ids, 0]
    assert np.array_equal(np.argsort(np.argsort(red)), CH.TIE_RANK)               # which is not the colour order
