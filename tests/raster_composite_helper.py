"""TEST INFRASTRUCTURE ONLY (not a test file): seeded scenes that put the compositing kernels' list walk (csrc/raster.hip
raster_composite_kernel<PX,PY>, csrc/raster_bwd_composite.h) at chosen edges, a numpy model of that walk, and the shared fp64 / fp32
references of tests/test_raster_composite_cpu.py and tests/test_raster_composite_gpu.py.

Cameras have the identity rotation (the second one of a pair: diag(-1,-1,1,1), exact in fp32, a point mirror of the image), focal F_SMALL
and the principal point at the image centre; Gaussians have quats (1,0,0,0) and colours given directly, so a Gaussian meant for pixel
(u, v) at depth z sits at ((u - W/2) z / f, (v - H/2) z / f, z).  Two kinds:
  small   3-D scale 0.05 z / 2 x SMALL_AXES = (1, 0.8, 0.9): a pixel of sigma, radius 4 on the axis and at most 6 at the corners of an
          80-pixel image (the perspective term of the Jacobian), centred within +-OFFSET = 1.5 px of a tile's centre: it stays inside
          its own tile.  Not isotropic, so that the gradient of the quaternions is not identically zero
  wide    3-D scale 50 z, opacity 0.8: alpha 0.8 (to 2e-4) on every pixel of every tile; the transmittance under n of them is 0.2^n,
          3.2e-4 at n = 5 and 6.4e-5 <= 1e-4 at n = 6, so the sixth wide one closes every pixel that is still open, well clear of 1e-4.

Scene 1 ("lists"): tile t holds t % 8 small Gaussians at distinct depths base + 0.03 j + 0.001 t, base 0.5 in odd tiles and 1.9 in even
ones; TIE_TILE = 8, which that rule leaves empty, holds four at one bit-equal depth (2.0) whose index order (the stable sort's order) is
not their colour order.
Scene 2 ("sat"): scene 1 plus n wide ones at WIDE_DEPTHS[n], all behind the odd tiles' small ones and around the even tiles'.  The odd
tiles' small ones weigh as in scene 1, so a misplaced entry shows in the image and the gradients are not those of the wide ones alone
(whose sums over a flat image the fp32 helper gets right to a tenth of an ulp: no scale for a yardstick); the even tiles' sit under one
to five wide ones.  n = 5: a list always runs out first ("never"); n = 7: in an even tile the sixth wide one, between small ones 2 and 3,
closes the region with 1 to 5 entries left, in an odd tile with one left; n = 6 is added to the issue's 5 and 7 because with those two
alone no region can close AT its last entry (the sixth wide one closes what is left and the seventh always follows it): with six, the
sixth is the deepest entry of every list.  Pixels under a strong small Gaussian close one or two wide ones earlier than their neighbours
(alpha 0.98 leaves 0.02, and 0.02 x 0.2^4 <= 1e-4), and under five wide ones at a small one with alpha >= 0.6875, so the pixels of a
lane, and the lanes of a wave, close at different steps.
Scene 3 ("edge"): three wide ones and a small one near the centre, at sizes from 1 x 1 up.
Scene 4 ("default"): two cameras at 1024 x 1024, 64 x 64 x 2 = 8192 tile-camera pairs: what the launcher's own choice sends to the
4-pixel kernel.  400 random Gaussians; DEFAULT_SEED is the first seed whose scene meets every margin floor."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import raster_grad_helper as RG
import raster_modes_helper as RM
from oracle import raster_ref as R

TILE = 16
EPS32 = 2.0 ** -23
F_SMALL = 40.0
OFFSET = 1.5
SMALL_AXES = (1.0, 0.8, 0.9)
TIE_TILE = 8
TIE_RANK = (2, 0, 3, 1)          # colour rank of the four tied Gaussians, in index order
WIDE_DEPTHS = {5: (1.0, 1.955, 2.9, 3.0, 3.1),
               6: (0.8, 0.9, 1.0, 1.1, 1.955, 3.0),
               7: (0.8, 0.9, 1.0, 1.1, 1.2, 1.985, 3.0)}
EDGE_SIZES = [(1, 1), (17, 1), (1, 17), (15, 15), (16, 16), (17, 17), (41, 29), (33, 8), (9, 40)]
# scene 4 is held to default_floors() below.  Seeds 1 to 38 each miss one of them: 17 (1 to 4, 7, 8, 11, 15, 20, 24, 27 to 29, 31, 34, 37, 38)
# the issue's own alpha_threshold floor 7.5e-9; 20 more (5, 6, 9, 10, ...) meet the issue's four floors but not the sixfold alpha_threshold
# one, with margins from 7.6e-9 to 4.3e-8, and on seed 5 (2.0e-8) the fp32 helper does flip a 1/255 decision: e32 = 3.9e-3; seed 22 (5.9e-8)
# misses the radius floor (1.9e-5).  39 is the first that meets all: alpha_threshold 6.1e-8, tile 2.6e-4, radius 1.0e-4; 8049 pairs,
# longest list 6, 4868 of 8192 tiles non-empty
DEFAULT_SEED = 39
NAMES = RM.NAMES


def floors(width):
    """the margin floors of tests/test_raster_modes_gpu.py's docstring, the tile one for this image's number of tiles across"""
    return {"alpha_threshold": 16 * EPS32 / 255, "alpha_cap": 16 * EPS32, "stop": 170 * EPS32 * 1e-4, "tile": 4 * EPS32 * math.ceil(width / TILE)}


def default_floors(max_radius):
    """scene 4's floors: the four above, with two made stricter by what its size adds.  alpha_threshold x 6: next to 1/255 an alpha's
    relative error is the absolute error of its exponent, and the exponent there is ln(255 opacity) <= 5.5 times factors that carry the 16 eps.
    radius, 16 eps x the largest radius: no ceil() differs between fp32 and fp64, so the GPU's list total is the reference's (the small
    scenes need no such floor: a ceil() that flips there leaves the Gaussian inside its tile, or the wide one over every tile)."""
    f = floors(1024)
    f["alpha_threshold"] *= 6
    f["radius"] = 16 * EPS32 * max_radius
    return f


# ------------------------------------------------------------------------------------------------ scene builders
def _cameras(W, H, f, second=None):
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    vms = [np.eye(4, dtype=np.float32)] + ([] if second is None else [second.astype(np.float32)])
    return np.stack(vms), np.stack([K] * len(vms))


class _Builder:
    def __init__(self, W, H, f):
        self.W, self.H, self.f = W, H, f
        self.rows = []

    def add(self, u, v, z, scales, opacity, colour):
        self.rows.append(((u - self.W / 2) * z / self.f, (v - self.H / 2) * z / self.f, z, *scales, opacity, *colour))

    def small(self, u, v, z, opacity, colour):
        self.add(u, v, z, [0.05 * z / 2 * a for a in SMALL_AXES], opacity, colour)

    def wide(self, z, colour):
        self.add(self.W / 2, self.H / 2, z, [50.0 * z] * 3, 0.8, colour)

    def scene(self, viewmats, Ks, order=None):
        a = np.array(self.rows, np.float64)
        if order is not None:
            a = a[order]
        n = len(a)
        inp = {"means": a[:, :3], "quats": np.tile([1.0, 0, 0, 0], (n, 1)), "scales": a[:, 3:6], "opacities": a[:, 6], "colors": a[:, 7:10],
               "viewmats": viewmats, "Ks": Ks}
        return {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}


def _lists_builder(W, H, seed):
    """scene 1's Gaussians -> builder, designed list length per tile of the first camera, indices of the tied four"""
    g = np.random.default_rng(seed)
    tw, th = math.ceil(W / TILE), math.ceil(H / TILE)
    b = _Builder(W, H, F_SMALL)
    design, tie = np.zeros(tw * th, np.int64), []
    for t in range(tw * th):
        cx, cy = (t % tw) * TILE + TILE / 2, (t // tw) * TILE + TILE / 2
        if t == TIE_TILE:
            for rank in TIE_RANK:
                du, dv = g.uniform(-OFFSET, OFFSET, 2)
                tie.append(len(b.rows))
                b.small(cx + du, cy + dv, 2.0, 0.6, (0.1 + 0.25 * rank, 0.9 - 0.25 * rank, 0.5))
            design[t] = len(TIE_RANK)
            continue
        for j in range(t % 8):
            du, dv = g.uniform(-OFFSET, OFFSET, 2)
            b.small(cx + du, cy + dv, (0.5 if t % 2 else 1.9) + 0.03 * j + 0.001 * t, g.uniform(0.5, 0.98), g.uniform(0.05, 1.0, 3))
        design[t] = t % 8
    return b, design, np.array(tie)


MIRROR = np.diag([-1.0, -1.0, 1.0, 1.0])


def lists_scene(W, H, cameras=1, n_wide=0, seed=0):
    """scenes 1 (n_wide = 0) and 2 -> inputs, designed list lengths [C, tiles].  The Gaussians are shuffled (seeded), except that the tied
    four keep their relative order, so that list order is never index order."""
    b, design, tie = _lists_builder(W, H, seed)
    for i, z in enumerate(WIDE_DEPTHS.get(n_wide, ())):
        b.wide(z, (0.9 - 0.1 * i, 0.15 + 0.1 * i, 0.3 + 0.05 * (i % 3)))
    g = np.random.default_rng(seed + 1000)
    order = g.permutation(len(b.rows))
    where = np.sort(np.nonzero(np.isin(order, tie))[0])
    order[where] = tie                       # the tied four in their own order at the places the shuffle gave them
    vm, Ks = _cameras(W, H, F_SMALL, MIRROR if cameras == 2 else None)
    design = design + n_wide
    if cameras == 2:
        assert W % TILE == 0 and H % TILE == 0          # the point mirror maps tiles onto tiles
        design = np.stack([design, design[::-1]])
    else:
        design = design[None]
    return b.scene(vm, Ks, order), design


def edge_scene(W, H):
    """scene 3: a small Gaussian (radius 4) 0.3 px off the image centre between three wide ones -> inputs, designed list lengths: 3, and 4
    in the tiles the small one's square touches"""
    b = _Builder(W, H, F_SMALL)
    b.wide(1.0, (0.9, 0.2, 0.1))
    b.small(W / 2 + 0.3, H / 2 - 0.2, 2.0, 0.9, (0.1, 0.8, 0.3))
    b.wide(1.5, (0.2, 0.3, 0.9))
    b.wide(3.0, (0.5, 0.5, 0.2))
    vm, Ks = _cameras(W, H, F_SMALL)
    tx, ty = np.arange(math.ceil(W / TILE)) * TILE, np.arange(math.ceil(H / TILE)) * TILE
    hit_x, hit_y = (tx < W / 2 + 0.3 + 4) & (tx + TILE > W / 2 + 0.3 - 4), (ty < H / 2 - 0.2 + 4) & (ty + TILE > H / 2 - 0.2 - 4)
    return b.scene(vm, Ks), (3 + (hit_y[:, None] & hit_x[None, :])).reshape(1, -1)


def default_scene(seed=DEFAULT_SEED, n=400, W=1024, H=1024, f=600.0):
    """scene 4: random Gaussians in front of two cameras 0.125 apart in x, sparse (a 3-sigma footprint of some 30 px)"""
    g = np.random.default_rng(seed)
    z = g.uniform(2.0, 6.0, n)
    xy = g.uniform(-0.9, 0.9, (n, 2)) * (W / 2 / f) * z[:, None]
    quats = g.normal(size=(n, 4))
    inp = {"means": np.concatenate([xy, z[:, None]], 1), "quats": quats / np.linalg.norm(quats, axis=1, keepdims=True),
           "scales": g.uniform(0.003, 0.012, (n, 3)) * z[:, None], "opacities": g.uniform(0.3, 0.95, n), "colors": g.uniform(0.05, 1.0, (n, 3))}
    vm, Ks = _cameras(W, H, f, np.eye(4))
    vm[1, 0, 3] = 0.125
    inp.update(viewmats=vm, Ks=Ks)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}, None


SCENES = {"lists_80x48": lambda: (*lists_scene(80, 48), 80, 48),
          "lists_77x45": lambda: (*lists_scene(77, 45), 77, 45),
          "lists_80x48_2c": lambda: (*lists_scene(80, 48, cameras=2), 80, 48),
          "sat5_80x48_2c": lambda: (*lists_scene(80, 48, cameras=2, n_wide=5), 80, 48),
          "sat6_80x48": lambda: (*lists_scene(80, 48, n_wide=6), 80, 48),
          "sat6_77x45": lambda: (*lists_scene(77, 45, n_wide=6), 77, 45),
          "sat7_80x48": lambda: (*lists_scene(80, 48, n_wide=7), 80, 48),
          "sat7_77x45": lambda: (*lists_scene(77, 45, n_wide=7), 77, 45),
          "default_1024_2c": lambda: (*default_scene(), 1024, 1024)}
SCENES.update({f"edge_{w}x{h}": (lambda w=w, h=h: (*edge_scene(w, h), w, h)) for w, h in EDGE_SIZES})
LISTS = [k for k in SCENES if k.startswith("lists")]
SAT = [k for k in SCENES if k.startswith("sat")]
EDGE = [k for k in SCENES if k.startswith("edge")]
DEFAULT = "default_1024_2c"


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> inputs (numpy fp32: what the GPU, the fp32 and the fp64 helper all start from), designed list lengths or None, W, H"""
    return SCENES[name]()


def backgrounds(C):
    return np.array([[0.1, 0.5, 0.9], [1.0, 0.0, 0.25]], np.float32)[:C]


# the two configurations every scene is rendered in: options of RM.rasterize (backgrounds filled in per scene)
MODES = {"plain": dict(depth_mode="ED"), "bg_D": dict(depth_mode="D")}


def _options(name, mode):
    inp = scene(name)[0]
    return dict(MODES[mode], backgrounds=backgrounds(len(inp["viewmats"]))) if mode == "bg_D" else dict(MODES[mode])


@functools.lru_cache(maxsize=None)
def reference(name, mode, dtype):
    """RM.rasterize in `dtype` -> (rgb, depth, alpha) as numpy fp64 [C,H,W,ch], margins (fp64 runs; None otherwise)"""
    inp, _, W, H = scene(name)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    opts = _options(name, mode)
    if "backgrounds" in opts:
        opts["backgrounds"] = torch.from_numpy(opts["backgrounds"]).to(dtype)
    margins = {} if dtype == torch.float64 else None
    with torch.no_grad():
        outs = RM.rasterize(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], False, t["viewmats"], t["Ks"], W, H, margins=margins, **opts)
    return tuple(o.double().numpy() for o in outs), margins


def cotangents(name, seed=3):
    inp, _, W, H = scene(name)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(len(inp["viewmats"]), H, W, ch, generator=g).numpy() for ch in (3, 1, 1)]


@functools.lru_cache(maxsize=None)
def reference_gradients(name, mode, dtype):
    """RM.gradients under cotangents(name) -> dict of gradients (numpy fp64), backgrounds included in mode "bg_D" """
    inp, _, W, H = scene(name)
    return RM.gradients(inp, cotangents(name), False, W, H, dtype, **_options(name, mode))[1]


# ------------------------------------------------------------------------------------------------ lists and the walk model
@functools.lru_cache(maxsize=None)
def projected(name):
    """the fp64 projection and the sorted lists -> dict: m2 [C,N,2], conics [C,N,3], depths [C,N], radii, vals, offs, tw, th"""
    inp, _, W, H = scene(name)
    t = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    radii, m2, depths, conics, _ = RG.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H)
    radii, m2, depths, conics = radii.numpy(), m2.numpy(), depths.numpy(), conics.numpy()
    _, vals, offs, tw, th = R.isect_tiles(m2, radii, depths, W, H)
    return dict(m2=m2, conics=conics, depths=depths, radii=radii, vals=vals, offs=offs, tw=tw, th=th)


def list_lengths(name):
    p = projected(name)
    return np.diff(p["offs"]).reshape(-1, p["tw"] * p["th"])


def walk(name, vals=None, offs=None):
    """The list walk by the rules of oracle.raster_ref.composite (skip: sigma < 0 or alpha < 1/255; cap 0.999; stop BEFORE blending when
    T (1 - alpha) <= 1e-4) in fp64, over the scene's own lists or the given (mutated) ones.
    -> rgb [C,H,W,3], accumulated depth [C,H,W], alpha [C,H,W], close [C,H,W]: the step (index within the tile's list) at which the pixel
    stops, -1 where its list runs out first"""
    inp, _, W, H = scene(name)
    p = projected(name)
    vals, offs = (p["vals"], p["offs"]) if vals is None else (vals, offs)
    C, N = p["depths"].shape
    tw, th = p["tw"], p["th"]
    m2, cn, dp = p["m2"].reshape(C * N, 2), p["conics"].reshape(C * N, 3), p["depths"].reshape(C * N)
    op, col = inp["opacities"].astype(np.float64), inp["colors"].astype(np.float64)
    rgb, dep, al = np.zeros((C, H, W, 3)), np.zeros((C, H, W)), np.zeros((C, H, W))
    close = np.full((C, H, W), -1, np.int64)
    for c in range(C):
        for t in range(tw * th):
            y0, x0 = (t // tw) * TILE, (t % tw) * TILE
            y1, x1 = min(y0 + TILE, H), min(x0 + TILE, W)
            py, px = np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5, indexing="ij")
            T, done = np.ones(py.shape), np.zeros(py.shape, bool)
            acc, when = np.zeros(py.shape + (4,)), np.full(py.shape, -1, np.int64)
            for step, g in enumerate(vals[offs[c * tw * th + t]:offs[c * tw * th + t + 1]]):
                dx, dy = m2[g, 0] - px, m2[g, 1] - py
                sigma = 0.5 * (cn[g, 0] * dx * dx + cn[g, 2] * dy * dy) + cn[g, 1] * dx * dy
                alpha = np.minimum(0.999, op[g % N] * np.exp(-sigma))
                use = ~done & ~((sigma < 0) | (alpha < R.ALPHA_THRESHOLD))
                nT = T * (1.0 - alpha)
                stop = use & (nT <= 1e-4)
                when[stop] = step
                done |= stop
                use &= ~stop
                acc += np.where(use, alpha * T, 0.0)[..., None] * np.concatenate([col[g % N], dp[g:g + 1]])
                T = np.where(use, nT, T)
            rgb[c, y0:y1, x0:x1], dep[c, y0:y1, x0:x1], al[c, y0:y1, x0:x1], close[c, y0:y1, x0:x1] = acc[..., :3], acc[..., 3], 1.0 - T, when
    return rgb, dep, al, close


REGIONS = {1: (8, 8), 2: (16, 8), 4: (16, 16)}      # pixels per lane -> the wave's region (width, height)


def region_closings(name, close, ppl):
    """per wave of raster_composite_kernel at `ppl` pixels per lane whose region touches the image and whose list is not empty:
    (list length, step at which the last of its pixels closes or -1 if one never does)"""
    _, _, W, H = scene(name)
    lens = list_lengths(name)
    tw = math.ceil(W / TILE)
    rw, rh = REGIONS[ppl]
    out = []
    for c in range(close.shape[0]):
        for y0 in range(0, H, rh):
            for x0 in range(0, W, rw):
                L = int(lens[c, (y0 // TILE) * tw + x0 // TILE])
                if L:
                    k = close[c, y0:y0 + rh, x0:x0 + rw]
                    out.append((L, -1 if (k < 0).any() else int(k.max())))
    return out


def drop_entry(vals, offs, tile, i):
    """the lists without entry i of tile (camera-tile index) `tile`"""
    at = offs[tile] + i
    assert at < offs[tile + 1]
    o = offs.copy()
    o[tile + 1:] -= 1
    return np.delete(vals, at), o


def swap_entries(vals, offs, tile, i, j):
    assert offs[tile] + max(i, j) < offs[tile + 1]
    v = vals.copy()
    v[[offs[tile] + i, offs[tile] + j]] = v[[offs[tile] + j, offs[tile] + i]]
    return v, offs


# ------------------------------------------------------------------------------------------------ the tolerance
def bounds(name, mode):
    """Per output the bound on the per-pixel max-abs error against the fp64 helper: max(4 e32, 16 eps (Lmax + 1) scale), e32 = max-abs
    (fp32 helper - fp64 helper), Lmax the scene's longest list, scale 1 for alpha, the largest colour (background included) for rgb, the
    largest depth for the accumulated depth.  Expected depth ED = D / alpha is compared where fp64 alpha > 1e-3 with the two analytic
    terms carried through the division: (tol_D + |ED| tol_alpha) / alpha per pixel.
    -> dict: e32 {rgb, depth, alpha}, tol {rgb, alpha, D} (floats), and depth_tol: [C,H,W,1] array (per-pixel bound of the depth output),
    depth_mask"""
    inp = scene(name)[0]
    (r64, d64, a64), _ = reference(name, mode, torch.float64)
    (r32, d32, a32), _ = reference(name, mode, torch.float32)
    lmax = int(list_lengths(name).max())
    unit = 16 * EPS32 * (lmax + 1)
    cmax = float(inp["colors"].max())
    if mode == "bg_D":
        cmax = max(cmax, float(backgrounds(len(inp["viewmats"])).max()))
    zmax = float(projected(name)["depths"][(projected(name)["radii"] > 0).all(-1)].max())
    e32 = {"rgb": float(np.abs(r32 - r64).max()), "alpha": float(np.abs(a32 - a64).max())}
    tol = {"rgb": max(4 * e32["rgb"], unit * cmax), "alpha": max(4 * e32["alpha"], unit)}
    if MODES[mode]["depth_mode"] == "D":
        mask = np.ones(a64.shape, bool)
        e32["depth"] = float(np.abs(d32 - d64).max())
        depth_tol = np.full(a64.shape, max(4 * e32["depth"], unit * zmax))
    else:
        mask = a64 > 1e-3
        e32["depth"] = float(np.abs(d32 - d64)[mask].max()) if mask.any() else 0.0
        depth_tol = np.maximum(4 * e32["depth"], (unit * zmax + np.abs(d64) * unit) / np.maximum(a64, 1e-3))
    return dict(e32=e32, tol=tol, depth_tol=depth_tol, depth_mask=mask, lmax=lmax)
