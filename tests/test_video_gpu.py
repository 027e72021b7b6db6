"""GPU: the fly-through video kernels (csrc/video.hip) and the driver (hunyuanworld_mirror_amd.video) against the fp64 restatement
tests/video_helper.py, which tests/test_video_cpu.py pins to the reference's recorded results.

Effect outputs follow the convention of test_bilagrid_gpu.py: the yardstick of a quantity is the restatement's own fp32-against-fp64 error
on the same inputs (largest element error over the largest element, never less than one fp32 ulp); the kernel may exceed it by FACTOR = 4.
A Gaussian is left out only where one of the two switches is numerically undecided in fp64 (|at - (t_n - 3.1416)| or
|random_vals - 0.8 flag| below 1e-5): at most 1 % per case, and the fp64 values alone are asserted to stay inside that cap first.

Depth bytes.  x = 1 - (ln max(d, 1e-9) - near) / (far - near + 1e-9) is evaluated in fp32 by kernel and reference alike; the test takes the
fp64 value x64 from the same fp32 near / far and allows the table row of floor(256 (x64 +- eps)).  eps, with u = 2^-24, L = ln max(d, 1e-9),
M = max(|L|, |near|, |far|), den = far - near + 1e-9, q = (L - near) / den = 1 - x64:
  logf is within 1 ulp: 2 u |L|; near and far are themselves within 2 ulp of the values x64 uses: 4 u |near|, 4 u |far|;
  num = fl(L - near): u |num| <= 2 u M, so the numerator is off by at most 8 u M;
  den = fl(fl(far - near) + 1e-9): 2 u |den| + 4 u (|far| + |near|) <= 2 u |den| + 8 u M, which moves q by |q| (2 u + 8 u M / |den|);
  the division u |q| and the final subtraction u max(1, |x|).
  eps = u ((8 M / |den|) (1 + |q|) + 3 |q| + 1 + |x64|)      (only |q| <= 2 matters: beyond it both ends clip to the same row).
With a log range of about 2.2 that is a band of order 1e-3 of the pixels; pixels that pass only through a neighbouring row are capped at
1 % per frame, and the inputs are asserted to keep the fp64 values inside that cap.  Degenerate frames (den = -inf or 1e-9) have exact
expectations instead."""
import functools

import numpy as np
import pytest
import torch

import video_helper as VH

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- effect
SHIFT, INV_SCALE = (0.3, -0.2, 0.1), 0.7


@functools.lru_cache(maxsize=None)
def _effect_case(N, xform):
    """inputs of one scene (as the kernel takes them) and, per (t_n, ignore_scale), the fp64 reference and the fp32 yardstick run"""
    sc = VH.effect_scene(N, 7000 + N)
    inp = {k: sc[k].copy() for k in ("means", "scales", "opacities", "colors", "random_vals", "quats")}
    kw = {}
    if xform:
        k32 = np.float32(INV_SCALE)
        inp["means"] = (sc["means"] / k32 + np.float32(SHIFT)).astype(np.float32)
        inp["means"][0] = np.float32(SHIFT)                              # lands on the origin exactly
        if N > 1:
            inp["means"][1] = np.float32(SHIFT) + np.float32([0, 0.8, 0])   # on the y axis exactly
        inp["scales"] = (sc["scales"] / k32).astype(np.float32)
        inp["colors"] = ((sc["colors"] - 0.5) / VH.SH_C0).astype(np.float32)
        kw = dict(shift=np.float32(SHIFT), inv_scale=INV_SCALE, sh=True)
    runs = {}
    for t_n in VH.T_CASES:
        for ig in (False, True):
            args = (inp["means"], inp["scales"], inp["opacities"], inp["colors"], inp["random_vals"], t_n, ig)
            runs[(t_n, ig)] = (VH.spread_effect(*args, torch.float64, **kw), VH.spread_effect(*args, torch.float32, **kw))
    return inp, kw, runs


@pytest.mark.parametrize("xform", [False, True], ids=["plain", "shift-scale-sh"])
@pytest.mark.parametrize("N", [255, 256, 257, 1000])
def test_gpu_spread_effect_matches_the_fp64_restatement(N, xform):
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    inp, kw, runs = _effect_case(N, xform)
    g = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    fails = []
    for (t_n, ig), (ref, f32) in runs.items():
        und = VH.undecided(ref, ig)
        assert und.mean() <= 0.01, ("the reference values alone leave the cap", N, t_n, ig, und.mean())
        fx = wm.GSEffects(start_time=0.25, end_time=10.0, random_vals=g["random_vals"])
        if xform:
            out, flag = fx.apply_splats(g["means"], g["scales"], g["opacities"], g["colors"], t_n + 0.25, ignore_scale=ig,
                                        shift=torch.tensor(SHIFT, device=dev), inv_scale=INV_SCALE, colors_are_sh0=True)
        else:
            out, flag = fx.apply_effect(g, t_n + 0.25, effect_type=2, ignore_scale=ig)
            assert set(out) == {"means", "quats", "scales", "opacities", "colors"} and torch.equal(out["quats"], g["quats"])
        stats = fx.last_stats.cpu().numpy()
        out["flag"] = flag
        keep = ~und
        for k in ("means", "scales", "opacities", "colors", "flag"):
            got = out[k].cpu().numpy()
            assert got.dtype == np.float32 and got.shape == tuple(ref[k].shape)
            r64, r32 = ref[k].numpy()[keep], f32[k].numpy()[keep]
            yard = max(VH.max_rel(r32, r64), VH.ULP)
            err = VH.max_rel(got[keep], r64)
            print(f"N={N} t_n={t_n} ignore_scale={ig} {k}: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.2f} left out {int(und.sum())}")
            if not err <= VH.FACTOR * yard:
                fails.append((t_n, ig, k, yard, err))
        # the two statistics: the count is exact away from the band, the sum is within N 2^-23 of the fp64 sum
        f64 = ref["flag"].numpy()
        lo, hi = int((f64 < 0.99 - VH.BAND).sum()), int((f64 < 0.99 + VH.BAND).sum())
        assert lo <= stats[0] <= hi and stats[0] == float((flag < 0.99).sum()), (t_n, ig, stats, lo, hi)
        assert abs(stats[1] - f64.sum()) <= N * 2.0 ** -23, (t_n, ig, stats[1], f64.sum())
        assert abs(stats[1] - float(flag.double().sum())) <= N * 2.0 ** -50
    assert not fails, fails


def test_gpu_spread_effect_is_reproducible_and_draws_once():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    inp, _, _ = _effect_case(1000, False)
    g = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k != "random_vals"}
    fx = wm.GSEffects()
    a, fa = fx.apply_effect(g, 5.0, effect_type=2)
    rv = fx.random_vals
    sa = fx.last_stats.clone()
    b, fb = fx.apply_effect(g, 5.0, effect_type=2)
    assert fx.random_vals is rv and rv.shape == (1000,) and rv.device.type == "cuda"
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(fa, fb) and torch.equal(sa, fx.last_stats)


# ---------------------------------------------------------------------------------------------- depth and rgb frames
def _regular(F, H, W, seed):
    g = np.random.default_rng(seed)
    d = g.uniform(0.5, 4.5, (F, H, W)).astype(np.float32)
    d[g.uniform(0, 1, (F, H, W)) < 0.05] = 0.0
    return d


def _degenerate(H, W, seed):
    """all zero | 0.99-quantile zero with a few valid pixels | constant 1.0 | constant 2.5 with holes | a single valid pixel"""
    g = np.random.default_rng(seed)
    n = H * W
    d = np.zeros((5, n), np.float32)
    few = max(1, n // 200)
    d[1, g.permutation(n)[:few]] = g.uniform(0.5, 4.5, few).astype(np.float32)
    d[2] = 1.0
    d[3] = 2.5
    d[3, g.permutation(n)[:n // 20]] = 0.0
    d[4, g.integers(n)] = 3.25
    return d.reshape(5, H, W)


def _near_far_cpu(d):
    out = np.zeros((d.shape[0], 2), np.float32)
    for f in range(d.shape[0]):
        _, near, far = VH.depth_vis_x(d[f], torch.float32)
        out[f] = float(near), float(far)
    return out


def _within_ulps(got, ref, k):
    fin = np.isfinite(ref)
    ok = np.array_equal(got[~fin], ref[~fin])
    return ok and bool((np.abs(got[fin].astype(np.float64) - ref[fin]) <= k * np.spacing(np.abs(ref[fin]))).all())


def _check_regular(d, bytes_, near_far, lut):
    ref_nf = _near_far_cpu(d)
    assert _within_ulps(near_far, ref_nf, 2), (near_far, ref_nf)
    for f in range(d.shape[0]):
        x64, near, far = VH.depth_vis_x(d[f], torch.float64)
        x64, near, far = x64.numpy(), float(near), float(far)
        L = np.log(np.maximum(d[f].astype(np.float64), 1e-9))
        den = far - near + 1e-9
        q = np.minimum(np.abs(1.0 - x64), 2.0)
        M = np.maximum(np.abs(L), max(abs(near), abs(far)))
        eps = U * ((8 * M / abs(den)) * (1 + q) + 3 * q + 1 + np.minimum(np.abs(x64), 2.0))
        k_mid, k_lo, k_hi = VH.turbo_rows(x64), VH.turbo_rows(x64 - eps), VH.turbo_rows(x64 + eps)
        band = (k_lo != k_hi).mean()
        assert band <= 0.01, ("the fp64 values alone leave the cap", f, band)
        got = bytes_[f]
        ok = (got == lut[k_lo]).all(-1) | (got == lut[k_hi]).all(-1) | (got == lut[k_mid]).all(-1)
        neighbour = ok & ~(got == lut[k_mid]).all(-1)
        print(f"frame {f}: eps max {eps.max():.2e}, undecided band {band:.2e}, through a neighbouring row {neighbour.mean():.2e}")
        assert ok.all(), (f, int((~ok).sum()))
        assert neighbour.mean() <= 0.01


@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 64, 48), (2, 518, 518)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_depth_frames_regular(shape):
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import video
    F, H, W = shape
    d = _regular(F, H, W, 100 + H)
    if H * W > 2 ** 17:     # here the fp32 rank q (n - 1) is not the fp64 product
        assert float(np.float32(0.99) * np.float32(H * W - 1)) != float(np.float32(0.99)) * (H * W - 1)
    out, nf = wm.depth_frames(torch.from_numpy(d).to(_dev()))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (F, H, W, 3) and nf.dtype == torch.float32 and tuple(nf.shape) == (F, 2)
    _check_regular(d, out.cpu().numpy(), nf.cpu().numpy(), video.turbo_lut().numpy())
    out2, nf2 = wm.depth_frames(torch.from_numpy(d).to(_dev())[..., None])      # the rasteriser's [F,H,W,1]
    assert torch.equal(out, out2) and torch.equal(nf, nf2)


@pytest.mark.parametrize("hw", [(37, 53), (64, 48)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_depth_frames_degenerate(hw):
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import video
    lut = video.turbo_lut().numpy()
    d = _degenerate(*hw, 5)
    out, nf = wm.depth_frames(torch.from_numpy(d).to(_dev()))
    out, nf = out.cpu().numpy(), nf.cpu().numpy()
    ref = _near_far_cpu(d)
    print(nf, ref)
    assert _within_ulps(nf, ref, 2)
    assert nf[0, 0] == 0.0 and np.isneginf(nf[0, 1])            # all zero: near is the plain number 0.0, far = log 0
    assert np.isfinite(nf[1, 0]) and np.isneginf(nf[1, 1])      # a 0.99-quantile of zero
    assert nf[2, 0] == 0.0 and nf[2, 1] == 0.0                  # constant 1.0
    assert nf[3, 0] == nf[3, 1] == ref[3, 0]                    # constant 2.5: far = near
    assert abs(nf[4, 0] - np.log(3.25)) < 1e-6 and np.isneginf(nf[4, 1])
    for f in (0, 1, 2, 4):                                       # x = 1 everywhere
        assert (out[f] == lut[255]).all(), f
    # constant depth with holes: the denominator is 1e-9; the holes saturate at x = 1, the constant pixels all take ONE of the two ends
    # (log d - near is zero or one ulp, on either side)
    holes = d[3] == 0
    assert (out[3][holes] == lut[255]).all()
    rows = np.unique(out[3][~holes].reshape(-1, 3), axis=0)
    assert len(rows) == 1 and ((rows[0] == lut[255]).all() or (rows[0] == lut[0]).all())


def test_gpu_depth_frames_one_pixel():
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import video
    lut = video.turbo_lut().numpy()
    d = np.float32([2.0, 0.0, 0.7]).reshape(3, 1, 1)
    out, nf = wm.depth_frames(torch.from_numpy(d).to(_dev()))
    out, nf = out.cpu().numpy(), nf.cpu().numpy()
    assert _within_ulps(nf, _near_far_cpu(d), 2)
    assert nf[1, 0] == 0.0 and np.isneginf(nf[1, 1]) and (out[1] == lut[255]).all()
    for f in (0, 2):       # a single valid pixel: far = near, one of the saturated ends
        assert nf[f, 0] == nf[f, 1] and ((out[f] == lut[255]).all() or (out[f] == lut[0]).all())


@pytest.mark.parametrize("shape", [(3, 37, 53), (1, 1, 1), (2, 64, 48)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_rgb_frames_are_torchs_bytes(shape):
    import hunyuanworld_mirror_amd as wm
    F, H, W = shape
    g = torch.Generator().manual_seed(H)
    x = torch.rand((F, H, W, 3), generator=g) * 2 - 0.5
    special = torch.tensor([0.0, 1.0, 254.5 / 255, -0.0, 1.0 - 2.0 ** -24, 2.0 ** -9])
    x.view(-1)[:min(6, x.numel())] = special[:min(6, x.numel())]
    x = x.to(_dev())
    got = wm.rgb_frames(x)
    assert got.dtype == torch.uint8 and torch.equal(got, (x.clamp(0, 1) * 255).to(torch.uint8))
    m = (x.numel() - 1) // 3
    if m:                                                           # an unaligned view takes the byte path
        tail = x.view(-1)[1:1 + 3 * m]
        assert torch.equal(wm.rgb_frames(tail.view(1, 1, m, 3)).view(-1), (tail.clamp(0, 1) * 255).to(torch.uint8))


# ---------------------------------------------------------------------------------------------- driver
def _images(ext, K, h, w):
    """deterministic images of the cameras [C,4,4] on their device: depth 0.5 .. 4.5 with holes"""
    dev = ext.device
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
    ph = (ext[:, :3, 3].abs().sum(-1) + K[:, 0, 0] * 1e-3)[:, None, None]
    u = torch.frac(torch.sin(xx * 12.9898 + yy * 78.233 + ph * 3.7) * 43758.5453).abs()
    v = torch.frac(torch.sin(xx * 39.346 + yy * 11.135 + ph * 1.3) * 24634.6345).abs()
    d = torch.where(v < 0.05, torch.zeros_like(u), 0.5 + 4.0 * u)
    return torch.stack([u * 1.2 - 0.1, v, 1.0 - u], -1)[None], d[None, ..., None]


class _Recorder:
    sh_degree, voxel_size = 0, 0.002

    def __init__(self):
        self.rasterizer = self
        self.ext, self.int, self.n_splats = [], [], []

    def rasterize_batches(self, means, quats, scales, opacities, colors, viewmats, Ks, width, height, sh_degree=None):
        assert viewmats.dtype == torch.float32 and viewmats.shape[0] == 1 and len(means) == 1
        self.ext.append(viewmats[0].cpu())
        self.int.append(Ks[0].cpu())
        self.n_splats.append((tuple(means.shape), tuple(colors.shape), sh_degree))
        c, d = _images(viewmats[0], Ks[0], height, width)
        return c, d, None


def _path_yardstick(z, n, shift=None, sf=None):
    """the restatement's cameras in fp64 and the fp32-against-fp64 yardstick, optionally normalised as render_utils.py:218"""
    e = {}
    for dt in (torch.float32, torch.float64):
        ext, ints = VH.interpolated_traj(z["c2w"], z["K"], n, dt)
        ext = ext.clone()
        if shift is not None:
            ext[0, :, :3, -1] = (ext[0, :, :3, -1] - shift.to(dt)) / sf.to(dt)
        e[dt] = (ext[0].numpy(), ints[0].numpy())
    yard = [max(VH.max_rel(e[torch.float32][i], e[torch.float64][i]), VH.ULP) for i in (0, 1)]
    return e[torch.float64], yard


def test_gpu_driver_without_effects_follows_the_reference():
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    z = VH.load_golden("frames")
    rec = _Recorder()
    N = 32
    splats = {"means": torch.zeros(1, N, 3, device=dev), "quats": torch.ones(1, N, 4, device=dev), "scales": torch.ones(1, N, 3, device=dev),
              "opacities": torch.ones(1, N, device=dev), "sh": torch.zeros(1, N, 1, 3, device=dev)}
    out = wm.render_interpolated_frames(rec, splats, torch.from_numpy(z["c2w"]).to(dev), torch.from_numpy(z["K"]).to(dev), (24, 32), interp_per_pair=4)
    ext, ints = torch.cat(rec.ext).numpy(), torch.cat(rec.int).numpy()
    assert len(rec.ext) == 1 and ext.shape == z["ext"].shape          # 10 views: one chunk of at most 40
    (e64, i64), yard = _path_yardstick(z, 4)
    for got, ref, gold, y in ((ext, e64, z["ext"], yard[0]), (ints, i64, z["int"], yard[1])):
        print("cameras: yardstick", y, "gpu", VH.max_rel(got, ref), "against the record", VH.max_rel(got, gold))
        assert VH.max_rel(got, ref) <= VH.FACTOR * y and VH.max_rel(got, gold) <= 2 * VH.FACTOR * y
    assert set(out) == {"rgb", "depth"} and out["rgb"].shape == z["video_rgb"].shape and out["depth"].shape == z["video_depth"].shape
    assert out["rgb"].dtype == torch.uint8 and out["depth"].dtype == torch.uint8
    F = ext.shape[0]
    for k in ("rgb", "depth"):                                       # video + video[::-1][1:-1]
        v = out[k]
        assert v.shape[0] == 2 * F - 2 and torch.equal(v[F:], v[:F].flip(0)[1:-1])
    both = wm.render_interpolated_frames(_Recorder(), splats, torch.from_numpy(z["c2w"]).to(dev), torch.from_numpy(z["K"]).to(dev), (24, 32),
                                         interp_per_pair=4, loop_reverse=False, save_mode="both")
    assert set(both) == {"both"} and torch.equal(both["both"], torch.cat([out["rgb"][:F], out["depth"][:F]], dim=1))


@pytest.mark.parametrize("name", ["fx_a", "fx_b"])
def test_gpu_driver_with_effects_follows_the_reference_schedule(name):
    import hunyuanworld_mirror_amd as wm
    dev = _dev()
    z = VH.load_golden(name)
    sched, seen, shift, sf = VH.golden_schedule(z)
    # our fp64 sum cannot legitimately flip the schedule against the reference's fp32 mean
    assert np.abs(seen - 0.01).min() > 1e-4 and np.abs(z["stats"][:, 1] - 0.01).min() > 1e-4
    ts = []

    class Rec(wm.GSEffects):
        def apply_splats(self, *a, **k):
            ts.append((float(a[4]), float(k.get("ignore_scale", False))))
            return super().apply_splats(*a, **k)

    fx = Rec(0.0, 10.0, random_vals=torch.from_numpy(z["random_vals"]).to(dev))
    rec = _Recorder()
    splats = {k[6:]: torch.from_numpy(v).to(dev) for k, v in z.items() if k.startswith("splat_")}
    n = int(z["n"])
    out = wm.render_interpolated_frames(rec, splats, torch.from_numpy(z["c2w"]).to(dev), torch.from_numpy(z["K"]).to(dev), (12, 16), interp_per_pair=n,
                                        effects=fx)
    assert [t for t, _ in ts] == list(z["t"][:, 0]) and [i for _, i in ts] == list(z["t"][:, 1])
    assert len(rec.ext) == z["ext"].shape[0] and out["rgb"].shape[0] == int(z["n_video"]) == out["depth"].shape[0]
    N = splats["means"].shape[1]
    assert all(s == ((1, N, 3), (1, N, 1, 3), 0) for s in rec.n_splats)
    ext, ints = torch.cat(rec.ext).numpy(), torch.cat(rec.int).numpy()
    (e64, i64), yard = _path_yardstick(z, n, shift, sf)
    views = [s[1] for s in sched]
    for got, ref, gold, y in ((ext, e64[views], z["ext"], yard[0]), (ints, i64[views], z["int"], yard[1])):
        print("cameras: yardstick", y, "gpu", VH.max_rel(got, ref), "against the record", VH.max_rel(got, gold))
        assert VH.max_rel(got, ref) <= VH.FACTOR * y and VH.max_rel(got, gold) <= 2 * VH.FACTOR * y


def test_gpu_end_to_end_through_the_rasteriser():
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd.worldmirror import _GSRenderer
    dev = _dev()
    z = VH.load_golden("fx_a")
    splats = {k[6:]: torch.from_numpy(v).to(dev) for k, v in z.items() if k.startswith("splat_")}
    splats["means"] = splats["means"] * 0.3 + torch.tensor([0.0, 0.0, 3.0], device=dev)
    splats["weights"] = torch.ones_like(splats["opacities"])
    c2w = torch.eye(4, device=dev).repeat(1, 3, 1, 1)
    c2w[0, :, 0, 3] = torch.tensor([-0.2, 0.0, 0.2], device=dev)
    K = torch.tensor([[60.0, 0, 32], [0, 60.0, 24], [0, 0, 1]], device=dev).repeat(1, 3, 1, 1)
    r = _GSRenderer()
    out = wm.render_interpolated_frames(r, splats, c2w, K, (48, 64), interp_per_pair=4)
    assert out["rgb"].shape == (18, 48, 64, 3) == out["depth"].shape and out["rgb"].dtype == torch.uint8 and out["rgb"].device.type == "cuda"
    assert int(out["rgb"].max()) > 0 and len(torch.unique(out["depth"].reshape(-1, 3), dim=0)) > 4      # something was rendered
    got = {}
    wm.render_interpolated_video(r, splats, c2w, K, (48, 64), "/nowhere/clip", interp_per_pair=4,
                                 writer=lambda frames, path, fps=30: got.__setitem__(path, (frames, fps)))
    assert set(got) == {"/nowhere/clip_rgb.mp4", "/nowhere/clip_depth.mp4"}
    for k in ("rgb", "depth"):
        frames, fps = got[f"/nowhere/clip_{k}.mp4"]
        assert fps == 30 and isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and np.array_equal(frames, out[k].cpu().numpy())
    wm.render_interpolated_video(r, splats, c2w, K, (48, 64), "/nowhere/clip", interp_per_pair=4, save_mode="both", loop_reverse=False,
                                 writer=lambda frames, path, fps=30: got.__setitem__(path, (frames, fps)))
    assert got["/nowhere/clip.mp4"][0].shape == (10, 96, 64, 3)
    fx = wm.render_interpolated_frames(r, splats, c2w, K, (48, 64), interp_per_pair=4, effects=wm.GSEffects())
    assert fx["rgb"].shape[1:] == (48, 64, 3) and fx["rgb"].shape[0] > 18 and fx["rgb"].shape == fx["depth"].shape
