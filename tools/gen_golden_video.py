"""Writes tests/golden/video_*.npz by running the REFERENCE's own fly-through code on the CPU.  Data only; nothing of it is copied.

    python tools/gen_golden_video.py <reference root>

* ``src.utils.gs_effects.GSEffects`` imports directly and is run in fp64.
* ``src.utils.render_utils.render_interpolated_video`` is run whole.  What its imports need and this machine need not have is replaced in
  sys.modules by stand-ins: ``moviepy.editor`` (an ImageSequenceClip that records the frames it is given), ``src.utils.color_map``
  (apply_color_map_to_image through ``matplotlib.colormaps``: the reference's ``cm.get_cmap`` left matplotlib in 3.9), ``tqdm`` (identity)
  and ``src.models.models.rasterization`` (imported for a type annotation; it needs gsplat).  ``gs_renderer`` is a recording stand-in: its
  ``rasterizer.rasterize_batches`` keeps the cameras it is called with and returns deterministic images; it has no ``prune_gs`` and no
  ``runner``, which sends the reference down its plain-splat branches (render_utils.py:208-209, :248-254, :299-305).

Files:
  video_turbo.npz     lut [256,3] u8: matplotlib's turbo rows through float32, clamp(0, 1) * 255 -> uint8 (the chain of color_map.py:18-21
                      and render_utils.py:355-357)
  video_traj.npz      c2w [2,6,4,4], K [2,6,3,3] (fp32-valued; the rotations take all four branches of rotation_matrix_to_quaternion, one
                      pair is nearly parallel (the linear branch of slerp) and one has a negative dot product), n = 4; ext32 / int32: the
                      cameras the renderer saw from an fp32 run; ext64r / int64r: from an fp64 run, rounded to fp32 by the reference's own
                      cast in front of the rasteriser; wob_c2w / wob_K / wob_means / wob_ext / wob_int: the single-camera path
  video_effect.npz    a 300-Gaussian scene (video_helper.effect_scene) and apply_effect's fp64 outputs at the t_n and ignore_scale cases
  video_frames.npz    3 views, n = 4, 24 x 32, no effects: the rendered depth / rgb the stand-in returned and the uint8 videos the reference
                      handed to moviepy (split mode, loop_reverse)
  video_fx_a.npz, video_fx_b.npz   3 views, n = 4 (a) and 14 (b), with effects: the scene, random_vals, the cameras of every call, the t of every
                      apply_effect call, the index of the first kept intro frame and the number of video frames.  a: an isotropic cloud;
                      b: a cloud that is flat in x z, which dissolves within the main loop and exercises t_ed / loop_dir."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
VIDEOS = {}


def install_stand_ins():
    import matplotlib

    class ImageSequenceClip:
        def __init__(self, frames, fps=30):
            self.frames, self.fps = np.stack(frames), fps

        def write_videofile(self, path, logger=None):
            VIDEOS[os.path.basename(path)] = self.frames

    editor = types.ModuleType("moviepy.editor")
    editor.ImageSequenceClip = ImageSequenceClip
    moviepy = types.ModuleType("moviepy")
    moviepy.editor = editor
    sys.modules["moviepy"], sys.modules["moviepy.editor"] = moviepy, editor

    def apply_color_map_to_image(image, color_map="inferno"):
        mapped = matplotlib.colormaps[color_map](image.detach().clip(min=0, max=1).cpu().numpy())[..., :3]
        return torch.tensor(mapped, device=image.device, dtype=torch.float32).movedim(-1, -3)

    cmap = types.ModuleType("src.utils.color_map")
    cmap.apply_color_map_to_image = apply_color_map_to_image
    sys.modules["src.utils.color_map"] = cmap
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = tq
    rz = types.ModuleType("src.models.models.rasterization")
    rz.GaussianSplatRenderer = object
    sys.modules["src.models.models.rasterization"] = rz


def stand_in_images(ext, K, h, w):
    """deterministic images of a camera: depth 0.5 .. 4.5 from a hash of the pixel and the camera's translation, 5 % holes"""
    C = ext.shape[0]
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out_c, out_d = [], []
    for c in range(C):
        ph = float(ext[c, :3, 3].abs().sum()) + float(K[c, 0, 0]) * 1e-3
        u = torch.frac(torch.sin(xx * 12.9898 + yy * 78.233 + ph * 3.7) * 43758.5453).abs()
        v = torch.frac(torch.sin(xx * 39.346 + yy * 11.135 + ph * 1.3) * 24634.6345).abs()
        d = 0.5 + 4.0 * u
        d[v < 0.05] = 0.0
        out_d.append(d[..., None])
        out_c.append(torch.stack([u * 1.2 - 0.1, v, 1.0 - u], -1))
    return torch.stack(out_c)[None], torch.stack(out_d)[None]


class Recorder:
    sh_degree, voxel_size = 0, 0.002

    def __init__(self):
        self.rasterizer = self
        self.ext, self.int, self.rgb, self.depth = [], [], [], []

    def rasterize_batches(self, means, quats, scales, opacities, colors, viewmats, Ks, width, height, sh_degree=None):
        assert viewmats.dtype == torch.float32 and viewmats.shape[0] == 1
        self.ext.append(viewmats[0].clone())
        self.int.append(Ks[0].clone())
        c, d = stand_in_images(viewmats[0], Ks[0], height, width)
        self.rgb.append(c[0])
        self.depth.append(d[0])
        return c, d, None


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def cameras(rots, seed, batch=1):
    g = np.random.default_rng(seed)
    S = len(rots)
    c2w = np.tile(np.eye(4), (batch, S, 1, 1))
    K = np.zeros((batch, S, 3, 3))
    for b in range(batch):
        for i, (ax, an) in enumerate(rots):
            c2w[b, i, :3, :3] = rotation(ax, an + 0.05 * b)
            c2w[b, i, :3, 3] = g.uniform(-1, 1, 3)
            f = g.uniform(20, 40)
            K[b, i] = [[f, 0, 16 + g.uniform(-1, 1)], [0, f * 1.1, 12 + g.uniform(-1, 1)], [0, 0, 1]]
    return c2w.astype(np.float32), K.astype(np.float32)


def splat_scene(N, seed, spread):
    g = np.random.default_rng(seed)
    means = (g.standard_normal((N, 3)) * np.asarray(spread) + np.array([0.3, -0.2, 0.5])).astype(np.float32)
    quats = g.standard_normal((N, 4)).astype(np.float32)
    return {"means": means[None], "quats": quats[None], "scales": g.uniform(0.01, 0.05, (1, N, 3)).astype(np.float32),
            "opacities": g.uniform(0.2, 1.0, (1, N)).astype(np.float32), "sh": g.uniform(-1.5, 1.5, (1, N, 1, 3)).astype(np.float32)}


def main(ref_root):
    import matplotlib
    import video_helper as VH
    sys.path.insert(0, ref_root)
    install_stand_ins()
    RU = importlib.import_module("src.utils.render_utils")
    RefEffects = importlib.import_module("src.utils.gs_effects").GSEffects
    T = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}

    lut = matplotlib.colormaps["turbo"](np.arange(256))[:, :3]
    lut8 = (torch.tensor(lut, dtype=torch.float32).clamp(0, 1) * 255).to(torch.uint8).numpy()
    np.savez_compressed(os.path.join(GOLD, "video_turbo.npz"), lut=lut8)

    # ---- trajectories
    rots = [((0, 1, 0), 0.2), ((1, 0, 0), 3.0), ((0, 1, 0), 3.0), ((0, 0, 1), 3.1), ((0, 0, 1), 3.1004), ((1, 1, 0), -2.5)]
    c2w, K = cameras(rots, 11, batch=2)
    dummy = T(splat_scene(8, 1, (1, 1, 1)))
    out = {"c2w": c2w, "K": K, "n": np.int64(4)}
    for tag, dt in (("32", torch.float32), ("64r", torch.float64)):
        rec = Recorder()
        RU.render_interpolated_video(rec, dummy, torch.from_numpy(c2w).to(dt), torch.from_numpy(K).to(dt), (4, 4), "/tmp/x", interp_per_pair=4)
        out["ext" + tag], out["int" + tag] = torch.cat(rec.ext).numpy(), torch.cat(rec.int).numpy()
    assert sorted(set(VH.quat_branch(torch.from_numpy(c2w[0, :, :3, :3])))) == [1, 2, 3, 4]
    wc2w, wK = cameras([((1, 2, 3), 0.7)], 12)
    wsplats = T(splat_scene(50, 2, (1, 1, 1)))
    rec = Recorder()
    RU.render_interpolated_video(rec, wsplats, torch.from_numpy(wc2w), torch.from_numpy(wK), (4, 4), "/tmp/x", interp_per_pair=2)
    out.update(wob_c2w=wc2w, wob_K=wK, wob_means=wsplats["means"].numpy(), wob_ext=torch.cat(rec.ext).numpy(), wob_int=torch.cat(rec.int).numpy())
    np.savez_compressed(os.path.join(GOLD, "video_traj.npz"), **out)

    # ---- apply_effect in fp64
    sc = VH.effect_scene(300, 20261020)
    out = dict(sc)
    for ti, t_n in enumerate(VH.T_CASES):
        for ig in (0, 1):
            fx = RefEffects(start_time=0.5, end_time=10.0)
            fx.random_vals = torch.from_numpy(sc["random_vals"]).double()
            g = {k: torch.from_numpy(sc[k]).double() for k in ("means", "scales", "opacities", "colors", "quats")}
            res, flag = fx.apply_effect(g, t_n + 0.5, effect_type=2, ignore_scale=bool(ig))
            for k in ("means", "scales", "opacities", "colors"):
                out[f"t{ti}_i{ig}_{k}"] = res[k].numpy()
            out[f"t{ti}_i{ig}_flag"] = flag.numpy()
    np.savez_compressed(os.path.join(GOLD, "video_effect.npz"), **out)

    # ---- frames, no effects
    c3, K3 = cameras([((0, 1, 0), 0.1), ((0, 1, 0), 0.5), ((1, 1, 0), 0.9)], 13)
    scene = splat_scene(300, 3, (1.0, 0.6, 1.0))
    rec = Recorder()
    VIDEOS.clear()
    RU.render_interpolated_video(rec, T(scene), torch.from_numpy(c3), torch.from_numpy(K3), (24, 32), "/tmp/gold", interp_per_pair=4)
    np.savez_compressed(os.path.join(GOLD, "video_frames.npz"), c2w=c3, K=K3, ext=torch.cat(rec.ext).numpy(), int=torch.cat(rec.int).numpy(),
                        rgb=torch.cat(rec.rgb).numpy(), depth=torch.cat(rec.depth).numpy()[..., 0], video_rgb=VIDEOS["gold_rgb.mp4"],
                        video_depth=VIDEOS["gold_depth.mp4"])

    # ---- the schedule with effects
    for name, spread, seed, n in (("fx_a", (1.0, 0.6, 1.0), 4, 4), ("fx_b", (0.02, 1.0, 0.02), 5, 14)):
        scene = splat_scene(300, seed, spread)
        rv = np.random.default_rng(seed + 100).uniform(0, 1, 300).astype(np.float32)
        ts, means_seen = [], []

        class Rec(RefEffects):
            def apply_effect(self, gsplat, t, effect_type, ignore_scale=False):
                ts.append((t, float(ignore_scale)))
                res, flag = super().apply_effect(gsplat, t, effect_type, ignore_scale=ignore_scale)
                means_seen.append((float((flag < 0.99).any()), float(flag.double().mean())))
                return res, flag

        fx = Rec(start_time=0.0, end_time=10.0)
        fx.random_vals = torch.from_numpy(rv)
        rec = Recorder()
        VIDEOS.clear()
        RU.render_interpolated_video(rec, T(scene), torch.from_numpy(c3), torch.from_numpy(K3), (12, 16), "/tmp/gold", interp_per_pair=n, effects=fx)
        n_video = VIDEOS["gold_rgb.mp4"].shape[0]
        st = np.array(means_seen)
        assert np.abs(st[:, 1] - 0.01).min() > 1e-4, "flag.mean() too close to the 0.01 threshold: choose another seed"
        np.savez_compressed(os.path.join(GOLD, f"video_{name}.npz"), c2w=c3, K=K3, random_vals=rv, ext=torch.cat(rec.ext).numpy(),
                            int=torch.cat(rec.int).numpy(), t=np.array(ts, np.float64), stats=st, n_video=np.int64(n_video), n=np.int64(n),
                            **{"splat_" + k: v for k, v in scene.items()})
        print(name, "calls", len(ts), "video frames", n_video, "t range", ts[0][0], max(t for t, _ in ts), "final t", ts[-1][0])
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("video_"):
            print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main(sys.argv[1])
