"""Times the fly-through video's two kernels paths against the reference's compositions on the same device (profiles/r19_video_frames.md).

    python tools/bench_video_frames.py [--frames 112] [--size 518] [--gaussians 1048576] [--repeats 7]

Frame packing: F rendered frames (rgb [F,H,W,3], depth [F,H,W] with 5 % holes, on the device) -> uint8 frames.
  ours      hunyuanworld_mirror_amd.video: one wm_video_frames call; timed to the device tensors (ten calls in a row, per call) and,
            separately, to host numpy arrays (one call and the two copies)
  baseline  the reference's depth_vis + _make_video composition (src/utils/render_utils.py:326-359) on the same tensors: per frame a boolean
            gather, two torch.quantile (two sorts), the colour map on the host through matplotlib (device -> host -> device), then the stack,
            clamp, * 255, uint8 and the copy to the host.  This is the measuring stick; it ends in host numpy arrays, as the encoder needs.
Effect: one apply_effect over N Gaussians at t = 5.
  ours      GSEffects.apply_effect (one kernel + the 2-value reduction)
  baseline  tests/video_helper.spread_effect in fp32 on the device: the reference's torch operations WITHOUT its zero-weighted 8-corner
            hash noise (about half of its launches), so a lower bound of the reference's time.
Each side is warmed up once and then timed `repeats` times, the two sides alternating; a host clock around work that ends in a device
synchronise.  Prints one JSON line per measurement with median / min / max in milliseconds, and how many depth bytes differ."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def alternate(sides, repeats, dev):
    """sides: {name: fn}; one warm-up each, then `repeats` rounds in turn -> {name: [ms]}, {name: last result}"""
    res, last = {k: [] for k in sides}, {}
    for k, fn in sides.items():
        timed(fn, dev)
    for _ in range(repeats):
        for k, fn in sides.items():
            ms, last[k] = timed(fn, dev)
            res[k].append(ms)
    return res, last


def report(tag, ms, **extra):
    print(json.dumps({"measurement": tag, "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                      "repeats": len(ms), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=112)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--gaussians", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_frames needs the GPU: there is no CPU path to time")
    import matplotlib
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import video
    import video_helper as VH
    dev = torch.device("cuda:0")
    F, H, W = a.frames, a.size, a.size
    g = torch.Generator(device=dev).manual_seed(1)
    depths = torch.rand((F, H, W), device=dev, generator=g) * 4 + 0.5
    depths[torch.rand((F, H, W), device=dev, generator=g) < 0.05] = 0
    rgbs = torch.rand((F, H, W, 3), device=dev, generator=g) * 1.2 - 0.1
    turbo = matplotlib.colormaps["turbo"]

    inner_frames = 10      # one call is well under a millisecond of kernels: time ten in a row

    def ours_device():
        for _ in range(inner_frames):
            out = video._frames(rgbs, depths)[:2]
        return out

    def ours_host():
        r, d = video._frames(rgbs, depths)[:2]
        return r.cpu().numpy(), d.cpu().numpy()

    def depth_vis(d):
        valid = d > 0
        near = d[valid].float().quantile(0.01).log() if valid.any() else torch.tensor(0.0, device=d.device)
        far = d.flatten().float().quantile(0.99).log()
        x = d.float().clamp(min=1e-9).log()
        x = 1.0 - (x - near) / (far - near + 1e-9)
        mapped = turbo(x.detach().clip(min=0, max=1).cpu().numpy())[..., :3]
        return torch.tensor(mapped, device=d.device, dtype=torch.float32).movedim(-1, 0)

    def make_video(frames):
        v = torch.stack(frames).clamp(0, 1).permute(0, 2, 3, 1)
        return (v * 255).to(torch.uint8).cpu().numpy()

    def baseline():
        rf, df = [], []
        for rgb, dep in zip(rgbs, depths):
            rf.append(rgb.permute(2, 0, 1))
            df.append(depth_vis(dep))
        return make_video(rf), make_video(df)

    res, last = alternate({"ours_device": ours_device, "ours_host": ours_host, "baseline": baseline}, a.repeats, dev)
    shape = {"frames": F, "height": H, "width": W}
    res["ours_device"] = [m / inner_frames for m in res["ours_device"]]
    for k in res:
        report(f"frame_packing/{k}", res[k], **shape)
    diff_d = float((last["ours_host"][1] != last["baseline"][1]).any(-1).mean())
    diff_r = float((last["ours_host"][0] != last["baseline"][0]).any(-1).mean())
    print(json.dumps({"measurement": "frame_packing/agreement", "depth_pixels_differing": diff_d, "rgb_pixels_differing": diff_r,
                      "ratio_baseline_over_ours_host": round(statistics.median(res["baseline"]) / statistics.median(res["ours_host"]), 2)}), flush=True)
    del last

    N = a.gaussians
    sc = {k: torch.from_numpy(v).to(dev) for k, v in VH.effect_scene(N, 3).items()}
    fx = wm.GSEffects(random_vals=sc["random_vals"])
    gs = {k: sc[k] for k in ("means", "scales", "opacities", "colors", "quats")}
    inner = 20

    def ours_fx():
        for _ in range(inner):
            out = fx.apply_effect(gs, 5.0, effect_type=2)
        return out

    def base_fx():
        for _ in range(inner):
            out = VH.spread_effect(sc["means"], sc["scales"], sc["opacities"], sc["colors"], sc["random_vals"], 5.0, False, torch.float32)
        return out

    res, last = alternate({"ours": ours_fx, "baseline_without_noise": base_fx}, a.repeats, dev)
    for k in res:
        report(f"effect/{k}", [m / inner for m in res[k]], gaussians=N, calls_per_repeat=inner)
    o, b = last["ours"][0], last["baseline_without_noise"]
    print(json.dumps({"measurement": "effect/agreement", "max_abs_diff": {k: float((o[k] - b[k]).abs().max()) for k in ("means", "scales", "opacities", "colors")},
                      "ratio_baseline_over_ours": round(statistics.median(res["baseline_without_noise"]) / statistics.median(res["ours"]), 2)}), flush=True)


if __name__ == "__main__":
    main()
