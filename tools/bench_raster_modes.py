"""Forward and forward + backward time of the rasteriser per call form, at the sizes of tools/bench_raster_sh.py
(profiles/r10_spherical_harmonics.md): one splat per pixel of V views at 518 x 518 (the splat distribution of the full-size raster tests),
rendered back into V views.  Forms:

    rasterizer   Rasterizer().rasterize_splats, no new keyword (runs on a tree from before the options too)
    defaults     rasterization() with gsplat's defaults, render_mode "RGB+ED"
    antialiased  rasterization(rasterize_mode="antialiased", render_mode="RGB+ED")
    aa_bg        rasterization(rasterize_mode="antialiased", backgrounds=[C,3] requiring grad, render_mode="RGB+ED")

The forms are timed interleaved, round after round (host clock around a device synchronise; the first round warms every form up and is
dropped); per form the median and the spread (min .. max) of the rounds are printed as one JSON line.

    python tools/bench_raster_modes.py [--views 8] [--rounds 9] [--forms rasterizer defaults antialiased aa_bg] [--tag NAME]

To compare the unchanged route between two commits, run a copy of the script from each tree with --forms rasterizer, alternating."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hunyuanworld_mirror_amd as wm  # noqa: E402


def scene(V, dev):
    g = torch.Generator().manual_seed(5)
    N = V * 518 * 518
    means = torch.cat([torch.rand(N, 2, generator=g) * 3 - 1.5, torch.rand(N, 1, generator=g) * 2 + 1.5], 1)
    quats = torch.randn(N, 4, generator=g)
    scales = torch.exp(torch.rand(N, 3, generator=g) * 1.5 - 6.5)
    opac = torch.rand(N, generator=g)
    sh = torch.rand(N, 1, 3, generator=g) * 2 - 1
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, 0, 3] = torch.linspace(-0.3, 0.3, V)
    K = torch.tensor([[500.0, 0, 259], [0, 500.0, 259], [0, 0, 1]]).repeat(V, 1, 1)
    return [x.to(dev) for x in (means, quats, scales, opac, sh)], c2w.to(dev), K.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--forms", nargs="+", default=["rasterizer", "defaults", "antialiased", "aa_bg"])
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    V = a.views
    plain, c2w, K = scene(V, dev)
    vm = torch.linalg.inv(c2w)
    rz = wm.Rasterizer()
    tgt = torch.rand(V, 518, 518, 3, device=dev)
    bg = torch.rand(V, 3, device=dev)
    leaves = {f: [x.clone().requires_grad_(True) for x in plain] for f in a.forms}
    bgs = {f: bg.clone().requires_grad_(True) for f in a.forms}

    def fwd(f, x, grad):
        if f == "rasterizer":
            return rz.rasterize_splats(*x, c2w, K, 518, 518, sh_degree=0)
        kw = dict(sh_degree=0, render_mode="RGB+ED")
        if f != "defaults":
            kw["rasterize_mode"] = "antialiased"
        if f == "aa_bg":
            kw["backgrounds"] = bgs[f] if grad else bg
        rc, al, _ = wm.rasterization(*x, vm, K, 518, 518, **kw)
        return rc[..., :3], rc[..., 3:], al

    def both(f):
        for x in leaves[f] + [bgs[f]]:
            x.grad = None
        rgb, dep, al = fwd(f, leaves[f], True)
        ((rgb - tgt).abs().mean() + 0.1 * dep.mean() + 0.1 * al.mean()).backward()

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_f, t_fb = {f: [] for f in a.forms}, {f: [] for f in a.forms}
    for r in range(a.rounds + 1):
        for f in a.forms:
            with torch.no_grad():
                tf = timed(lambda: fwd(f, plain, False))
            tfb = timed(lambda: both(f))
            if r > 0:
                t_f[f].append(tf); t_fb[f].append(tfb)
    for f in a.forms:
        row = dict(tag=a.tag, form=f, views=V, gaussians=V * 518 * 518, rounds=a.rounds,
                   forward_ms_median=round(statistics.median(t_f[f]), 3), forward_ms_min=round(min(t_f[f]), 3), forward_ms_max=round(max(t_f[f]), 3),
                   fwd_bwd_ms_median=round(statistics.median(t_fb[f]), 3), fwd_bwd_ms_min=round(min(t_fb[f]), 3),
                   fwd_bwd_ms_max=round(max(t_fb[f]), 3))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
