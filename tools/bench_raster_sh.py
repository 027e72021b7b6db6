"""Forward and forward + backward time of the rasteriser per colour mode (sh_degree None, 0, 1, 2, 3), at the sizes of
tools/bench_raster_backward.py (profiles/r05_raster_backward.md): one splat per pixel of V views at 518 x 518, rendered back into V
views.  The modes are timed interleaved, round after round; per mode the median and the spread (min .. max) of the rounds are printed
as one JSON line, with the counts a traffic model of the SH kernels needs (visible pairs, (Gaussian, tile) pairs).

    python tools/bench_raster_sh.py [--views 8 2] [--rounds 7] [--degrees none 0 1 2 3] [--tag NAME]

--degrees none 0 runs on a tree that has no SH kernels yet (the comparison of the unchanged routes between two commits: run a copy of
the script from each tree, alternating).  Under rocprofv3 --kernel-trace --stats a short run (--rounds 2) gives the kernels' own times."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hunyuanworld_mirror_amd import Rasterizer  # noqa: E402


def scene(V, dev):
    g = torch.Generator().manual_seed(5)
    N = V * 518 * 518
    means = torch.cat([torch.rand(N, 2, generator=g) * 3 - 1.5, torch.rand(N, 1, generator=g) * 2 + 1.5], 1)
    quats = torch.randn(N, 4, generator=g)
    scales = torch.exp(torch.rand(N, 3, generator=g) * 1.5 - 6.5)
    opac = torch.rand(N, generator=g)
    sh = torch.cat([torch.rand(N, 1, 3, generator=g) * 2 - 1, torch.rand(N, 15, 3, generator=g) * 0.6 - 0.3], 1)
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, 0, 3] = torch.linspace(-0.3, 0.3, V)
    K = torch.tensor([[500.0, 0, 259], [0, 500.0, 259], [0, 0, 1]]).repeat(V, 1, 1)
    return [x.to(dev) for x in (means, quats, scales, opac)], sh.to(dev), c2w.to(dev), K.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 2])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--degrees", nargs="+", default=["none", "0", "1", "2", "3"])
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for V in a.views:
        geo, sh, c2w, K = scene(V, dev)
        rz = Rasterizer()
        tgt = torch.rand(V, 518, 518, 3, device=dev)
        colours = {"none": (torch.clamp_min(0.28209479177387814 * sh[:, 0] + 0.5, 0).contiguous(), None), "0": (sh[:, :1].contiguous(), 0)}
        for L in (1, 2, 3):
            colours[str(L)] = (sh, L)

        def fwd(leaves, mode):
            return rz.rasterize_splats(*leaves, c2w, K, 518, 518, sh_degree=colours[mode][1])

        def both(leaves, mode):
            for x in leaves:
                x.grad = None
            rgb, dep, al = fwd(leaves, mode)
            ((rgb - tgt).abs().mean() + 0.1 * dep.mean() + 0.1 * al.mean()).backward()

        def timed(fn):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        plain = {m: geo + [colours[m][0]] for m in a.degrees}
        leaves = {m: [x.clone().requires_grad_(True) for x in plain[m]] for m in a.degrees}
        with torch.no_grad():
            info = rz.rasterize_splats(*plain[a.degrees[0]], c2w, K, 518, 518, sh_degree=colours[a.degrees[0]][1], return_info=True)[3]
        visible = int((info["radii"] > 0).all(-1).sum())
        t_f, t_fb = {m: [] for m in a.degrees}, {m: [] for m in a.degrees}
        for r in range(a.rounds + 1):      # the first round warms every mode up and is dropped
            for m in a.degrees:
                with torch.no_grad():
                    f = timed(lambda: fwd(plain[m], m))
                fb = timed(lambda: both(leaves[m], m))
                if r > 0:
                    t_f[m].append(f); t_fb[m].append(fb)
        for m in a.degrees:
            row = dict(tag=a.tag, views=V, gaussians=V * 518 * 518, sh_degree=m, visible_pairs=visible, tile_pairs=rz.last_n_isects)
            row.update(rounds=a.rounds, forward_ms_median=round(statistics.median(t_f[m]), 3), forward_ms_min=round(min(t_f[m]), 3),
                       forward_ms_max=round(max(t_f[m]), 3), fwd_bwd_ms_median=round(statistics.median(t_fb[m]), 3),
                       fwd_bwd_ms_min=round(min(t_fb[m]), 3), fwd_bwd_ms_max=round(max(t_fb[m]), 3))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
