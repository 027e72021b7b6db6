"""Forward and forward + backward time of the rasteriser at the sizes of profiles/r03_raster_ab.md: one splat per pixel of V views
at 518 x 518, rendered back into V views (V = 8 and 2).  Prints one line per size (also the pair count and the bytes of pair
records the backward writes).

    python tools/bench_raster_backward.py [--views 8 2] [--iters 5]
"""
import argparse
import os
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
    sh = torch.rand(N, 1, 3, generator=g) * 2 - 1
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, 0, 3] = torch.linspace(-0.3, 0.3, V)
    K = torch.tensor([[500.0, 0, 259], [0, 500.0, 259], [0, 0, 1]]).repeat(V, 1, 1)
    return [x.to(dev) for x in (means, quats, scales, opac, sh)], c2w.to(dev), K.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 2])
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for V in a.views:
        splats, c2w, K = scene(V, dev)
        rz = Rasterizer()
        tgt = torch.rand(V, 518, 518, 3, device=dev)

        def fwd(leaves):
            return rz.rasterize_splats(*leaves, c2w, K, 518, 518, sh_degree=0)

        def timed(fn):
            best = float("inf")
            for _ in range(a.iters + 1):          # the first round warms up
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
            return best * 1e3

        t_f = timed(lambda: fwd(splats))
        leaves = [x.clone().requires_grad_(True) for x in splats]

        def both():
            for x in leaves:
                x.grad = None
            rgb, dep, al = fwd(leaves)
            ((rgb - tgt).abs().mean() + 0.1 * dep.mean() + 0.1 * al.mean()).backward()

        t_fb = timed(both)
        n = rz.last_n_isects
        print(f"views {V}: pairs {n}, pair records {n * 40 / 1e6:.1f} MB, forward {t_f:.2f} ms, forward + backward {t_fb:.2f} ms "
              f"(ratio {t_fb / t_f:.2f})", flush=True)


if __name__ == "__main__":
    main()
