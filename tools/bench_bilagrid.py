"""Forward and forward + backward time of the bilateral-grid slice at the trainer's size: V views of 518 x 518 on the pixel-centre
meshgrid, the default 16 x 16 x 8 grids, one grid per view.  Forms:

    fused   hunyuanworld_mirror_amd.slice (csrc/bilagrid.hip)
    torch   the same function composed of torch ops in fp32 on the same GPU (tests/bilagrid_helper.py: 5-D F.grid_sample + the 3 x 4
            product) -- what lib_bilagrid.py does on this hardware

Timed the way tools/bench_raster_modes.py does: the forms interleaved, round after round (host clock around a device synchronise; the
first round warms every form up and is dropped); per form the median and the spread (min .. max) as one JSON line.  The backward is
driven by an L1 distance to a fixed target; both the grids and rgb require grad.

    python tools/bench_bilagrid.py [--views 8] [--rounds 9] [--tag NAME]"""
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
import hunyuanworld_mirror_amd as wm  # noqa: E402
import bilagrid_helper as BH  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = a.views, 518, 518
    g = torch.Generator().manual_seed(5)
    rgb0 = torch.rand(V, H, W, 3, generator=g).to(dev)
    tgt = torch.rand(V, H, W, 3, generator=g).to(dev)
    gy, gx = torch.meshgrid((torch.arange(H, device=dev) + 0.5) / H, (torch.arange(W, device=dev) + 0.5) / W, indexing="ij")
    xy = torch.stack([gx, gy], -1).unsqueeze(0).expand(V, -1, -1, -1)
    ids = torch.arange(V, device=dev)
    grids0 = (wm.BilateralGrid(V).grids.detach() + 0.1 * torch.randn(V, 12, 8, 16, 16, generator=g)).to(dev)
    forms = {"fused": lambda gr, c: wm.slice(gr, xy, c, ids.unsqueeze(-1))["rgb"], "torch": lambda gr, c: BH.slice_rgb(gr, xy, c, ids)}
    leaves = {f: (grids0.clone().requires_grad_(True), rgb0.clone().requires_grad_(True)) for f in forms}

    def both(f):
        gr, c = leaves[f]
        gr.grad = None; c.grad = None
        (forms[f](gr, c) - tgt).abs().mean().backward()

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_f, t_fb = {f: [] for f in forms}, {f: [] for f in forms}
    for r in range(a.rounds + 1):
        for f in forms:
            with torch.no_grad():
                tf = timed(lambda: forms[f](grids0, rgb0))
            tfb = timed(lambda: both(f))
            if r > 0:
                t_f[f].append(tf); t_fb[f].append(tfb)
    for f in forms:
        print(json.dumps(dict(tag=a.tag, form=f, views=V, rounds=a.rounds,
                              forward_ms_median=round(statistics.median(t_f[f]), 3), forward_ms_min=round(min(t_f[f]), 3), forward_ms_max=round(max(t_f[f]), 3),
                              fwd_bwd_ms_median=round(statistics.median(t_fb[f]), 3), fwd_bwd_ms_min=round(min(t_fb[f]), 3),
                              fwd_bwd_ms_max=round(max(t_fb[f]), 3))), flush=True)
    gf, gt = leaves["fused"][0].grad, leaves["torch"][0].grad
    print(json.dumps(dict(grids_grad_max_rel_fused_vs_torch=float((gf - gt).abs().max() / gt.abs().max()),
                          rgb_grad_max_rel_fused_vs_torch=float((leaves["fused"][1].grad - leaves["torch"][1].grad).abs().max() / leaves["torch"][1].grad.abs().max()))))


if __name__ == "__main__":
    main()
