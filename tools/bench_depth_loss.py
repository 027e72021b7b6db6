"""Forward and forward + backward time of the sparse disparity loss at the trainer's size, and of the point projection.  Forms:

    fused   hunyuanworld_mirror_amd.depth_loss / project_depth_points (csrc/depthloss.hip)
    torch   the same loss from torch ops in fp32 on the same GPU, in the same process: tests/depth_loss_helper.sample (the normalisation
            by a span tensor made once outside the timed region, one F.grid_sample on a [C,1,H,W] view of the channel), one torch.where,
            F.l1_loss (torch_ops below: no mask, no boolean index, nothing that synchronises the host); for the projection
            tests/depth_loss_helper.project (torch.linalg.inv with its host-side status check, two einsums, the comparisons; no compaction)

Loss shapes: V views of 518 x 518 as channel 3 of a [V,518,518,4] render (the trainer's `renders[..., 3:4]`), M points per view, uniform
over the image; all rows valid.  Timed the way tools/bench_bilagrid.py does: the forms interleaved, round after round, a host clock around
a device synchronise over `--inner` back-to-back calls (200 by default: one call is tens of microseconds, a window 5 to 200 ms), the
first round dropped; per form the median and the spread (min .. max) of the per-call time as one JSON line.

    python tools/bench_depth_loss.py [--rounds 9] [--inner 200] [--tag NAME]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
import depth_loss_helper as DH  # noqa: E402


def timed(fn, inner):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def torch_ops(depths, points, depths_gt, scale):
    """depths [C,H,W] (any strides), points [C,M,2], depths_gt [C,M], scale = DH.pixel_span(depths, points) -> the loss over all rows from
    torch ops: the restatement's own sampler (the normalisation and one F.grid_sample on a view), one torch.where, F.l1_loss"""
    d = DH.sample(depths, points, scale)
    return F.l1_loss(torch.where(d > 0, d.reciprocal(), 0.0), depths_gt.reciprocal())


def stats(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def bench_loss(dev, V, M, rounds, inner, tag):
    H = W = 518
    g = torch.Generator().manual_seed(5 + V + M)
    render = torch.rand(V, H, W, 4, generator=g).to(dev)
    render[..., 3] = 0.5 + 3.0 * render[..., 3]
    points = (torch.rand(V, M, 2, generator=g) * torch.tensor([W, H])).to(dev)
    gt = (0.4 + 3.6 * torch.rand(V, M, generator=g)).to(dev)
    scale = DH.pixel_span(render[..., 3], points)
    forms = {"fused": lambda r: wm.depth_loss(r[..., 3:4], points, gt), "torch": lambda r: torch_ops(r[..., 3], points, gt, scale)}
    leaves = {f: render.clone().requires_grad_(True) for f in forms}

    def both(f):
        leaves[f].grad = None
        forms[f](leaves[f]).backward()

    t_f, t_fb = {f: [] for f in forms}, {f: [] for f in forms}
    for r in range(rounds + 1):
        for f in forms:
            with torch.no_grad():
                tf = timed(lambda: forms[f](render), inner)
            tfb = timed(lambda: both(f), inner)
            if r > 0:
                t_f[f].append(tf); t_fb[f].append(tfb)
    for f in forms:
        print(json.dumps(dict(tag=tag, what="depth_loss", form=f, views=V, points_per_view=M, rounds=rounds, inner=inner, forward_ms=stats(t_f[f]),
                              fwd_bwd_ms=stats(t_fb[f]))), flush=True)
    gf, gt_ = leaves["fused"].grad[..., 3], leaves["torch"].grad[..., 3]
    with torch.no_grad():
        lf, lt = forms["fused"](render), forms["torch"](render)
    print(json.dumps(dict(what="depth_loss", views=V, points_per_view=M, loss_fused=float(lf), loss_torch=float(lt),
                          grad_max_rel_fused_vs_torch=float((gf - gt_).abs().max() / gt_.abs().max()))), flush=True)


def bench_projection(dev, V, P, rounds, inner, tag):
    g = torch.Generator().manual_seed(9)
    W = H = 518
    pw = ((torch.rand(P, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 8.0]) + torch.tensor([0.0, 0.0, 3.0])).to(dev)
    c2w = torch.eye(4).repeat(V, 1, 1)
    for c in range(V):
        co, si = math.cos(0.1 * c), math.sin(0.1 * c)
        c2w[c, :3, :3] = torch.tensor([[co, 0, si], [0, 1, 0], [-si, 0, co]])
        c2w[c, :3, 3] = torch.tensor([0.1 * c, -0.05 * c, 0.02 * c])
    c2w = c2w.to(dev)
    Ks = torch.tensor([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]]).repeat(V, 1, 1).to(dev)
    forms = {"fused": lambda: wm.project_depth_points(pw, c2w, Ks, W, H), "torch": lambda: DH.project(pw, c2w, Ks, W, H)}
    ts = {f: [] for f in forms}
    for r in range(rounds + 1):
        for f in forms:
            t = timed(forms[f], inner)
            if r > 0:
                ts[f].append(t)
    for f in forms:
        print(json.dumps(dict(tag=tag, what="project_depth_points", form=f, views=V, points=P, rounds=rounds, inner=inner, ms=stats(ts[f]))), flush=True)
    a, b = forms["fused"](), forms["torch"]()
    print(json.dumps(dict(what="project_depth_points", valid_fused=int(a[2].sum()), valid_torch=int(b[2].sum()),
                          points_max_abs_diff_on_common_valid=float((a[0] - b[0])[a[2] & b[2]].abs().max()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for V in (1, 8):
        for M in (4096, 262144):
            bench_loss(dev, V, M, a.rounds, a.inner, a.tag)
    bench_projection(dev, 8, 1 << 20, a.rounds, a.inner, a.tag)


if __name__ == "__main__":
    main()
