"""Time wm_point_filter_mask (app.py:172-206 in one call) at the demo's defaults on S views of H x W: warm-up, then the median
of event-timed calls through the C ABI with a preallocated workspace.  Prints one JSON line.

    python tools/bench_point_masks.py [--views 32] [--size 518] [--iters 30]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hunyuanworld_mirror_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    S, H = a.views, a.size
    W = H
    g = torch.Generator().manual_seed(0)
    conf = (1 + torch.round(torch.rand(S, H, W, generator=g) * 32) / 8).cuda()
    depth = (1 + torch.rand(S, H, W, generator=g)).cuda()
    nrm = torch.randn(S, H, W, 3, generator=g)
    nrm = (nrm / nrm.norm(dim=-1, keepdim=True)).cuda()
    out = torch.empty(S, H, W, dtype=torch.uint8, device="cuda")
    thr = torch.empty(S, device="cuda")
    L = _lib.lib()
    wsb = L.wm_point_filter_mask_workspace_bytes(S, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        st = L.wm_point_filter_mask(p(conf), p(depth), p(nrm), S, H, W, 1, C.c_double(10.0), 1, C.c_double(5.0), C.c_float(0.03),
                                    p(thr), p(out), p(ws), wsb, s)
        assert st == 0, st

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    us = float(np.median(ts))
    px = S * H * W
    nbytes = px * (4 * 4 + 4 + 4 + 12 + 1)   # four radix-select passes over conf; conf, depth, normals read and the mask written once
    print(json.dumps({"op": "wm_point_filter_mask", "views": S, "H": H, "W": W, "median_us": round(us, 1),
                      "min_us": round(min(ts), 1), "us_per_view": round(us / S, 2), "nominal_bytes": nbytes,
                      "nominal_GBps": round(nbytes / us / 1e3, 1), "iters": a.iters}))


if __name__ == "__main__":
    main()
