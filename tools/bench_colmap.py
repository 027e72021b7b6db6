"""Time of the COLMAP hand-off at 8 and 32 views of 518 x 518 (what one forward pass produces), conf_threshold 30 %:

    select    colmap_points_from_depth: the candidate rule, the global top-k, the ordered compaction and the kept points / colours / pixel
              coordinates on the device (its one stream synchronisation inside)
    pack      wm_colmap_pack alone on buffers made once: the bodies of points3D.bin (59 B per point) and images.bin (24 B per point)
    copy      the two bodies to the host (pageable, as save_colmap copies them)
    save      save_colmap as a whole: pack + copy + the host's headers + the file writes (a temporary directory), points3D.ply included
    torch     the same result from torch ops on the same device tensors (depth_to_world_coords_points of this library, boolean indexing,
              torch.topk, the gathers) and numpy structured packing on the host (tests/colmap_helper.py); bytes in memory, no file write
    loop      the reference's own Python loop (build_pycolmap_recon.py's add_point3D / Point2D / track.add_element per point) is not
              timed on the full set: its three calls per point are run with do-nothing stand-ins over a 10^5-point sample and the time is
              scaled to the kept count.  Marked "extrapolated"; pycolmap's own work inside the calls is not in it, so it is a floor.

The forms are interleaved round after round, a host clock around a device synchronise per call (every form ends on the host anyway), the
first round dropped; median and spread (min .. max) in ms, one JSON line per size.  No time is gated.

    python tools/bench_colmap.py [--rounds 5] [--views 8 32] [--tag NAME]"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
from hunyuanworld_mirror_amd import _lib, colmap  # noqa: E402
import colmap_helper as CH  # noqa: E402


def _one(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ts):
    ts = ts[1:] if len(ts) > 1 else ts
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def _scene(S, H, W, dev):
    g = torch.Generator(device="cpu").manual_seed(S)
    depth = (1.5 + 2.0 * torch.rand(S, H, W, generator=g)).to(dev)
    depth[:, :4, :] = 0.0
    conf = (1.0 + 9.0 * torch.rand(S, H, W, generator=g)).to(dev)
    images = torch.rand(S, 3, H, W, generator=g).to(dev)
    w2c = torch.eye(4).repeat(S, 1, 1)
    for i in range(S):
        a = 0.05 * i
        w2c[i, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float64).float()
        w2c[i, :3, 3] = torch.tensor([0.1 * i, 0.0, 0.02 * i])
    K = torch.tensor([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]]).repeat(S, 1, 1)
    return depth, conf, images, w2c.to(dev), K.to(dev)


def _torch_form(depth, conf, images, w2c, K, percent, out_size, names):
    """infer.py:296-349 as torch ops on the device and numpy packing on the host -> the bytes of the three files"""
    S, H, W = depth.shape
    c2w = torch.linalg.inv(w2c.cpu().double()).float().to(depth.device)
    world, _, mask = wm.depth_to_world_coords_points(depth, c2w, K)
    cols = (images.permute(0, 2, 3, 1).clamp(0, 1) * 255).to(torch.uint8)
    valid = mask.reshape(-1)
    all_conf = conf.reshape(-1)[valid]
    cm = wm.create_confidence_mask(all_conf, percent)
    idx = torch.nonzero(valid)[:, 0][cm]
    pts, col = world.reshape(-1, 3)[idx].cpu().numpy(), cols.reshape(-1, 3)[idx].cpu().numpy()
    idx = idx.cpu().numpy()
    view, rem = idx // (H * W), idx % (H * W)
    xyf = np.stack([((rem % W) * (out_size[0] / W)).astype(np.int32), ((rem // W) * (out_size[1] / H)).astype(np.int32), view.astype(np.int32)], 1)
    counts = np.bincount(view, minlength=S)
    w2c_h = w2c.cpu().numpy()
    quats = [colmap.rotation_to_quaternion(w2c_h[i, :3, :3].astype(np.float64)) for i in range(S)]
    return (CH.points3d_bytes(pts, col, counts), CH.images_bytes(xyf, counts, quats, w2c_h, names), CH.cameras_bytes(K.cpu().numpy(), out_size, "SIMPLE_PINHOLE"))


def _loop_floor(n_sample, P):
    """the reference's per-point statements with do-nothing stand-ins, over n_sample points; scaled to P"""
    class Track:
        def __init__(self):
            self.e = []

        def add_element(self, a, b):
            self.e.append((a, b))

    pts, cols = np.random.rand(n_sample, 3).astype(np.float32), np.zeros((n_sample, 3), np.uint8)
    xyf = np.zeros((n_sample, 3), np.int32)
    t0 = time.perf_counter()
    store = {}
    for i in range(n_sample):
        store[i + 1] = (pts[i], Track(), cols[i])                                   # scene.add_point3D(points[i], pycolmap.Track(), point_colors[i])
    valid = np.nonzero(xyf[:, 2].astype(np.int32) == 0)[0]
    out = []
    for j, b in enumerate(valid):
        out.append((xyf[b][:2], b + 1))                                             # pycolmap.Point2D(xy, point3D_id)
        store[b + 1][1].add_element(1, j)                                           # track.add_element(frame + 1, idx)
    dt = (time.perf_counter() - t0) * 1e3
    return dt * P / n_sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for S in a.views:
        H = W = a.size
        depth, conf, images, w2c, K = _scene(S, H, W, dev)
        names = [f"image_{i:04d}.png" for i in range(S)]
        out_size = (W, H)
        sel = wm.colmap_points_from_depth(depth, conf, images, w2c, K, 30.0, out_size)
        pts, col, xyf, counts = sel
        P = int(pts.shape[0])
        ws_b = L.wm_colmap_pack_workspace_bytes(P, S)
        ws = torch.empty(ws_b, device=dev, dtype=torch.uint8)
        b3 = torch.empty(P * 59, device=dev, dtype=torch.uint8)
        b2 = torch.empty(P * 24, device=dev, dtype=torch.uint8)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def pack():
            st = L.wm_colmap_pack(vp(pts), vp(col), vp(xyf), vp(counts), S, P, vp(ws), ws_b, vp(b3), P * 59, vp(b2), P * 24, stream)
            assert st == 0, st

        tmp = tempfile.mkdtemp()
        forms = {
            "select": lambda: wm.colmap_points_from_depth(depth, conf, images, w2c, K, 30.0, out_size),
            "pack": pack,
            "copy": lambda: (b3.cpu(), b2.cpu()),
            "save": lambda: wm.save_colmap(tmp, pts, col, xyf, counts, w2c, K, names, out_size),
            "torch": lambda: _torch_form(depth, conf, images, w2c, K, 30.0, out_size, names),
        }
        times = {k: [] for k in forms}
        for _ in range(a.rounds + 1):
            for k, fn in forms.items():
                times[k].append(_one(fn))
        # the two forms give the same files
        ref3, ref2, refc = _torch_form(depth, conf, images, w2c, K, 30.0, out_size, names)
        # (points3D.bin holds fp32 positions: the torch form inverts the pose by elimination, the library by transposition, a last-bit difference)
        same = {f: open(os.path.join(tmp, f), "rb").read() == r for f, r in (("points3D.bin", ref3), ("images.bin", ref2), ("cameras.bin", refc))}
        line = dict(tool="bench_colmap", tag=a.tag, views=S, size=a.size, pixels=S * H * W, kept=P, body_MB=round(P * 83 / 1e6, 1),
                    files_equal_torch_form=same, ms={k: _stats(v) for k, v in times.items()},
                    pack_payload_GBps=round(P * 83 / 1e9 / (statistics.median(times["pack"][1:]) / 1e3), 1),
                    reference_loop_floor_ms_extrapolated=round(_loop_floor(100000, P), 1))
        print(json.dumps(line), flush=True)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
