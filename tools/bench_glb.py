"""Timings of the GLB scene hand-off (profiles/r20_glb_scene.md): S views of 518 x 518 with an iid mask of keep rate 0.8.

    python tools/bench_glb.py --views 8 32 [--out glb_bench.jsonl]     on the GPU
    python tools/bench_glb.py --views 8 32 --reference <reference root>           the reference's host path, no GPU needed

GPU: wm_image_mesh_count by a host clock (the entry returns after its one synchronisation), wm_image_mesh_pack by device events around ten calls in a row (per call), the copy of the
packed body to the host, image_mesh as a whole, convert_predictions_to_glb_scene and export by a host clock around work that ends in a
synchronise.  Every shape is warmed up; medians and minima over --iters runs.  The bytes the pack must move (mask and remap reads, the
vertices' inputs and outputs, the faces) over its time give its achieved rate.

--reference: per view the reference's create_image_mesh(points, colors, mask=, triangulate=True) and the two uint8 conversions of
visual_util.py:400-428 on the same arrays on the host (cv2 / requests / trimesh replaced by empty modules: the function needs none of them)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HW = 518
PACK_CALLS = 10


def make(S, seed=0):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((S, HW, HW, 3)).astype(np.float32)
    img = rng.random((S, HW, HW, 3), dtype=np.float32)
    mask = rng.random((S, HW, HW)) < 0.8
    poses = np.tile(np.eye(4), (S, 1, 1))
    return pts, img, mask, poses


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "n": len(xs)}


def run_reference(ref_root, views, iters):
    for name in ("cv2", "requests", "trimesh"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["trimesh"].Scene = sys.modules["trimesh"].Trimesh = object      # named in annotations only
    sys.path.insert(0, ref_root)
    from src.utils.visual_util import create_image_mesh
    for S in views:
        pts, img, mask, _ = make(S)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            for i in range(S):
                frame = img[i] * 255      # (the reference does this in place)
                faces, v, c = create_image_mesh(pts[i] * np.array([1, -1, 1], np.float32), frame / 255.0, mask=mask[i], triangulate=True)
                v = v * np.array([1, -1, 1], np.float32)
                c8 = (c * 255).astype(np.uint8)
            ts.append((time.perf_counter() - t0) * 1e3)
        yield {"what": "reference_host_meshes", "views": S, **stats(ts)}


def run_gpu(views, iters):
    import torch
    from hunyuanworld_mirror_amd import _lib, convert_predictions_to_glb_scene, image_mesh
    from hunyuanworld_mirror_amd._lib import check, ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (use --reference for the host path)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for S in views:
        pts, img, mask, poses = make(S)
        d_pts, d_img, d_mask = (torch.from_numpy(a).to(dev) for a in (pts, img, mask))
        m8 = d_mask.to(torch.uint8)
        ws_bytes = L.wm_image_mesh_workspace_bytes(S, HW, HW)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        nv, nq = (C.c_int64 * (S + 1))(), (C.c_int64 * (S + 1))()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t_count, t_pack, t_copy, t_mesh, t_scene, t_export = [], [], [], [], [], []
        pred = {"world_points": d_pts, "images": d_img, "camera_poses": poses, "final_mask": d_mask}
        for it in range(iters + 2):      # two warm-up rounds
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            check(L.wm_image_mesh_count(ptr(m8), S, HW, HW, ptr(ws), ws_bytes, nv, nq, stream(dev)), "count")      # returns after its synchronise
            t6 = time.perf_counter()
            V, Q = int(nv[S]), int(nq[S])
            buf = torch.empty(16 * V + 24 * Q, device=dev, dtype=torch.uint8)
            bounds = torch.empty((S, 6), device=dev)
            ev[0].record()
            for _ in range(PACK_CALLS):      # a window of several calls: one call is well under a millisecond of kernels
                check(L.wm_image_mesh_pack(ptr(d_pts), ptr(d_img), None, ptr(m8), S, HW, HW, ptr(ws), ws_bytes, V, Q, ptr(buf), ptr(buf[12 * V:]),
                                           None, ptr(buf[16 * V:]), ptr(bounds), stream(dev)), "pack")
            ev[1].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = buf.cpu()
            t1 = time.perf_counter()
            mesh = image_mesh(d_pts, d_img, d_mask)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            scene = convert_predictions_to_glb_scene(pred, "all", True, False, True, True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            data = scene.export()
            t4 = time.perf_counter()
            if it >= 2:
                t_count.append((t6 - t5) * 1e3)
                t_pack.append(ev[0].elapsed_time(ev[1]) / PACK_CALLS)
                t_copy.append((t1 - t0) * 1e3)
                t_mesh.append((t2 - t1) * 1e3)
                t_scene.append((t3 - t2) * 1e3)
                t_export.append((t4 - t3) * 1e3)
            del host, mesh, scene
        px = S * HW * HW
        pack_bytes = px * (9 + 9) + V * (24 + 16 + 4) + Q * (4 * 4 + 24)      # 3 x 3 mask reads twice; vertex in / out + remap; remap reads + faces
        base = {"views": S, "vertices": V, "quads": Q, "body_bytes": int(buf.numel()), "glb_bytes": len(data)}
        yield {"what": "count_with_sync", **base, **stats(t_count)}
        yield {"what": "pack_device", **base, **stats(t_pack), "bytes_counted": pack_bytes,
               "GBps_at_median": round(pack_bytes / statistics.median(t_pack) / 1e6, 1)}
        yield {"what": "body_copy_to_host", **base, **stats(t_copy), "GBps_at_median": round(buf.numel() / statistics.median(t_copy) / 1e6, 2)}
        yield {"what": "image_mesh_call", **base, **stats(t_mesh)}
        yield {"what": "convert_predictions_to_glb_scene", **base, **stats(t_scene)}
        yield {"what": "export_to_bytes", **base, **stats(t_export)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run_reference(a.reference, a.views, a.iters) if a.reference else run_gpu(a.views, a.iters)
    out = open(a.out, "a") if a.out else None
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
