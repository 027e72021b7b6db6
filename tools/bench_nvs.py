"""Time the target-view validity mask (wm_in_frustum_mask, csrc/frustum.hip) against the torch restatement of the reference's
algorithm (tests/nvs_helper.py in_frustum_mask: frustum.py:26-89 with its [b, v1, v2, h, w, 3] intermediates) on the same GPU, at
S context + V target views of size x size.  Outside the timed bench.py.

    python tools/bench_nvs.py [--context 8] [--target 8] [--size 518] [--iters 20] [--warmup 3] [--no-match]

Scene: the wall of tools/gen_golden_nvs.py (mask_scene) at the given size.  After the warm-up the three candidates run interleaved,
one after the other in every repetition, each timed with device events; the medians are reported:
  kernel   the C-ABI call alone, matrices precomputed (what the GPU does)
  call     calculate_in_frustum_mask as a caller sees it (the two fp64 inverses on the host, five small uploads, the kernel)
  torch    the restatement
Peak memory is torch's max_memory_allocated over one call of each, above what the inputs hold.  The byte count the kernel is
held against: depth_1 read once, the mask written once, depth_2 read once from HBM (its further reads are cache traffic).
--no-match zeroes the context depths: no pixel matches, so no wave of the kernel stops before the last context view (its worst case).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nvs_helper as NH  # noqa: E402
from gen_golden_nvs import mask_scene  # noqa: E402
from hunyuanworld_mirror_amd import _lib, nvs  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=8)
    ap.add_argument("--target", type=int, default=8)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-match", action="store_true", help="zero context depths: nothing matches, no wave stops early (the kernel's worst case)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nvs.py measures on the GPU: no HIP device visible")
    V2, V1, H = a.context, a.target, a.size
    W = H
    sc = mask_scene(1, V1, V2, H, W, seed=3)
    d1, K1, c1, d2, K2, c2 = NH.scene_tensors(sc, device="cuda")
    if a.no_match:
        d2 = torch.zeros_like(d2)
    kinv, rel = nvs.frustum_matrices(K1, c1, c2)
    kinv, rel = kinv.to("cuda", torch.float32).contiguous(), rel.to("cuda", torch.float32).contiguous()
    mask = torch.empty((1, V1, H, W), dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def kernel():
        st = L.wm_in_frustum_mask(p(d1), p(d2), p(kinv), p(rel), p(K2), 1, V1, V2, H, W, p(mask), s)
        assert st == 0, st
        return mask

    cands = {"kernel": kernel, "call": lambda: nvs.calculate_in_frustum_mask(d1, K1, c1, d2, K2, c2),
             "torch": lambda: NH.in_frustum_mask(d1, K1, c1, d2, K2, c2)}
    for _ in range(a.warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    outs = {}
    for _ in range(a.iters):
        for k, fn in cands.items():
            t, outs[k] = timed(fn)
            ts[k].append(t)
    got, ref = outs["call"], outs["torch"]
    assert torch.equal(outs["kernel"].bool(), got)
    free = NH.marginal_pixels(d1, K1, c1, d2, K2, c2)
    res = {"op": "wm_in_frustum_mask", "no_match": bool(a.no_match), "context": V2, "target": V1, "H": H, "W": W, "iters": a.iters}
    for k in cands:
        res[k + "_median_us"], res[k + "_min_us"] = round(float(np.median(ts[k])), 1), round(min(ts[k]), 1)
    res["torch_over_kernel"] = round(res["torch_median_us"] / res["kernel_median_us"], 1)
    res["torch_over_call"] = round(res["torch_median_us"] / res["call_median_us"], 1)
    res["mask_true"] = round(float(got.float().mean()), 4)
    res["differs_from_torch_fp32"] = int((got != ref).sum())
    res["differs_off_marginal"] = int(((got != ref) & ~free).sum())
    res["marginal"] = int(free.sum())
    del outs, free, ref, got
    res["kernel_peak_bytes"] = peak_above_inputs(cands["call"])
    res["torch_peak_bytes"] = peak_above_inputs(cands["torch"])
    nbytes = V1 * H * W * 5 + V2 * H * W * 4
    res["nominal_bytes"] = nbytes
    res["kernel_nominal_GBps"] = round(nbytes / res["kernel_median_us"] / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
