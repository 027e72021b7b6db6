"""Time of the splat export at the two sizes that matter: 8 x 518^2 Gaussians with K = 0 (what one forward pass of eight views produces)
and 2^20 Gaussians with K = 15 (a trained degree-3 scene).  Per format ("ply", "splat", "ply_compressed"):

    fused     hunyuanworld_mirror_amd.export_splats: device tensors -> the file's bytes on the host (header, kernels, the one copy)
    kernels   the C entry wm_export_splats alone, workspace and output buffer allocated once outside: the flag / scan / scatter
              kernels, the wait for the kept count, the sort and the packing kernels; no copy of the body
    torch     tests/export_helper.py, the vectorised torch composition of the same format on the same device tensors -> bytes on the host
              (the reference's own exporter walks chunks and records in Python loops and is not on this machine)

and save_gs_ply at the first size against its torch composition.  The forms are interleaved round after round, a host clock around a device
synchronise per call (a call is milliseconds and ends on the host anyway), the first round dropped; median and spread (min .. max) in
ms as one JSON line per size.  `payload_GBps` is the body's bytes over the kernels' time; `moved_GBps` adds the input bytes read once
(the sort's and the scan's own traffic is not counted), to be read beside the chip's measured streaming rate of about 6.3 TB/s.
No time is gated.

    python tools/bench_export.py [--rounds 7] [--tag NAME]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
from hunyuanworld_mirror_amd import _lib, exporter  # noqa: E402
import export_helper as EH  # noqa: E402


def _one(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ts):
    ts = ts[1:]
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def _kernels_call(t, fmt):
    """a closure that runs the C entry on buffers made once"""
    L = _lib.lib()
    N, K, f = int(t[0].shape[0]), int(t[5].shape[1]), exporter.FORMATS[fmt]
    ws_b, out_b = L.wm_export_splats_workspace_bytes(N, K, f), L.wm_export_splats_payload_bytes(N, K, f)
    ws = torch.empty(ws_b, device=t[0].device, dtype=torch.uint8)
    out = torch.empty(out_b, device=t[0].device, dtype=torch.uint8)
    n_kept = C.c_int(0)
    ptrs = [C.c_void_p(x.data_ptr() if x.numel() else None) for x in t]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        st = L.wm_export_splats(*ptrs, N, K, f, 1 / 255, C.c_void_p(ws.data_ptr()), ws_b, C.c_void_p(out.data_ptr()), out_b, C.byref(n_kept), stream)
        assert st == 0, st
    return call, n_kept, (ws, out)


def bench(dev, N, K, rounds, tag, label):
    g = torch.Generator().manual_seed(1)
    t = [torch.randn(N, 3, generator=g) * 3.0, torch.randn(N, 3, generator=g) - 3.0, torch.randn(N, 4, generator=g),
         torch.rand(N, generator=g) * 12.0 - 6.0, torch.randn(N, 1, 3, generator=g), torch.randn(N, K, 3, generator=g)]
    t = [x.to(dev) for x in t]
    res = dict(tag=tag, size=label, N=N, K=K)
    in_bytes = sum(x.numel() * 4 for x in t)
    for fmt in EH.FORMATS:
        kcall, n_kept, _keep = _kernels_call(t, fmt)
        forms = {"fused": lambda: exporter.export_splats(*t, format=fmt), "kernels": kcall,
                 "torch": lambda: EH.export_splats(*t, format=fmt)}
        ts = {k: [] for k in forms}
        for _ in range(rounds + 1):
            for k, fn in forms.items():
                ts[k].append(_one(fn))
        r = {k: _stats(v) for k, v in ts.items()}
        payload = _lib.lib().wm_export_splats_payload_bytes(int(n_kept.value), K, exporter.FORMATS[fmt])
        r["n_kept"], r["payload_bytes"] = int(n_kept.value), int(payload)
        r["payload_GBps"] = round(payload / (r["kernels"]["median"] * 1e-3) / 1e9, 1)
        r["moved_GBps"] = round((payload + in_bytes) / (r["kernels"]["median"] * 1e-3) / 1e9, 1)
        r["torch_over_fused"] = round(r["torch"]["median"] / r["fused"]["median"], 1)
        res[fmt] = r
    if K == 0:
        s = [t[0], torch.exp(t[1]), t[2], t[4][:, 0].contiguous(), torch.sigmoid(t[3])]
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "gs.ply")

            def torch_form():
                data, _ = EH.save_gs_ply(*s)
                with open(path, "wb") as f:
                    f.write(data)
            forms = {"fused": lambda: wm.save_gs_ply(path, *s), "torch": torch_form}
            ts = {k: [] for k in forms}
            for _ in range(rounds + 1):
                for k, fn in forms.items():
                    ts[k].append(_one(fn))
            res["save_gs_ply"] = {k: _stats(v) for k, v in ts.items()}
            res["save_gs_ply"]["file_bytes"] = os.path.getsize(path)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bench(dev, 8 * 518 * 518, 0, a.rounds, a.tag, "8 x 518^2, K = 0")
    bench(dev, 1 << 20, 15, a.rounds, a.tag, "2^20, K = 15")


if __name__ == "__main__":
    main()
