"""Measures the splat compression (hunyuanworld_mirror_amd.compression, csrc/compress.hip) on the GPU and writes a profile in Markdown.

  python tools/bench_compress.py --out DIR [--profile FILE.md] [--n 1000000] [--k 65536]

Every GPU step runs in a child process of its own under ``timeout``; the driver stops at the first step that does not end cleanly and
writes what it has.  A step writes DIR/<step>.json.  There is no CPU path: a step that finds no GPU fails.

Steps
  assign_D    one k-means assignment at N x K x D (D = 9, 24, 45): the kernel through its own C-ABI entry, device events around
              ``reps`` calls behind a warm-up; against the same assignment by torch on the same GPU in the same process, chunked
              ``torch.cdist(x, c, p=1).argmin(1)`` with the chunk sized to 1 GiB of distances or, where that is fewer rows, to the
              2^24 - 1 pairs torch's p = 1 kernel accepts in one call on HIP (255 rows at K = 65536).  torch is timed over whole chunks until
              ``--torch-seconds`` have passed; when it has not reached N by then, its time for N rows is extrapolated from the rows it did
              (and marked so).  The labels of the two are compared on the rows torch did.
              Rate: one |x - c| term is a subtract and an add, counted as 2 of the peak's FLOP: 2 N K D / time against 157.3 TF.
  kmeans      a full kmeans_l1 of 15 iterations (tol = 0 so that none is skipped), host clock around the call (it ends in a synchronise)
  compress    compress and decompress of an N-splat degree-3 scene with use_sort, files included: time per stage (each stage timed
              in a call of its own behind a synchronise, then the whole call) and the peak extra device memory
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_VECTOR = 157.3e12


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_compress: no GPU; nothing is measured on a CPU")
    return torch


def _data(torch, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    proto = torch.randn(4096, D, device="cuda", generator=g) * 0.3
    pick = torch.randint(0, 4096, (N,), device="cuda", generator=g)
    return (proto[pick] + 0.05 * torch.randn(N, D, device="cuda", generator=g)).contiguous()


def step_assign(a, D):
    torch = _need_gpu()
    from hunyuanworld_mirror_amd.compression import _assign
    N, K = a.n, a.k
    x = _data(torch, N, D, 1)
    c = x[torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))[:K]].contiguous()
    labels, _ = _assign(x, c)      # warm-up
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record()
    for r in range(a.reps):
        labels, dist = _assign(x, c)
        ev[r + 1].record()
    torch.cuda.synchronize()
    ms = [ev[r].elapsed_time(ev[r + 1]) for r in range(a.reps)]
    best = min(ms)
    # 1 GiB of fp32 distances, but no more pairs than torch's p = 1 kernel takes in one call: it launches one 256-thread block per
    # (row, centroid) pair, and HIP refuses a launch of 2^32 threads or more ("invalid configuration argument" at 256 x 65536 pairs)
    chunk = max(1, min((1 << 28) // K, ((1 << 24) - 1) // K))
    probe = min(chunk, 128)
    torch.cdist(x[:probe], c, p=1).argmin(1)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cdist(x[:probe], c, p=1).argmin(1)
    torch.cuda.synchronize()
    est = (time.perf_counter() - t0) * chunk / probe
    if est > a.torch_seconds:      # one 1-GiB chunk would outlast the window: time what fits (the result says so: torch_chunk_rows)
        chunk = max(1, int(chunk * a.torch_seconds / est))
    done, t0, same = 0, time.perf_counter(), 0
    while done < N and time.perf_counter() - t0 < a.torch_seconds:
        ref = torch.cdist(x[done:done + chunk], c, p=1).argmin(1)
        same += int((ref == labels[done:done + chunk].long()).sum())      # ends in a synchronise
        done += min(chunk, N - done)
    t_torch = time.perf_counter() - t0
    torch_ms = t_torch * 1e3 * N / done
    terms = float(N) * K * D
    return {"step": f"assign_D{D}", "N": N, "K": K, "D": D, "ms_each": ms, "ms": best, "flop_rate": 2 * terms / (best * 1e-3),
            "share_of_fp32_vector_peak": 2 * terms / (best * 1e-3) / PEAK_FP32_VECTOR, "torch_rows": done, "torch_chunk_rows": chunk, "torch_ms_for_N": torch_ms,
            "torch_extrapolated": done < N, "torch_over_kernel": torch_ms / best, "labels_equal_to_torch": same, "labels_compared": done}


def step_kmeans(a):
    torch = _need_gpu()
    from hunyuanworld_mirror_amd import kmeans_l1
    x = _data(torch, a.n, 45, 3)
    init = torch.randperm(a.n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))[:a.k]
    kmeans_l1(x[:70000], 1024, max_iter=2, init=init[:1024] % 70000)      # warm-up of every kernel
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    labels, cent, errors = kmeans_l1(x, a.k, max_iter=15, tol=0.0, init=init)
    t = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    return {"step": "kmeans", "N": a.n, "K": a.k, "D": 45, "iterations": int(errors.numel()), "seconds": t, "errors": errors.tolist(),
            "peak_extra_bytes": int(peak), "claim_bytes": 20 * a.n + 4 * a.k + 4 * a.k * 45 + 12 * a.n}


def step_compress(a):
    torch = _need_gpu()
    from hunyuanworld_mirror_amd import PngCompression, sort_splats
    from hunyuanworld_mirror_amd.compression import log_transform
    n = math.isqrt(a.n)
    N = n * n + 7      # a crop
    g = torch.Generator(device="cuda").manual_seed(5)
    u = torch.rand(N, 2, device="cuda", generator=g)
    s = {"means": torch.cat([4 * u - 2, torch.sin(3 * u[:, :1]) * torch.cos(2 * u[:, 1:])], dim=1) * 3,
         "scales": torch.cat([u - 4, u[:, :1] * u[:, 1:] - 5], dim=1), "quats": torch.randn(N, 4, device="cuda", generator=g),
         "opacities": torch.randn(N, device="cuda", generator=g), "sh0": torch.cat([u, 1 - u[:, :1]], dim=1).reshape(N, 1, 3),
         "shN": _data(torch, N, 45, 6).reshape(N, 15, 3)}
    out = {"step": "compress", "N": N, "n": n, "K": a.k}
    with tempfile.TemporaryDirectory() as d:
        small = {k: v[:4096] for k, v in s.items()}
        PngCompression(verbose=False, n_clusters=64).compress(os.path.join(d, "warm"), small)      # warm-up of every kernel
        PngCompression(verbose=False).decompress(os.path.join(d, "warm"))
        torch.cuda.synchronize()
        sq = {k: v[:n * n] for k, v in s.items()}
        sq["means"] = log_transform(sq["means"])
        t0 = time.perf_counter()
        sort_splats(sq, verbose=False)
        torch.cuda.synchronize()
        out["sort_seconds"] = time.perf_counter() - t0
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        c = PngCompression(verbose=False, n_clusters=a.k, generator=torch.Generator(device="cuda").manual_seed(7))
        t0 = time.perf_counter()
        c.compress(os.path.join(d, "full"), s)
        out["compress_seconds"] = time.perf_counter() - t0
        out["compress_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        out["input_bytes"] = int(sum(v.numel() * v.element_size() for v in s.values()))
        out["files"] = {f: os.path.getsize(os.path.join(d, "full", f)) for f in sorted(os.listdir(os.path.join(d, "full")))}
        t0 = time.perf_counter()
        got = c.decompress(os.path.join(d, "full"))
        torch.cuda.synchronize()
        out["decompress_seconds"] = time.perf_counter() - t0
        out["decoded_fields"] = {k: list(v.shape) for k, v in got.items()}
        c2 = PngCompression(verbose=False, use_sort=False, n_clusters=64, max_iter=1)
        t0 = time.perf_counter()
        c2.compress(os.path.join(d, "nosort"), {k: v for k, v in s.items()})
        out["compress_seconds_unsorted_64_clusters_1_iteration"] = time.perf_counter() - t0
    return out


def write_profile(path, results, remarks):
    L = ["# r23: PNG compression of trained splats (csrc/compress.hip)", "",
         "Written by `tools/bench_compress.py`; every figure below is from one MI355X run unless it says otherwise.", ""]
    rows = [r for r in results if r["step"].startswith("assign")]
    L += ["## kmeans assignment, one iteration", "",
          "One `|x - c|` term = 2 FLOP of the 157.3 TF fp32 vector peak (a subtract and an add with the absolute-value modifier).", "",
          "| D | N | K | kernel ms (best of reps) | all reps ms | TFLOP/s | share of peak | torch cdist(p=1).argmin ms for N | torch / kernel | labels equal to torch |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        t = f"{r['torch_ms_for_N']:.0f}" + (f" (extrapolated from {r['torch_rows']} rows)" if r["torch_extrapolated"] else "")
        L.append(f"| {r['D']} | {r['N']} | {r['K']} | {r['ms']:.1f} | {', '.join(f'{m:.1f}' for m in r['ms_each'])} | {r['flop_rate'] / 1e12:.1f} | "
                 f"{100 * r['share_of_fp32_vector_peak']:.1f} % | {t} | {r['torch_over_kernel']:.1f} x | {r['labels_equal_to_torch']} of {r['labels_compared']} |")
    if not rows:
        L.append("| not measured |")
    L.append("")
    for r in results:
        if r["step"] == "kmeans":
            L += ["## full kmeans_l1", "", f"N = {r['N']}, K = {r['K']}, D = {r['D']}, {r['iterations']} iterations and the final assignment: "
                  f"**{r['seconds']:.2f} s** (host clock around the call, which ends in its synchronise).", "",
                  f"Peak extra device memory {r['peak_extra_bytes'] / 2 ** 20:.1f} MiB, of which the outputs and the workspace by the O(N + K D) count "
                  f"(32 N + 4 K + 4 K D bytes) are {r['claim_bytes'] / 2 ** 20:.1f} MiB; the rest is the sort's scratch and torch's int64 copies of the labels.", "",
                  "Mean L1 error per iteration: " + ", ".join(f"{e:.5f}" for e in r["errors"]), ""]
        if r["step"] == "compress":
            L += ["## full compress / decompress", "", f"{r['N']} splats, SH degree 3, grid {r['n']} x {r['n']}, {r['K']} clusters, files included.", "",
                  "| stage | seconds |", "|---|---|", f"| sort_splats alone (two radix sorts and the gather of all fields) | {r['sort_seconds']:.4f} |",
                  f"| compress, unsorted, 64 clusters, 1 iteration (everything but the clustering and the sort) | {r['compress_seconds_unsorted_64_clusters_1_iteration']:.2f} |",
                  f"| compress, sorted, {r['K']} clusters, up to 15 iterations | {r['compress_seconds']:.2f} |", f"| decompress | {r['decompress_seconds']:.2f} |", "",
                  f"Peak extra device memory in compress {r['compress_peak_extra_bytes'] / 2 ** 20:.0f} MiB for {r['input_bytes'] / 2 ** 20:.0f} MiB of input "
                  "(the working copies of every field, twice while a gather runs, the planes, and the k-means workspace): O(N), no [N, K] array.", "",
                  "Files: " + ", ".join(f"{k} {v}" for k, v in r["files"].items()), ""]
    L += ["## compiler resource remarks for kmeans_assign (-Rpass-analysis=kernel-resource-usage, gfx950)", ""] + remarks + [""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def resource_remarks():
    """cross-compile csrc/compress.hip and pick the assign kernels' figures; needs hipcc, not a GPU"""
    import re
    src = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc", "compress.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-x", "hip",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(d, "c.o")], capture_output=True, text=True)
    if r.returncode != 0:
        return ["not compiled here: " + r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "not compiled here"]
    out, cur = ["| kernel | VGPRs | SGPRs | scratch bytes/lane | VGPR spill | occupancy waves/SIMD |", "|---|---|---|---|---|---|"], None
    vals = {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            vals[cur] = {}
        for key, pat in (("v", r" VGPRs: (\d+)"), ("s", r"TotalSGPRs: (\d+)"), ("scr", r"ScratchSize \[bytes/lane\]: (\d+)"), ("sp", r"VGPRs Spill: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                vals[cur][key] = m.group(1)
    for name, v in vals.items():
        m = re.search(r"km_assign_kernelILi(\d+)E", name)
        if m:
            out.append(f"| km_assign_kernel<{m.group(1)}> | {v.get('v')} | {v.get('s')} | {v.get('scr')} | {v.get('sp')} | {v.get('occ')} |")
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    p.add_argument("--profile")
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--k", type=int, default=65536)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--torch-seconds", type=float, default=20.0)
    p.add_argument("--steps", default="assign_D9,assign_D24,assign_D45,kmeans,compress")
    p.add_argument("--step")
    p.add_argument("--step-timeout", type=int, default=240)
    a = p.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:      # the child
        res = step_assign(a, int(a.step[8:])) if a.step.startswith("assign_D") else {"kmeans": step_kmeans, "compress": step_compress}[a.step](a)
        with open(os.path.join(a.out, a.step + ".json"), "w") as f:
            json.dump(res, f)
        print(json.dumps(res))
        return 0
    results = []
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--out", a.out, "--step", step, "--n", str(a.n),
               "--k", str(a.k), "--reps", str(a.reps), "--torch-seconds", str(a.torch_seconds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"bench_compress: step {step} ended with status {rc}; nothing further is started", file=sys.stderr)
            break
        results.append(json.load(open(os.path.join(a.out, step + ".json"))))
    if a.profile:
        write_profile(a.profile, results, resource_remarks())
    return 0 if len(results) == len(a.steps.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
