"""Records tests/golden/compress_a/: what the reference's PngCompression writes and reads back for one small seeded scene.

Runs on the CPU and is no part of any test.  Usage:  python tools/gen_golden_compress.py <reference checkout> [out dir]

The reference's gsplat/compression/png_compression.py is loaded by file path.  Its imports that are not installed, or that would pull in
gsplat's CUDA backend, are stood in for: ``imageio.v2`` by Pillow (imwrite / imread), the parent packages ``gsplat`` and
``gsplat.compression`` by empty modules, ``gsplat.compression.sort`` by a module whose sort_splats refuses to run (use_sort=False is
the only mode recorded: PLAS is not installed), and ``gsplat.utils`` by the reference's own gsplat/utils.py, also loaded by path.

Recorded (data the reference's programs read and write, nothing of its program text):
  inputs.npz            the scene: means 3 randn, scales, quats (4 channels), opacities (distinct), sh0 [N,1,3], extra [N,2]; N = 1000
  ref/                  the reference's files as written (N is cropped to 961 = 31^2): *.png, extra.npz, meta.json
  ref_decompressed.npz  the reference's decompress() of ref/
  kmeans/               a hand-made shN.npz (K = 300 centroid codes at 6 bits, 961 uint16 labels, D = 24) with its meta.json
  kmeans_decompressed.npz   the reference's _decompress_kmeans of kmeans/ (numpy and torch only; torchpq is not needed to decode)
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, SEED = 1000, 20260


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    from PIL import Image
    gs = os.path.join(ref_root, "submodules", "gsplat", "gsplat")
    v2 = types.ModuleType("imageio.v2")
    v2.imwrite = lambda path, arr: Image.fromarray(np.asarray(arr)).save(path)
    v2.imread = lambda path: np.array(Image.open(path))
    imageio = types.ModuleType("imageio")
    imageio.v2 = v2
    sys.modules["imageio"], sys.modules["imageio.v2"] = imageio, v2
    for pkg in ("gsplat", "gsplat.compression"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    sort = types.ModuleType("gsplat.compression.sort")

    def sort_splats(*a, **k):
        raise RuntimeError("PLAS is not installed: only use_sort=False is recorded")
    sort.sort_splats = sort_splats
    sys.modules["gsplat.compression.sort"] = sort
    _load("gsplat.utils", os.path.join(gs, "utils.py"))
    return _load("gsplat.compression.png_compression", os.path.join(gs, "compression", "png_compression.py"))


def scene():
    g = torch.Generator().manual_seed(SEED)
    return {
        "means": 3.0 * torch.randn(N, 3, generator=g),
        "scales": torch.randn(N, 3, generator=g) - 4.0,
        "quats": torch.randn(N, 4, generator=g),
        "opacities": (torch.randperm(N, generator=g).float() + torch.rand(N, generator=g) * 0.5) / N * 8.0 - 4.0,      # distinct
        "sh0": torch.randn(N, 1, 3, generator=g) * 0.6,
        "extra": torch.rand(N, 2, generator=g),
    }


def main():
    ref_root = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "..", "tests", "golden", "compress_a")
    R = load_reference(ref_root)
    os.makedirs(os.path.join(out, "ref"), exist_ok=True)
    os.makedirs(os.path.join(out, "kmeans"), exist_ok=True)
    splats = scene()
    assert len(torch.unique(splats["opacities"])) == N
    np.savez_compressed(os.path.join(out, "inputs.npz"), **{k: v.numpy() for k, v in splats.items()})
    comp = R.PngCompression(use_sort=False, verbose=False)
    comp.compress(os.path.join(out, "ref"), {k: v.clone() for k, v in splats.items()})
    dec = comp.decompress(os.path.join(out, "ref"))
    np.savez_compressed(os.path.join(out, "ref_decompressed.npz"), **{k: v.numpy() for k, v in dec.items()})

    rng = np.random.default_rng(SEED)
    K, D, n2 = 300, 24, 961
    np.savez_compressed(os.path.join(out, "kmeans", "shN.npz"), centroids=rng.integers(0, 64, size=(K, D)).astype(np.uint8),
                        labels=rng.integers(0, K, size=n2).astype(np.uint16))
    meta = {"shape": [n2, 8, 3], "dtype": "float32", "mins": float(np.float32(-0.7318)), "maxs": float(np.float32(0.9023)), "quantization": 6}
    with open(os.path.join(out, "kmeans", "meta.json"), "w") as f:
        json.dump({"shN": meta}, f)
    shn = R._decompress_kmeans(os.path.join(out, "kmeans"), "shN", meta)
    np.savez_compressed(os.path.join(out, "kmeans_decompressed.npz"), shN=shn.numpy())
    print("wrote", os.path.abspath(out), sorted(os.listdir(os.path.join(out, "ref"))))


if __name__ == "__main__":
    main()
