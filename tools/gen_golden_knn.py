"""Writes tests/golden/knn_a.npz: the REFERENCE's own ``knn`` and ``rgb_to_sh`` (submodules/gsplat/examples/utils.py:141-150) and the
scale statements of its create_splats_with_optimizers (simple_trainer_worldmirror.py:335-337) on one 3000-point fp32 cloud.  Data only.

    python tools/gen_golden_knn.py <reference root>

examples/utils.py is executed from its file into a private module (matplotlib, which it imports for its colour maps, is replaced by an
empty stand-in when it is not installed); nothing of it is copied.  scikit-learn must be installed: it IS the reference's knn.

The cloud (seed 20261020, shuffled): 1500 normal points, sigma 0.05, around (1, 2, 3); 1200 uniform points in [-2, 2]^3; 290 normal points,
sigma 50; 10 copies of (1000, -1000, 500); then 5 further rows overwritten with row 0.  Dense cluster, sparse field, far outliers and
duplicates in one bounding box.

Recorded: points [3000,3] f32; dist64_k16: scikit-learn's kneighbors(K = 16) on the fp32-valued cloud widened to fp64 (fp64 distances; its
first 4 columns are asserted equal to the K = 4 call, which is therefore not stored twice); knn4_ref: the reference's knn(points, 4)
(fp32); scales_1, scales_05: column 0 of the statements of :335-337 on knn4_ref at init_scale 1.0 and 0.5 (the three columns are one
value repeated, asserted); dup_rows: the 16 rows that have a duplicate (the 10 copies, row 0 and the 5 rows overwritten with it);
rgb [256,3] f32 in [0,1] and sh = rgb_to_sh(rgb); brute_err: max |dist64_k16 - fp64 brute force| (asserted below 1e-12: on this cloud
scikit-learn picks its kd-tree and is exact to rounding)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference_utils(ref_root):
    path = os.path.join(ref_root, "submodules", "gsplat", "examples", "utils.py")
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.colormaps = {}
        sys.modules["matplotlib"] = mpl
        sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
    spec = importlib.util.spec_from_file_location("_reference_examples_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference_utils(sys.argv[1])
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(20261020)
    pts = np.concatenate([rng.normal(0.0, 0.05, (1500, 3)) + np.array([1.0, 2.0, 3.0]), rng.uniform(-2.0, 2.0, (1200, 3)),
                          rng.normal(0.0, 50.0, (290, 3)), np.tile(np.array([1000.0, -1000.0, 500.0]), (10, 1))]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    over = rng.choice(np.arange(1, len(pts)), 5, replace=False)
    over = over[~np.all(pts[over] == np.array([1000.0, -1000.0, 500.0], np.float32), axis=1)]
    assert len(over) == 5, "an overwritten row was one of the 10 copies: change the seed"
    pts[over] = pts[0]
    far = np.flatnonzero(np.all(pts == np.array([1000.0, -1000.0, 500.0], np.float32), axis=1))
    dup_rows = np.sort(np.concatenate([far, over, [0]]))
    assert len(far) == 10 and len(dup_rows) == 16

    x64 = pts.astype(np.float64)
    model = NearestNeighbors(n_neighbors=16, metric="euclidean").fit(x64)
    d16, _ = model.kneighbors(x64)
    d4, _ = NearestNeighbors(n_neighbors=4, metric="euclidean").fit(x64).kneighbors(x64)
    print("scikit-learn's method:", model._fit_method)
    diff = x64[:, None, :] - x64[None, :, :]
    brute = np.sort(np.sqrt((diff ** 2).sum(-1)), axis=1)[:, :16]
    brute_err = float(np.abs(brute - d16).max())
    print("max |scikit-learn fp64 - fp64 brute force|:", brute_err)
    assert brute_err < 1e-12 and np.array_equal(d16[:, :4], d4)

    points = torch.from_numpy(pts)
    knn4 = ref.knn(points, 4)
    assert knn4.dtype == torch.float32

    def scales(init_scale):      # simple_trainer_worldmirror.py:335-337
        dist2_avg = (knn4[:, 1:] ** 2).mean(dim=-1)
        dist_avg = torch.sqrt(dist2_avg)
        s = torch.log(dist_avg * init_scale).unsqueeze(-1).repeat(1, 3)
        assert s.shape == (len(pts), 3) and torch.equal(s[:, 0], s[:, 1]) and torch.equal(s[:, 0], s[:, 2])
        return s[:, 0].contiguous()

    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, (256, 3)).astype(np.float32))
    sh = ref.rgb_to_sh(rgb)
    out = os.path.join(ROOT, "tests", "golden", "knn_a.npz")
    np.savez_compressed(out, points=pts, dist64_k16=d16, knn4_ref=knn4.numpy(), scales_1=scales(1.0).numpy(),
                        scales_05=scales(0.5).numpy(), dup_rows=dup_rows.astype(np.int64), rgb=rgb.numpy(), sh=sh.numpy(),
                        brute_err=np.float64(brute_err))
    print(out, os.path.getsize(out), "bytes; -inf scales:", int(np.isinf(scales(1.0).numpy()).sum()))


if __name__ == "__main__":
    main()
