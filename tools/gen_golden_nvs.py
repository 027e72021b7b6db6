"""Writes tests/golden/nvs_*.npz: the REFERENCE's own novel-view arithmetic run on the CPU.  Data only: inputs and recorded results.

    python tools/gen_golden_nvs.py <reference root>

Nothing of the reference is copied or imported as a package (rasterization.py imports gsplat, which is CUDA-only):
  * src/models/utils/frustum.py is parsed with `ast`; the one obstacle to an fp64 run, the pixel grid of unproject_depth that is
    hard-wired to torch.float32, is patched to follow `depth.dtype`, and the module's source is executed in a fresh namespace.  Its
    calculate_in_frustum_mask then runs in fp64 (`mask64`, the golden) and in fp32 (`mask32`, the reference as shipped).
  * apply_confidence_filter and the scale-factor statements of render (rasterization.py:248-299, :194-202) are cut out of the class
    with `ast`, compiled on their own and called with a stub `self`.

Mask scenes a..d, (B, V1, V2, H, W) = (2,3,2,37,45), (1,2,3,19,70), (1,1,1,5,7), (1,1,2,16,16): a wavy wall at z ~ 3 seen from cameras on a
small arc (yaw within +-0.45 rad, focal 0.9 w), depths by fixed-point ray marching and rounded to fp32, a block of zero depth in one
corner of every view, and a patch scaled by 0.55 in the first context view and in the first target view (an occluder only that view
sees).  Per pixel the file also holds `marginal` (tests/nvs_helper.py marginal_pixels, fp64); a scene may hold at most 0.1 % of them.
Hand-built scenes: hand_split (8 x 8, two context views: the column x = 1 lies inside view A's frustum only and matches only in view B,
through a sample whose footprint hangs over B's left border) and hand_nan (NaN in depth_1 and in depth_2)."""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nvs_helper as NH  # noqa: E402


# ------------------------------------------------------------------------------------------------ the reference's code, by ast
def load_frustum(ref_root):
    path = os.path.join(ref_root, "src", "models", "utils", "frustum.py")
    tree = ast.parse(open(path).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "unproject_depth")
    patched = 0
    for call in ast.walk(fn):
        if isinstance(call, ast.Call) and ast.unparse(call.func) == "torch.arange":
            for kw in call.keywords:
                if kw.arg == "dtype":
                    assert ast.unparse(kw.value) == "torch.float32"
                    kw.value = ast.parse("depth.dtype", mode="eval").body
                    patched += 1
    assert patched == 2, patched
    ns = {"__name__": "reference_frustum"}
    exec(compile(ast.fix_missing_locations(tree), path, "exec"), ns)
    return ns


def load_renderer_parts(ref_root):
    path = os.path.join(ref_root, "src", "models", "models", "rasterization.py")
    tree = ast.parse(open(path).read())
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "GaussianSplatRenderer")
    filt = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "apply_confidence_filter")
    ns = {"torch": torch, "np": np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[filt], type_ignores=[])), path, "exec"), ns)
    render = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "render")
    stmts = [n for n in render.body if (isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) in ("scale_factor", "pred_all_extrinsic[..., :3, 3]"))
             or (isinstance(n, ast.If) and ast.unparse(n.test) == "context_predictions is not None")]
    assert [type(n).__name__ for n in stmts] == ["Assign", "If", "Assign"], [ast.unparse(n)[:60] for n in stmts]
    scale_code = compile(ast.fix_missing_locations(ast.Module(body=stmts, type_ignores=[])), path, "exec")
    return ns["apply_confidence_filter"], scale_code


# ------------------------------------------------------------------------------------------------ mask scenes
def wall(x, y, phase):
    return 3.0 + 0.15 * np.sin(2.1 * x + phase) * np.cos(1.7 * y - 0.5 * phase)


def camera(a, k):
    """camera k of the arc at parameter a in [-1, 1]: (c2w [4,4], yaw)"""
    cx = 1.4 * a
    yaw = -np.arctan2(cx, 3.0)                                  # looks back at the wall's centre: |yaw| <= 0.437
    c, s = np.cos(yaw), np.sin(yaw)
    m = np.eye(4)
    m[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    m[:3, 3] = [cx, 0.06 * (k % 3 - 1), 0.13 * a * a]
    return m.astype(np.float32).astype(np.float64), yaw


def march(c2w, K, h, w, phase):
    """z-depth of the wall along every pixel's ray, by fixed-point iteration (the wall's slope is < 0.32: a contraction)"""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.einsum("ij,hwj->hwi", np.linalg.inv(K), np.stack([xs, ys, np.ones_like(xs)], -1))
    dw = np.einsum("ij,hwj->hwi", c2w[:3, :3], d)
    t = np.full((h, w), 3.0)
    for _ in range(60):
        p = c2w[:3, 3] + t[..., None] * dw
        t = (wall(p[..., 0], p[..., 1], phase) - c2w[2, 3]) / dw[..., 2]
    return t


def mask_scene(B, V1, V2, h, w, seed):
    rng = np.random.default_rng(seed)
    n = V1 + V2
    K = np.array([[0.9 * w, 0, w / 2], [0, 0.9 * w, h / 2], [0, 0, 1]], np.float32).astype(np.float64)
    depth, poses, yaws = np.zeros((B, n, h, w)), np.zeros((B, n, 4, 4)), []
    for b in range(B):
        a = np.linspace(-1.0, 1.0, n)[rng.permutation(n)]
        phase = 0.7 * b + rng.uniform(0.0, 3.0)
        for k in range(n):
            poses[b, k], yaw = camera(a[k], k)
            yaws.append(yaw)
            depth[b, k] = march(poses[b, k], K, h, w, phase)
    assert max(abs(y) for y in yaws) <= 0.45
    depth[..., :max(h // 5, 1), :max(w // 6, 1)] = 0.0                                         # the zero block
    for k in (0, V2):                                                                          # the occluder of one view
        y0, x0 = h // 3 + (k > 0), w // 2 - (k > 0) * (w // 4)
        depth[:, k, y0:y0 + max(h // 4, 1), x0:x0 + max(w // 5, 1)] *= 0.55
    depth = depth.astype(np.float32)
    Ks = np.broadcast_to(K.astype(np.float32), (B, n, 3, 3)).copy()
    poses = poses.astype(np.float32)
    return {"depth_1": depth[:, V2:], "K1": Ks[:, V2:], "c2w_1": poses[:, V2:], "depth_2": depth[:, :V2], "K2": Ks[:, :V2], "c2w_2": poses[:, :V2]}


def hand_scenes():
    h = w = 8
    K = np.array([[8, 0, 4], [0, 8, 4], [0, 0, 1]], np.float32)[None, None]
    eye = np.eye(4, dtype=np.float32)
    shifted = eye.copy()
    shifted[0, 3] = 0.3125                               # view B: px_B = px - 8 * 0.3125 / 2 = px - 1.25 at depth 2
    d1 = np.full((1, 1, h, w), 2.0, np.float32)
    d2 = np.full((1, 2, h, w), 5.0, np.float32)          # view A (= the target's pose): depth 5 matches nothing
    d2[0, 1, :, 0] = 8.0                                 # view B: the pixels x = 1 sample 0.25 * 8 = 2 from beyond its left border
    base = {"depth_1": d1, "K1": K.copy(), "c2w_1": eye[None, None].copy(), "depth_2": d2, "K2": np.repeat(K, 2, 1),
            "c2w_2": np.stack([eye, shifted])[None]}
    nan = {k: v.copy() for k, v in base.items()}
    nan["depth_2"][0, 0] = 2.0                           # view A now matches everywhere ...
    nan["depth_2"][0, 0, 5, 5] = np.nan                  # ... but where a sample touches this pixel
    nan["depth_1"][0, 0, 3, 3] = np.nan
    return {"hand_split": base, "hand_nan": nan}


def run_mask(fr, sc, name, limit):
    out = dict(sc)
    for dt, key in ((torch.float64, "mask64"), (torch.float32, "mask32")):
        t = [torch.from_numpy(sc[k]).to(dt) for k in ("depth_1", "K1", "c2w_1", "depth_2", "K2", "c2w_2")]
        m = fr["calculate_in_frustum_mask"](*t)
        assert m.shape == sc["depth_1"].shape and m.dtype == torch.bool
        out[key] = m.numpy()
    t32 = NH.scene_tensors(sc)
    out["marginal"] = NH.marginal_pixels(*t32).numpy()
    with torch.no_grad():
        _, z = NH.project(*(x.double() for x in (t32[0], t32[1], t32[2], t32[4], t32[5])))
    n_marg, n = int(out["marginal"].sum()), out["marginal"].size
    diff = int(((out["mask64"] != out["mask32"]) & ~out["marginal"]).sum())
    print(f"nvs_{name}: {tuple(sc['depth_1'].shape)} + {sc['depth_2'].shape[1]} views, mask true {out['mask64'].mean():.1%}, marginal {n_marg} of {n}, "
          f"points behind a camera {int((z < 0).sum())}, fp32 reference differs from fp64 off the marginal pixels on {diff}")
    if limit:
        assert n_marg <= NH.MAX_MARGINAL * n, (name, n_marg, n)
        assert 0.15 < out["mask64"].mean() < 0.95, name       # both outcomes well represented
    assert diff == 0, name
    np.savez_compressed(os.path.join(NH.GOLD, f"nvs_{name}.npz"), **out)
    return out


# ------------------------------------------------------------------------------------------------ filter and scale factor
def filter_cases(ref_filter):
    rng = np.random.default_rng(5)
    cases = {}
    for name, (B, N, p, cap) in {"p30": (2, 1000, 30.0, 5_000_000), "p0": (1, 257, 0.0, 5_000_000), "cap": (2, 4099, 30.0, 100),
                                 "k1": (1, 700, 99.99, 5_000_000), "p333": (1, 1000, 33.3, 5_000_000)}.items():
        conf = (rng.permutation(B * N).reshape(B, N).astype(np.float32) + 1.0) / 64.0       # distinct, > 1e-5
        low = rng.random((B, N)) < 0.1
        conf = np.where(low, conf * 1e-9, conf).astype(np.float32)                          # a tenth counts as -inf (never among the kept here)
        assert len(np.unique(conf[~low])) == (~low).sum()
        idx = np.broadcast_to(np.arange(N, dtype=np.float64), (B, N))
        splats = {"means": torch.from_numpy(np.stack([idx] * 3, -1).copy()), "weights": torch.from_numpy(idx.copy()), "extra": torch.zeros(3)}
        me = types.SimpleNamespace(enable_conf_filter=True, conf_threshold_percent=p, max_gaussians=cap)
        got = ref_filter(me, splats, torch.from_numpy(conf))
        kept = np.sort(got["means"][..., 0].numpy().astype(np.int64), axis=1)
        assert got["extra"] is splats["extra"] and np.array_equal(np.sort(got["weights"].numpy().astype(np.int64), 1), kept)
        assert kept.shape[1] == N or kept.shape[1] <= (~low).sum(1).min(), "the kept set must be unambiguous"
        assert np.array_equal(kept, NH.filter_indices(conf, p, cap)), name
        cases[name + "_conf"], cases[name + "_kept"], cases[name + "_params"] = conf, kept, np.array([p, cap], np.float64)
        print(f"nvs_filter {name}: B {B} N {N} p {p} cap {cap} -> K {kept.shape[1]}")
    np.savez_compressed(os.path.join(NH.GOLD, "nvs_filter.npz"), **cases)


def scale_case(scale_code):
    rng = np.random.default_rng(9)
    B, S, V = 2, 3, 2
    def poses(n, s):
        m = np.tile(np.eye(4), (B, n, 1, 1))
        m[..., :3, 3] = rng.normal(0.2, s, (B, n, 3))
        return m.astype(np.float32)
    all_c2w, ctx_c2w = poses(S + V, 0.5), poses(S, 0.8)
    stub = types.SimpleNamespace(prepare_prediction_cameras=lambda preds, nums, hw: (preds.reshape(-1, 4, 4), None))
    pa = torch.from_numpy(all_c2w).double()
    ns = {"self": stub, "context_predictions": torch.from_numpy(ctx_c2w).double(), "S": S, "H": 8, "W": 8, "Bx": B, "pred_all_extrinsic": pa,
          "pred_all_source_extrinsic": pa[:, :S]}
    exec(scale_code, ns)
    sf = ns["scale_factor"].numpy()
    mine = NH.translation_scale(torch.from_numpy(ctx_c2w).double(), torch.from_numpy(all_c2w).double(), S).numpy()
    assert sf.shape == (B, 1, 1) and np.abs(sf - mine).max() <= 4 * np.finfo(np.float64).eps * np.abs(sf).max()
    print("nvs_scale: factors", sf.ravel())
    np.savez_compressed(os.path.join(NH.GOLD, "nvs_scale.npz"), all_c2w=all_c2w, ctx_c2w=ctx_c2w, S=np.int64(S), scale_factor=sf,
                        scaled_c2w=ns["pred_all_extrinsic"].numpy())


def main():
    ref_root = sys.argv[1]
    fr = load_frustum(ref_root)
    ref_filter, scale_code = load_renderer_parts(ref_root)
    # (shape, seed): the seed draws the camera order and the wall's phase; these four keep the share of marginal pixels under the limit
    # that run_mask asserts (scene d, 256 pixels, may hold none), and a and b put the zero block's points behind a context camera
    shapes = {"a": ((2, 3, 2, 37, 45), 3), "b": ((1, 2, 3, 19, 70), 5), "c": ((1, 1, 1, 5, 7), 5), "d": ((1, 1, 2, 16, 16), 1)}
    for name, (shp, seed) in shapes.items():
        run_mask(fr, mask_scene(*shp, seed=seed), name, limit=True)
    for name, sc in hand_scenes().items():
        out = run_mask(fr, sc, name, limit=False)
        if name == "hand_split":      # the column x = 1 (rows 1..7) is true through the two independent any, and robustly so
            assert out["mask64"][0, 0, 1:, 1].all() and not out["marginal"][0, 0, 1:, 1].any()
            assert not out["mask64"][0, 0, :, 2:].any() and not out["marginal"][0, 0, 1:, 2:].any()
        else:
            assert not out["mask64"][0, 0, 3, 3] and not out["mask64"][0, 0, 5:7, 5:7].any() and out["mask64"][0, 0, 4, 4]
            assert not out["marginal"][0, 0, 1:, 1:].any()
    filter_cases(ref_filter)
    scale_case(scale_code)


if __name__ == "__main__":
    main()
