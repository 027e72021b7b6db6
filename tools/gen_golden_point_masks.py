"""Generate tests/golden/point_masks.npz by running the REFERENCE's depth_edge / normals_edge and app.py's mask composition
(build container only; no test imports this file).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_point_masks.py

Inputs: piecewise-planar scenes (depth steps and ramps, plane normals plus small noise normalised in fp32, so the
reference's arccos meets self-dots above 1), quantised confidences (ties at the quantile), zero-depth pixels and a fully
masked-out region; three view groups: 3 x 37x52, 2 x 61x83, 1 x 518x518.  The inputs are stored in a compact integer
form (decode() below gives the fp32 arrays, a digest of which is stored) and the masks bit-packed (np.packbits, last axis
flattened), so the fixture stays small.
Cases: depth_edge / normals_edge with k in {3, 5}, with and without a mask, depth with atol and with rtol; app.py's
composition (app.py:172-206) with each of its four flag combinations at the app's defaults (app.py:79-86).
Stored per case: the reference's mask and a boundary band = the pixels whose result changes when the call is re-run at
tol +- 1e-4 degrees and atol / rtol * (1 +- 1e-6): only these may differ through a few-ulp arccos difference.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
from src.utils.geometry import depth_edge, normals_edge  # noqa: E402

rng = np.random.Generator(np.random.Philox(key=[2024, 11]))
PCT, NTOL, DRTOL, DATOL = 10.0, 5.0, 0.03, 0.05   # app.py:79-86 defaults; atol for the standalone depth cases


def scene(S, H, W):
    """Piecewise-planar views in a compact integer form (decode() turns it into the fp32 inputs): plane index per pixel,
    per-plane unit normals, sparse noise of 1/128 on the normals' x, depth in steps of 1/256, confidence in steps of 1/8."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    region = np.empty((S, H, W), np.uint8)
    planes = np.empty((S, 5, 3), np.float32)
    noise = np.empty((S, H, W), np.int8)
    depth_q = np.empty((S, H, W), np.int32)
    conf_q = np.empty((S, H, W), np.uint8)
    mask = np.ones((S, H, W), bool)
    for s in range(S):
        reg = np.zeros((H, W), np.int64)
        for j in range(1, 5):   # four random half-planes painted over each other
            a, b = rng.standard_normal(2)
            c = -(a * rng.uniform(0, W) + b * rng.uniform(0, H))
            reg[a * xx + b * yy + c > 0] = j
        nrm = rng.standard_normal((5, 3))
        nrm[:, 2] = np.abs(nrm[:, 2]) + 0.5
        planes[s] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        base = 1.0 + 3.0 * rng.random(5)
        slope = 0.002 * rng.standard_normal((5, 2))
        d = np.round((base[reg] + slope[reg, 0] * xx + slope[reg, 1] * yy) * 256)
        d[rng.random((H, W)) < 0.02] = 0                                                    # invalid depth
        c = np.repeat(np.repeat(8 + rng.integers(0, 17, ((H + 3) // 4, (W + 3) // 4)), 4, 0), 4, 1)[:H, :W]  # 17 levels in [1, 3], 4x4 blocks: ties
        y0, x0 = rng.integers(0, H - 12), rng.integers(0, W - 14)
        c[y0:y0 + 9, x0:x0 + 11] = 4                                                        # 0.5: below the quantile, fully masked out
        m = np.repeat(np.repeat(rng.random(((H + 1) // 2, (W + 1) // 2)) > 0.15, 2, 0), 2, 1)[:H, :W]
        m[y0 + 1:y0 + 11, x0 + 2:x0 + 14] = False                                           # fully masked region of the input mask
        region[s], depth_q[s], conf_q[s], mask[s] = reg, d, c, m
        noise[s] = rng.choice(np.array([-1] + [0] * 8 + [1], np.int8), (H, W))
    return {"region": region, "planes": planes, "noise": noise, "depth_q": depth_q, "conf_q": conf_q, "mask": mask}


def decode(z, g):
    """The fp32 inputs of view group g (tests/test_point_masks*.py decode the fixture the same way and check the digest).
    Normals are plane + noise renormalised in fp32, so the reference's own normalisation meets self-dots above 1."""
    n = z[f"{g}_planes"][np.arange(len(z[f"{g}_region"]))[:, None, None], z[f"{g}_region"]]
    n[..., 0] += z[f"{g}_noise"].astype(np.float32) * np.float32(1 / 128)
    n = n / (np.linalg.norm(n, axis=-1, keepdims=True) + np.float32(1e-12))
    depth = z[f"{g}_depth_q"].astype(np.float32) * np.float32(1 / 256)
    cq = z[f"{g}_conf_q"]
    conf = np.where(cq == 255, np.float32(np.nan), cq.astype(np.float32) * np.float32(1 / 8))
    return conf, depth, n, z[f"{g}_mask"]


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def ref_normals(normals, tol, k, mask):
    if mask is None:
        return normals_edge(normals, tol=tol, kernel_size=k)
    return np.stack([normals_edge(normals[i], tol=tol, kernel_size=k, mask=mask[i]) for i in range(len(normals))])


def app_mask(conf, depth, normals, apply_conf, apply_edge, ntol=NTOL, drtol=DRTOL):
    """app.py:172-206, per view, in the app's order (depth_preds[i, :, :, 0] is depth[i] here)."""
    out, thr = [], []
    for i in range(conf.shape[0]):
        final_mask = None
        if apply_conf:
            t = np.quantile(conf[i], PCT / 100.0)
            thr.append(t)
            final_mask = conf[i] >= t
        if apply_edge:
            ne = normals_edge(normals[i], tol=ntol, mask=final_mask)
            de = depth_edge(depth[i], rtol=drtol, mask=final_mask)
            edge = ~(de & ne)
            final_mask = edge if final_mask is None else final_mask & edge
        out.append(final_mask)
    if out[0] is None:
        return np.ones(conf.shape, bool), None
    return np.stack(out), np.array(thr, np.float32)


def band(base, *others):
    b = np.zeros_like(base)
    for o in others:
        b |= o != base
    return b


store = {}
for g, (S, H, W) in {"a": (3, 37, 52), "b": (2, 61, 83), "c": (1, 518, 518)}.items():
    enc = scene(S, H, W)
    if g == "a":
        enc["conf_q"][2, 5, 7] = 255    # NaN: numpy's quantile is NaN for that view, its mask is all false
    store.update({f"{g}_{k}": v for k, v in enc.items()})
    conf, depth, normals, mask = decode(store, g)
    assert conf.dtype == depth.dtype == normals.dtype == np.float32
    store[f"{g}_digest"] = np.array(digest(conf, depth, normals, mask))
    for k in (3, 5):
        for mk, m in (("nomask", None), ("mask", mask)):
            for kind, tol in (("atol", DATOL), ("rtol", DRTOL)):
                run = lambda t: depth_edge(depth, kernel_size=k, mask=m, **{kind: t})
                name = f"{g}_depth_k{k}_{mk}_{kind}"
                store["case_" + name] = run(tol)
                store["band_" + name] = band(store["case_" + name], run(tol * (1 + 1e-6)), run(tol * (1 - 1e-6)))
            name = f"{g}_normals_k{k}_{mk}"
            store["case_" + name] = ref_normals(normals, NTOL, k, m)
            store["band_" + name] = band(store["case_" + name], ref_normals(normals, NTOL + 1e-4, k, m),
                                         ref_normals(normals, NTOL - 1e-4, k, m))
    for ac in (0, 1):
        for ae in (0, 1):
            name = f"{g}_app_c{ac}e{ae}"
            res, thr = app_mask(conf, depth, normals, ac, ae)
            store["case_" + name] = res
            store["band_" + name] = band(res, *(app_mask(conf, depth, normals, ac, ae, ntol=t, drtol=r)[0]
                                                for t, r in ((NTOL + 1e-4, DRTOL), (NTOL - 1e-4, DRTOL),
                                                             (NTOL, DRTOL * (1 + 1e-6)), (NTOL, DRTOL * (1 - 1e-6)))))
            if ac:
                store[f"thr_{g}"] = thr
    # share of stage-1 NaNs in the unmasked reference (the path item 2 of csrc/pointmask.hip describes)
    n = normals / (np.linalg.norm(normals, axis=-1, keepdims=True) + 1e-12)
    print(g, "self-dot > 1:", f"{float(((n * n).sum(-1) > 1).mean()):.2f}",
          "edges:", {k[5:]: int(v.sum()) for k, v in store.items() if k.startswith(f"case_{g}_")},
          "band:", sum(int(v.sum()) for k, v in store.items() if k.startswith(f"band_{g}_")))
store["params"] = np.array([PCT, NTOL, DRTOL, DATOL], np.float64)
for k in [k for k in store if k.startswith(("case_", "band_"))]:
    store[k] = np.packbits(store[k].ravel())
out = os.path.join(ROOT, "tests", "golden", "point_masks.npz")
np.savez_compressed(out, **store)
print("wrote", out, os.path.getsize(out) // 1024, "KiB")
