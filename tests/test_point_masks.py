"""GPU: point-cloud filter masks (csrc/pointmask.hip) against the reference's own depth_edge / normals_edge and app.py's
composition (tests/golden/point_masks.npz, written by tools/gen_golden_point_masks.py from the reference)."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

GROUPS = "abc"


def load_fixture():
    """tests/golden/point_masks.npz decoded: fp32 inputs <g>_conf / _depth / _normals and the bool <g>_mask per view group g,
    case_* / band_* as bool [S, H, W], thr_<g>, params.  The inputs are stored in a compact integer form and rebuilt exactly
    as tools/gen_golden_point_masks.py decode() builds them (checked against the stored digest); the masks are bit-packed."""
    z = dict(np.load(os.path.join(GOLD, "point_masks.npz")))
    out = {"params": z["params"]}
    for g in GROUPS:
        region = z[f"{g}_region"]
        n = z[f"{g}_planes"][np.arange(len(region))[:, None, None], region]
        n[..., 0] += z[f"{g}_noise"].astype(np.float32) * np.float32(1 / 128)
        n = n / (np.linalg.norm(n, axis=-1, keepdims=True) + np.float32(1e-12))
        depth = z[f"{g}_depth_q"].astype(np.float32) * np.float32(1 / 256)
        cq = z[f"{g}_conf_q"]
        conf = np.where(cq == 255, np.float32(np.nan), cq.astype(np.float32) * np.float32(1 / 8))
        mask = z[f"{g}_mask"]
        h = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (conf, depth, n, mask))).hexdigest()
        assert h == str(z[f"{g}_digest"]), f"decoded inputs of group {g} differ from the generator's"
        out.update({f"{g}_conf": conf, f"{g}_depth": depth, f"{g}_normals": n, f"{g}_mask": mask, f"thr_{g}": z[f"thr_{g}"]})
        for k, v in z.items():
            if k.startswith((f"case_{g}_", f"band_{g}_")):
                out[k] = np.unpackbits(v, count=region.size).astype(bool).reshape(region.shape)
    return out


@pytest.fixture(scope="module")
def Z():
    return load_fixture()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_case(Z, name):
    """The GPU result of one fixture case (key without the case_ prefix)."""
    from hunyuanworld_mirror_amd import depth_edge, filter_points_mask, normals_edge
    pct, ntol, drtol, datol = (float(x) for x in Z["params"])
    g, kind = name.split("_", 2)[:2]
    conf, depth, normals, mask = (_cuda(Z[f"{g}_{t}"]) for t in ("conf", "depth", "normals", "mask"))
    parts = name.split("_")
    if kind == "app":
        ac, ae = int(parts[2][1]), int(parts[2][3])
        return filter_points_mask(conf, depth, normals, pct, ntol, drtol, bool(ac), bool(ae))
    k = int(parts[2][1])
    m = mask if parts[3] == "mask" else None
    if kind == "depth":
        tol = {"atol": datol, "rtol": drtol}[parts[4]]
        return depth_edge(depth, kernel_size=k, mask=m, **{parts[4]: tol})
    return normals_edge(normals, ntol, kernel_size=k, mask=m)


def case_names(Z):
    return sorted(k[5:] for k in Z if k.startswith("case_"))


def test_every_case_matches_the_reference_outside_the_boundary_band(Z):
    names = case_names(Z)
    assert len(names) == 3 * 16
    bad = {}
    for name in names:
        got = run_case(Z, name).cpu().numpy()
        ref, band = Z["case_" + name], Z["band_" + name]
        assert got.shape == ref.shape and got.dtype == np.bool_, (name, got.shape, got.dtype)
        off = int(((got != ref) & ~band).sum())
        if off:
            bad[name] = off
        if "_depth_" in name:   # max / min / add / correctly rounded divide: no arccos, exact everywhere
            assert (got == ref).all(), name
    assert not bad, bad


def test_thresholds_are_bit_exact(Z):
    from hunyuanworld_mirror_amd import filter_points_mask
    pct, ntol, drtol, _ = (float(x) for x in Z["params"])
    for g in GROUPS:
        _, thr = filter_points_mask(_cuda(Z[f"{g}_conf"]), _cuda(Z[f"{g}_depth"]), _cuda(Z[f"{g}_normals"]), pct, ntol, drtol,
                                    return_thresholds=True)
        got, ref = thr.cpu().numpy(), Z[f"thr_{g}"]
        nan = np.isnan(ref)
        assert (np.isnan(got) == nan).all(), (g, got, ref)
        assert (got[~nan].view(np.uint32) == ref[~nan].view(np.uint32)).all(), (g, got, ref)
    assert np.isnan(Z["thr_a"][2])   # the fixture's NaN view: its mask is all false
    assert not Z["case_a_app_c1e1"][2].any()


@pytest.mark.parametrize("pct", [0.0, 10.0, 33.3, 50.0, 99.99, 100.0])
def test_thresholds_match_numpy_quantile_on_random_views(pct):
    from hunyuanworld_mirror_amd import filter_points_mask
    g = torch.Generator().manual_seed(int(pct * 100))
    conf = torch.rand(3, 45, 67, generator=g) * 5
    conf[1] = torch.round(conf[1] * 4) / 4    # ties
    conf[2, :20] = -conf[2, :20]              # negatives, and -0 / +0
    conf[2, 0, :5] = 0.0
    conf[2, 0, 5:9] = -0.0
    z = torch.zeros(3, 45, 67, 3)
    _, thr = filter_points_mask(conf.cuda(), z[..., 0].cuda(), z.cuda(), pct, apply_edge_mask=False, return_thresholds=True)
    ref = np.array([np.quantile(conf[i].numpy(), pct / 100.0) for i in range(3)], np.float32)
    assert (thr.cpu().numpy() == ref).all(), (thr.cpu().numpy(), ref)


def test_masks_are_bit_identical_across_runs(Z):
    for name in case_names(Z):
        a = run_case(Z, name).cpu().numpy()
        b = run_case(Z, name).cpu().numpy()
        assert (a == b).all(), name


def test_k7_and_invalid_kernel_sizes(Z):
    from hunyuanworld_mirror_amd import depth_edge, normals_edge
    dn = Z["b_depth"]
    d, n = _cuda(dn), _cuda(Z["b_normals"])
    # k = 7 depth edges against numpy: max - min over the clipped 7 x 7 window, compared in fp32
    S, H, W = dn.shape
    P = np.full((S, H + 6, W + 6), np.nan, np.float32)
    P[:, 3:-3, 3:-3] = dn
    win = np.stack([P[:, p:p + H, q:q + W] for p in range(7) for q in range(7)])
    ref = (np.nanmax(win, 0) + np.nanmax(-win, 0)) > np.float32(0.05)
    assert np.array_equal(depth_edge(d, atol=0.05, kernel_size=7).cpu().numpy(), ref)
    m7 = normals_edge(n, 5.0, kernel_size=7)
    assert m7.shape == (S, H, W) and m7.any()
    for k in (1, 4, 9):
        with pytest.raises(ValueError):
            depth_edge(d, atol=0.05, kernel_size=k)


def test_full_size_fused_equals_per_view_calls_and_throughput():
    """32 x 518^2 in the forward's own shapes: the fused call equals 32 per-view standalone calls (conf mask from the same
    quantile, then depth_edge / normals_edge with that mask, composed as app.py does)."""
    from hunyuanworld_mirror_amd import depth_edge, filter_points_mask, normals_edge
    S, H, W = 32, 518, 518
    g = torch.Generator().manual_seed(7)
    conf = (1 + torch.round(torch.rand(1, S, H, W, generator=g) * 32) / 8).cuda()
    yy = torch.arange(H).view(H, 1).float()
    depth = (1 + 0.002 * yy + (torch.arange(W).view(1, W) > W // 2).float() + 0.01 * torch.rand(S, H, W, generator=g))
    depth = depth.view(1, S, H, W, 1).cuda()
    nrm = torch.randn(1, S, 1, 1, 3, generator=g) + 0.03 * torch.randn(1, S, H, W, 3, generator=g)
    nrm[:, :, :, W // 2:] += torch.tensor([0.5, 0.0, 0.0])   # a crease on the depth step
    nrm = (nrm / (nrm.norm(dim=-1, keepdim=True) + 1e-12)).cuda()
    fused, thr = filter_points_mask(conf, depth, nrm, return_thresholds=True)
    assert fused.shape == (S, H, W)
    kept = 0
    for i in range(S):
        cm, ti = filter_points_mask(conf[0, i:i + 1], depth[0, i:i + 1], nrm[0, i:i + 1], apply_edge_mask=False,
                                    return_thresholds=True)
        assert ti.view(torch.int32).item() == thr[i:i + 1].view(torch.int32).item()
        cm = cm[0]
        kept += int(cm.sum())
        ne = normals_edge(nrm[0, i], 5.0, mask=cm)
        de = depth_edge(depth[0, i, :, :, 0], rtol=0.03, mask=cm)
        assert torch.equal(fused[i], cm & ~(de & ne)), i
    assert 0.5 * S * H * W < int(fused.sum()) < kept   # the confidence mask keeps most points, the crease removes some
    # timing: median of 30 event-timed fused calls after a warm-up
    for _ in range(5):
        filter_points_mask(conf, depth, nrm)
    ts = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        filter_points_mask(conf, depth, nrm)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    us = float(np.median(ts))
    nbytes = S * H * W * (4 * 4 + 4 + 4 + 12 + 1)   # 4 select passes over conf + conf, depth, normals in, mask out
    print(f"filter_points_mask 32x518^2: {us:.1f} us median (incl. Python binding), {nbytes / us / 1e3:.0f} GB/s nominal")
