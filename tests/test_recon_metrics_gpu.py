"""GPU: hunyuanworld_mirror_amd.recon_metrics (csrc/knn.hip wm_nearest_*, csrc/reconmetrics.hip) against the brute-force restatements of
tests/recon_metrics_helper.py (checked by hand in tests/test_recon_metrics_cpu.py).

    nearest      idx equal on every row (the lowest row attaining the minimum fp32 square), dist within 1 fp32 ulp of the fp32 square root of
                 the helper's fp32 minimum square (both are the same correctly rounded operations, so the expected difference is 0)
    statistics   means within 2 2^-24 relative (each term may be 1 ulp off, the fp64 sum adds nothing visible), medians within 1 fp32 ulp,
                 threshold counts exact (no helper distance within 4 ulp of a threshold: asserted), |n . n'| within 8 2^-24 absolute
    umeyama      max|dR|, |ds| / s <= 1e-10, |dt| <= 1e-10 extent against numpy's fp64 SVD on the same fp32 inputs, for P <= 1e4 and a covariance
                 whose second singular value is at least 0.1 of the first (asserted): P 2^-53 ~ 1.2e-12 times that conditioning leaves ~ 10
    icp          the final transform within 4 e32 of the helper's fp64 run (floor 1e-6), e32 = the helper's own fp32 run against its fp64 run
Every figure is printed in front of its assertion."""
import numpy as np
import pytest
import torch

import recon_metrics_helper as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gpu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _rotation(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


# ------------------------------------------------------------------------------------------------ clouds
def _ref_cloud(kind, N, rng):
    if kind == "uniform":
        return rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    if kind == "dup":          # N copies of one point: a box without extent
        return np.repeat(np.array([[0.25, -3.0, 7.5]], np.float32), N, 0)
    if kind == "blobs":          # two blobs of the same count, 10 x the width: 10^3 x the density
        a = rng.normal(0, 0.01, (N // 2, 3)) + [1.0, 0.0, 0.0]
        b = rng.normal(0, 0.1, (N - N // 2, 3)) - [1.0, 0.0, 0.0]
        return np.concatenate([a, b]).astype(np.float32)
    if kind == "plane":
        p = rng.uniform(-1, 1, (N, 3))
        p[:, 2] = 0.5
        return (p @ _rotation([1, 1, 0], 30.0).T).astype(np.float32)
    if kind == "lattice":          # 9^3 sites for N points: duplicates and exact ties everywhere
        return rng.integers(0, 9, (N, 3)).astype(np.float32)
    if kind == "onecell":          # all but one point inside one finest cell (2^-21 of the extent the outlier spans)
        p = 1.0 + rng.integers(0, 8, (N, 3)) * 2.0 ** -23
        p[N // 2] = [100.0, 100.0, 100.0]
        return p.astype(np.float32)
    raise KeyError(kind)


def _queries(kind, M, ref, rng):
    lo, hi = ref.min(0).astype(np.float64), ref.max(0).astype(np.float64)
    ext = max(float((hi - lo).max()), 1e-3)
    if kind == "near":          # in and a little around the box
        return (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (M, 3)) + rng.normal(0, 0.01 * ext, (M, 3)) * (hi == lo)).astype(np.float32)
    if kind == "same":          # reference points themselves: distance exactly 0
        return ref[rng.integers(0, len(ref), M)].copy()
    if kind == "far":          # 10^3 extents outside the box, in all directions
        d = rng.normal(size=(M, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return ((lo + hi) / 2 + 1e3 * ext * d + rng.uniform(-ext, ext, (M, 3))).astype(np.float32)
    if kind == "faces":          # one coordinate exactly on a face of the box
        q = (lo + (hi - lo) * rng.uniform(0, 1, (M, 3))).astype(np.float32)
        ax, side = rng.integers(0, 3, M), rng.integers(0, 2, M)
        q[np.arange(M), ax] = np.where(side == 0, ref.min(0)[ax], ref.max(0)[ax])
        return q
    if kind == "halves":          # lattice sites and their midpoints: exact ties between 2, 4 or 8 rows
        return (rng.integers(0, 17, (M, 3)) * 0.5).astype(np.float32)
    raise KeyError(kind)


# (cloud, N, queries, M): N over 1, 2 (duplicates), 63, 64, 65, 255, 257, 5 000, 20 000 and M over 1, 65, 1 000, 20 000; not a full cross
NEAREST_CASES = [
    ("uniform", 1, "near", 1), ("uniform", 1, "far", 65), ("dup", 2, "near", 65), ("dup", 2, "same", 1),
    ("uniform", 63, "near", 1000), ("uniform", 64, "faces", 65), ("uniform", 65, "same", 65), ("uniform", 255, "far", 1000),
    ("uniform", 257, "faces", 1000), ("uniform", 5000, "near", 1000), ("uniform", 5000, "far", 1000), ("uniform", 5000, "same", 1000),
    ("blobs", 5000, "near", 1000), ("blobs", 5000, "far", 65), ("plane", 5000, "near", 1000), ("plane", 5000, "faces", 1000),
    ("lattice", 5000, "halves", 1000), ("lattice", 255, "same", 1000), ("onecell", 257, "near", 65), ("onecell", 5000, "same", 1000),
    ("dup", 257, "near", 65), ("uniform", 20000, "near", 20000),
]


def _case(cloud, N, queries, M):
    rng = np.random.default_rng(N * 7919 + M * 31 + len(cloud) + 3 * len(queries))
    ref = _ref_cloud(cloud, N, rng)
    return ref, _queries(queries, M, ref, rng)


def _check_nearest(dist, idx, q, ref, what):
    d2, want = H.nearest_bruteforce(q, ref)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert dist.dtype == np.float32 and idx.dtype == np.int32 and dist.shape == (len(q),) and idx.shape == (len(q),)
    wrong = int((idx != want).sum())
    root = np.sqrt(d2)          # fp32, correctly rounded
    ulps = np.abs(dist.astype(np.float64) - root.astype(np.float64)) / H.ulp32(root)
    worst = float(ulps.max()) if len(q) else 0.0
    print(f"[recon_metrics] nearest {what}: wrong rows {wrong} of {len(q)}, dist error {worst:.2f} ulp (bound 1)")
    assert wrong == 0, np.nonzero(idx != want)[0][:10]
    assert worst <= 1.0


@pytest.mark.parametrize("cloud,N,queries,M", NEAREST_CASES)
def test_nearest_matches_bruteforce(cloud, N, queries, M):
    from hunyuanworld_mirror_amd import nearest
    ref, q = _case(cloud, N, queries, M)
    dist, idx = nearest(_gpu(q), _gpu(ref))
    _check_nearest(dist, idx, q, ref, f"{cloud} N={N} {queries} M={M}")
    if queries == "same":
        assert float(dist.abs().max()) == 0.0


def test_nearest_nonfinite_rows_repeat_strides_and_reuse():
    from hunyuanworld_mirror_amd import NearestIndex, nearest
    ref, q = _case("uniform", 5000, "near", 1000)
    index = NearestIndex(_gpu(ref))
    d0, i0 = index.query(_gpu(q))
    # a NaN or infinite query row answers NaN and -1 and disturbs nothing else
    bad = q.copy()
    rows = [0, 17, 64, 999]
    bad[0, 0], bad[17, 1], bad[64, 2], bad[999] = np.nan, np.inf, -np.inf, np.nan
    d1, i1 = index.query(_gpu(bad))
    keep = np.ones(len(q), bool)
    keep[rows] = False
    keep = torch.as_tensor(keep, device=DEV)
    assert bool(torch.isnan(d1[rows]).all()) and i1[rows].tolist() == [-1] * 4
    assert torch.equal(d1[keep], d0[keep]) and torch.equal(i1[keep], i0[keep])
    # a non-finite ref raises, as knn does
    for v in (np.nan, np.inf):
        r = ref.copy()
        r[1234, 1] = v
        with pytest.raises(ValueError):
            NearestIndex(_gpu(r))
        with pytest.raises(ValueError):
            nearest(_gpu(q), _gpu(r))
    # without the check nothing raises and every row answers NaN and -1
    r = ref.copy()
    r[7, 0] = np.nan
    dn, iN = NearestIndex(_gpu(r), check=False).query(_gpu(q))
    assert bool(torch.isnan(dn).all()) and bool((iN == -1).all())
    # the same input gives the same bits, from the same index and from a fresh one
    d2, i2 = index.query(_gpu(q))
    d3, i3 = nearest(_gpu(q), _gpu(ref))
    assert torch.equal(d0, d2) and torch.equal(i0, i2) and torch.equal(d0, d3) and torch.equal(i0, i3)
    # a strided or sliced input equals its contiguous copy
    wide = torch.zeros(len(q), 7, device=DEV)
    wide[:, 2:5] = _gpu(q)
    ds, is_ = index.query(wide[:, 2:5])
    assert torch.equal(ds, d0) and torch.equal(is_, i0)
    rwide = torch.zeros(2 * len(ref), 3, device=DEV)
    rwide[::2] = _gpu(ref)
    dr, ir = NearestIndex(rwide[::2]).query(_gpu(q)[100:300])
    assert torch.equal(dr, d0[100:300]) and torch.equal(ir, i0[100:300])
    # one index queried with another M gives the rows of a fresh build
    da, ia = index.query(_gpu(q[:65]))
    db, ib = NearestIndex(_gpu(ref)).query(_gpu(q[:65]))
    assert torch.equal(da, d0[:65]) and torch.equal(ia, i0[:65]) and torch.equal(da, db) and torch.equal(ia, ib)
    # an empty query is an empty answer
    de, ie = index.query(torch.zeros(0, 3, device=DEV))
    assert de.shape == (0,) and ie.shape == (0,)
    _check_nearest(d0, i0, q, ref, "uniform N=5000 near M=1000 (shared index)")


# ------------------------------------------------------------------------------------------------ statistics
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("M", [1000, 999, 1, 2])
def test_direction_statistics(M):
    from hunyuanworld_mirror_amd import NearestIndex, direction_statistics
    rng = np.random.default_rng(100 + M)
    ref = _ref_cloud("blobs", 5000, rng)
    q = _queries("near", M, ref, rng)
    na, nb = _unit(rng, M), _unit(rng, len(ref))
    d2, idx = H.nearest_bruteforce(q, ref)
    d32 = np.sqrt(d2)
    # thresholds between the helper's distances: none within 4 ulp of a threshold, so a count cannot hinge on the last bit
    s = np.sort(d32)
    taus = [0.5 * float(s[0])] + [float(np.float32(0.5 * (float(s[k]) + float(s[k + 1])))) for k in (M // 3, (2 * M) // 3) if k + 1 < M]
    taus.append(float(s[-1]) * 2.0 + 1.0)
    for t in taus:
        assert np.abs(d32.astype(np.float64) - t).min() > 4 * float(H.ulp32(t)), "a threshold within 4 ulp of a distance: choose another"
    want = H.direction_stats_np(d32, idx, na, nb, taus)
    dist, gi = NearestIndex(_gpu(ref)).query(_gpu(q))
    got = direction_statistics(dist, gi, _gpu(na), _gpu(nb), taus)
    assert all(v.dtype == torch.float64 and v.device.type == "cuda" for v in got.values())
    mean_err = abs(float(got["mean"]) - want["mean"]) / want["mean"]
    med_ulp = abs(float(got["median"]) - want["median"]) / float(H.ulp32(want["median"]))
    nc_err = max(abs(float(got["nc_mean"]) - want["nc_mean"]), abs(float(got["nc_median"]) - want["nc_median"]))
    print(f"[recon_metrics] statistics M={M}: mean error / bound {mean_err / (2 * H.U32):.3f}, median {med_ulp:.2f} ulp (bound 1), "
          f"nc error / bound {nc_err / (8 * H.U32):.3f}, counts {got['counts'].tolist()} vs {want['counts']}")
    assert mean_err <= 2 * H.U32
    assert med_ulp <= 1.0
    assert got["counts"].tolist() == [float(c) for c in want["counts"]]
    assert nc_err <= 8 * H.U32
    again = direction_statistics(dist, gi, _gpu(na), _gpu(nb), taus)
    assert all(torch.equal(got[k], again[k]) for k in got)          # the same bits


def test_accuracy_completeness_matches_helper():
    from hunyuanworld_mirror_amd import accuracy_completeness
    rng = np.random.default_rng(7)
    gt = _ref_cloud("plane", 3001, rng)
    pred = (gt[:2500] + rng.normal(0, 0.01, (2500, 3))).astype(np.float32)
    gn, pn = _unit(rng, len(gt)), _unit(rng, len(pred))
    taus = (0.0123, 0.0371)
    want = H.accuracy_completeness_ref(pred, gt, pn, gn, taus)
    got = accuracy_completeness(_gpu(pred), _gpu(gt), _gpu(pn), _gpu(gn), taus)
    assert set(got) == set(want)
    for k in ("acc", "comp", "chamfer"):
        assert abs(float(got[k]) - want[k]) <= 2 * H.U32 * want[k], k
    for k in ("acc_med", "comp_med"):
        assert abs(float(got[k]) - want[k]) <= float(H.ulp32(want[k])), k
    for k in ("nc_acc", "nc_comp", "nc", "nc_acc_med", "nc_comp_med"):
        assert abs(float(got[k]) - want[k]) <= 8 * H.U32, k
    for k in ("precision", "recall", "fscore"):
        assert got[k].shape == (2,) and np.abs(got[k].cpu().numpy() - np.array(want[k])).max() <= 1e-15, k
    plain = accuracy_completeness(_gpu(pred), _gpu(gt))
    assert set(plain) == {"acc", "acc_med", "comp", "comp_med", "chamfer"} and torch.equal(plain["acc"], got["acc"])


# ------------------------------------------------------------------------------------------------ umeyama
def _umeyama_case(kind, rng):
    P = {"full": 10000, "planar": 4000, "mirrored": 1000, "noscale": 777, "masked": 3000, "three": 3}[kind]
    src = rng.normal(size=(P, 3)) * [1.0, 0.7, 0.5]
    if kind == "planar":
        src[:, 2] = 0.0
    if kind == "three":
        src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.8, 0.0]])
    src = (src @ _rotation([3, 1, 2], 50.0).T + [2.0, -1.0, 0.5]).astype(np.float32)
    lin = 1.7 * _rotation([1, -2, 1], 73.0)
    if kind == "mirrored":
        lin = lin @ np.diag([1.0, 1.0, -1.0])
    noise = 0.0 if kind == "three" else 1e-3
    dst = (src.astype(np.float64) @ lin.T + [0.5, 4.0, -3.0] + rng.normal(0, noise, (P, 3))).astype(np.float32)
    mask = (np.arange(P) % 3 != 1) if kind == "masked" else None
    return src, dst, mask


@pytest.mark.parametrize("kind", ["full", "planar", "mirrored", "noscale", "masked", "three"])
def test_umeyama_matches_numpy_svd(kind):
    from hunyuanworld_mirror_amd import umeyama
    src, dst, mask = _umeyama_case(kind, np.random.default_rng(len(kind)))
    with_scale = kind != "noscale"
    s_src, s_dst = (src, dst) if mask is None else (src[mask], dst[mask])
    sv = H.cov_singular_values(s_src, s_dst)
    assert len(s_src) <= 10 ** 4 and sv[1] >= 0.1 * sv[0], sv          # the conditioning the bound is derived for
    want = H.umeyama_np(s_src, s_dst, with_scale)
    s, R, t = umeyama(_gpu(src), _gpu(dst), None if mask is None else _gpu(mask), with_scale)
    assert s.dtype == R.dtype == t.dtype == torch.float64 and s.shape == () and R.shape == (3, 3) and t.shape == (3,)
    got = (float(s), R.cpu().numpy(), t.cpu().numpy())
    extent = float((s_dst.max(0) - s_dst.min(0)).max())
    eR, es, et = np.abs(got[1] - want[1]).max(), abs(got[0] - want[0]) / want[0], np.abs(got[2] - want[2]).max() / extent
    print(f"[recon_metrics] umeyama {kind}: |dR| {eR:.2e}, |ds|/s {es:.2e}, |dt|/extent {et:.2e} (bound 1e-10), sv {sv}")
    assert eR <= 1e-10 and es <= 1e-10 and et <= 1e-10
    assert abs(np.linalg.det(got[1]) - 1.0) <= 1e-12          # a proper rotation, also for the mirrored target
    if not with_scale:
        assert got[0] == 1.0
    if mask is not None:          # the mask equals the call on the compacted pairs
        s2, R2, t2 = umeyama(_gpu(s_src), _gpu(s_dst), None, with_scale)
        assert max(abs(float(s2) - got[0]), np.abs(R2.cpu().numpy() - got[1]).max(), np.abs(t2.cpu().numpy() - got[2]).max()) <= 1e-12
        m8 = _gpu(mask.astype(np.uint8))
        s3, R3, t3 = umeyama(_gpu(src), _gpu(dst), m8, with_scale)
        assert torch.equal(s3, s) and torch.equal(R3, R) and torch.equal(t3, t)


# ------------------------------------------------------------------------------------------------ icp and evaluate_pointmaps
@pytest.fixture(scope="module")
def icp_case():
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ref = (g + rng.uniform(-0.1, 0.1, g.shape)).astype(np.float32)
    extent = float((ref.max(0) - ref.min(0)).max())
    c = ref.astype(np.float64).mean(0)
    R0, t0 = _rotation([1, 2, 3], 2.0), 0.01 * extent * np.array([0.6, -0.64, 0.48])
    src = (((ref[::2].astype(np.float64) - c) @ R0.T) + c + t0).astype(np.float32)
    iters = 8
    t64, rms64, gap = H.icp_ref(src, ref, max_dist=1.0, iters=iters, dtype=torch.float64)
    t32, rms32, _ = H.icp_ref(src, ref, max_dist=1.0, iters=iters, dtype=torch.float32)
    assert gap >= 1e-3, gap          # the correspondences do not hinge on rounding
    return dict(ref=ref, src=src, extent=extent, iters=iters, t64=t64, t32=t32, rms64=rms64)


def test_icp_matches_helper(icp_case):
    from hunyuanworld_mirror_amd import NearestIndex, icp
    c = icp_case
    index = NearestIndex(_gpu(c["ref"]))
    (s, R, t), rms = icp(_gpu(c["src"]), index, max_dist=1.0, iters=c["iters"])
    got = (float(s), R.cpu().numpy(), t.cpu().numpy())
    e32 = H.transform_error(c["t32"], c["t64"], c["extent"])
    err = H.transform_error(got, c["t64"], c["extent"])
    bound = max(4 * e32, 1e-6)
    print(f"[recon_metrics] icp: error {err:.3e}, e32 {e32:.3e}, error / bound {err / bound:.3f}, error / (4 e32) {err / max(4 * e32, 1e-300):.3f}")
    assert err <= bound
    h = rms.cpu().numpy()
    assert h.shape == (c["iters"],) and rms.dtype == torch.float64
    # the RMS does not increase, down to the floor the number format sets: every transformed coordinate is rounded to fp32 (2^-24 of its
    # size per axis), which moves a pair distance by at most sqrt(3) 2^-24 max|coordinate|
    floor = np.sqrt(3.0) * H.U32 * float(np.abs(c["ref"]).max() + 1.0)
    print(f"[recon_metrics] icp rms {h}, floor {floor:.2e}")
    assert all(b <= a + floor for a, b in zip(h, h[1:])), h
    assert np.abs(h - np.array(c["rms64"])).max() <= 1e-5 * h[0]
    assert got[0] == 1.0
    # tol=None and a tol that never triggers: identical bits
    (s1, R1, t1), rms1 = icp(_gpu(c["src"]), index, max_dist=1.0, iters=4)
    (s2, R2, t2), rms2 = icp(_gpu(c["src"]), index, max_dist=1.0, iters=4, tol=0.0)
    assert rms2.shape == (4,) and torch.equal(rms1, rms2) and torch.equal(s1, s2) and torch.equal(R1, R2) and torch.equal(t1, t2)
    # a tol that triggers ends the loop early
    _, rms3 = icp(_gpu(c["src"]), index, max_dist=1.0, iters=30, tol=0.5)
    assert 2 <= rms3.shape[0] < 30
    # a max_dist that keeps fewer than 3 pairs returns init
    init = (torch.tensor(1.0, dtype=torch.float64, device=DEV), _gpu(_rotation([0, 1, 0], 1.0)), _gpu(np.array([0.01, 0.02, 0.03])))
    (s4, R4, t4), rms4 = icp(_gpu(c["src"]), index, init=init, max_dist=1e-9, iters=3)
    assert torch.equal(s4, init[0]) and torch.equal(R4, init[1]) and torch.equal(t4, init[2]) and bool((rms4 == 0).all())
    # with_scale: the scale of a shrunken source is found
    mid = c["src"].mean(0)
    (s5, _, _), _ = icp(_gpu(mid + np.float32(0.99) * (c["src"] - mid)), index, max_dist=1.0, iters=c["iters"], with_scale=True)
    assert abs(float(s5) - 1 / 0.99) < 1e-4


def test_evaluate_pointmaps():
    from hunyuanworld_mirror_amd import accuracy_completeness, evaluate_pointmaps
    rng = np.random.default_rng(13)
    S, Hh, W = 2, 24, 32
    u, v = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, Hh))
    gt = np.stack([np.stack([u + 2.5 * k, v, 2.0 + 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * k], -1) for k in range(S)]).astype(np.float32)
    mask = rng.uniform(size=(S, Hh, W)) > 0.3
    gn, pn = _unit(rng, S * Hh * W).reshape(S, Hh, W, 3), _unit(rng, S * Hh * W).reshape(S, Hh, W, 3)
    pred = (gt + rng.normal(0, 0.01, gt.shape)).astype(np.float32)
    taus = (0.011, 0.023)
    # align="none" equals accuracy_completeness on the compacted points
    m, tr = evaluate_pointmaps(_gpu(pred), _gpu(gt), _gpu(mask), _gpu(pn), _gpu(gn), align="none", thresholds=taus)
    want = accuracy_completeness(_gpu(pred[mask]), _gpu(gt[mask]), _gpu(pn[mask]), _gpu(gn[mask]), taus)
    assert set(m) == set(want) and all(torch.equal(m[k], want[k]) for k in m)
    assert float(tr[0]) == 1.0 and torch.equal(tr[1], torch.eye(3, dtype=torch.float64, device=DEV)) and not bool(tr[2].any())
    m8, _ = evaluate_pointmaps(_gpu(pred), _gpu(gt), _gpu(mask.astype(np.uint8)), align="none")
    assert torch.equal(m8["acc"], m["acc"]) and "nc" not in m8
    # a known Sim(3) applied to pred: umeyama takes it back
    extent = float((gt[mask].max(0) - gt[mask].min(0)).max())
    R0, s0, t0 = _rotation([2, -1, 1], 25.0), 0.6, np.array([1.0, -2.0, 0.5])
    moved = (s0 * gt.astype(np.float64) @ R0.T + t0).astype(np.float32)
    m2, tr2 = evaluate_pointmaps(_gpu(moved), _gpu(gt), _gpu(mask), align="umeyama")
    print(f"[recon_metrics] evaluate_pointmaps umeyama: acc / extent {float(m2['acc']) / extent:.2e}, comp / extent {float(m2['comp']) / extent:.2e} (bound 1e-5)")
    assert float(m2["acc"]) < 1e-5 * extent and float(m2["comp"]) < 1e-5 * extent
    assert abs(float(tr2[0]) - 1 / s0) < 1e-6 and np.abs(tr2[1].cpu().numpy() - R0.T).max() < 1e-6
    # and with ICP behind it the result stays there
    m3, tr3 = evaluate_pointmaps(_gpu(moved), _gpu(gt), _gpu(mask), align="umeyama+icp", icp_iters=3)
    assert float(m3["acc"]) < 1e-5 * extent and float(m3["comp"]) < 1e-5 * extent
    with pytest.raises(ValueError):
        evaluate_pointmaps(_gpu(pred), _gpu(gt), _gpu(np.zeros_like(mask)))          # nothing valid
