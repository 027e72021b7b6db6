"""CPU: what of the point-cloud evaluation (hunyuanworld_mirror_amd.recon_metrics, csrc/knn.hip, csrc/reconmetrics.hip) needs no GPU: the
exports and their bindings, the size calls and the refusals of the C entries (all made before anything is launched), the argument checks
of the Python layer, and the yardsticks of tests/test_recon_metrics_gpu.py (tests/recon_metrics_helper.py) on cases worked out by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

import recon_metrics_helper as H

WM_OK, WM_ERR_INVALID = 0, 1
NEW = ["wm_nearest_build_workspace_bytes", "wm_nearest_build", "wm_nearest_query_workspace_bytes", "wm_nearest_query",
       "wm_cloud_stats_workspace_bytes", "wm_cloud_stats", "wm_umeyama_workspace_bytes", "wm_umeyama"]


@pytest.fixture(scope="module")
def L():
    from hunyuanworld_mirror_amd import _lib
    return _lib.lib()


def test_new_symbols_are_exported_and_bound(L):
    from hunyuanworld_mirror_amd import _lib
    import hunyuanworld_mirror_amd as wm
    for n in NEW:
        assert n in _lib.EXPORTS, n
        fn = getattr(L, n)
        assert fn.argtypes is not None, n
        assert (fn.restype is C.c_size_t) == n.endswith("_workspace_bytes"), n
    for n in ("NearestIndex", "nearest", "umeyama", "icp", "accuracy_completeness", "evaluate_pointmaps", "direction_statistics"):
        assert hasattr(wm, n), n


def test_workspace_bytes_rules(L):
    for fn in (L.wm_nearest_build_workspace_bytes, L.wm_cloud_stats_workspace_bytes, L.wm_umeyama_workspace_bytes):
        assert fn(0) == 0 and fn(-1) == 0 and fn(1 << 31) == 0
        assert fn(1) > 0 and fn((1 << 31) - 1) > 0
    q = L.wm_nearest_query_workspace_bytes
    assert q(-1) == 0 and q(1 << 31) == 0 and q(0) > 0          # M = 0 is a valid (empty) query
    assert L.wm_nearest_build_workspace_bytes(1000) == L.wm_knn_workspace_bytes(1000, 4)          # the index IS knn's
    sizes = [L.wm_nearest_build_workspace_bytes(n) for n in (1, 1000, 100000)]
    assert sizes == sorted(sizes) and sizes[2] >= 40 * 100000
    qs = [q(m) for m in (0, 1, 1000, 100000)]
    assert qs == sorted(qs) and qs[3] >= 24 * 100000
    assert L.wm_cloud_stats_workspace_bytes(100000) >= 4 * 100000          # the |n . n'| values
    assert L.wm_umeyama_workspace_bytes(10) == L.wm_umeyama_workspace_bytes(10 ** 6)          # partial sums only


def test_entries_refuse_before_any_launch(L):
    """no device is touched: every pointer below is a host address or null, and the refusal comes first"""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    big = C.c_size_t(1 << 40)
    nb = L.wm_nearest_build_workspace_bytes(10)
    assert L.wm_nearest_build(None, 10, p, nb, p, None) == WM_ERR_INVALID
    assert L.wm_nearest_build(p, 10, None, nb, p, None) == WM_ERR_INVALID
    assert L.wm_nearest_build(p, 10, p, nb, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_build(p, 10, p, nb - 1, p, None) == WM_ERR_INVALID
    assert L.wm_nearest_build(p, 0, p, big, p, None) == WM_ERR_INVALID
    assert L.wm_nearest_build(p, 1 << 31, p, big, p, None) == WM_ERR_INVALID
    nq = L.wm_nearest_query_workspace_bytes(5)
    assert L.wm_nearest_query(None, nb, 10, p, 5, p, nq, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, nb - 1, 10, p, 5, p, nq, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, nb, 10, None, 5, p, nq, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, nb, 10, p, 5, None, nq, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, nb, 10, p, 5, p, nq - 1, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, nb, 10, p, 5, p, nq, None, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, big, 0, p, 5, p, nq, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, big, 10, p, -1, p, big, p, None, None) == WM_ERR_INVALID
    assert L.wm_nearest_query(p, big, 10, p, 1 << 31, p, big, p, None, None) == WM_ERR_INVALID
    # M = 0: accepted, nothing launched, queries and dist may be null
    assert L.wm_nearest_query(p, nb, 10, None, 0, p, L.wm_nearest_query_workspace_bytes(0), None, None, None) == WM_OK
    ns = L.wm_cloud_stats_workspace_bytes(5)
    taus = (C.c_float * 17)(*([0.5] * 17))
    assert L.wm_cloud_stats(None, None, 5, None, None, 0, taus, 1, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, taus, 1, None, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, taus, 1, p, ns - 1, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, taus, 1, p, ns, None, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, taus, 17, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, taus, -1, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, None, None, 0, None, 1, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 5, p, p, 5, taus, 0, p, ns, p, None) == WM_ERR_INVALID          # normals without idx
    assert L.wm_cloud_stats(p, p, 5, p, None, 5, taus, 0, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, p, 5, p, p, 0, taus, 0, p, ns, p, None) == WM_ERR_INVALID
    assert L.wm_cloud_stats(p, None, 0, None, None, 0, taus, 0, p, big, p, None) == WM_ERR_INVALID
    nu = L.wm_umeyama_workspace_bytes(5)
    assert L.wm_umeyama(None, p, None, 5, 1, p, nu, p, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, None, None, 5, 1, p, nu, p, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, p, None, 5, 1, None, nu, p, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, p, None, 5, 1, p, nu - 1, p, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, p, None, 5, 1, p, nu, None, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, p, None, 0, 1, p, big, p, None) == WM_ERR_INVALID
    assert L.wm_umeyama(p, p, None, 1 << 31, 1, p, big, p, None) == WM_ERR_INVALID


def test_argument_checks_come_before_any_gpu_call():
    import hunyuanworld_mirror_amd as wm
    x = torch.zeros(10, 3)
    with pytest.raises(RuntimeError):
        wm.NearestIndex(x)          # a CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError):
        wm.NearestIndex(x.numpy())
    with pytest.raises(RuntimeError):
        wm.nearest(x, x)
    with pytest.raises(RuntimeError):
        wm.umeyama(x, x)
    with pytest.raises(RuntimeError):
        wm.accuracy_completeness(x, x)
    with pytest.raises(RuntimeError):
        wm.direction_statistics(torch.zeros(4))
    with pytest.raises(RuntimeError):
        wm.evaluate_pointmaps(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), torch.ones(1, 2, 2, dtype=torch.bool))
    # shapes and options are refused whatever the device
    with pytest.raises(ValueError):
        wm.NearestIndex(torch.zeros(10, 2))
    with pytest.raises(ValueError):
        wm.NearestIndex(torch.zeros(0, 3))
    with pytest.raises(ValueError):
        wm.nearest(torch.zeros(4), x)
    with pytest.raises(ValueError):
        wm.umeyama(x, torch.zeros(9, 3))
    with pytest.raises(ValueError):
        wm.umeyama(x, x, mask=torch.zeros(10))          # a float mask
    with pytest.raises(ValueError):
        wm.icp(x, "not an index")
    with pytest.raises(ValueError):
        wm.accuracy_completeness(x, x, pred_normals=x)          # one normal set
    with pytest.raises(ValueError):
        wm.accuracy_completeness(x, x, thresholds=[0.1] * 17)
    with pytest.raises(ValueError):
        wm.accuracy_completeness(x, x, thresholds=[-1.0])
    with pytest.raises(ValueError):
        wm.direction_statistics(torch.zeros(4, dtype=torch.float64))
    m = torch.ones(1, 2, 2, dtype=torch.bool)
    with pytest.raises(ValueError):
        wm.evaluate_pointmaps(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), m, align="icp")
    with pytest.raises(ValueError):
        wm.evaluate_pointmaps(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 3, 3), m)
    with pytest.raises(ValueError):
        wm.evaluate_pointmaps(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), m.float())
    with pytest.raises(ValueError):
        wm.evaluate_pointmaps(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), m, icp_max_dist=float("nan"))


# ------------------------------------------------------------------------------------------------ the yardsticks
def _rotation(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def test_helper_nearest_lowest_row_and_both_dtypes():
    ref = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 0, 0], [5, 5, 5]], np.float32)
    q = np.array([[1, 0, 0], [2, 0, 0], [0.25, 0, 0], [4, 4, 4]], np.float32)
    for dt in (torch.float32, torch.float64):
        d2, idx = H.nearest_bruteforce(q, ref, dt)
        assert idx.tolist() == [0, 1, 0, 4]          # the tie between rows 0..3 at q0 goes to row 0, the duplicates to the lower row
        assert d2.tolist() == [1.0, 0.0, 0.0625, 3.0]
    assert H.nearest_bruteforce(np.zeros((0, 3), np.float32), ref)[0].shape == (0,)


def test_helper_umeyama_recovers_a_known_similarity():
    rng = np.random.default_rng(3)
    src = rng.normal(size=(200, 3)) * [1.0, 0.7, 0.4]
    R0, s0, t0 = _rotation([1, 2, 3], 37.0), 1.75, np.array([0.3, -2.0, 5.0])
    s, R, t = H.umeyama_np(src, s0 * src @ R0.T + t0)
    assert abs(s - s0) < 1e-12 and np.abs(R - R0).max() < 1e-12 and np.abs(t - t0).max() < 1e-11
    s, R, t = H.umeyama_np(src, src @ R0.T + t0, with_scale=False)
    assert s == 1.0 and np.abs(R - R0).max() < 1e-12


def test_helper_umeyama_mirrored_target_gives_a_rotation():
    # the corners of a 2 x 1.2 x 0.6 box: a diagonal covariance, so the answer can be read off
    src = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-0.6, 0.6) for c in (-0.3, 0.3)]) + [3.0, 1.0, -2.0]
    dst = src * [1.0, 1.0, -1.0]          # a reflection: no rotation maps src onto it
    s, R, t = H.umeyama_np(src, dst)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    # the best rotation leaves the two strong axes alone and gives up on the weakest one
    assert np.abs(R - np.eye(3)).max() < 1e-12
    var = (src - src.mean(0)).var(0)
    assert abs(s - (var[0] + var[1] - var[2]) / var.sum()) < 1e-12


def test_helper_metrics_on_a_five_point_case():
    pred = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], np.float32)
    gt = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)
    pn = np.array([[0, 0, 1]] * 4 + [[1, 0, 0]], np.float32)
    gn = np.array([[0, 0, -1]] * 5, np.float32)
    r = H.accuracy_completeness_ref(pred, gt, pn, gn, thresholds=(0.5, 2.0))
    # pred -> gt: 0 0 0 0 6; gt -> pred: 0 0 0 0 1
    assert r["acc"] == pytest.approx(1.2) and r["acc_med"] == 0.0 and r["comp"] == pytest.approx(0.2) and r["comp_med"] == 0.0
    assert r["chamfer"] == pytest.approx(0.7)
    # |n . n'|: pred -> gt 1 1 1 1 0 (the absolute value: the flipped normals agree); gt -> pred all 1 (gt 4 pairs with pred 3)
    assert r["nc_acc"] == pytest.approx(0.8) and r["nc_acc_med"] == 1.0 and r["nc_comp"] == 1.0 and r["nc"] == pytest.approx(0.9)
    assert r["precision"] == [0.8, 0.8] and r["recall"] == [0.8, 1.0]
    assert r["fscore"] == pytest.approx([0.8, 2 * 0.8 / 1.8])
    even = H.direction_stats_np(np.array([4, 1, 3, 2], np.float32))
    assert even["median"] == 2.5 and even["mean"] == 2.5


def test_helper_icp_recovers_a_small_motion():
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ref = (g + rng.uniform(-0.1, 0.1, g.shape)).astype(np.float32)
    R0, t0 = _rotation([0, 0, 1], 2.0), np.array([0.04, 0.0, -0.02])
    c = ref.astype(np.float64).mean(0)
    src = (((ref[::2].astype(np.float64) - c) @ R0.T) + c + t0).astype(np.float32)
    (s, R, t), rms, gap = H.icp_ref(src, ref, max_dist=1.0, iters=6, dtype=torch.float64)
    assert gap > 1e-3 and rms[-1] < 1e-6 and all(b <= a * (1 + 1e-9) for a, b in zip(rms, rms[1:]))
    assert np.abs(R - R0.T).max() < 1e-6 and s == 1.0
    back = H.apply((s, R, t), src)
    assert np.abs(back - ref[::2]).max() < 1e-5
    (s, R, t), rms, _ = H.icp_ref(src, ref, max_dist=1e-9, iters=3)          # nothing kept: the transform stays
    assert s == 1.0 and np.array_equal(R, np.eye(3)) and rms == [0.0, 0.0, 0.0]
