"""GPU: the edges of the post-path geometry kernels, each against a host reference in numpy / fp64.

create_confidence_mask (select.hip): exact equality with oracle/geometry_ref (itself held against torch.topk by test_geometry_cpu.py) at
  the count K for p = 33.3, the 4096-element block edges with the threshold inside a plateau, 257 blocks (the scan's multi-entry path
  with need_eq < total_eq), NaN of both signs, all-equal inputs, the 1e-5f validity boundary, and the entry's refusals.
depth_to_world (elementwise.hip), through the C ABI: cam bitwise equal to the fp32 oracle, mask exact, world per element within
  8 * 2^-24 * (sum_j |E_ij| |cam_j| + |E_i3|) of an fp64 evaluation of R cam + t on the GPU's own fp32 cam: the gamma_4 bound of three
  products and three additions with a factor 2 of margin.  4-pixel vectors that straddle views, unaligned pointers (scalar fallback)
  inside guarded buffers, a second grid-stride trip of the scalar kernel, NULL outputs, depths at and around eps and non-finite.
prune_gs (splat_prune.hip) against oracle/worldmirror_ref.prune_gs: means at and next to voxel boundaries (true fp32 division), sums in
  index order (bit-equal), and sizes around a wave and a block."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_fixtures as F
from oracle import geometry_ref as G
from oracle import worldmirror_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WM_OK, WM_ERR_INVALID = 0, 1


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


NEG_NAN, POS_NAN = _bits(0xFFC00000), _bits(0x7FC00000)


def _mask(conf, percent):
    from hunyuanworld_mirror_amd import create_confidence_mask
    m = create_confidence_mask(torch.from_numpy(conf).to(DEV), percent)
    assert m.dtype == torch.bool and m.shape == (conf.size,)
    return m.cpu().numpy()


# ------------------------------------------------------------------------------------------------ create_confidence_mask
@pytest.mark.parametrize("n,K", [(1000, 667), (10000, 6670)])
def test_confidence_mask_count_at_33_3(n, K):
    """p = 33.3 as the caller's Python float: the reference keeps ceil(n * 66.7 / 100) in double; an fp32 image of p keeps one more"""
    g = torch.Generator().manual_seed(n)
    conf = (1.0 + torch.randperm(n, generator=g).float()).numpy()          # distinct: no tie anywhere
    want = G.create_confidence_mask(conf, 33.3)
    got = _mask(conf, 33.3)
    print(f"n={n} p=33.3: kept {int(got.sum())}, reference {K}")
    assert int(want.sum()) == K
    assert int(got.sum()) == K
    assert np.array_equal(got, want)


def _plateau_check(conf, percent):
    """equality with the oracle; the threshold value is a plateau of which only a part is kept: its first members in index order"""
    want = G.create_confidence_mask(conf, percent)
    K = int(want.sum())
    kth = np.sort(conf)[::-1][K - 1]
    plateau = np.nonzero(conf == kth)[0]
    need = K - int((conf > kth).sum())
    assert 0 < need < len(plateau), "the fixture must cut a plateau"
    got = _mask(conf, percent)
    assert np.array_equal(got, want)
    assert np.array_equal(np.nonzero(got & (conf == kth))[0], plateau[:need])
    return plateau, need


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
@pytest.mark.parametrize("percent", [30.0, 50.0])
def test_confidence_mask_block_edges(n, percent):
    """one block less one element, one block, one block and one element, two and one: values in {1, 2, 3}, so the K-th value is a third
    of the array spread over every block"""
    g = torch.Generator().manual_seed(n)
    conf = torch.randint(1, 4, (n,), generator=g).float().numpy()
    conf[-1] = 1.0 if percent == 30.0 else 2.0          # the K-th value: a plateau member in the last (for 4097 and 8193: one-element) block
    plateau, need = _plateau_check(conf, percent)
    assert conf[plateau[0]] == conf[-1]
    if n > 4096:
        assert plateau[0] < 4096 <= plateau[-1]


def test_confidence_mask_257_blocks():
    """1 048 577 elements are 257 blocks: the scan of the per-block tie counts takes two entries per thread, and with values in {1..5} at
    p = 30 the threshold value 2 is kept in part (need_eq < total_eq), so every block's scanned offset decides its elements"""
    n = 1048577
    g = torch.Generator().manual_seed(257)
    conf = torch.randint(1, 6, (n,), generator=g).float().numpy()
    conf[-1] = 2.0
    plateau, need = _plateau_check(conf, 30.0)
    assert conf[plateau[0]] == 2.0 and 100 * 4096 < plateau[need - 1] < 200 * 4096, "the cut falls in the middle blocks, past a hundred offsets"


@pytest.mark.parametrize("first,second", [(NEG_NAN, POS_NAN), (POS_NAN, NEG_NAN)], ids=["neg_first", "pos_first"])
def test_confidence_mask_nan_of_both_signs(first, second):
    g = torch.Generator().manual_seed(21)
    conf = torch.randn(5000, generator=g).numpy()
    conf[0], conf[4500] = np.inf, np.inf
    conf[7], conf[4099] = -np.inf, -np.inf
    conf[40], conf[4100], conf[4999] = first, second, first          # NaNs in both blocks, +inf in front of them
    for percent in (0.0, 30.0, 99.99):
        want = G.create_confidence_mask(conf, percent)
        got = _mask(conf, percent)
        assert np.array_equal(got, want), percent
    assert G.confidence_mask_count(conf.size, 99.99) == 1
    assert np.array_equal(np.nonzero(got)[0], [40]), "K = 1: the lowest-index NaN, above both +inf"
    assert np.array_equal(np.nonzero(_mask(conf, 99.95))[0], [40, 4100, 4999]), "K = 3: the three NaNs, either sign"


def test_confidence_mask_all_equal_and_everything_kept():
    conf = np.full(10007, 3.5, np.float32)
    for percent in (30.0, 80.0, 99.99):
        got = _mask(conf, percent)
        K = G.confidence_mask_count(conf.size, percent)
        assert np.array_equal(np.nonzero(got)[0], np.arange(K)), percent          # the first K in index order
    g = torch.Generator().manual_seed(2)
    conf = torch.rand(5000, generator=g).numpy()
    conf[::7] = 0.0
    assert G.confidence_mask_count(5000, 1e-9) == 5000          # a tiny positive p: ceil(n (100 - p) / 100) = n
    assert _mask(conf, 1e-9).all() and _mask(np.full(5000, 3.5, np.float32), 1e-9).all()


def test_confidence_mask_validity_boundary():
    """1e-5f counts as -inf, its successor is a live value.  100 successors, 100 x 1e-5f and 800 zeros, shuffled: K = 100 keeps exactly the
    successors; K = 150 keeps them and the first 50 of the -inf group in index order, zeros and 1e-5f alike"""
    g = torch.Generator().manual_seed(15)
    e5 = np.float32(1e-5)
    succ = np.nextafter(e5, np.float32(1))
    conf = np.zeros(1000, np.float32)
    where = torch.randperm(1000, generator=g).numpy()
    conf[where[:100]], conf[where[100:200]] = succ, e5
    for percent, K in ((90.0, 100), (85.0, 150)):
        assert G.confidence_mask_count(1000, percent) == K
        want = G.create_confidence_mask(conf, percent)
        got = _mask(conf, percent)
        assert np.array_equal(got, want), percent
        assert got[conf == succ].all()
    assert np.array_equal(np.nonzero(_mask(conf, 90.0))[0], np.sort(where[:100]))
    dead = np.nonzero(conf != succ)[0]
    assert np.array_equal(np.nonzero(got & (conf != succ))[0], dead[:50]) and (conf[dead[:50]] == e5).any() and (conf[dead[:50]] == 0).any()


def test_confidence_mask_refusals_leave_the_mask_alone():
    from hunyuanworld_mirror_amd import _lib
    from hunyuanworld_mirror_amd._lib import ptr, stream
    L = _lib.lib()
    n = 5000
    conf = torch.rand(n, device=DEV)
    wsb = L.wm_confidence_mask_workspace_bytes(n)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    mask = torch.full((n,), 0xAB, device=DEV, dtype=torch.uint8)
    s = stream(torch.device(DEV))
    assert L.wm_confidence_mask(None, n, 30.0, ptr(mask), ptr(ws), wsb, s) == WM_ERR_INVALID
    assert L.wm_confidence_mask(ptr(conf), n, 30.0, None, ptr(ws), wsb, s) == WM_ERR_INVALID
    assert L.wm_confidence_mask(ptr(conf), n, 30.0, ptr(mask), None, wsb, s) == WM_ERR_INVALID
    assert L.wm_confidence_mask(ptr(conf), n, 30.0, ptr(mask), ptr(ws), wsb - 1, s) == WM_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((mask == 0xAB).all()), "a refused call launches nothing"
    assert L.wm_confidence_mask(ptr(conf), n, 30.0, ptr(mask), ptr(ws), wsb, s) == WM_OK          # the same arguments, whole: accepted
    torch.cuda.synchronize()
    assert int(mask.sum()) == 3500 and int(mask.max()) == 1


# ------------------------------------------------------------------------------------------------ depth_to_world
U = 2.0 ** -24          # fp32 unit roundoff
SENT_F, SENT_B = -12345.678, 0xAB
GUARD = 4               # floats / bytes on either side of an output: 16 B keeps an aligned output aligned


def _cameras(B, seed):
    g = torch.Generator().manual_seed(seed)
    ext = torch.eye(4).repeat(B, 1, 1)
    ext[:, :3, :3] = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    ext[:, :3, 3] = torch.randn(B, 3, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 400.0 + 50.0 * torch.rand(B, generator=g)          # a different K per view
    K[:, 1, 1] = 410.0 + 50.0 * torch.rand(B, generator=g)
    K[:, 0, 2] = 1.0 + torch.rand(B, generator=g)
    K[:, 1, 2] = 1.0 + torch.rand(B, generator=g)
    K[:, 2, 2] = 1.0
    return ext.numpy(), K.numpy()


class _Run:
    """one call of wm_depth_to_world with every buffer inside a sentinel-filled one: d_off floats in front of the depth, m_off bytes in
    front of the mask move the pointers off their alignment; world / cam / mask may be left out (NULL)"""

    def __init__(self, depth, ext, intr, d_off=0, m_off=0, world=True, cam=True, mask=True, eps=1e-8):
        from hunyuanworld_mirror_amd import _lib
        from hunyuanworld_mirror_amd._lib import ptr, stream
        B, H, W = depth.shape
        n = B * H * W
        dbuf = torch.zeros(n + d_off, device=DEV)
        d = dbuf[d_off:]
        d.copy_(torch.from_numpy(depth).reshape(-1))
        e, k = torch.from_numpy(ext).to(DEV).contiguous(), torch.from_numpy(intr).to(DEV).contiguous()
        self.n, self.m_off, self.shape = n, m_off, (B, H, W)
        self.wbuf = torch.full((3 * n + 2 * GUARD,), SENT_F, device=DEV)
        self.cbuf = torch.full((3 * n + 2 * GUARD,), SENT_F, device=DEV)
        self.mbuf = torch.full((n + 2 * GUARD + m_off,), SENT_B, device=DEV, dtype=torch.uint8)
        w, c, m = self.wbuf[GUARD:GUARD + 3 * n], self.cbuf[GUARD:GUARD + 3 * n], self.mbuf[GUARD + m_off:GUARD + m_off + n]
        assert d.data_ptr() % 16 == (4 * d_off) % 16 and w.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0 and m.data_ptr() % 4 == m_off % 4
        st = _lib.lib().wm_depth_to_world(ptr(d), ptr(e), ptr(k), ptr(w) if world else None, ptr(c) if cam else None, ptr(m) if mask else None,
                                          B, H, W, C.c_float(eps), stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert st == WM_OK
        self.wbits, self.cbits, self.mbits = (self.wbuf.cpu().numpy().view(np.uint32), self.cbuf.cpu().numpy().view(np.uint32),
                                              self.mbuf.cpu().numpy())

    def guards_intact(self):
        s = np.array([SENT_F], np.float32).view(np.uint32)[0]
        n, mo = self.n, self.m_off
        return bool((self.wbits[:GUARD] == s).all() and (self.wbits[GUARD + 3 * n:] == s).all() and (self.cbits[:GUARD] == s).all()
                    and (self.cbits[GUARD + 3 * n:] == s).all() and (self.mbits[:GUARD + mo] == SENT_B).all()
                    and (self.mbits[GUARD + mo + n:] == SENT_B).all())

    def outputs(self):
        B, H, W = self.shape
        n, mo = self.n, self.m_off
        return (self.wbits[GUARD:GUARD + 3 * n].view(np.float32).reshape(B, H, W, 3), self.cbits[GUARD:GUARD + 3 * n].view(np.float32).reshape(B, H, W, 3),
                self.mbits[GUARD + mo:GUARD + mo + n].reshape(B, H, W))


def _world_within_bound(world, cam, ext, where=None):
    """per element: |world - (R cam + t in fp64)| <= 8 u (sum_j |E_ij| |cam_j| + |E_i3|), cam the GPU's own fp32 values"""
    E, c = ext.astype(np.float64), cam.astype(np.float64)
    want = np.einsum("bij,bhwj->bhwi", E[:, :3, :3], c) + E[:, None, None, :3, 3]
    bound = 8 * U * (np.einsum("bij,bhwj->bhwi", np.abs(E[:, :3, :3]), np.abs(c)) + np.abs(E[:, None, None, :3, 3]))
    err = np.abs(world.astype(np.float64) - want)
    if where is not None:
        err, bound = err[where], bound[where]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"world: worst error / bound = {worst:.3f} over {err.size} elements")
    return bool((err <= bound).all())


def _check_finite(run, depth, ext, intr, eps=1e-8):
    world, cam, mask = run.outputs()
    ow, oc, om = G.depth_to_world_coords_points(depth, ext, intr, eps)
    assert run.guards_intact()
    assert np.array_equal(mask, om.astype(np.uint8))
    assert np.array_equal(cam.view(np.uint32), oc.view(np.uint32)), "camera points: the reference's fp32 expressions, bit for bit"
    assert _world_within_bound(world, cam, ext)


def _straddle_case():
    B, H, W = 4, 3, 3          # 9 pixels per view, 36 in all: the vector kernel's 4-pixel groups 2, 4 and 6 hold pixels of two views
    g = torch.Generator().manual_seed(33)
    depth = (0.5 + 4.0 * torch.rand(B, H, W, generator=g)).numpy()
    depth[1, 1, 1] = 0.0
    ext, intr = _cameras(B, 34)
    return depth, ext, intr


@pytest.mark.parametrize("d_off,m_off", [(0, 0), (1, 0), (0, 1)], ids=["aligned_vector", "depth_plus_one_float", "mask_plus_one_byte"])
def test_depth_to_world_vectors_straddle_views_and_unaligned_pointers(d_off, m_off):
    depth, ext, intr = _straddle_case()
    _check_finite(_Run(depth, ext, intr, d_off=d_off, m_off=m_off), depth, ext, intr)


def test_depth_to_world_scalar_second_grid_trip():
    """725 x 725 = 525 625 pixels, odd: the scalar kernel, whose grid is capped at 2048 x 256 = 524 288 threads, loops a second time"""
    B, H, W = 1, 725, 725
    g = torch.Generator().manual_seed(725)
    depth = (0.5 + 4.0 * torch.rand(B, H, W, generator=g))
    depth[depth < 0.7] = 0.0
    depth = depth.numpy()
    ext, intr = _cameras(B, 726)
    intr[:, 0, 2], intr[:, 1, 2] = 362.3, 361.9
    _check_finite(_Run(depth, ext, intr), depth, ext, intr)


@pytest.mark.parametrize("d_off", [0, 1], ids=["vector", "scalar"])
def test_depth_to_world_null_outputs(d_off):
    depth, ext, intr = _straddle_case()
    full = _Run(depth, ext, intr, d_off=d_off)
    sent = np.array([SENT_F], np.float32).view(np.uint32)[0]
    for skip in ("world", "cam", "mask"):
        r = _Run(depth, ext, intr, d_off=d_off, **{skip: False})
        assert r.guards_intact()
        for name, got, ref, s in (("world", r.wbits, full.wbits, sent), ("cam", r.cbits, full.cbits, sent), ("mask", r.mbits, full.mbits, SENT_B)):
            if name == skip:
                assert (got == s).all(), f"{name} = NULL: its buffer is not written"
            else:
                assert np.array_equal(got, ref), f"{skip} = NULL changes {name}"


@pytest.mark.parametrize("shape", [(2, 4, 6), (2, 3, 5)], ids=["vector", "scalar"])
def test_depth_to_world_depths_at_eps_and_non_finite(shape):
    B, H, W = shape
    eps = np.float32(1e-8)
    special = np.array([eps, np.nextafter(eps, np.float32(1)), 0.0, -0.0, -1.5, np.inf, np.nan, np.nextafter(eps, np.float32(0)), -np.inf], np.float32)
    g = torch.Generator().manual_seed(B * H * W)
    depth = (0.5 + torch.rand(B, H, W, generator=g)).numpy()
    flat = depth.reshape(-1)
    flat[1:1 + len(special)] = special          # view 0
    flat[H * W + 2:H * W + 2 + len(special)] = special[::-1]          # view 1, other pixel columns
    ext, intr = _cameras(B, 77)
    depth[0, H - 1, 2] = np.inf
    intr[0, 0, 2] = 2.0          # u - cx = 0 at u = 2: 0 * inf = NaN in x there, beside an infinite z
    run = _Run(depth, ext, intr)
    world, cam, mask = run.outputs()
    with np.errstate(all="ignore"):
        ow, oc, om = G.depth_to_world_coords_points(depth, ext, intr)
        assert run.guards_intact()
        assert np.array_equal(mask, (depth > eps).astype(np.uint8)) and np.array_equal(mask, om.astype(np.uint8))
        assert np.isnan(oc).any() and np.isinf(oc).any() and np.isnan(ow).any() and np.isinf(ow).any()          # the case does what it is for
        assert np.array_equal(np.isnan(cam), np.isnan(oc))
        assert np.array_equal(cam.view(np.uint32)[~np.isnan(oc)], oc.view(np.uint32)[~np.isnan(oc)])          # +-inf and +-0 included
        assert np.array_equal(np.isnan(world), np.isnan(ow))
        assert np.array_equal(np.isinf(world), np.isinf(ow)) and np.array_equal(world[np.isinf(ow)], ow[np.isinf(ow)])
        ok = np.isfinite(cam).all(-1)
        assert np.isfinite(world[ok]).all()
        cam0 = np.where(ok[..., None], cam, np.float32(0))
        assert _world_within_bound(world, cam0, ext, where=np.broadcast_to(ok[..., None], world.shape))


# ------------------------------------------------------------------------------------------------ prune_gs
def _prune_both(sp):
    from hunyuanworld_mirror_amd.worldmirror import prune_gs
    ref = WR.prune_gs(sp)
    got = prune_gs({k: v[None].to(DEV) for k, v in sp.items()})
    return {k: got[k][0].cpu() for k in ref}, ref


def _prune_close(got, ref):
    for k in ("means", "quats", "scales", "opacities", "sh"):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)          # the same number of voxels K
        tol = 1e-5 if k == "quats" else 2e-6   # quats: torch.norm's own reduction order in the normalisation
        assert torch.allclose(got[k], ref[k], rtol=tol, atol=tol / 10), (k, float((got[k] - ref[k]).abs().max()))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_prune_gs_voxel_boundaries(axis):
    """means at fp32(k * 0.002) and one float to either side: the voxel index hangs on the last bit of the quotient, and floor(m * (1 / v))
    differs from floor(m / v) at hundreds of them (test_geometry_cpu.py).  A splat in the wrong voxel changes K, or pulls a merged mean
    by a fraction of a voxel (0.002), a thousand times the tolerance; rows are compared in place, so the voxel order is checked too"""
    sp = F.prune_boundary_splats(axis)
    got, ref = _prune_both(sp)
    K = ref["means"].shape[0]
    print(f"axis {axis}: {sp['means'].shape[0]} splats, {K} voxels")
    assert got["means"].shape[0] == K
    assert bool((ref["means"][1:, axis] > ref["means"][:-1, axis]).all())          # torch.unique's order: ascending along the axis
    _prune_close(got, ref)


def test_prune_gs_sums_in_index_order():
    """weights over six decades in a handful of voxels: fp32 sums in another order differ in the last bits (7.6e-7 relative for the
    reversed order), so bit equality with the oracle's index-order scatter_add_ pins the order of the additions"""
    sp = F.prune_order_splats()
    got, ref = _prune_both(sp)
    assert 1 <= ref["means"].shape[0] <= 8
    for k in ("means", "scales", "sh", "opacities"):
        assert got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    assert torch.allclose(got["quats"], ref["quats"], rtol=1e-5, atol=1e-6)          # torch.norm's own reduction order


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("one_voxel", [False, True], ids=["distinct_voxels", "one_voxel"])
def test_prune_gs_wave_and_block_edges(n, one_voxel):
    """a partial last wave (its idle lanes must not reach the min / max of the voxel indices), a full one, one lane into the next; the
    same at the 256-thread block edge; voxel indices of both signs"""
    sp = F.prune_small_splats(n, one_voxel)
    got, ref = _prune_both(sp)
    assert ref["means"].shape[0] == (1 if one_voxel else n)
    _prune_close(got, ref)
