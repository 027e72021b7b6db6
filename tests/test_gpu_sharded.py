"""GPU: the view-sharded forward (wm_forward_sharded) with 2 in-process ranks (host threads, one
handle each, sharing cuda:0; K/V + camera tokens exchanged by the library's local communicator)
equals the single-rank forward.  Multi-GPU RCCL runs use exactly this code path with
comm_allgather -> ncclAllGather."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["tiny_2v_70x70_noprior", "tiny_12v_56x70_allpriors"])
def test_two_virtual_ranks_match_single(name):
    from hunyuanworld_mirror_amd import WorldMirror, _lib
    cfg, views, flags, outs, z = load_golden(name)
    tv = {k: torch.from_numpy(v).cuda() for k, v in views.items()}
    single = WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0")
    ref = single(tv, flags)
    torch.cuda.synchronize()
    L = _lib.lib()
    world = 2
    grp = C.c_void_p(L.wm_local_group_create(world))
    models = [WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0").shard_local(grp, r, world) for r in range(world)]
    res, errs = [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(0)
            res[r] = models[r](tv, flags)
            torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errs, errs
    assert all(not t.is_alive() for t in th), "sharded forward deadlocked"
    for k in ("pts3d", "depth", "normals"):
        got = torch.cat([res[r][k] for r in range(world)], 1)
        e = rel_l2(got.cpu().numpy(), ref[k].cpu().numpy())
        print(name, k, f"sharded vs single: {e:.2e}")
        assert e < 2e-3, k          # same arithmetic, different K/V tile boundaries
        assert rel_l2(got.cpu().numpy(), outs[k]) < 6e-3  # and still close to the reference
    for r in range(world):
        assert rel_l2(res[r]["camera_params"].cpu().numpy(), ref["camera_params"].cpu().numpy()) < 2e-3
    del models
    L.wm_local_group_destroy(grp)


def test_two_virtual_ranks_long_sequences_use_split_kv():
    """6 views of 392 x 392 on the scaled-down architecture: 791 tokens per view, so on the sharded path cross-view
    attention sees 2 chunks x 38 key tiles and the launcher's automatic 4-way split-KV (+ combine pass) engages.
    No golden at this size: the sharded result must equal the single-rank result (bf16 noise floor)."""
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig, _lib
    cfg = WMConfig.tiny()
    g = torch.Generator().manual_seed(7)
    tv = {"img": torch.rand(1, 6, 3, 392, 392, generator=g).cuda()}
    single = WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0")
    ref = single(tv)
    torch.cuda.synchronize()
    L = _lib.lib()
    world = 2
    grp = C.c_void_p(L.wm_local_group_create(world))
    models = [WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0").shard_local(grp, r, world) for r in range(world)]
    res, errs = [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(0)
            res[r] = models[r](tv)
            torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(180)
    assert not errs, errs
    assert all(not t.is_alive() for t in th), "sharded forward deadlocked"
    for k in ("pts3d", "depth", "normals"):
        got = torch.cat([res[r][k] for r in range(world)], 1)
        assert torch.isfinite(got).all(), k
        e = rel_l2(got.cpu().numpy(), ref[k].cpu().numpy())
        print("392^2 x 6 views", k, f"sharded (split-KV) vs single: {e:.2e}")
        assert e < 3e-3, k
    del models
    L.wm_local_group_destroy(grp)


def test_bench_two_pass_gather_decision_with_virtual_ranks():
    """bench.py's N > 1 path: time the serial gather and the overlapped gather, compare one forward of each
    on every rank, headline the faster one only if the comparison passed.  Here the same function (bench.two_pass_overlap) runs on
    two in-process ranks of one GPU (host threads; reductions through a barrier instead of torch.distributed): both modes must
    execute (the 3-view x 791-token chunks are long enough for the overlapped form), agree within the key-partition-order floor,
    and the function must leave the tuning at its choice."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import bench
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig, _lib
    cfg = WMConfig.tiny()
    g = torch.Generator().manual_seed(7)
    tv = {"img": torch.rand(1, 6, 3, 392, 392, generator=g).cuda()}
    L = _lib.lib()
    world = 2
    grp = C.c_void_p(L.wm_local_group_create(world))
    models = [WorldMirror(arch=cfg).init_synthetic_weights().to("cuda:0").shard_local(grp, r, world) for r in range(world)]
    bar = threading.Barrier(world)
    box, infos, errs = [0.0] * world, [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(0)

            def allmax(x):
                box[r] = float(x)
                bar.wait(120)
                v = max(box)
                bar.wait(120)
                return v

            def set_overlap(v):   # the tuning is process-wide: nobody may still be inside a forward of the other mode
                bar.wait(120)
                if r == 0:
                    assert L.wm_set_tuning(b"comm_overlap", v) == 0
                bar.wait(120)

            def fwd():
                o = models[r](tv)
                torch.cuda.synchronize()
                return o

            def timed():
                import time
                bar.wait(120)
                t0 = time.perf_counter()
                for _ in range(2):
                    models[r](tv)
                torch.cuda.synchronize()
                bar.wait(120)
                return (time.perf_counter() - t0) / 2 * 1e3
            infos[r] = bench.two_pass_overlap(set_overlap, fwd, timed, allmax)
        except Exception as e:  # pragma: no cover
            errs.append(e)
            bar.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    try:
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        assert not errs, errs
        assert all(not t.is_alive() for t in th), "two-pass bench path deadlocked"
        pick, ms, info = infos[0]
        print(info)
        assert infos[1][0] == pick and info["comparison_passed"], info
        assert info["max_rel_l2_between_modes_over_ranks"] < info["bound"]
        assert set(info["ms_per_step"]) == {"comm_overlap_0", "comm_overlap_1"} and abs(ms - info["ms_per_step"][f"comm_overlap_{pick}"]) < 1e-3
    finally:
        L.wm_set_tuning(b"comm_overlap", -1)
        del models
        L.wm_local_group_destroy(grp)


def test_rccl_allgather_path_single_rank():
    """The RCCL collective itself (ncclAllGather on the handle's own communicator) at world size 1: the tuning key
    force_gather routes global attention through the gathered-K/V path (the shipped library reads no environment
    switch).  Run in a subprocess so that the RCCL communicator lives and dies with it."""
    import os, subprocess, sys
    code = r"""
import sys, ctypes as C, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
from conftest import load_golden, rel_l2
from hunyuanworld_mirror_amd import WorldMirror, _lib
cfg, views, flags, outs, z = load_golden('tiny_2v_70x70_noprior')
m = WorldMirror(arch=cfg).init_synthetic_weights().to('cuda:0')
L = _lib.lib()
ident = (C.c_uint8 * 128)()
assert L.wm_rccl_unique_id(ident) == 0
assert L.wm_comm_init_rccl(m._handle, ident, 0, 1) == 0, m._err()
assert L.wm_set_tuning(b"force_gather", 1) == 0
out = m({k: torch.from_numpy(v).cuda() for k, v in views.items()}, flags)
torch.cuda.synchronize()
e = rel_l2(out['pts3d'].cpu().numpy(), outs['pts3d'])
print('rccl world-1 pts3d', e)
assert e < 5e-3
# the opt-in point-to-point form of the gather (bench.py --gather p2p): at world 1 the group of sends / receives is empty and the
# rank's own chunk is a device copy -- same result bit for bit
assert L.wm_set_tuning(b"comm_p2p", 1) == 0
out2 = m({k: torch.from_numpy(v).cuda() for k, v in views.items()}, flags)
torch.cuda.synchronize()
assert torch.equal(out2['pts3d'], out['pts3d']) and torch.equal(out2['depth'], out['depth'])
print('rccl world-1 p2p gather: bit-identical')
"""
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:], r.stderr[-1500:])
    assert r.returncode == 0


def _run_ranks(models, views, flags, timeout=600):
    world = len(models)
    res, errs = [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(0)
            res[r] = models[r](views, flags)
            torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not errs, errs
    assert all(not t.is_alive() for t in th), "sharded forward deadlocked"
    return res


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_view_per_rank_at_native_resolution(dtype):
    """2 views of 518 x 518 over 2 ranks = ONE view per rank: the local chunk is 1376 keys (21.5 key tiles, <= 2048 rows).
    With the K/V gather overlapped (comm_overlap = 1) the local chunk is a piecewise (partial-writing) launch: round 2's kernel
    choice took the 128-row kernel for such a chunk, which has no partial form, and the forward failed on every rank (8 views over
    8 GPUs, 2 over 2).  Full architecture, both gather modes, both backbone dtypes, against the single-rank forward."""
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig, _lib
    g = torch.Generator().manual_seed(7)
    views = {"img": torch.rand(1, 2, 3, 518, 518, generator=g).cuda()}
    single = WorldMirror(arch=WMConfig(), dtype=dtype).init_synthetic_weights(preset="refinit").to("cuda:0")
    ref = single(views)
    torch.cuda.synchronize()
    L = _lib.lib()
    grp = C.c_void_p(L.wm_local_group_create(2))
    models = [WorldMirror(arch=WMConfig(), dtype=dtype).to("cuda:0").share_weights_from(single).shard_local(grp, r, 2) for r in range(2)]
    for overlap in (1, 0):
        assert L.wm_set_tuning(b"comm_overlap", overlap) == 0
        try:
            res = _run_ranks(models, views, [0, 0, 0])
        finally:
            L.wm_set_tuning(b"comm_overlap", -1)
        for k in ("pts3d", "depth", "normals"):
            got = torch.cat([res[r][k] for r in range(2)], 1)
            e = rel_l2(got.cpu().numpy(), ref[k].cpu().numpy())
            print(f"{dtype} overlap={overlap} {k}: sharded (1 view per rank) vs single {e:.2e}")
            assert torch.isfinite(got).all() and e < 2e-3, (k, e)
        assert rel_l2(res[1]["camera_params"].cpu().numpy(), ref["camera_params"].cpu().numpy()) < 3e-3
    del models
    L.wm_local_group_destroy(grp)


def test_c5_eight_virtual_ranks_f16_gs_head_cross_rank_prune():
    """BASELINE config 5 in its real form, on one GPU: 32 views x 518 x 518, f16 backbone, 3D-Gaussian head, sharded 4 views per
    rank over 8 in-process ranks, prune_gs ON.  prune_gs merges voxels over ALL views (rasterization.py:301-387): every rank
    gathers the ranks' raw splats (wm_allgather) and merges the full set, so preds['splats'] is one merged set, the same on
    every rank — not 8 separately merged ones.  Checked: (i) the gathered raw splats are the ranks' raw splats in view order;
    (ii) every rank's merged set is bit-identical and equals prune_gs of the concatenation; (iii) dense outputs equal the
    single-rank 32-view forward at the decorrelation floor, and the merged set has the single-rank set's size to within 1 %
    (voxel membership of a splat moves when its mean moves by the recipe's noise)."""
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig, _lib
    from hunyuanworld_mirror_amd.worldmirror import prune_gs
    world, per = 8, 4
    g = torch.Generator().manual_seed(5)
    views = {"img": torch.rand(1, world * per, 3, 518, 518, generator=g).cuda()}
    single = WorldMirror(arch=WMConfig(enable_gs=True), dtype="f16").init_synthetic_weights(preset="refinit").to("cuda:0")
    ref = single(views)
    torch.cuda.synchronize()
    n_ref = int(ref["splats"]["means"][0].shape[0])
    ref = {k: ref[k].cpu() for k in ("pts3d", "depth", "normals")}
    L = _lib.lib()
    grp = C.c_void_p(L.wm_local_group_create(world))
    models = [WorldMirror(arch=WMConfig(enable_gs=True), dtype="f16").to("cuda:0").share_weights_from(single).shard_local(grp, r, world) for r in range(world)]
    res = _run_ranks(models, views, [0, 0, 0])
    for k in ("pts3d", "depth", "normals"):
        got = torch.cat([res[r][k] for r in range(world)], 1).cpu()
        e = rel_l2(got.numpy(), ref[k].numpy())
        print(f"C5 sharded vs single {k}: {e:.2e}")
        assert torch.isfinite(got).all() and e < 2e-3, (k, e)
    raw_all = {k: torch.cat([res[r]["splats_raw"][k] for r in range(world)], 1) for k in res[0]["splats_raw"]}
    want = prune_gs(raw_all)
    n0 = int(res[0]["splats"]["means"][0].shape[0])
    print(f"C5 merged splats: {n0} (single rank {n_ref}) of {raw_all['means'].shape[1]} raw")
    assert abs(n0 - n_ref) < 0.01 * n_ref
    for r in range(world):
        for k in ("means", "sh", "opacities", "scales", "quats"):
            assert torch.equal(res[r]["splats"][k][0], want[k][0]), (r, k)
    del models
    L.wm_local_group_destroy(grp)
